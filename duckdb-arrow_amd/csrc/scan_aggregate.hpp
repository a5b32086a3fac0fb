// scan_aggregate.hpp -- the fused aggregates (K9, K10, K11) as the scan and c_api.cpp see them: agg_bind (a call's specs bound
// into a plan; host code), agg_result (what it returns, merged across devices; host code), agg_run (its device side).
#pragma once

#include "agg_bind.hpp"
#include "agg_result.hpp"
#include "agg_run.hpp"
