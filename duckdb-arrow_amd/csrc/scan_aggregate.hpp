// scan_aggregate.hpp -- the host side of the fused aggregates (mi_scan_aggregate, mi_scan_group_aggregate; K9 and K10):
// what a call is given by column name, what it returns, and the helpers the vector calls of c_api.cpp share with it.
// scan_aggregate.cpp holds the ArrowScan / MultiDeviceScan methods that bind, enqueue and drain them, and their C ABI.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi_arrow_ipc.h"
#include "agg_merge.hpp"
#include "group_key.hpp"

namespace miarrow {

//! One aggregate of mi_scan_aggregate by column name, and what a draining call returns: the accumulators, the value class
//! each is merged by (aggmerge::kClass*: what the host's merge of several devices needs), the rows seen
struct AggFactorSpec {
  bool has_column = false;   // false: the constant `add`
  std::string column;
  int64_t mul = 1, add = 0;  // MI_AGG_CONST_INT
  double fmul = 1.0, fadd = 0.0;   // MI_AGG_CONST_DOUBLE
  int32_t constants = MI_AGG_CONST_INT;
};
struct AggSpec {
  int32_t op = 0;            // aggmerge::kOp*
  std::string a, b;
  std::vector<AggFactorSpec> factors;   // kOpSumExpr
};
//! the constants of one factor as the kernels take them: int64 two's complement for an integer expression, the bits of a
//! double for a floating-point one.  Double constants on an integer expression are MI_ENOTSUP; integer constants a double
//! does not hold exactly are MI_EINVAL.  `what` begins the message.
void ExprFactorConstants(const std::string& what, bool is_float, int32_t constants, int64_t mul, int64_t add, double fmul, double fadd,
                         uint64_t* mul_bits, uint64_t* add_bits);
struct AggResult {
  std::vector<aggmerge::Partial> values;
  std::vector<int32_t> classes;
  int64_t rows_scanned = 0, rows_selected = 0;
};

//! What mi_scan_group_aggregate returns: the groups' normalised keys (group_key.hpp) and one partial per group and
//! aggregate, values[g * classes.size() + a]; kinds: groupkey::kKind* per key part.  In the result order once SortGroups ran.
struct GroupResult {
  std::vector<int32_t> kinds;
  std::vector<int32_t> classes;
  std::vector<groupkey::Key> keys;
  std::vector<aggmerge::Partial> values;
  int64_t rows_scanned = 0, rows_selected = 0;
};
//! copies the scan-wide table of K10 back (one copy: keys, accumulators, group count, flags), throws for the MI_ST_* bits it
//! carries and appends its groups to out->keys / out->values
void ReadGroupTable(const void* d_table, int n_keys, int n_aggs, hipStream_t stream, GroupResult* out);
//! the result order: ascending by key, NULLS LAST (groupkey::KeyLess)
void SortGroups(GroupResult* r);
//! a sorted result as the C ABI returns it; more groups than `capacity` is MI_EINVAL with *n_groups set
void FillGroupOutputs(const GroupResult& r, const std::vector<int32_t>& ops, mi_group_key_value* out_keys, mi_agg_value* out_values,
                      int32_t capacity, int32_t* n_groups);

//! a finished accumulator as the C ABI returns it (mi_scan_aggregate, mi_aggregate_vectors)
inline void FillAggValue(int32_t op, int32_t cls, const aggmerge::Partial& p, mi_agg_value* v) {
  std::memset(v, 0, sizeof(*v));
  v->count = static_cast<int64_t>(p.count);
  if (op == aggmerge::kOpCountStar || op == aggmerge::kOpCount) {
    v->kind = MI_AGG_VALUE_INT128;
    v->lo = p.count;
    return;
  }
  v->kind = cls == aggmerge::kClassFloat ? MI_AGG_VALUE_DOUBLE : MI_AGG_VALUE_INT128;
  v->is_null = aggmerge::IsNull(op, p) ? 1 : 0;
  if (v->is_null) return;
  v->lo = p.lo;
  v->hi = static_cast<int64_t>(p.hi);
}
//! "SUM", "MIN", ... for messages
const char* AggOpName(int32_t op);
//! MI_AGG_TIMING=1: device milliseconds of agg_windows / agg_combine summed over this process's calls of mi_scan_aggregate,
//! and of group_windows / group_combine over its calls of mi_scan_group_aggregate
void AggTimingTotals(double out_ms[2]);
void GroupTimingTotals(double out_ms[2]);

}  // namespace miarrow
