// agg_run.hpp -- the device side of one fused-aggregate call (K9, K10 or K11): the buffers its mode needs, the launches a
// batch of rows gets, the read-back.  The scan gives it every record batch behind the filter; the vector calls of c_api.cpp
// give it their one batch.  The only unit of the aggregates that calls HIP.
#pragma once

#include <hip/hip_runtime_api.h>

#include <vector>

#include "agg_bind.hpp"
#include "agg_result.hpp"
#include "hip_resources.hpp"
#include "kernels.hpp"

namespace miarrow {

class AggRun {
 public:
  //! the shape of the programs Batch will be given: `key_cls` is K11's one key class (groupkey::kKey*), ops / classes one per
  //! aggregate (the class SUM / MIN / MAX merge by).  `count_time`: with MI_AGG_TIMING=1 in the environment the device time
  //! of this run's launches is added to the mode's totals (AggTimingTotals)
  AggRun(AggMode mode, int n_keys, int32_t key_cls, const std::vector<int32_t>& ops, const std::vector<int32_t>& classes, uint32_t max_groups, bool count_time);
  //! allocates and clears the call-wide state -- K9's accumulators, K10's table, K11's table and collect arrays -- on `stream`
  void Begin(hipStream_t stream);
  //! the mode's launches over `nrows` rows on `stream` (none for no rows).  The per-batch scratch grows geometrically, and what
  //! it outgrew lives until the run ends (earlier batches may still read it).  Allocates when it grows; never synchronises.
  void Batch(const device::GroupProgram& prog, const device::AggExprTable* exprs, const mi_sel_t* sel, const uint32_t* sel_count, int64_t nrows,
             hipStream_t stream);
  //! K11: hash_group_collect; then the state copied back once `stream` is idle (K11: the head, then exactly the records in
  //! use), the MI_ST_* bits it carries thrown, and the values -- and the groups' keys, unsorted -- appended to *out
  void Finish(hipStream_t stream, GroupResult* out);

 private:
  void Stamp(hipStream_t stream);
  const AggMode mode_;
  const int n_keys_, n_aggs_;
  const uint32_t max_groups_;
  device::GroupProgram shape_;       // for hash_group_clear / _collect, whose launchers read a program's operations and classes
  bool timed_;
  DeviceBuffer d_state_, d_scratch_;
  std::vector<DeviceBuffer> outgrown_;
  std::vector<HipEvent> events_;     // timed: around every launch of a batch, launches + 1 per batch
};

//! MI_AGG_TIMING=1: device milliseconds of the mode's two kernels, summed over this process's runs that count time
void AggTimingTotals(AggMode mode, double out_ms[2]);

}  // namespace miarrow
