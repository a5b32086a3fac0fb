// kernels_aggregate.hip -- K9: up to 8 aggregates (COUNT(*), COUNT, SUM, SUM of a product, MIN, MAX, SUM of a product of up
// to 4 affine factors) over decoded vectors, under the selection vectors of the pushed-down filter (K6) or over every row
// (mi_scan_aggregate, mi_aggregate_vectors).  How a row is read and folded into a lane's partial, and how a wave reduces its
// lanes' partials, is kernels_agg_fold.inl, the one place for it: K10 (kernels_group.hip) includes the same text.
//
// agg_windows: one 256-thread workgroup per 2048-row window.  With a selection vector the lanes read sel[0 .. count)
// coalesced and gather the rows it names (ascending inside the window, as kernels_gather.hip reads them); without one they
// stream the window's rows.  Per aggregate: a lane-local partial, a wave reduction by shuffles, the four wave results
// through LDS, one record to partials[window][aggregate].  The aggregate loop is OUTSIDE the row loop: a lane holds one
// partial (4 words) at a time whatever the program's length, at the price of reading the window's <= 8 KiB of `sel` again
// per aggregate -- from L2 / the vector L1, the first aggregate brought it in -- so 8 aggregates cost no more registers
// than one and nothing spills.
// agg_combine: one workgroup, lane a folds partials[0 .. n_windows)[a] in ascending window order into the running
// accumulator of aggregate a.
// No atomics, no waiting on another workgroup: the only reduction across workgroups is the launch boundary between the
// two kernels, so every sum -- the double sums included -- is folded in one fixed order.  How two partials become one is
// agg_merge.hpp, shared with the host.
// No loaded value is used as an address except a selection index, which may come from memory the caller filled: the count
// of a window is clamped to the rows the window has, and an index at or past them is skipped and raises MI_ST_SEL_RANGE in
// the partial's flags, so nothing outside the vectors is read.
#include "device_common.hpp"
#include "agg_merge.hpp"

#include <atomic>

namespace miarrow {
namespace device {

namespace {

using aggmerge::Partial;

#include "kernels_agg_fold.inl"

// The kernel's text, once.  EXPR: the program may hold kOpSumExpr aggregates and `exprs` is their table; without it the
// branch is not compiled and `exprs` not looked at, so agg_windows<HAS_SEL> below is the kernel it was before expressions.
template <bool HAS_SEL, bool EXPR>
__device__ __forceinline__ void agg_windows_body(const AggProgram& prog, const AggExprTable* exprs, const mi_sel_t* __restrict__ sel_p,
                                                 const uint32_t* __restrict__ sel_count_p, int64_t nrows, Partial* __restrict__ partials_p) {
  __shared__ Partial wave_part[kBlockThreads / 64];
  const int64_t window = blockIdx.x;
  const int64_t row0 = window * kTileRows;
  const int64_t left = nrows - row0;
  const uint32_t n = left < kTileRows ? static_cast<uint32_t>(left < 0 ? 0 : left) : static_cast<uint32_t>(kTileRows);
  uint32_t cnt = n;
  if (HAS_SEL) {
    const uint32_t c = GC<uint32_t>(sel_count_p)[window];
    cnt = c < n ? c : n;   // a count past the window's rows is clamped: sel[] is read inside the window's slots only
  }
  gptr<const mi_sel_t> sel = GC<mi_sel_t>(sel_p) + row0;
  gptr<Partial> partials = GM<Partial>(partials_p) + window * prog.n_aggs;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma clang loop unroll(disable)
  for (int a = 0; a < prog.n_aggs; a++) {
    const AggDescDev& d = prog.aggs[a];
    const int op = d.op, cls = d.a.cls;
    Partial p = {0ull, 0ull, 0ull, 0ull};
    for (uint32_t i = threadIdx.x; i < cnt; i += kBlockThreads) {
      uint32_t r = i;
      if (HAS_SEL) {
        r = sel[i];
        if (r >= n) {   // not a row of this window: never dereferenced
          p.flags |= MI_ST_SEL_RANGE;
          continue;
        }
      }
      const int64_t row = row0 + r;
      if (EXPR && op == aggmerge::kOpSumExpr) fold_expr_row(exprs->exprs[a], cls, row, &p);
      else fold_row(d, op, cls, row, &p);
    }
#pragma unroll
    for (int dist = 32; dist >= 1; dist >>= 1) {   // wave reduction: lane l takes lane l + dist while that lane exists
      const Partial o = shfl_down_partial(p, dist);
      if (lane + dist < 64) aggmerge::Merge<EXPR>(op, cls, &p, o);
    }
    if (lane == 0) wave_part[wave] = p;
    __syncthreads();
    if (threadIdx.x == 0) {
      Partial q = wave_part[0];
#pragma unroll
      for (int k = 1; k < kBlockThreads / 64; k++) aggmerge::Merge<EXPR>(op, cls, &q, wave_part[k]);
      store_partial(partials + a, q);
    }
    __syncthreads();   // wave_part is written again by the next aggregate
  }
}

template <bool HAS_SEL>
__global__ __launch_bounds__(kBlockThreads) void agg_windows(const AggProgram prog, const mi_sel_t* __restrict__ sel_p,
                                                             const uint32_t* __restrict__ sel_count_p, int64_t nrows,
                                                             Partial* __restrict__ partials_p) {
  agg_windows_body<HAS_SEL, false>(prog, nullptr, sel_p, sel_count_p, nrows, partials_p);
}

// launched only for a program that holds a kOpSumExpr: the expression table rides behind the arguments of agg_windows
template <bool HAS_SEL>
__global__ __launch_bounds__(kBlockThreads) void agg_windows_expr(const AggProgram prog, const mi_sel_t* __restrict__ sel_p,
                                                                  const uint32_t* __restrict__ sel_count_p, int64_t nrows,
                                                                  Partial* __restrict__ partials_p, const AggExprTable exprs) {
  agg_windows_body<HAS_SEL, true>(prog, &exprs, sel_p, sel_count_p, nrows, partials_p);
}

// ops / classes: 4 bits per aggregate (a lane picks its own: no indexing of the kernel argument by a lane's number)
__global__ __launch_bounds__(64) void agg_combine(uint32_t ops, uint32_t classes, int32_t n_aggs, const Partial* __restrict__ partials_p,
                                                  int64_t n_windows, Partial* __restrict__ acc_p) {
  const int a = threadIdx.x;
  if (a >= n_aggs) return;
  const int op = static_cast<int>((ops >> (4 * a)) & 15u), cls = static_cast<int>((classes >> (4 * a)) & 15u);
  gptr<const Partial> partials = GC<Partial>(partials_p);
  gptr<Partial> acc = GM<Partial>(acc_p);
  Partial p = load_partial(acc + a);
#pragma unroll 4
  for (int64_t w = 0; w < n_windows; w++) {
    const Partial q = load_partial(partials + (w * n_aggs + a));
    aggmerge::Merge<false>(op, cls, &p, q);
  }
  store_partial(acc + a, p);
}

bool ColumnOk(const AggColumnDev& c, bool needs_values) {
  if (!needs_values) return true;
  if (!c.data) return false;
  switch (c.cls) {
    case aggmerge::kClassSigned: case aggmerge::kClassUnsigned: return c.width == 1 || c.width == 2 || c.width == 4 || c.width == 8;
    case aggmerge::kClassFloat: return c.width == 4 || c.width == 8;
    case aggmerge::kClassWide: return c.width == 16;
    default: return false;
  }
}

}  // namespace

namespace {
std::atomic<int64_t> g_agg_launches[2];   // agg_windows, agg_combine
}  // namespace

void AggLaunchCounts(int64_t out[2]) {
  out[0] = g_agg_launches[0].load();
  out[1] = g_agg_launches[1].load();
}

namespace {
// a kOpSumExpr: 1 .. 4 factors, at least one column; every column factor has data and a width of its class, none of 16 bytes;
// all integer-like or all floating point, and aggs[a].a is the first column factor's column
bool ExprOk(const AggDescDev& d, const AggExprDev& e) {
  if (e.n_factors < 1 || e.n_factors > aggmerge::kMaxExprFactors) return false;
  int columns = 0;
  for (int f = 0; f < e.n_factors; f++) {
    const AggColumnDev& c = e.factors[f].col;
    if (c.cls == aggmerge::kClassAny) continue;   // a constant
    if (c.cls == aggmerge::kClassWide || !ColumnOk(c, true)) return false;
    if (columns == 0 && (c.data != d.a.data || c.validity != d.a.validity || c.width != d.a.width || c.cls != d.a.cls)) return false;
    if ((c.cls == aggmerge::kClassFloat) != (d.a.cls == aggmerge::kClassFloat)) return false;
    columns++;
  }
  return columns > 0;
}
}  // namespace

bool AggProgramHasExpr(const AggProgram& prog) {
  for (int a = 0; a < prog.n_aggs && a < aggmerge::kMaxAggregates; a++)
    if (prog.aggs[a].op == aggmerge::kOpSumExpr) return true;
  return false;
}

bool AggProgramIsValid(const AggProgram& prog, const AggExprTable* exprs) {
  if (prog.n_aggs < 1 || prog.n_aggs > aggmerge::kMaxAggregates) return false;
  for (int a = 0; a < prog.n_aggs; a++) {
    const AggDescDev& d = prog.aggs[a];
    if (d.op < aggmerge::kOpCountStar || d.op > aggmerge::kOpSumExpr) return false;
    if (d.op == aggmerge::kOpSumExpr) {
      if (!exprs || !ExprOk(d, exprs->exprs[a])) return false;
      continue;
    }
    const bool values = d.op != aggmerge::kOpCountStar && d.op != aggmerge::kOpCount;
    if (!ColumnOk(d.a, values)) return false;
    if (d.op == aggmerge::kOpSum && d.a.cls == aggmerge::kClassWide) return false;
    if (d.op == aggmerge::kOpSumProduct) {
      if (!ColumnOk(d.b, true) || d.a.cls == aggmerge::kClassWide || d.b.cls == aggmerge::kClassWide) return false;
      if ((d.a.cls == aggmerge::kClassFloat) != (d.b.cls == aggmerge::kClassFloat)) return false;
    }
  }
  return true;
}

void PackOpsClasses(const AggProgram& prog, uint32_t* ops, uint32_t* classes) {
  *ops = *classes = 0;
  for (int a = 0; a < prog.n_aggs; a++) {
    const int op = prog.aggs[a].op == aggmerge::kOpSumExpr ? aggmerge::kOpSum : prog.aggs[a].op;   // partials of either merge as sums
    *ops |= static_cast<uint32_t>(op) << (4 * a);
    *classes |= static_cast<uint32_t>(prog.aggs[a].a.cls) << (4 * a);
  }
}

hipError_t LaunchAggWindows(const AggProgram& prog, const mi_sel_t* sel, const uint32_t* sel_count, int64_t nrows,
                            aggmerge::Partial* d_partials, hipStream_t stream, const AggExprTable* exprs) {
  MI_DROP_STALE_ERROR();
  if (nrows <= 0) return hipSuccess;
  if (!AggProgramIsValid(prog, exprs) || (sel == nullptr) != (sel_count == nullptr) || !d_partials) return hipErrorInvalidValue;
  const int64_t windows = (nrows + kTileRows - 1) / kTileRows;
  if (windows > 0x7FFFFFFFll) return hipErrorInvalidValue;
  const dim3 grid(static_cast<uint32_t>(windows)), block(kBlockThreads);
  if (AggProgramHasExpr(prog)) {
    if (sel) hipLaunchKernelGGL(agg_windows_expr<true>, grid, block, 0, stream, prog, sel, sel_count, nrows, d_partials, *exprs);
    else hipLaunchKernelGGL(agg_windows_expr<false>, grid, block, 0, stream, prog, sel, sel_count, nrows, d_partials, *exprs);
  } else if (sel) hipLaunchKernelGGL(agg_windows<true>, grid, block, 0, stream, prog, sel, sel_count, nrows, d_partials);
  else hipLaunchKernelGGL(agg_windows<false>, grid, block, 0, stream, prog, sel, sel_count, nrows, d_partials);
  g_agg_launches[0]++;
  return hipGetLastError();
}

hipError_t LaunchAggCombine(const AggProgram& prog, const aggmerge::Partial* d_partials, int64_t n_windows, aggmerge::Partial* d_acc,
                            hipStream_t stream, const AggExprTable* exprs) {
  MI_DROP_STALE_ERROR();
  if (n_windows <= 0) return hipSuccess;
  if (!AggProgramIsValid(prog, exprs) || !d_partials || !d_acc) return hipErrorInvalidValue;
  uint32_t ops, classes;
  PackOpsClasses(prog, &ops, &classes);
  hipLaunchKernelGGL(agg_combine, dim3(1), dim3(64), 0, stream, ops, classes, prog.n_aggs, d_partials, n_windows, d_acc);
  g_agg_launches[1]++;
  return hipGetLastError();
}

}  // namespace device
}  // namespace miarrow
