// kernels_run_end.hip -- run-end encoded Arrow arrays -> flat DuckDB vectors of the values' type (MI_K_RUN_END).
//
// A run-end encoded array owns no buffers: child 0 holds the run ends (int16 / int32 / int64, positive, strictly increasing),
// child 1 the values, one per run.  The values child is an ordinary task of the same plan (any flat kind) that decodes into a
// scratch vector; its run-end parent is launched after every other slice (engine.cpp) and expands it here: row p of the
// array takes the value of the first run k with run_ends[k] > offset + p -- the flat vector DuckDB's own Arrow scan makes of
// such a column.
//
// One workgroup per 2048-row tile, like every decode kernel.  Two waves find the runs of the tile's first and last row
// (64-ary search in HBM, one ballot per round), the window of run ends between them goes to LDS (at most 2048 of them: every
// row lies in exactly one run), and every lane finds the runs of its rows there.  A tile inside a single run -- the common
// case for long runs -- broadcasts one value and searches nothing.  Validity words come from a wave ballot.
//
// Damaged run ends (not increasing, or ending before the array does) raise MI_ST_BAD_RUN_ENDS; every search is clamped to
// [0, n_runs), so no read leaves the run ends or the values, whatever the file holds.
#include "device_common.hpp"

namespace miarrow {
namespace device {

namespace {

constexpr int kRunWindow = kTileRows;  // run ends staged per tile

__device__ __forceinline__ int64_t run_end_at(const mi_col_task& t, int rw, int64_t k) {
  if (rw == 8) return GC<int64_t>(t.buf1)[k];
  if (rw == 4) return GC<int32_t>(t.buf1)[k];
  return GC<int16_t>(t.buf1)[k];
}

// First k in [0, n_runs) with run_ends[k] > p, n_runs when there is none.  One whole wave: 64 probes per round, so a batch of
// a million runs takes 4 dependent loads.  Unsorted (damaged) run ends still give an answer inside [0, n_runs].
__device__ int64_t wave_upper_bound(const mi_col_task& t, int rw, int64_t n_runs, int64_t p) {
  const int lane = threadIdx.x & 63;
  int64_t lo = 0, hi = n_runs;  // the answer lies in [lo, hi]
  while (hi - lo > 64) {        // uniform: lo and hi come from ballots
    const int64_t step = (hi - lo + 63) / 64;
    const int64_t k = lo + (lane + 1) * step - 1;  // lane 63 probes at or past hi - 1
    const uint64_t m = __ballot(k >= hi || run_end_at(t, rw, k) > p);
    if (m == 0) return hi;
    const int f = __builtin_ctzll(m);
    const int64_t nhi = lo + (f + 1) * step - 1;
    lo = lo + f * step;  // run_ends[lo + f * step - 1] <= p when f > 0
    hi = nhi < hi ? nhi : hi;
  }
  const int64_t k = lo + lane;
  const uint64_t m = __ballot(k >= hi || run_end_at(t, rw, k) > p);
  return m ? lo + __builtin_ctzll(m) : hi;
}

template <typename V>
__device__ __forceinline__ void copy_value(gptr<const uint8_t> vals, int64_t run, gptr<uint8_t> out, int r) {
  const V v = ((gptr<const V>)vals)[run];
  __builtin_nontemporal_store(v, (gptr<V>)out + r);
}

// Rows of the tile: lane rows r = threadIdx.x + 256 k ascend, so each search starts where the lane's previous one ended.
template <typename V>
__device__ __forceinline__ void expand_tile(const mi_col_task& t, int64_t row0, int n, int64_t first, int cnt, const int64_t* s_ends) {
  gptr<const uint8_t> vals = GC<uint8_t>(t.buf2);
  gptr<uint8_t> out = GM<uint8_t>(t.out_data) + row0 * static_cast<int64_t>(sizeof(V));
  const bool vnull = t.validity != nullptr && t.null_count != 0;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t p0 = t.row_offset + row0;
  int lo = 0;
#pragma clang loop unroll(disable)
  for (int k = 0; k < kTileRows / kBlockThreads; k++) {
    if (k * kBlockThreads >= n) break;  // uniform
    const int r = threadIdx.x + k * kBlockThreads;
    bool ok = true;  // pad rows past the tile: canonical 1
    if (r < n) {
      if (cnt > 1) {
        const int64_t p = p0 + r;
        int hi = cnt - 1;  // no entry above p (damaged run ends): the last run of the window
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (s_ends[mid] > p) hi = mid;
          else lo = mid + 1;
        }
      }
      const int64_t run = first + lo;
      copy_value<V>(vals, run, out, r);
      if (vnull) ok = (GC<uint64_t>(t.validity)[run >> 6] >> (run & 63)) & 1ull;
    }
    if (t.out_validity != nullptr) {
      const int j = wave + (kBlockThreads / 64) * k;  // the wave's 64 rows of this step are word j of the tile
      uint64_t word = __ballot(ok);
      if (t.out_aux != nullptr && 64 * j < n) {
        word &= GC<uint64_t>(t.out_aux)[(row0 >> 6) + j];  // struct parent, same rows
        const int rem = n - 64 * j;
        if (rem < 64) word |= ~0ull << rem;  // canonical pad bits, whatever the parent's are (as tile_valid_word)
      }
      if (lane == 0 && 64 * j < n) GM<uint64_t>(t.out_validity)[(row0 >> 6) + j] = word;
    }
  }
}

__global__ __launch_bounds__(kBlockThreads) void transcode_run_end(const mi_col_task* __restrict__ tasks,
                                                                   const uint32_t* __restrict__ tile_begin,
                                                                   const uint32_t* __restrict__ tile_task, int n_tasks,
                                                                   uint32_t total_tiles, uint32_t* __restrict__ status) {
  __shared__ int64_t s_ends[kRunWindow];
  __shared__ int64_t s_bounds[2];
  for (uint32_t tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
    MI_TILE_PROLOGUE();
    const int rw = static_cast<int>(t.param & 0xFF), w = static_cast<int>((t.param >> 8) & 0xFF);
    const int64_t n_runs = t.param2;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t err = 0;
    // FULL validation: the task's run ends are split evenly over its tiles and every one is compared with its predecessor
    // once (the first with 0: run ends are positive); the last must reach the end of the array
    const int64_t tile_in_task = static_cast<int64_t>(tile - tile_begin[ti]);
    const int64_t ntiles = static_cast<int64_t>(tile_begin[ti + 1] - tile_begin[ti]);
    const int64_t per = (n_runs + ntiles - 1) / ntiles;
    const int64_t c1 = min(n_runs, (tile_in_task + 1) * per);
    for (int64_t k = tile_in_task * per + threadIdx.x; k < c1; k += kBlockThreads) {
      const int64_t e = run_end_at(t, rw, k);
      if (e <= (k > 0 ? run_end_at(t, rw, k - 1) : 0)) err = MI_ST_BAD_RUN_ENDS;
      if (k == n_runs - 1 && e < t.row_offset + t.nrows) err = MI_ST_BAD_RUN_ENDS;
    }
    // the runs of the tile's first and last row
    if (wave < 2) {
      const int64_t f = wave_upper_bound(t, rw, n_runs, t.row_offset + row0 + (wave ? n - 1 : 0));
      if (lane == 0) s_bounds[wave] = f < n_runs ? f : n_runs - 1;
    }
    __syncthreads();
    const int64_t first = s_bounds[0];
    const int64_t last = s_bounds[1] > first ? s_bounds[1] : first;
    const int cnt = static_cast<int>(min<int64_t>(last - first + 1, kRunWindow));
    if (cnt > 1) {
      for (int i = threadIdx.x; i < cnt; i += kBlockThreads) s_ends[i] = run_end_at(t, rw, first + i);
      __syncthreads();
    }
    switch (w) {  // uniform
      case 1: expand_tile<uint8_t>(t, row0, n, first, cnt, s_ends); break;
      case 2: expand_tile<uint16_t>(t, row0, n, first, cnt, s_ends); break;
      case 4: expand_tile<uint32_t>(t, row0, n, first, cnt, s_ends); break;
      case 8: expand_tile<uint64_t>(t, row0, n, first, cnt, s_ends); break;
      default: expand_tile<u32x4>(t, row0, n, first, cnt, s_ends); break;
    }
    raise(status, err);
    __syncthreads();  // s_bounds / s_ends are the next tile's
  }
}

}  // namespace

hipError_t LaunchRunEnd(const mi_col_task* d_tasks, const uint32_t* d_tile_begin, const uint32_t* d_tile_task, int32_t n_tasks,
                        uint32_t total_tiles, uint32_t* d_status, hipStream_t stream) {
  MI_DROP_STALE_ERROR();
  if (total_tiles == 0) return hipSuccess;
  if (d_tile_task == nullptr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(transcode_run_end, dim3(total_tiles), dim3(kBlockThreads), 0, stream, d_tasks, d_tile_begin, d_tile_task,
                     n_tasks, total_tiles, d_status);
  return hipGetLastError();
}

}  // namespace device
}  // namespace miarrow
