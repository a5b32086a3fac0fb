// encode_common.hpp -- device helpers the K7 encode kernels share (kernels_encode.hip, kernels_encode_view.hip): the always-present
// Arrow validity bitmap and the NULL count of one tile.
#pragma once

#include "device_common.hpp"

namespace miarrow {
namespace device {
namespace {

// K7a: DuckDB validity words have Arrow's bit order and polarity, so the bitmap is a byte copy of the words with
// the pad bits of the last byte forced to 1 (ResizeValidity fills with 0xFF) and NULLs counted on the way.
// In two halves, so that a kernel can put its own loads between the request for the validity word and its use.
struct EncValidity {
  uint64_t w;
  bool active;
};
__device__ __forceinline__ EncValidity enc_tile_validity_load(const mi_col_task& t, int64_t row0, int n, const uint64_t* s_valid = nullptr) {
  EncValidity v{~0ull, false};
  if (threadIdx.x >= 64 || (t.out_validity == nullptr && s_valid == nullptr)) return v;  // wave 0, uniform
  const int lane = threadIdx.x;
  v.active = lane < ((n + 63) >> 6);
  if (v.active && t.validity != nullptr) v.w = GC<uint64_t>(t.validity)[(row0 >> 6) + lane];
  return v;
}
__device__ __forceinline__ void enc_tile_validity_finish(const mi_col_task& t, int64_t row0, int n, int64_t* null_counts, EncValidity v,
                                                         uint64_t* s_valid = nullptr) {
  if (threadIdx.x >= 64 || (t.out_validity == nullptr && s_valid == nullptr)) return;  // wave 0, uniform
  const int lane = threadIdx.x;
  const bool active = v.active;
  uint64_t w = v.w;
  const int rem = n - 64 * lane;
  if (active) {
    if (rem < 64) w |= ~0ull << rem;
    if (s_valid) s_valid[lane] = w;
  }
  if (t.out_validity == nullptr) return;
  // one counter update per tile: the counter of a column is ONE address for all of its tiles
  int nulls = active ? 64 - __builtin_popcountll(w) : 0;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) nulls += __shfl_down(nulls, d, 64);
  if (lane == 0 && nulls) atomicAdd(reinterpret_cast<unsigned long long*>(null_counts + t.param2), static_cast<unsigned long long>(nulls));
  if (!active) return;
  gptr<uint8_t> out = GM<uint8_t>(t.out_validity) + (row0 >> 3) + 8 * lane;
  const int nbytes = rem >= 64 ? 8 : (rem + 7) >> 3;
  if (nbytes == 8 && (reinterpret_cast<uintptr_t>(out) & 7) == 0) {
    *(gptr<uint64_t>)out = w;
  } else {
    for (int k = 0; k < nbytes; k++) out[k] = static_cast<uint8_t>(w >> (8 * k));
  }
}
__device__ __forceinline__ void enc_tile_validity(const mi_col_task& t, int64_t row0, int n, int64_t* null_counts,
                                                  uint64_t* s_valid = nullptr) {
  enc_tile_validity_finish(t, row0, n, null_counts, enc_tile_validity_load(t, row0, n, s_valid), s_valid);
}

__device__ __forceinline__ bool enc_row_valid(gptr<const uint64_t> v, bool has, int64_t row) {
  return !has || ((v[row >> 6] >> (row & 63)) & 1);
}

}  // namespace
}  // namespace device
}  // namespace miarrow
