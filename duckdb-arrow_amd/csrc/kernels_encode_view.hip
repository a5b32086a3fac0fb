// kernels_encode_view.hip -- K7e: string_t vectors -> Arrow string views (Utf8View, produce_arrow_string_view), DuckDB's
// ArrowVarcharToStringViewData restated: one validity bitmap, 16 bytes of view per row and ONE data buffer that holds the
// strings of more than 12 bytes of the valid rows back to back, in row order.
#include "device_common.hpp"
#include "encode_common.hpp"

namespace miarrow {
namespace device {

namespace {

// Task fields (MI_K_ENC_STRVIEW): validity = DuckDB validity words (NULL = all valid), buf1 = string_t rows, buf2 = string
// heap (long rows point at ptr - ptr_base in it), out_validity = bitmap, out_data = views, out_aux = data buffer,
// param2 = index of the task's NULL counter.
//
// A string_t and an Arrow view are the same 16 bytes for a valid row of <= 12 bytes but for the padding, which the view
// must have zero; a longer row keeps its length and its 4 prefix bytes and trades the pointer for {buffer 0, int32 offset};
// a NULL row is 16 zero bytes.  So the tile (2048 rows, 8 per thread, all 8 coalesced 16-byte loads in flight before the
// validity words are asked for) is a masked copy, and only rows of more than 12 bytes need to know where the tile's bytes
// begin in the data buffer: the sum of the long lengths of every tile before it in the column.
//
// That sum comes from encode_string_1p's decoupled look-back (tile = workgroup id; tile_state[tile] bits 62..63 = 0 nothing
// yet, 1 = sum of this tile, 2 = sum of every tile of the column up to and including this one; RELAXED agent-scope atomics
// whose value is the whole message; a bounded spin that ends in MI_ST_INTERNAL).  The difference: a tile WITHOUT long rows
// publishes its sum of 0 and never looks back -- its views need no base -- so a column of flags or ship modes is not
// serialised by the walk at all, and a tile behind it walks through its zero.  Such a tile never learns its inclusive
// prefix; the int32 limit is therefore checked by every tile that has long rows, on its own end: the last of them in the
// column sees the size of the data buffer.  The price: a zero tile's word stays a sum, so a tile with long rows behind k zero
// tiles walks k / kViewLookBack steps on wave 0 while its other waves wait -- O(tiles of the column) per such tile at worst.
// Record batches of the writer have about 60 tiles (15 steps); a caller of the task API with far longer columns of mostly
// inline strings pays that walk per tile that has long rows.
//
// Long payload, positions in 64 bits throughout (a single string may be anything a uint32 length can say):
//   * the tile's long strings lie in the heap back to back in row order (every long row at the same distance from its
//     place in the data buffer: DuckDB's own heaps, the staged heap of the host path): the heap range IS the tile's part
//     of the data buffer, copied by the whole workgroup as one coalesced stream;
//   * anything else (vectors decoded from Arrow buffers, where the inline strings lie in between; shuffled or shared
//     pointers): every long row brings its own bytes in unaligned 16-byte pieces -- rows below kViewWaveCopy bytes by their
//     own lane, longer ones by their whole wave, one after the other.
// No workgroup reads bytes another workgroup wrote, and every piece lies inside [string, string + length) on the source
// side and inside the row's own part of the data buffer on the other: the last piece of a copy ends where the string
// ends and overlaps the one before it (the same bytes twice).
constexpr uint64_t kViewStateMask = (1ull << 62) - 1ull;
constexpr int kViewLookBack = 4;         // predecessors inspected per look-back step
constexpr uint32_t kViewWaveCopy = 256;  // long rows of at least this many bytes are copied by their wave, 16 bytes per lane
constexpr int kViewRowsPerThread = kTileRows / kBlockThreads;

typedef u32x2 u32x2_v1 __attribute__((aligned(1)));

// `len` bytes src -> dst, both at any byte alignment, by `nthreads` lanes of which this one is `id`: pieces of 16 bytes, the
// first at 0, the following at dst's 16-byte boundaries, the last one ending at `len`.  Never touches a byte outside
// [src, src + len) or [dst, dst + len).
__device__ __forceinline__ void view_copy_stream(gptr<uint8_t> dst, gptr<const uint8_t> src, uint64_t len, uint32_t id, uint32_t nthreads) {
  if (len < 16) {
    if (id < len) dst[id] = src[id];
    return;
  }
  const uint64_t last = len - 16;
  const uint64_t head = (16u - (static_cast<uint32_t>(reinterpret_cast<uintptr_t>(dst)) & 15u)) & 15u;
  if (id == 0) *(gptr<u32x4_a1>)dst = __builtin_nontemporal_load((gptr<const u32x4_a1>)src);
#pragma clang loop unroll(disable)
  for (uint64_t o = head + 16ull * id; o < len; o += 16ull * nthreads) {
    const uint64_t at = o < last ? o : last;
    *(gptr<u32x4_a1>)(dst + at) = __builtin_nontemporal_load((gptr<const u32x4_a1>)(src + at));
  }
}

// one row of 13 .. kViewWaveCopy - 1 bytes, by its own lane
__device__ __forceinline__ void view_copy_row(gptr<uint8_t> dst, gptr<const uint8_t> src, uint32_t len) {
  if (len < 16) {  // 13..15: two overlapping 8-byte pieces
    const u32x2 a = *(gptr<const u32x2_v1>)src, e = *(gptr<const u32x2_v1>)(src + (len - 8));
    *(gptr<u32x2_v1>)dst = a;
    *(gptr<u32x2_v1>)(dst + (len - 8)) = e;
    return;
  }
  const uint32_t last = len - 16;
#pragma clang loop unroll(disable)
  for (uint32_t o = 0; o < len; o += 16) {
    const uint32_t at = o < last ? o : last;
    *(gptr<u32x4_a1>)(dst + at) = __builtin_nontemporal_load((gptr<const u32x4_a1>)(src + at));
  }
}

__device__ __forceinline__ uint64_t wave_inclusive_scan_u64(uint64_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t up = __shfl_up(static_cast<unsigned long long>(v), d, 64);
    if (lane >= d) v += up;
  }
  return v;
}

__global__ __launch_bounds__(kBlockThreads) void encode_string_view(const mi_col_task* __restrict__ tasks,
                                                                    const uint32_t* __restrict__ tile_begin,
                                                                    const uint32_t* __restrict__ tile_task, int n_tasks,
                                                                    uint32_t total_tiles, unsigned long long* __restrict__ tile_state,
                                                                    int64_t* __restrict__ null_counts, uint32_t* __restrict__ status) {
  constexpr int kWaves = kBlockThreads / 64;
  constexpr int kGroups = kTileRows / 64;              // 64-row groups of the tile: group g = k * kWaves + wave
  __shared__ uint64_t s_valid[kTileRows / 64];
  __shared__ uint64_t s_gbase[kGroups + 1];             // long bytes of every group, then their exclusive prefix (+ the tile total)
  __shared__ int64_t s_prefix;
  __shared__ uint64_t s_delta[kWaves];
  __shared__ uint32_t s_dflag[kWaves];                  // bit 0: the wave has long rows, bit 1: they are not at one distance
  (void)n_tasks;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t tile = blockIdx.x;
  if (tile >= total_tiles) return;
  MI_TILE_PROLOGUE();
  // ---- the tile's rows, all in flight before the validity words are asked for (a NULL row is read and then ignored)
  gptr<const u32x4> str = GC<u32x4>(t.buf1) + row0;
  u32x4 s[kViewRowsPerThread];
#pragma unroll
  for (int k = 0; k < kViewRowsPerThread; k++) {
    const int r = static_cast<int>(threadIdx.x) + k * kBlockThreads;
    s[k] = __builtin_nontemporal_load(str + (r < n ? r : n - 1));
  }
  enc_tile_validity(t, row0, n, null_counts, s_valid);
  __syncthreads();  // s_valid
  // ---- views but for the offsets, and the long bytes of every 64-row group (64 bits: lengths are uint32)
  uint64_t exw[kViewRowsPerThread];  // long bytes in front of the row inside its group
  uint32_t long_rows = 0;            // bit k: row k of this thread is valid and longer than 12 bytes
#pragma unroll
  for (int k = 0; k < kViewRowsPerThread; k++) {
    const int r = static_cast<int>(threadIdx.x) + k * kBlockThreads;
    const bool ok = r < n && ((s_valid[r >> 6] >> (r & 63)) & 1);
    const uint32_t len = s[k].x;
    const bool is_long = ok && len > 12;
    if (!ok) {
      s[k] = u32x4{0u, 0u, 0u, 0u};
    } else if (!is_long) {  // the bytes behind the string are zero whatever the source slot holds there
      const uint32_t k0 = len >= 4 ? 4 : len, k1 = len >= 8 ? 4 : (len > 4 ? len - 4 : 0), k2 = len > 8 ? len - 8 : 0;
      s[k].y = k0 == 4 ? s[k].y : (s[k].y & ((1u << (8 * k0)) - 1u));
      s[k].z = k1 == 4 ? s[k].z : (s[k].z & ((1u << (8 * k1)) - 1u));
      s[k].w = k2 == 4 ? s[k].w : (s[k].w & ((1u << (8 * k2)) - 1u));
    }
    exw[k] = 0;
    uint64_t group = 0;
    if (__ballot(is_long) != 0) {  // wave-uniform
      const uint64_t c = is_long ? len : 0u;
      const uint64_t incl = wave_inclusive_scan_u64(c, lane);
      exw[k] = incl - c;
      group = incl;
    }
    if (lane == 63) s_gbase[k * kWaves + wave] = group;
    long_rows |= is_long ? (1u << k) : 0u;
  }
  __syncthreads();
  // ---- wave 0: the groups' exclusive prefix, the tile's sum, and (only with long rows) the look-back
  const uint32_t first_tile = tile_begin[ti];
  if (wave == 0) {
    const uint64_t v = lane < kGroups ? s_gbase[lane] : 0ull;
    const uint64_t inc = wave_inclusive_scan_u64(v, lane);
    const uint64_t tile_total = __shfl(static_cast<unsigned long long>(inc), kGroups - 1, 64);
    if (lane < kGroups) s_gbase[lane] = inc - v;
    if (lane == kGroups - 1) s_gbase[kGroups] = inc;
    if (lane == 0) {
      const unsigned long long mine = (tile == first_tile ? (2ull << 62) : (1ull << 62)) | (tile_total & kViewStateMask);
      __hip_atomic_store(&tile_state[tile], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tile_total != 0) {  // uniform
      int64_t prefix = 0;
      int64_t hi = static_cast<int64_t>(tile) - 1;  // nearest predecessor not yet accounted for
      while (hi >= static_cast<int64_t>(first_tile)) {
        const int64_t j = hi - lane;
        unsigned long long st = 2ull << 62;             // lanes past the column's first tile: a finished, empty prefix
        if (lane >= kViewLookBack) st = 1ull << 62;     // lanes outside the step: an empty sum that ends nothing
        else if (j >= static_cast<int64_t>(first_tile)) {
          st = __hip_atomic_load(&tile_state[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          // a predecessor is dispatched before this tile and publishes after one load and one scan, without waiting for
          // anybody when it has no long rows; the bound only keeps a logic error from hanging the device
          for (int spins = 0; (st >> 62) == 0; spins++) {
            if (spins > (1 << 22)) {
              atomicOr(status, MI_ST_INTERNAL);
              st = 2ull << 62;
              break;
            }
            __builtin_amdgcn_s_sleep(2);
            st = __hip_atomic_load(&tile_state[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
        const uint64_t done_mask = __ballot((st >> 62) == 2ull);
        const int stop = done_mask ? __builtin_ctzll(done_mask) : 64;
        int64_t v2 = lane <= stop ? static_cast<int64_t>(st & kViewStateMask) : 0;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v2 += __shfl_down(v2, d, 64);
        prefix += __shfl(v2, 0, 64);
        if (done_mask) break;
        hi -= kViewLookBack;
      }
      if (lane == 0) {
        if (tile != first_tile)
          __hip_atomic_store(&tile_state[tile], (2ull << 62) | (static_cast<unsigned long long>(prefix + static_cast<int64_t>(tile_total)) & kViewStateMask),
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_prefix = prefix;
        // view offsets are int32 and there is no large variant
        if (prefix + static_cast<int64_t>(tile_total) > 0x7FFFFFFFll) atomicOr(status, MI_ST_OFFSET_OVERFLOW);
      }
    }
  }
  __syncthreads();
  const uint64_t tile_total = s_gbase[kGroups];
  gptr<u32x4> views = GM<u32x4>(t.out_data) + row0;
  if (tile_total == 0) {  // uniform: no row needs a base
#pragma unroll
    for (int k = 0; k < kViewRowsPerThread; k++) {
      const int r = static_cast<int>(threadIdx.x) + k * kBlockThreads;
      if (r < n) __builtin_nontemporal_store(s[k], views + r);
    }
    return;
  }
  const uint64_t base = static_cast<uint64_t>(s_prefix);
  gptr<const uint8_t> heap = GC<uint8_t>(t.buf2);
  gptr<uint8_t> data = GM<uint8_t>(t.out_aux);
  // ---- the views; and: is every long row of the tile at one distance from its place in the tile's bytes?
  uint64_t my_delta = 0;
  bool my_same = true;
#pragma unroll
  for (int k = 0; k < kViewRowsPerThread; k++) {
    const int r = static_cast<int>(threadIdx.x) + k * kBlockThreads;
    if ((long_rows >> k) & 1u) {
      exw[k] += s_gbase[k * kWaves + wave];  // now: long bytes in front of the row inside the tile
      const uint64_t off = (static_cast<uint64_t>(s[k].z) | (static_cast<uint64_t>(s[k].w) << 32)) - t.ptr_base;
      const uint64_t delta = off - exw[k];
      if ((long_rows & ((1u << k) - 1u)) == 0) my_delta = delta;
      else if (delta != my_delta) my_same = false;
      u32x4 v = s[k];
      v.z = 0u;
      v.w = static_cast<uint32_t>(base + exw[k]);
      __builtin_nontemporal_store(v, views + r);
    } else if (r < n) {
      __builtin_nontemporal_store(s[k], views + r);
    }
  }
  {
    const uint64_t has = __ballot(long_rows != 0);
    if (has != 0) {  // wave-uniform
      const int fl = __builtin_ctzll(has);
      const uint64_t d0 = __shfl(static_cast<unsigned long long>(my_delta), fl, 64);
      const bool bad = __ballot(long_rows != 0 && (!my_same || my_delta != d0)) != 0;
      if (lane == 0) {
        s_delta[wave] = d0;
        s_dflag[wave] = 1u | (bad ? 2u : 0u);
      }
    } else if (lane == 0) {
      s_delta[wave] = 0;
      s_dflag[wave] = 0u;
    }
  }
  __syncthreads();
  bool contig = true;  // uniform
  uint64_t delta0 = 0;
  {
    bool have = false;
#pragma unroll
    for (int w = 0; w < kWaves; w++) {
      const uint32_t f = s_dflag[w];
      if (!(f & 1u)) continue;
      if (f & 2u) contig = false;
      if (!have) { delta0 = s_delta[w]; have = true; }
      else if (s_delta[w] != delta0) contig = false;
    }
  }
  if (contig) {  // the heap range is the tile's part of the data buffer
    view_copy_stream(data + base, heap + delta0, tile_total, threadIdx.x, kBlockThreads);
    return;
  }
#pragma unroll  // s[] and exw[] stay in registers
  for (int k = 0; k < kViewRowsPerThread; k++) {
    const bool is_long = (long_rows >> k) & 1u;
    const uint32_t len = is_long ? s[k].x : 0u;
    const uint64_t off = (static_cast<uint64_t>(s[k].z) | (static_cast<uint64_t>(s[k].w) << 32)) - t.ptr_base;
    const uint64_t at = base + exw[k];
    if (len != 0 && len < kViewWaveCopy) view_copy_row(data + at, heap + off, len);
    uint64_t todo = __ballot(len >= kViewWaveCopy);
    while (todo != 0) {  // wave-uniform
      const int l = __builtin_ctzll(todo);
      todo &= todo - 1;
      const uint64_t o = __shfl(static_cast<unsigned long long>(off), l, 64), a = __shfl(static_cast<unsigned long long>(at), l, 64);
      const uint32_t ln = __shfl(len, l, 64);
      view_copy_stream(data + a, heap + o, ln, lane, 64);
    }
  }
}

}  // namespace

// d_tile_state: total_tiles look-back words, zeroed here
hipError_t LaunchEncodeStringView(const mi_col_task* d_tasks, const uint32_t* d_tile_begin, const uint32_t* d_tile_task, int32_t n_tasks,
                                  uint32_t total_tiles, int64_t* d_tile_state, int64_t* d_null_counts, uint32_t* d_status, hipStream_t stream) {
  MI_DROP_STALE_ERROR();
  if (total_tiles == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(d_tile_state, 0, static_cast<size_t>(total_tiles) * sizeof(int64_t), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(encode_string_view, dim3(total_tiles), dim3(kBlockThreads), 0, stream, d_tasks, d_tile_begin, d_tile_task, n_tasks,
                     total_tiles, reinterpret_cast<unsigned long long*>(d_tile_state), d_null_counts, d_status);
  return hipGetLastError();
}

}  // namespace device
}  // namespace miarrow
