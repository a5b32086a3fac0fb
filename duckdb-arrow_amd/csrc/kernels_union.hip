// kernels_union.hip -- Arrow union columns (sparse and dense) -> the vector tree of a DuckDB UNION (MI_K_UNION,
// MI_K_UNION_DENSE; the contracts of both kinds are in mi_arrow_ipc.h, the rule for a row in union_format.hpp).
//
// A union owns type ids (int8 per row) and, when dense, int32 offsets; it has no validity.  The tag pass (transcode_union)
// turns the ids into member indices through the id -> member table of the task, finds every row's validity -- the bit of
// the selected member's Arrow bitmap at the row (sparse) or at the row's offset (dense), ANDed with a struct parent's word --
// and writes the tag vector, the union's validity words and one mask per member: bit r = row r selects this member and is
// not NULL.  The masks are the parent words (out_aux) of the member vectors' own tasks, which are one level deeper and so
// run in a later launch: a sparse member is decoded like a struct child and comes out NULL wherever another member is
// selected.  A dense member decodes into a scratch vector in its own row space and is expanded by offset under its mask
// afterwards (transcode_union_dense), as a run-end array's values are.
//
// One workgroup per 2048-row tile, like every decode kernel; row per lane, 64 consecutive rows per wave step, so a word of a
// validity vector or of a mask is one ballot.  Only the members present in a 64-row group are balloted (the group's rows are
// peeled member by member); the masks of a tile are gathered in LDS (32 members x 32 words = 8 KiB) and leave as coalesced
// words.  All loads of a tile -- ids, offsets, parent words, the table, then the bitmap bytes they name -- are issued before
// its first store.  Both kernels wait for memory more than they move it: a tile reads 2 to 10 KiB.
//
// FULL validation: a type id that is negative or names no member raises MI_ST_BAD_UNION_TAG, a dense offset outside its
// member array MI_ST_BAD_UNION_OFFSET; the row becomes NULL and neither value is ever used as an index.
#include "device_common.hpp"
#include "union_format.hpp"

namespace miarrow {
namespace device {

namespace {

constexpr int kSteps = kTileRows / kBlockThreads;   // rows per lane
constexpr int kTileWords = kTileRows / 64;
constexpr int kWaves = kBlockThreads / 64;
constexpr int kTableMax = unionfmt::kTableWords + unionfmt::kMemberWords * unionfmt::kMaxMembers;
static_assert(kTableMax <= kBlockThreads, "one lane per word of the union table");
static_assert(unionfmt::kMaxMembers == MI_MAX_UNION_MEMBERS && unionfmt::kStBadTag == MI_ST_BAD_UNION_TAG &&
              unionfmt::kStBadOffset == MI_ST_BAD_UNION_OFFSET, "union_format.hpp restates the header");

__global__ __launch_bounds__(kBlockThreads) void transcode_union(const mi_col_task* __restrict__ tasks,
                                                                 const uint32_t* __restrict__ tile_begin,
                                                                 const uint32_t* __restrict__ tile_task, int n_tasks,
                                                                 uint32_t total_tiles, uint32_t* __restrict__ status) {
  __shared__ uint64_t s_table[kTableMax];
  __shared__ uint64_t s_mask[unionfmt::kMaxMembers * kTileWords];
  for (uint32_t tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
    MI_TILE_PROLOGUE();
    int m = static_cast<int>(t.param);
    m = m < 1 ? 1 : m > unionfmt::kMaxMembers ? unionfmt::kMaxMembers : m;
    const bool dense = t.ptr_base != 0;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int nwords = (n + 63) >> 6;
    // ---- first round of loads: the table, the rows' ids and offsets, the parent's words
    const int ntab = unionfmt::kTableWords + unionfmt::kMemberWords * m;
    uint64_t tab = 0;
    if (static_cast<int>(threadIdx.x) < ntab) tab = GC<uint64_t>(t.buf2)[threadIdx.x];
    gptr<const int8_t> ids = GC<int8_t>(t.buf1) + (t.row_offset + row0);
    gptr<const int32_t> offs = GC<int32_t>(reinterpret_cast<const void*>(static_cast<uintptr_t>(t.ptr_base))) + (t.row_offset + row0);
    int8_t id[kSteps];
    int32_t off[kSteps];
    uint64_t pw[kSteps];
#pragma unroll
    for (int k = 0; k < kSteps; k++) {
      const int r = threadIdx.x + k * kBlockThreads;
      const int j = wave + kWaves * k;
      id[k] = -1;
      off[k] = 0;
      pw[k] = ~0ull;
      if (r < n) {
        id[k] = __builtin_nontemporal_load(ids + r);
        if (dense) off[k] = __builtin_nontemporal_load(offs + r);
      }
      if (t.out_aux != nullptr && j < nwords) pw[k] = GC<uint64_t>(t.out_aux)[(row0 >> 6) + j];  // struct parent, same rows
    }
    if (static_cast<int>(threadIdx.x) < ntab) s_table[threadIdx.x] = tab;
    // every mask word of the tile starts as its pad bits
    for (int i = threadIdx.x; i < m * kTileWords; i += kBlockThreads) {
      const int rem = n - 64 * (i & (kTileWords - 1));
      s_mask[i] = (rem > 0 && rem < 64) ? ~0ull << rem : 0ull;
    }
    __syncthreads();
    // ---- the member of every row (checked before it indexes anything) and where its validity bit lies
    const int8_t* map = reinterpret_cast<const int8_t*>(s_table);
    int8_t tg[kSteps];
    int64_t bit[kSteps];
    uint64_t bitmap[kSteps];
    uint32_t err = 0;
#pragma unroll
    for (int k = 0; k < kSteps; k++) {
      const int r = threadIdx.x + k * kBlockThreads;
      tg[k] = -1;
      bit[k] = 0;
      bitmap[k] = 0;
      if (r < n) {
        const int mem = unionfmt::MemberOfId(map, id[k]);
        if (mem < 0 || mem >= m) {
          err |= MI_ST_BAD_UNION_TAG;
        } else {
          const uint64_t* rec = s_table + unionfmt::kTableWords + unionfmt::kMemberWords * mem;
          const int64_t len = static_cast<int64_t>(rec[1]);
          if (dense && (off[k] < 0 || static_cast<int64_t>(off[k]) >= len)) {
            err |= MI_ST_BAD_UNION_OFFSET;
          } else if (!(rec[3] & unionfmt::kMemberNullType)) {
            tg[k] = static_cast<int8_t>(mem);
            if (rec[0] != 0 && rec[2] != 0) {
              bitmap[k] = rec[0];
              bit[k] = dense ? static_cast<int64_t>(off[k]) : t.row_offset + row0 + r;
            }
          }
        }
      }
    }
    // ---- second round of loads: the bitmap bytes
    uint8_t vb[kSteps];
#pragma unroll
    for (int k = 0; k < kSteps; k++) {
      vb[k] = 0xFF;
      if (bitmap[k] != 0) vb[k] = GC<uint8_t>(reinterpret_cast<const void*>(static_cast<uintptr_t>(bitmap[k])))[bit[k] >> 3];
    }
    // ---- tags, the union's words, the masks
    gptr<uint8_t> tags = GM<uint8_t>(t.out_data) + row0;
#pragma unroll
    for (int k = 0; k < kSteps; k++) {
      const int r = threadIdx.x + k * kBlockThreads;
      const int j = wave + kWaves * k;
      if (j >= nwords) continue;  // uniform
      const bool sel = r < n && tg[k] >= 0 && ((vb[k] >> (bit[k] & 7)) & 1) && ((pw[k] >> lane) & 1ull);
      if (r < n) __builtin_nontemporal_store(static_cast<uint8_t>(sel ? tg[k] : 0), tags + r);
      const uint64_t word = __ballot(sel || r >= n);  // pad bits ones
      if (t.out_validity != nullptr && lane == 0) GM<uint64_t>(t.out_validity)[(row0 >> 6) + j] = word;
      uint64_t todo = __ballot(sel);
      while (todo) {  // uniform: one round per member present among the 64 rows
        const int first = __builtin_amdgcn_readfirstlane(__builtin_ctzll(todo));
        const int mem = __builtin_amdgcn_readlane(static_cast<int>(tg[k]), first);
        const uint64_t mk = __ballot(sel && tg[k] == mem);
        if (lane == 0) s_mask[mem * kTileWords + j] |= mk;  // word j of the tile is this wave's alone
        todo &= ~mk;
      }
    }
    __syncthreads();
    gptr<uint8_t> masks = GM<uint8_t>(t.out_data) + t.param2;
    for (int i = threadIdx.x; i < m * nwords; i += kBlockThreads) {
      const int mem = i / nwords, j = i - mem * nwords;
      ((gptr<uint64_t>)(masks + mem * t.buf2_len))[(row0 >> 6) + j] = s_mask[mem * kTileWords + j];
    }
    raise(status, err);
    __syncthreads();  // s_table / s_mask are the next tile's
  }
}

template <typename V>
__device__ __forceinline__ V zero_value() {
  V z;
  __builtin_memset(&z, 0, sizeof(V));
  return z;
}

// Rows of the tile whose mask bit is set take value and validity bit of scratch row offsets[r]; all others are zero and NULL.
template <typename V>
__device__ __forceinline__ void expand_member(const mi_col_task& t, int64_t row0, int n, uint32_t* status) {
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int nwords = (n + 63) >> 6;
  gptr<const int32_t> offs = GC<int32_t>(t.buf1) + (t.row_offset + row0);
  gptr<const V> vals = GC<V>(t.buf2);
  gptr<V> out = GM<V>(t.out_data) + row0;
  const bool vnull = t.validity != nullptr && t.null_count != 0;
  int32_t off[kSteps];
  uint64_t mw[kSteps];
#pragma unroll
  for (int k = 0; k < kSteps; k++) {
    const int r = threadIdx.x + k * kBlockThreads;
    const int j = wave + kWaves * k;
    off[k] = r < n ? __builtin_nontemporal_load(offs + r) : 0;
    mw[k] = j < nwords ? GC<uint64_t>(t.out_aux)[(row0 >> 6) + j] : 0ull;
  }
  V v[kSteps];
  uint64_t vw[kSteps];
  uint32_t selbits = 0, err = 0;
#pragma unroll
  for (int k = 0; k < kSteps; k++) {
    const int r = threadIdx.x + k * kBlockThreads;
    v[k] = zero_value<V>();
    vw[k] = ~0ull;
    if (r < n && ((mw[k] >> lane) & 1ull)) {
      if (off[k] < 0 || static_cast<int64_t>(off[k]) >= t.buf2_len) {
        err = MI_ST_BAD_UNION_OFFSET;
      } else {
        selbits |= 1u << k;
        v[k] = vals[off[k]];
        if (vnull) vw[k] = GC<uint64_t>(t.validity)[off[k] >> 6];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kSteps; k++) {
    const int r = threadIdx.x + k * kBlockThreads;
    const int j = wave + kWaves * k;
    if (j >= nwords) continue;  // uniform
    const bool ok = ((selbits >> k) & 1u) && ((vw[k] >> (off[k] & 63)) & 1ull);
    if (r < n) __builtin_nontemporal_store(ok ? v[k] : zero_value<V>(), out + r);
    const uint64_t word = __ballot(ok || r >= n);  // pad bits ones
    if (t.out_validity != nullptr && lane == 0) GM<uint64_t>(t.out_validity)[(row0 >> 6) + j] = word;
  }
  raise(status, err);
}

__global__ __launch_bounds__(kBlockThreads) void transcode_union_dense(const mi_col_task* __restrict__ tasks,
                                                                       const uint32_t* __restrict__ tile_begin,
                                                                       const uint32_t* __restrict__ tile_task, int n_tasks,
                                                                       uint32_t total_tiles, uint32_t* __restrict__ status) {
  for (uint32_t tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
    MI_TILE_PROLOGUE();
    switch (static_cast<int>(t.param)) {  // uniform
      case 1: expand_member<uint8_t>(t, row0, n, status); break;
      case 2: expand_member<uint16_t>(t, row0, n, status); break;
      case 4: expand_member<uint32_t>(t, row0, n, status); break;
      case 8: expand_member<uint64_t>(t, row0, n, status); break;
      default: expand_member<u32x4>(t, row0, n, status); break;
    }
  }
}

}  // namespace

hipError_t LaunchUnion(bool dense, const mi_col_task* d_tasks, const uint32_t* d_tile_begin, const uint32_t* d_tile_task, int32_t n_tasks,
                       uint32_t total_tiles, uint32_t* d_status, hipStream_t stream) {
  MI_DROP_STALE_ERROR();
  if (total_tiles == 0) return hipSuccess;
  if (d_tile_task == nullptr) return hipErrorInvalidValue;
  if (dense)
    hipLaunchKernelGGL(transcode_union_dense, dim3(total_tiles), dim3(kBlockThreads), 0, stream, d_tasks, d_tile_begin, d_tile_task, n_tasks,
                       total_tiles, d_status);
  else
    hipLaunchKernelGGL(transcode_union, dim3(total_tiles), dim3(kBlockThreads), 0, stream, d_tasks, d_tile_begin, d_tile_task, n_tasks,
                       total_tiles, d_status);
  return hipGetLastError();
}

}  // namespace device
}  // namespace miarrow
