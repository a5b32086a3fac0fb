// kernels_encode_union.hip -- K7g: the union's own pass of a DuckDB UNION vector on its way to an Arrow sparse union
// (MI_K_ENC_UNION; the contract is in mi_arrow_ipc.h, the rule for a row in union_format.hpp: EncodeRow).  The inverse of
// transcode_union's tag pass (kernels_union.hip) and the same shape of kernel.
//
// An Arrow union has type ids and no bitmap: a NULL row is a NULL of the member its type id names.  So the pass writes the
// int8 type id of every row -- the tag, 0 for a NULL union row -- and one EFFECTIVE validity mask per member: bit r = the union
// row is valid (and its struct parent's) AND tag[r] names the member AND the member's own validity bit r is set.  The masks are
// the `validity` of the members' ordinary encode tasks: a fixed-width member marks every row it does not own NULL, a string or
// list member repeats its offset there, and every member's NULL count comes out of the usual bitmap pass.  This kernel is
// launched ahead of every other encode kernel of its plan (LaunchEncodeFixed), on the same stream: no workgroup waits for
// another.
//
// One workgroup per 2048-row tile; row per lane, 64 consecutive rows per wave step, so a word of a mask is one ballot.  Only
// the members present in a 64-row group are balloted (the group's rows are peeled member by member); the masks of a tile are
// gathered in LDS (32 members x 32 words = 8 KiB) and leave as coalesced words.  A tile reads 2 KiB of tags and at most
// (m + 2) x 256 bytes of words: the kernel waits for memory more than it moves it.
//
// A tag >= m under a valid row raises MI_ST_BAD_UNION_TAG; the row takes type id 0 and is NULL in every mask.  The member
// index that addresses LDS and the table is EncodeRow's, which lies in 0 .. m - 1 whatever was loaded.
#include "device_common.hpp"
#include "union_format.hpp"

namespace miarrow {
namespace device {

namespace {

constexpr int kSteps = kTileRows / kBlockThreads;   // rows per lane
constexpr int kTileWords = kTileRows / 64;
constexpr int kWaves = kBlockThreads / 64;
static_assert(unionfmt::kMaxMembers == MI_MAX_UNION_MEMBERS && unionfmt::kStBadTag == MI_ST_BAD_UNION_TAG, "union_format.hpp restates the header");
static_assert(unionfmt::kMaxMembers <= kBlockThreads, "one lane per member address");

__global__ __launch_bounds__(kBlockThreads) void encode_union(const mi_col_task* __restrict__ tasks, const uint32_t* __restrict__ tile_begin,
                                                              const uint32_t* __restrict__ tile_task, int n_tasks, uint32_t total_tiles,
                                                              uint32_t* __restrict__ status) {
  __shared__ uint64_t s_member[unionfmt::kMaxMembers];              // device address of every member's validity words, 0 = all valid
  __shared__ uint64_t s_mask[unionfmt::kMaxMembers * kTileWords];
  for (uint32_t tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
    MI_TILE_PROLOGUE();
    if (t.kind != MI_K_ENC_UNION) continue;  // uniform: a tile of encode_fixed or encode_uuid_text
    int m = static_cast<int>(t.param);
    m = m < 1 ? 1 : m > unionfmt::kMaxMembers ? unionfmt::kMaxMembers : m;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int nwords = (n + 63) >> 6;
    const int64_t word0 = row0 >> 6;
    // ---- the loads of the tile that need no other: member addresses, tags, the union's and the parent's words
    uint64_t maddr = 0;
    if (static_cast<int>(threadIdx.x) < m) maddr = GC<uint64_t>(t.buf2)[threadIdx.x];
    gptr<const uint8_t> tags = GC<uint8_t>(t.buf1) + row0;
    gptr<const uint64_t> parent = GC<uint64_t>(reinterpret_cast<const void*>(static_cast<uintptr_t>(t.ptr_base)));
    uint8_t tg[kSteps];
    uint64_t uw[kSteps];
#pragma unroll
    for (int k = 0; k < kSteps; k++) {
      const int r = threadIdx.x + k * kBlockThreads;
      const int j = wave + kWaves * k;
      tg[k] = 0;
      uw[k] = ~0ull;
      if (r < n) tg[k] = __builtin_nontemporal_load(tags + r);
      if (j < nwords) {
        if (t.validity != nullptr) uw[k] = GC<uint64_t>(t.validity)[word0 + j];
        if (t.ptr_base != 0) uw[k] &= parent[word0 + j];
      }
    }
    if (static_cast<int>(threadIdx.x) < m) s_member[threadIdx.x] = maddr;
    // every mask word of the tile starts as its pad bits
    for (int i = threadIdx.x; i < m * kTileWords; i += kBlockThreads) s_mask[i] = unionfmt::WithPadBits(0ull, n, i & (kTileWords - 1));
    __syncthreads();
    // ---- type ids, and the masks member by member
    gptr<int8_t> ids = GM<int8_t>(t.out_data) + row0;
    uint32_t err = 0;
#pragma unroll
    for (int k = 0; k < kSteps; k++) {
      const int r = threadIdx.x + k * kBlockThreads;
      const int j = wave + kWaves * k;
      if (j >= nwords) continue;  // uniform
      unionfmt::EncodedRow row{0, 0, false, 0u};
      if (r < n) {
        row = unionfmt::EncodeRow(static_cast<int>(tg[k]), m, ((uw[k] >> lane) & 1ull) != 0);
        err |= row.status;
        __builtin_nontemporal_store(static_cast<int8_t>(row.type_id), ids + r);
      }
      uint64_t todo = __ballot(row.selects);
      while (todo) {  // uniform: one round per member present among the 64 rows
        const int first = __builtin_amdgcn_readfirstlane(__builtin_ctzll(todo));
        const int mem = __builtin_amdgcn_readlane(row.member, first);   // 0 .. m - 1: EncodeRow clamps
        const uint64_t mk = __ballot(row.selects && row.member == mem);
        const uint64_t own = s_member[mem];
        uint64_t vw = ~0ull;
        if (own != 0) vw = GC<uint64_t>(reinterpret_cast<const void*>(static_cast<uintptr_t>(own)))[word0 + j];
        if (lane == 0) s_mask[mem * kTileWords + j] |= mk & vw;  // word j of the tile is this wave's alone
        todo &= ~mk;
      }
    }
    __syncthreads();
    gptr<uint8_t> masks = GM<uint8_t>(t.out_aux);
    for (int i = threadIdx.x; i < m * nwords; i += kBlockThreads) {
      const int mem = i / nwords, j = i - mem * nwords;
      ((gptr<uint64_t>)(masks + mem * t.buf2_len))[word0 + j] = s_mask[mem * kTileWords + j];
    }
    raise(status, err);
    __syncthreads();  // s_member / s_mask are the next tile's
  }
}

}  // namespace

hipError_t LaunchEncodeUnion(const mi_col_task* d_tasks, const uint32_t* d_tile_begin, const uint32_t* d_tile_task, int32_t n_tasks,
                             uint32_t total_tiles, uint32_t* d_status, hipStream_t stream) {
  MI_DROP_STALE_ERROR();
  if (total_tiles == 0) return hipSuccess;
  if (d_tile_task == nullptr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(encode_union, dim3(total_tiles), dim3(kBlockThreads), 0, stream, d_tasks, d_tile_begin, d_tile_task, n_tasks, total_tiles,
                     d_status);
  return hipGetLastError();
}

}  // namespace device
}  // namespace miarrow
