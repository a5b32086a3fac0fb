// kernels_lz4_encode.hip -- the writer's LZ4 block compressor and the compaction of its output into the IPC body.
//
// lz4_compress_blocks: one wave (one workgroup of 64 lanes) per 64 KiB block of an encoded record-batch body; the blocks of
// every buffer of the body go in one launch.  The wave stages its block in LDS (64 KiB; the match finder reads every
// position several times, unaligned) beside a hash table of 4096 positions (16 KiB), then works through the positions 64
// at a time exactly as lz4_encode_format.hpp states: every lane hashes the 4 bytes at its position and reads the table's
// candidate, a ballot picks the first lane whose candidate holds the same 4 bytes, THEN the lanes up to that one enter
// their positions with an LDS atomicMax -- the table holds the largest position of a hash whichever lane's write lands
// last, so the bytes written depend on the input bytes alone and equal CompressBlockSerial's.  All lanes extend the
// match 256 bytes a round (4 per lane, ballot, first mismatch), the sequence goes out with cooperative byte copies and the
// wave continues behind the match.  A block of <= 12 bytes, or one whose output would reach its input size, is stored:
// its size word says so and the compaction kernel takes its bytes from the encoded body.
//
// Bounds: the block table comes from the host's span table (writer_plan.cpp); a block's n bytes lie inside the encoded
// body, and its staging loads round n up to 16 bytes inside the body's allocation (spans are 64-byte aligned and padded).
// Every write of block b lies in [b * kSlotStride, b * kSlotStride + n): a sequence is written only when the output stays
// below n.  Input bytes are compared and copied, never used as an address; table entries are positions < n by
// construction.
//
// compact_body: one workgroup per copy of the host's table (frame headers, prefixes and size words as immediates, blocks
// from the slots, stored blocks and raw buffers from the encoded body) into the final body, which the launcher zeroed.
#include "device_common.hpp"
#include "lz4_encode_format.hpp"

namespace miarrow {
namespace device {

namespace {

using namespace lz4enc;

// Two workgroups share a CU's 160 KiB.  The funnel read of byte position `at` touches word at / 4 + 1: positions read are
// < n - 5 (match starts end at n - 12, extension at n - 6), so that word is at most word n / 4 - 1.
constexpr uint32_t kStageWords = kBlockSize / 4;

// the 4 bytes at byte position `at` of the staged block
__device__ __forceinline__ uint32_t lds_read32(const uint32_t* s_in, uint32_t at) {
  const uint32_t w = at >> 2, sh = (at & 3u) * 8u;
  const uint64_t two = static_cast<uint64_t>(s_in[w]) | static_cast<uint64_t>(s_in[w + 1]) << 32;
  return static_cast<uint32_t>(two >> sh);
}
__device__ __forceinline__ uint8_t lds_read8(const uint32_t* s_in, uint32_t at) {
  return static_cast<uint8_t>(s_in[at >> 2] >> ((at & 3u) * 8u));
}

__global__ __launch_bounds__(64) void lz4_compress_blocks(const uint8_t* __restrict__ body, const BlockIn* __restrict__ blocks,
                                                          uint32_t n_blocks, uint8_t* __restrict__ slots, uint32_t* __restrict__ words) {
  __shared__ uint32_t s_in[kStageWords];
  __shared__ uint32_t s_table[kHashSize];
  const uint32_t b = blockIdx.x, lane = threadIdx.x;
  if (b >= n_blocks) return;
  const uint32_t n = blocks[b].n;
  if (n == 0 || n > kBlockSize) return;   // (the planner makes no such block)
  if (TooShort(n)) {
    if (lane == 0) words[b] = kStoredFlag | n;
    return;
  }
  const uint4* in16 = reinterpret_cast<const uint4*>(body + blocks[b].in_off);   // in_off is a multiple of 64
  uint8_t* out = slots + static_cast<size_t>(b) * kSlotStride;
  for (uint32_t i = lane; i < (n + 15) / 16; i += 64) reinterpret_cast<uint4*>(s_in)[i] = in16[i];
  for (uint32_t i = lane; i < kHashSize; i += 64) s_table[i] = 0;
  __syncthreads();

  const uint32_t last_start = LastMatchStart(n), end_limit = MatchEndLimit(n);
  uint32_t anchor = 0, p = 0, op = 0;   // wave-uniform
  bool stored = false;
  while (p <= last_start) {
    const uint32_t q = p + lane;
    const bool active = q <= last_start;
    uint32_t value = 0, hash = 0, entry = 0;
    if (active) {
      value = lds_read32(s_in, q);
      hash = Hash(value);
      entry = s_table[hash];
    }
    const bool match = active && CandidateInReach(entry, q) && lds_read32(s_in, entry - 1) == value;
    const uint64_t hits = __ballot(match);
    const int first = hits ? __builtin_ctzll(hits) : 64;
    __syncthreads();   // every candidate is read before any position of this group is entered
    if (active && static_cast<int>(lane) <= first) atomicMax(&s_table[hash], q + 1);   // up to the match start
    if (hits == 0) {
      p += kGroup;
      continue;
    }
    const uint32_t s = p + static_cast<uint32_t>(first);
    const uint32_t ref = static_cast<uint32_t>(__shfl(static_cast<int>(entry), first)) - 1;
    uint32_t len = kMinMatch;
    while (true) {   // 4 bytes a lane; a lane at or past the limit reports a mismatch at its first byte
      const uint32_t at = s + len + lane * 4;
      uint32_t equal = 0;
      if (at < end_limit) {
        const uint32_t diff = lds_read32(s_in, at) ^ lds_read32(s_in, ref + len + lane * 4);
        equal = diff ? static_cast<uint32_t>(__builtin_ctz(diff)) >> 3 : 4u;
        equal = min(equal, end_limit - at);
      }
      const uint64_t ends = __ballot(equal < 4);
      if (ends == 0) {
        len += 256;
        continue;
      }
      const int stop = __builtin_ctzll(ends);
      len += static_cast<uint32_t>(stop) * 4 + static_cast<uint32_t>(__shfl(static_cast<int>(equal), stop));
      break;
    }
    const uint32_t literals = s - anchor, size = SequenceSize(literals, len);
    if (op + size >= n) {
      stored = true;
      break;
    }
    const uint32_t lit_ext = ExtBytes(literals), match_ext = ExtBytes(len - kMinMatch), offset = s - ref;
    for (uint32_t j = lane; j < 1 + lit_ext; j += 64) out[op + j] = j == 0 ? Token(literals, len) : ExtByte(literals, j - 1);
    op += 1 + lit_ext;
    for (uint32_t j = lane; j < literals; j += 64) out[op + j] = lds_read8(s_in, anchor + j);
    op += literals;
    for (uint32_t j = lane; j < 2 + match_ext; j += 64)
      out[op + j] = j == 0 ? static_cast<uint8_t>(offset & 255) : j == 1 ? static_cast<uint8_t>(offset >> 8) : ExtByte(len - kMinMatch, j - 2);
    op += 2 + match_ext;
    anchor = p = s + len;
  }
  if (!stored) {
    const uint32_t literals = n - anchor, lit_ext = ExtBytes(literals);
    if (op + LastSequenceSize(literals) >= n) {
      stored = true;
    } else {
      for (uint32_t j = lane; j < 1 + lit_ext; j += 64) out[op + j] = j == 0 ? Token(literals, 0) : ExtByte(literals, j - 1);
      op += 1 + lit_ext;
      for (uint32_t j = lane; j < literals; j += 64) out[op + j] = lds_read8(s_in, anchor + j);
      op += literals;
    }
  }
  if (lane == 0) words[b] = stored ? (kStoredFlag | n) : op;
}

__global__ __launch_bounds__(kBlockThreads) void compact_body(const uint8_t* __restrict__ body, const uint8_t* __restrict__ slots,
                                                              const BodyCopy* __restrict__ copies, uint32_t n_copies,
                                                              uint8_t* __restrict__ out) {
  if (blockIdx.x >= n_copies) return;
  const BodyCopy c = copies[blockIdx.x];
  uint8_t* dst = out + c.dst;
  if (c.from == kFromImmediate) {
    if (threadIdx.x < c.len && threadIdx.x < 8) dst[threadIdx.x] = static_cast<uint8_t>(c.imm >> (8 * threadIdx.x));
    return;
  }
  const uint8_t* src = (c.from == kFromSlots ? slots : body) + c.src;
  // the destination follows a 7-byte frame header and 4-byte size words: bytes up to its first 4-byte boundary, then words
  // put together from the source's bytes
  const uint32_t head = min(c.len, static_cast<uint32_t>((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3));
  if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
  const uint32_t n_words = (c.len - head) / 4;
  uint32_t* dst4 = reinterpret_cast<uint32_t*>(dst + head);
  const uint8_t* s = src + head;
  if (((reinterpret_cast<uintptr_t>(s)) & 3) == 0) {
    const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s);
    for (uint32_t i = threadIdx.x; i < n_words; i += kBlockThreads) dst4[i] = s4[i];
  } else {
    for (uint32_t i = threadIdx.x; i < n_words; i += kBlockThreads) {
      const uint8_t* q = s + static_cast<size_t>(i) * 4;
      dst4[i] = static_cast<uint32_t>(q[0]) | static_cast<uint32_t>(q[1]) << 8 | static_cast<uint32_t>(q[2]) << 16 | static_cast<uint32_t>(q[3]) << 24;
    }
  }
  const uint32_t done = head + n_words * 4;
  if (threadIdx.x < c.len - done) dst[done + threadIdx.x] = src[done + threadIdx.x];
}

}  // namespace

hipError_t LaunchLz4CompressBlocks(const uint8_t* d_body, const lz4enc::BlockIn* d_blocks, uint32_t n_blocks, uint8_t* d_slots,
                                   uint32_t* d_words, hipStream_t stream) {
  MI_DROP_STALE_ERROR();
  if (n_blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(lz4_compress_blocks, dim3(n_blocks), dim3(64), 0, stream, d_body, d_blocks, n_blocks, d_slots, d_words);
  return hipGetLastError();
}

hipError_t LaunchCompactBody(const uint8_t* d_body, const uint8_t* d_slots, const lz4enc::BodyCopy* d_copies, uint32_t n_copies,
                             uint8_t* d_out, hipStream_t stream) {
  MI_DROP_STALE_ERROR();
  if (n_copies == 0) return hipSuccess;
  hipLaunchKernelGGL(compact_body, dim3(n_copies), dim3(kBlockThreads), 0, stream, d_body, d_slots, d_copies, n_copies, d_out);
  return hipGetLastError();
}

}  // namespace device
}  // namespace miarrow
