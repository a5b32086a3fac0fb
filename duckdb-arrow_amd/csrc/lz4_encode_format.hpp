// lz4_encode_format.hpp -- the LZ4 block format as the writer's compressor produces it (lz4_Block_format.md), and the one
// LZ4 frame shape it wraps the blocks in (lz4_Frame_format.md), written once for two compilers: hipcc builds the rules into
// the compress kernel (kernels_lz4_encode.hip), g++ builds the same text into tests/sanitize/lz4_encode_check.cpp, where
// liblz4 decompresses what the serial restatement below wrote.  Nothing here allocates or touches a global.
//
//   block     = sequences; sequence = token, [literal length bytes], literals, offset (2 bytes LE), [match length bytes]
//   token     = min(literals, 15) << 4 | min(match - 4, 15); a field of 15 goes on in bytes of 255 and one byte < 255
//   rules     = matches are >= 4 bytes at offsets 1 .. 65535; the last sequence is literals only; the last 5 bytes of a
//               block are literals; no match starts within the last 12 bytes
//   frame     = 04 22 4D 18, FLG 0x60 (version 01, independent blocks), BD 0x40 (64 KiB blocks), HC 0x82, blocks behind
//               their 4-byte size words (bit 31: stored), end mark 00 00 00 00.  The descriptor is constant, so is HC.
//
// The match finder is the kernel's, and the serial restatement visits it in the same order: positions are looked at 64 at
// a time.  Every position of a group reads the hash table's candidate FIRST; the first position of the group whose
// candidate holds the same 4 bytes starts the match; then the positions of the group up to and including that one (all 64
// when there is no match) enter themselves with max(); the match is extended forwards and the next group starts behind
// it.  The table therefore holds only positions the scan has passed, and an entry is always the LARGEST position entered
// for its hash so far, whichever lane's write landed last: the compressed bytes are a function of the input bytes alone.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define MI_L4E __host__ __device__ inline __attribute__((always_inline))
#else
#define MI_L4E inline
#endif

namespace miarrow {
namespace lz4enc {

constexpr uint32_t kBlockSize = 64u << 10;     // BD 0x40
constexpr uint32_t kHashLog = 12;
constexpr uint32_t kHashSize = 1u << kHashLog;   // entries: position + 1, 0 = empty
constexpr uint32_t kGroup = 64;                // positions looked at together
constexpr uint32_t kMinMatch = 4;
constexpr uint32_t kLastLiterals = 5;          // the last 5 bytes of a block are literals
constexpr uint32_t kMatchStartGap = 12;        // no match starts within the last 12 bytes
constexpr uint32_t kMaxOffset = 65535;
constexpr uint32_t kStoredFlag = 0x80000000u;  // size word: the block holds its bytes as they are
constexpr uint32_t kFrameHeaderSize = 7, kFrameEndSize = 4;
constexpr uint64_t kFrameHeader = 0x00824060184D2204ull;   // the 7 header bytes, little-endian

MI_L4E uint32_t Hash(uint32_t four_bytes) { return (four_bytes * 2654435761u) >> (32 - kHashLog); }
//! worst case of one block's output
MI_L4E uint32_t BlockBound(uint32_t n) { return n + n / 255 + 16; }
//! the compress kernel writes block b at b * kSlotStride of its scratch buffer
constexpr uint32_t kSlotStride = (kBlockSize + kBlockSize / 255 + 16 + 15) / 16 * 16;
MI_L4E int64_t BlocksOf(int64_t buffer_len) { return (buffer_len + kBlockSize - 1) / kBlockSize; }

//! bytes that follow the token for a length field of value v (a literal count, or a match length - 4)
MI_L4E uint32_t ExtBytes(uint32_t v) { return v < 15 ? 0 : (v - 15) / 255 + 1; }
//! byte j of them: 255 ... 255, then the rest (< 255)
MI_L4E uint8_t ExtByte(uint32_t v, uint32_t j) {
  const uint32_t k = ExtBytes(v);
  return static_cast<uint8_t>(j + 1 < k ? 255u : (v - 15) - 255u * (k - 1));
}
MI_L4E uint8_t Token(uint32_t literals, uint32_t match_len /* 0: last sequence */) {
  const uint32_t m = match_len ? match_len - kMinMatch : 0;
  return static_cast<uint8_t>((literals < 15 ? literals : 15u) << 4 | (m < 15 ? m : 15u));
}
MI_L4E uint32_t SequenceSize(uint32_t literals, uint32_t match_len) {
  return 1 + ExtBytes(literals) + literals + 2 + ExtBytes(match_len - kMinMatch);
}
MI_L4E uint32_t LastSequenceSize(uint32_t literals) { return 1 + ExtBytes(literals) + literals; }
//! a block this short has no position at which a match may start: it is stored
MI_L4E bool TooShort(uint32_t n) { return n <= kMatchStartGap; }
//! last position at which a match may start, and the position no match reaches past (n > 12)
MI_L4E uint32_t LastMatchStart(uint32_t n) { return n - kMatchStartGap; }
MI_L4E uint32_t MatchEndLimit(uint32_t n) { return n - kLastLiterals; }
//! table entry `entry` (position + 1, 0 empty) names a position before q within reach
MI_L4E bool CandidateInReach(uint32_t entry, uint32_t q) { return entry != 0 && entry - 1 < q && q - (entry - 1) <= kMaxOffset; }

//! a frame of blocks with these size words
inline int64_t FrameSize(const uint32_t* words, int64_t n_blocks) {
  int64_t size = kFrameHeaderSize + kFrameEndSize;
  for (int64_t b = 0; b < n_blocks; b++) size += 4 + static_cast<int64_t>(words[b] & ~kStoredFlag);
  return size;
}
//! a buffer is written as its frame only when that is smaller than its bytes (else: prefix -1 and the bytes)
inline bool FrameWins(int64_t frame_size, int64_t buffer_len) { return frame_size < buffer_len; }

// ---- what the host planner hands the two kernels (writer_plan.cpp fills them, kernels_lz4_encode.hip reads them)
struct BlockIn {
  uint64_t in_off;   // the block's bytes inside the encoded body
  uint32_t n;        // 1 .. kBlockSize
  uint32_t _pad;
};
constexpr uint32_t kFromBody = 0, kFromSlots = 1, kFromImmediate = 2;
struct BodyCopy {
  int64_t dst;       // position in the compressed body
  int64_t src;       // position in the encoded body / in the compress kernel's slots
  uint32_t len;      // <= kBlockSize; immediate: <= 8
  uint32_t from;     // kFrom*
  uint64_t imm;      // kFromImmediate: the bytes, little-endian
};

// ------------------------------------------------------------------------------------------------ serial restatement
inline uint32_t Read32(const uint8_t* p, uint32_t at) {
  return static_cast<uint32_t>(p[at]) | static_cast<uint32_t>(p[at + 1]) << 8 | static_cast<uint32_t>(p[at + 2]) << 16 |
         static_cast<uint32_t>(p[at + 3]) << 24;
}

//! One block of n <= kBlockSize bytes -> `out` (BlockBound(n) bytes of room).  Returns the size word: the compressed size,
//! or kStoredFlag | n when the block does not shrink (then `out` holds nothing of use).  `table`: kHashSize words.
inline uint32_t CompressBlockSerial(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t* table) {
  if (TooShort(n)) return kStoredFlag | n;
  for (uint32_t i = 0; i < kHashSize; i++) table[i] = 0;
  const uint32_t last_start = LastMatchStart(n), end_limit = MatchEndLimit(n);
  uint32_t anchor = 0, p = 0, op = 0;
  while (p <= last_start) {
    const uint32_t lanes = last_start - p + 1 < kGroup ? last_start - p + 1 : kGroup;
    uint32_t value[kGroup], entry[kGroup];
    for (uint32_t l = 0; l < lanes; l++) {
      value[l] = Read32(in, p + l);
      entry[l] = table[Hash(value[l])];
    }
    uint32_t hit = lanes;
    for (uint32_t l = 0; l < lanes && hit == lanes; l++)
      if (CandidateInReach(entry[l], p + l) && Read32(in, entry[l] - 1) == value[l]) hit = l;
    for (uint32_t l = 0; l < lanes && l <= hit; l++) {   // the positions up to the match start: the table never runs ahead
      uint32_t& slot = table[Hash(value[l])];
      if (slot < p + l + 1) slot = p + l + 1;
    }
    if (hit == lanes) {
      p += kGroup;
      continue;
    }
    const uint32_t s = p + hit, ref = entry[hit] - 1;
    uint32_t len = kMinMatch;
    while (s + len < end_limit && in[s + len] == in[ref + len]) len++;
    const uint32_t literals = s - anchor, size = SequenceSize(literals, len);
    if (op + size >= n) return kStoredFlag | n;   // the output only grows from here
    out[op++] = Token(literals, len);
    for (uint32_t j = 0; j < ExtBytes(literals); j++) out[op++] = ExtByte(literals, j);
    for (uint32_t j = 0; j < literals; j++) out[op++] = in[anchor + j];
    const uint32_t offset = s - ref;
    out[op++] = static_cast<uint8_t>(offset & 255);
    out[op++] = static_cast<uint8_t>(offset >> 8);
    for (uint32_t j = 0; j < ExtBytes(len - kMinMatch); j++) out[op++] = ExtByte(len - kMinMatch, j);
    anchor = p = s + len;
  }
  const uint32_t literals = n - anchor;
  if (op + LastSequenceSize(literals) >= n) return kStoredFlag | n;
  out[op++] = Token(literals, 0);
  for (uint32_t j = 0; j < ExtBytes(literals); j++) out[op++] = ExtByte(literals, j);
  for (uint32_t j = 0; j < literals; j++) out[op++] = in[anchor + j];
  return op;
}

//! Worst case of CompressBufferSerial's output
inline int64_t BufferBound(int64_t n) { return n == 0 ? 0 : 8 + kFrameHeaderSize + kFrameEndSize + BlocksOf(n) * (4 + static_cast<int64_t>(kBlockSize)); }

//! One buffer of a record-batch body as the writer stores it with BodyCompression LZ4_FRAME: nothing when it is empty, the
//! int64 length and one frame, or -1 and the bytes when the frame would not be smaller.  Returns the bytes written, or -1
//! when `cap` < BufferBound(n).  `block_out` (BlockBound(kBlockSize) bytes) and `table` (kHashSize words) are scratch.
inline int64_t CompressBufferSerial(const uint8_t* in, int64_t n, uint8_t* out, int64_t cap, uint8_t* block_out, uint32_t* table) {
  if (n == 0) return 0;
  if (cap < BufferBound(n)) return -1;
  auto put = [&](int64_t at, uint64_t v, int bytes) { for (int i = 0; i < bytes; i++) out[at + i] = static_cast<uint8_t>(v >> (8 * i)); };
  put(0, static_cast<uint64_t>(n), 8);
  put(8, kFrameHeader, kFrameHeaderSize);
  int64_t at = 8 + kFrameHeaderSize;
  for (int64_t b = 0; b < BlocksOf(n); b++) {
    const uint8_t* src = in + b * kBlockSize;
    const uint32_t bn = static_cast<uint32_t>(n - b * kBlockSize < kBlockSize ? n - b * kBlockSize : kBlockSize);
    const uint32_t word = CompressBlockSerial(src, bn, block_out, table);
    put(at, word, 4);
    at += 4;
    const uint32_t size = word & ~kStoredFlag;
    const uint8_t* data = (word & kStoredFlag) ? src : block_out;
    for (uint32_t i = 0; i < size; i++) out[at + i] = data[i];
    at += size;
  }
  put(at, 0, kFrameEndSize);
  at += kFrameEndSize;
  if (FrameWins(at - 8, n)) return at;
  put(0, ~0ull, 8);
  for (int64_t i = 0; i < n; i++) out[8 + i] = in[i];
  return 8 + n;
}

}  // namespace lz4enc
}  // namespace miarrow
