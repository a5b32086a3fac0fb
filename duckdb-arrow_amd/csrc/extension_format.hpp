// extension_format.hpp -- the rules of the Arrow canonical extension types this path reads: arrow.uuid, arrow.bool8 and
// arrow.json.  One header for hipcc and a plain C++ compiler, as union_format.hpp and group_key.hpp are: the schema decode
// (ipc_format.cpp: which name is honoured on which storage type), the decode tiles (kernels_decode.hip: tile_uuid,
// tile_bool8), the gather kernel, the host copy of a dictionary's values (scan_dictionary.cpp) and the stand-alone check
// under tests/sanitize/ all compile it; tests/extension_cases.py restates it in numpy.
//
// arrow.uuid  fixed_size_binary(16), the 16 bytes in the order of the canonical text -> DuckDB UUID, a hugeint_t{uint64
//             lower; int64 upper}: `upper` = bytes 0..7 read big-endian with bit 63 flipped, `lower` = bytes 8..15 read
//             big-endian.  Signed 128-bit order then equals the order of the text.
// arrow.bool8 int8, 0 = false, anything else = true -> DuckDB BOOLEAN, one byte 0 / 1.
// arrow.json  utf8 / large_utf8 / utf8_view -> DuckDB JSON: the strings as they are, only the logical type differs.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MI_EXT_FN __host__ __device__ __forceinline__
#else
#define MI_EXT_FN inline
#endif

namespace miarrow {
namespace extfmt {

enum Extension : int32_t { kNone = 0, kUuid = 1, kBool8 = 2, kJson = 3 };

constexpr int kUuidBytes = 16;
constexpr int kUuidTextBytes = 36;   // 8-4-4-4-12
constexpr uint64_t kSignBit = 0x8000000000000000ull;

struct UuidValue {
  uint64_t lower;
  int64_t upper;
};

MI_EXT_FN uint64_t ByteSwap64(uint64_t v) { return __builtin_bswap64(v); }

//! the two little-endian halves of the 16 stored bytes (first = bytes 0..7) -> the hugeint_t image
MI_EXT_FN UuidValue UuidFromHalves(uint64_t first, uint64_t second) {
  return UuidValue{ByteSwap64(second), static_cast<int64_t>(ByteSwap64(first) ^ kSignBit)};
}

MI_EXT_FN UuidValue UuidFromArrow(const uint8_t* bytes) {
  uint64_t hi = 0, lo = 0;
  for (int i = 0; i < 8; i++) {
    hi = (hi << 8) | bytes[i];
    lo = (lo << 8) | bytes[8 + i];
  }
  return UuidValue{lo, static_cast<int64_t>(hi ^ kSignBit)};
}

//! DuckDB's UUID::ToString: lower-case hex, 8-4-4-4-12, of upper ^ 2^63 and then lower; 36 bytes, no terminator
MI_EXT_FN void UuidToText(uint64_t lower, int64_t upper, char* out) {
  const uint64_t hi = static_cast<uint64_t>(upper) ^ kSignBit;
  int at = 0;
  for (int i = 0; i < 32; i++) {
    if (i == 8 || i == 12 || i == 16 || i == 20) out[at++] = '-';
    const uint32_t nibble = static_cast<uint32_t>(((i < 16 ? hi : lower) >> (60 - 4 * (i & 15))) & 0xFu);
    out[at++] = static_cast<char>(nibble < 10 ? '0' + nibble : 'a' + (nibble - 10));
  }
}

//! two lower-case hex characters of one byte, the high nibble's in the low byte (the first in memory)
MI_EXT_FN uint32_t HexPair(uint32_t byte) {
  uint32_t hi = (byte >> 4) & 0xFu, lo = byte & 0xFu;
  hi += hi < 10u ? 0x30u : 0x57u;   // '0', 'a' - 10
  lo += lo < 10u ? 0x30u : 0x57u;
  return hi | (lo << 8);
}

//! The same 36 bytes as UuidToText as nine little-endian dwords: what the text encoder's lanes put together in registers
MI_EXT_FN void UuidTextWords(uint64_t lower, int64_t upper, uint32_t (&w)[9]) {
  const uint64_t hi = static_cast<uint64_t>(upper) ^ kSignBit;
  uint32_t h[16];   // h[i] = the two characters of byte i of the text order
  for (int i = 0; i < 8; i++) {
    h[i] = HexPair(static_cast<uint32_t>(hi >> (56 - 8 * i)) & 0xFFu);
    h[8 + i] = HexPair(static_cast<uint32_t>(lower >> (56 - 8 * i)) & 0xFFu);
  }
  constexpr uint32_t dash = 0x2Du;
  w[0] = h[0] | (h[1] << 16);
  w[1] = h[2] | (h[3] << 16);
  w[2] = dash | (h[4] << 8) | ((h[5] & 0xFFu) << 24);
  w[3] = (h[5] >> 8) | (dash << 8) | (h[6] << 16);
  w[4] = h[7] | (dash << 16) | ((h[8] & 0xFFu) << 24);
  w[5] = (h[8] >> 8) | (h[9] << 8) | (dash << 24);
  w[6] = h[10] | (h[11] << 16);
  w[7] = h[12] | (h[13] << 16);
  w[8] = h[14] | (h[15] << 16);
}

MI_EXT_FN uint8_t Bool8(int8_t v) { return v != 0 ? 1 : 0; }

//! four bool8 rows held in one dword -> four BOOLEAN bytes: a byte becomes 1 when any of its bits is set
MI_EXT_FN uint32_t Bool8x4(uint32_t v) {
  v |= v >> 4;
  v |= v >> 2;
  v |= v >> 1;
  return v & 0x01010101u;
}

}  // namespace extfmt
}  // namespace miarrow
