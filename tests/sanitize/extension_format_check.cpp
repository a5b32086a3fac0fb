// extension_format_check.cpp -- extension_format.hpp alone, as a program of its own under ASan + UBSan
// (tests/test_extension_schema_host.py builds and runs it).  Every function of the header against a byte-wise restatement
// written here: the UUID image and its order, the two text forms against each other and against snprintf, bool8.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "extension_format.hpp"

using namespace miarrow::extfmt;

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                \
    }                                                            \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t Next() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

// the canonical text of 16 bytes in text order, by snprintf
static void TextOfBytes(const uint8_t* b, char* out37) {
  std::snprintf(out37, 37, "%02x%02x%02x%02x-%02x%02x-%02x%02x-%02x%02x-%02x%02x%02x%02x%02x%02x", b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7],
                b[8], b[9], b[10], b[11], b[12], b[13], b[14], b[15]);
}

static __int128 Wide(const UuidValue& v) {
  return static_cast<__int128>((static_cast<unsigned __int128>(static_cast<uint64_t>(v.upper)) << 64) | v.lower);
}

int main() {
  std::vector<std::vector<uint8_t>> cases;
  cases.push_back(std::vector<uint8_t>(16, 0x00));
  cases.push_back(std::vector<uint8_t>(16, 0xFF));
  {
    std::vector<uint8_t> v(16, 0xFF);
    v[0] = 0x7F;
    cases.push_back(v);
    std::vector<uint8_t> w(16, 0x00);
    w[0] = 0x80;
    cases.push_back(w);
    std::vector<uint8_t> seq(16);
    for (int i = 0; i < 16; i++) seq[static_cast<size_t>(i)] = static_cast<uint8_t>(i * 17);
    cases.push_back(seq);
  }
  for (int i = 0; i < 4000; i++) {
    std::vector<uint8_t> v(16);
    const uint64_t a = Next(), b = Next();
    std::memcpy(v.data(), &a, 8);
    std::memcpy(v.data() + 8, &b, 8);
    cases.push_back(v);
  }
  for (size_t i = 0; i < cases.size(); i++) {
    // heap copies of exactly 16 / 36 bytes: a read or a write past either end is ASan's to find
    uint8_t* bytes = static_cast<uint8_t*>(std::malloc(16));
    std::memcpy(bytes, cases[i].data(), 16);
    const UuidValue u = UuidFromArrow(bytes);
    uint64_t hi = 0, lo = 0;
    for (int k = 0; k < 8; k++) {
      hi |= static_cast<uint64_t>(bytes[k]) << (56 - 8 * k);
      lo |= static_cast<uint64_t>(bytes[8 + k]) << (56 - 8 * k);
    }
    CHECK(u.lower == lo);
    CHECK(static_cast<uint64_t>(u.upper) == (hi ^ 0x8000000000000000ull));
    uint64_t first, second;   // the halves as a little-endian load sees them
    std::memcpy(&first, bytes, 8);
    std::memcpy(&second, bytes + 8, 8);
    const UuidValue h = UuidFromHalves(first, second);
    CHECK(h.lower == u.lower && h.upper == u.upper);
    char want[37];
    TextOfBytes(bytes, want);
    char* text = static_cast<char*>(std::malloc(36));
    UuidToText(u.lower, u.upper, text);
    CHECK(std::memcmp(text, want, 36) == 0);
    uint32_t words[9];
    UuidTextWords(u.lower, u.upper, words);
    CHECK(std::memcmp(words, want, 36) == 0);
    // signed 128-bit order == byte order of the 16 bytes == order of the text
    if (i > 0) {
      const UuidValue p = UuidFromArrow(cases[i - 1].data());
      const int by_bytes = std::memcmp(cases[i - 1].data(), bytes, 16);
      const __int128 a = Wide(p), b = Wide(u);
      CHECK((by_bytes < 0) == (a < b) && (by_bytes == 0) == (a == b));
      char prev[37];
      TextOfBytes(cases[i - 1].data(), prev);
      CHECK((by_bytes < 0) == (std::strcmp(prev, want) < 0));
    }
    std::free(text);
    std::free(bytes);
  }
  for (int v = -128; v <= 127; v++) {
    CHECK(Bool8(static_cast<int8_t>(v)) == (v != 0 ? 1 : 0));
    CHECK(HexPair(static_cast<uint32_t>(v & 0xFF)) ==
          (static_cast<uint32_t>("0123456789abcdef"[(v >> 4) & 15]) | (static_cast<uint32_t>("0123456789abcdef"[v & 15]) << 8)));
  }
  for (int i = 0; i < 100000; i++) {
    const uint32_t v = i < 256 ? static_cast<uint32_t>(i) * 0x01010101u : static_cast<uint32_t>(Next());
    uint32_t want = 0;
    for (int k = 0; k < 4; k++) want |= static_cast<uint32_t>(((v >> (8 * k)) & 0xFFu) != 0 ? 1u : 0u) << (8 * k);
    CHECK(Bool8x4(v) == want);
  }
  if (failures) {
    std::printf("extension_format: %d checks failed\n", failures);
    return 1;
  }
  std::printf("extension_format: ok\n");
  return 0;
}
