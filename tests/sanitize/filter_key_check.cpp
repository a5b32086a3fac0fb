// filter_key_check.cpp -- the order-preserving float key and the 128-bit comparison of the pushed-down filter
// (duckdb-arrow_amd/csrc/filter_key.hpp, the header the filter kernel compiles) against naive comparisons, as a program
// of its own for g++ -fsanitize=address,undefined.
//
//   filter_key_check <corpus32> <corpus64> <keys out>
// corpus32 / corpus64: raw uint32 / uint64 bit patterns of floats / doubles.  Every pattern is compared with every one of
// the first `kDense` patterns (the caller puts the special values there) and with a stride of the others:
//   naive order: NaN == NaN whatever sign / payload, NaN > everything else, otherwise the IEEE comparison (-0.0 == +0.0)
// and the sign of key(a) - key(b) must say the same.  The 64-bit corpus, taken pairwise as {lower, upper}, feeds WideLess /
// WideInRange against __int128.  The keys are written out (int64 each, corpus32 first) so that the caller can hold them
// against the library's own.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../duckdb-arrow_amd/csrc/filter_key.hpp"

using namespace miarrow::filterkey;

namespace {
long failed = 0, checks = 0;

template <typename F>
int NaiveCompare(F a, F b) {
  const bool na = std::isnan(a), nb = std::isnan(b);
  if (na || nb) return na && nb ? 0 : na ? 1 : -1;
  return a < b ? -1 : a > b ? 1 : 0;
}
int Sign(int64_t a, int64_t b) { return a < b ? -1 : a > b ? 1 : 0; }

template <typename U>
std::vector<U> ReadAll(const char* path) {
  std::vector<U> v;
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::fprintf(stderr, "FAILED: cannot open %s\n", path); failed++; return v; }
  U x;
  while (std::fread(&x, sizeof(U), 1, f) == 1) v.push_back(x);
  std::fclose(f);
  return v;
}

constexpr size_t kDense = 64;

template <typename U, typename S, typename F>
void CheckFloats(const std::vector<U>& bits, std::vector<int64_t>* keys) {
  std::vector<F> vals(bits.size());
  std::vector<int64_t> key(bits.size());
  for (size_t i = 0; i < bits.size(); i++) {
    std::memcpy(&vals[i], &bits[i], sizeof(U));
    S s;
    std::memcpy(&s, &bits[i], sizeof(U));
    key[i] = FloatKey(s);
    // the host's way to a constant's key agrees with the key of the bits (a NaN may change payload on its way through double)
    const int64_t via_double = FloatKeyOfDouble(static_cast<double>(vals[i]), static_cast<int32_t>(sizeof(U)));
    checks++;
    if (via_double != key[i]) {
      if (failed++ < 10) std::fprintf(stderr, "FAILED: width %zu pattern %llx: key %lld, through a double %lld\n", sizeof(U),
                                      static_cast<unsigned long long>(bits[i]), static_cast<long long>(key[i]), static_cast<long long>(via_double));
    }
  }
  auto pair = [&](size_t i, size_t j) {
    checks++;
    if (NaiveCompare(vals[i], vals[j]) != Sign(key[i], key[j])) {
      if (failed++ < 10) std::fprintf(stderr, "FAILED: width %zu: %llx vs %llx: naive %d, keys %lld %lld\n", sizeof(U),
                                      static_cast<unsigned long long>(bits[i]), static_cast<unsigned long long>(bits[j]),
                                      NaiveCompare(vals[i], vals[j]), static_cast<long long>(key[i]), static_cast<long long>(key[j]));
    }
  };
  for (size_t i = 0; i < bits.size(); i++) {
    for (size_t j = 0; j < bits.size() && j < kDense; j++) pair(i, j);
    for (size_t j = i % 37; j < bits.size(); j += 37) pair(i, j);
  }
  keys->insert(keys->end(), key.begin(), key.end());
}

void CheckWide(const std::vector<uint64_t>& words) {
  struct W { uint64_t lower; int64_t upper; __int128 v; };
  std::vector<W> w;
  for (size_t i = 0; i + 1 < words.size(); i += 2) {
    W x;
    x.lower = words[i];
    std::memcpy(&x.upper, &words[i + 1], 8);
    x.v = static_cast<__int128>((static_cast<unsigned __int128>(words[i + 1]) << 64) | words[i]);
    w.push_back(x);
  }
  // words that differ in one half only, and the extremes
  const uint64_t edge[] = {0ull, 1ull, ~0ull, 1ull << 63, (1ull << 63) - 1};
  for (uint64_t a : edge)
    for (uint64_t b : edge) {
      W x;
      x.lower = a;
      std::memcpy(&x.upper, &b, 8);
      x.v = static_cast<__int128>((static_cast<unsigned __int128>(b) << 64) | a);
      w.push_back(x);
    }
  for (size_t i = 0; i < w.size(); i++)
    for (size_t j = i % 29; j < w.size(); j += 29) {
      checks++;
      if (WideLess(w[i].upper, w[i].lower, w[j].upper, w[j].lower) != (w[i].v < w[j].v)) {
        if (failed++ < 10) std::fprintf(stderr, "FAILED: WideLess at %zu, %zu\n", i, j);
      }
      const size_t k = (i * 31 + j * 7) % w.size();
      checks++;
      if (WideInRange(w[k].upper, w[k].lower, w[i].upper, w[i].lower, w[j].upper, w[j].lower) != (w[i].v <= w[k].v && w[k].v <= w[j].v)) {
        if (failed++ < 10) std::fprintf(stderr, "FAILED: WideInRange at %zu in [%zu, %zu]\n", k, i, j);
      }
    }
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: %s <corpus32> <corpus64> <keys out>\n", argv[0]);
    return 2;
  }
  const std::vector<uint32_t> c32 = ReadAll<uint32_t>(argv[1]);
  const std::vector<uint64_t> c64 = ReadAll<uint64_t>(argv[2]);
  std::vector<int64_t> keys;
  CheckFloats<uint32_t, int32_t, float>(c32, &keys);
  CheckFloats<uint64_t, int64_t, double>(c64, &keys);
  CheckWide(c64);
  FILE* f = std::fopen(argv[3], "wb");
  if (!f || std::fwrite(keys.data(), 8, keys.size(), f) != keys.size()) { std::fprintf(stderr, "FAILED: cannot write %s\n", argv[3]); failed++; }
  if (f) std::fclose(f);
  std::printf("%zu + %zu patterns, %ld checks, %ld failed\n", c32.size(), c64.size(), checks, failed);
  return failed ? 1 : 0;
}
