// hash_group_check.cpp -- the rules of the hash GROUP BY (duckdb-arrow_amd/csrc/hash_group.hpp, the header the kernels of
// kernels_hash_group.hip compile) as a program of its own for ASan + UBSan:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I duckdb-arrow_amd/csrc tests/sanitize/hash_group_check.cpp
// It checks the hash (a bijection's inverse, the spread over a table), SlotsFor and TableBytes, the carry rule over wraps
// against unsigned __int128, the ordered-word maps and their inverses over the type edges, +-0.0, +-inf and NaN payloads,
// HashProgramIsValid, and the serial table model against std::map; and it prints "hash <key> <hash>" for a fixed key list,
// which tests/test_hash_aggregate_host.py holds the Python restatement of the hash to.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <limits>
#include <map>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "hash_group.hpp"

using namespace miarrow;
using aggmerge::Partial;

static long g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    g_checks++;                                                          \
    if (!(cond)) {                                                       \
      g_failed++;                                                        \
      if (g_failed < 20) printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); \
    }                                                                    \
  } while (0)

// the inverse of hashgroup::Hash, step by step: it exists exactly when every step is a bijection
static uint64_t Unshift(uint64_t x, int s) {
  uint64_t r = x;
  for (int i = s; i < 64; i += s) r = x ^ (r >> s);
  return r;
}
static uint64_t InverseOdd(uint64_t a) {   // Newton: five steps double 3 correct bits to 64 and more
  uint64_t x = a;
  for (int i = 0; i < 6; i++) x *= 2 - a * x;
  return x;
}
static uint64_t Unhash(uint64_t h) {
  uint64_t x = Unshift(h, 32);
  x *= InverseOdd(0xBB67AE8584CAA73Bull);
  x = Unshift(x, 29);
  x *= InverseOdd(0x6A09E667F3BCC909ull);
  return Unshift(x, 31);
}

static void CheckHash(std::mt19937_64& rng) {
  for (int i = 0; i < 100000; i++) {
    const uint64_t k = i < 1000 ? static_cast<uint64_t>(i) : rng();
    CHECK(Unhash(hashgroup::Hash(k)) == k);
  }
  // consecutive keys (rows of one order lie side by side) spread: no slot of a table at load 1 / 2 collects a long chain
  const uint32_t slots = hashgroup::SlotsFor(1u << 15);
  std::vector<uint32_t> fill(slots, 0);
  for (uint64_t k = 0; k < (1u << 15); k++) fill[hashgroup::Hash(k) & (slots - 1)]++;
  uint32_t worst = 0;
  for (uint32_t f : fill) worst = f > worst ? f : worst;
  CHECK(worst <= 8);
  for (uint64_t k = 0; k < (1u << 15); k++) CHECK(hashgroup::Hash(k << 32) != hashgroup::Hash((k + 1) << 32));
}

static void CheckSlots() {
  CHECK(hashgroup::SlotsFor(1) == 64 && hashgroup::SlotsFor(32) == 64 && hashgroup::SlotsFor(33) == 128);
  CHECK(hashgroup::SlotsFor(hashgroup::kMaxHashGroups) == (1u << 25));
  for (uint32_t g = 1; g <= hashgroup::kMaxHashGroups; g = g * 3 / 2 + 1) {
    const uint32_t s = hashgroup::SlotsFor(g);
    CHECK((s & (s - 1)) == 0 && s >= 64 && s >= 2 * g && (s == 64 || s / 2 < 2 * g));
    for (int n = 1; n <= aggmerge::kMaxAggregates; n++)
      CHECK(hashgroup::TableBytes(g, n) == 32 + 8 * static_cast<size_t>(s) + 24 * (static_cast<size_t>(s) + 2) * static_cast<size_t>(n));
  }
  CHECK(hashgroup::kEmptyKey == ~0ull && hashgroup::kExtraRecords == 2 && hashgroup::kExtraNull != hashgroup::kExtraEmptyKey);
}

// a record's {lo, hi} under the kernel's two adds, in any order of the contributors, against unsigned __int128
static void CheckCarry(std::mt19937_64& rng) {
  typedef unsigned __int128 u128;
  for (int round = 0; round < 2000; round++) {
    uint64_t lo = 0, hi = 0;
    u128 want = 0;
    const int n = 1 + static_cast<int>(rng() % 64);
    for (int i = 0; i < n; i++) {
      uint64_t vlo, vhi;
      switch (rng() % 4) {
        case 0: vlo = rng() | (1ull << 63); vhi = 0; break;                       // uint64 of 2^63 and more: lo wraps every other add
        case 1: vlo = static_cast<uint64_t>(-static_cast<int64_t>(rng() % 1000)); vhi = vlo ? ~0ull : 0; break;   // small negatives
        case 2: vlo = ~0ull; vhi = ~0ull; break;                                  // -1
        default: vlo = rng(); vhi = rng(); break;
      }
      const uint64_t old = lo;   // what the returning add hands back
      lo += vlo;
      hi += vhi + hashgroup::CarryOf(old, vlo);
      want += (static_cast<u128>(vhi) << 64) | vlo;
    }
    CHECK(lo == static_cast<uint64_t>(want) && hi == static_cast<uint64_t>(want >> 64));
  }
  CHECK(hashgroup::CarryOf(~0ull, 1) == 1 && hashgroup::CarryOf(~0ull, 0) == 0 && hashgroup::CarryOf(0, ~0ull) == 0 && hashgroup::CarryOf(1ull << 63, 1ull << 63) == 1);
}

static void CheckOrderedWords(std::mt19937_64& rng) {
  // integers: the order of the words is the order of the values, and the map comes back with the right extension
  std::vector<int64_t> s = {0, 1, -1, -2, INT64_MIN, INT64_MIN + 1, INT64_MAX, INT64_MAX - 1, INT8_MIN, INT8_MAX, INT16_MIN, INT16_MAX, INT32_MIN, INT32_MAX};
  for (int i = 0; i < 200; i++) s.push_back(static_cast<int64_t>(rng()));
  for (int64_t a : s)
    for (int64_t b : s) {
      const uint64_t wa = hashgroup::OrderedWord(aggmerge::kClassSigned, static_cast<uint64_t>(a)), wb = hashgroup::OrderedWord(aggmerge::kClassSigned, static_cast<uint64_t>(b));
      CHECK((a < b) == (wa < wb) && (a == b) == (wa == wb));
      const uint64_t ua = static_cast<uint64_t>(a), ub = static_cast<uint64_t>(b);
      CHECK((ua < ub) == (hashgroup::OrderedWord(aggmerge::kClassUnsigned, ua) < hashgroup::OrderedWord(aggmerge::kClassUnsigned, ub)));
    }
  for (int64_t a : s) {
    uint64_t lo, hi;
    hashgroup::FromOrderedWord(aggmerge::kClassSigned, hashgroup::OrderedWord(aggmerge::kClassSigned, static_cast<uint64_t>(a)), &lo, &hi);
    CHECK(lo == static_cast<uint64_t>(a) && hi == (a < 0 ? ~0ull : 0ull));
    hashgroup::FromOrderedWord(aggmerge::kClassUnsigned, hashgroup::OrderedWord(aggmerge::kClassUnsigned, static_cast<uint64_t>(a)), &lo, &hi);
    CHECK(lo == static_cast<uint64_t>(a) && hi == 0);
  }
  CHECK(hashgroup::OrderedWord(aggmerge::kClassSigned, static_cast<uint64_t>(INT64_MAX)) == ~0ull && hashgroup::OrderedWord(aggmerge::kClassSigned, static_cast<uint64_t>(INT64_MIN)) == 0);
  CHECK(hashgroup::RecordInit(aggmerge::kOpMin) == ~0ull && hashgroup::RecordInit(aggmerge::kOpMax) == 0 && hashgroup::RecordInit(aggmerge::kOpSum) == 0);

  // doubles: the total order of filter_key.hpp over canonical bits; the way back gives the canonical bits
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> d = {0.0, -0.0, 1.0, -1.0, inf, -inf, std::numeric_limits<double>::min(), -std::numeric_limits<double>::min(),
                           std::numeric_limits<double>::denorm_min(), -std::numeric_limits<double>::denorm_min(), std::numeric_limits<double>::max(),
                           std::numeric_limits<double>::lowest(), 1e-300, -1e300, static_cast<double>(1.5f)};
  for (int i = 0; i < 200; i++) d.push_back(std::ldexp(static_cast<double>(static_cast<int64_t>(rng())), static_cast<int>(rng() % 200) - 100));
  std::vector<uint64_t> nans = {0x7FF8000000000000ull, 0xFFF8000000000000ull, 0x7FF0000000000001ull, 0xFFF0000000000001ull, 0x7FFFFFFFFFFFFFFFull, 0xFFFFFFFFFFFFFFFFull,
                                0x7FF4000000000000ull};
  auto word = [](double v) { return hashgroup::OrderedWord(aggmerge::kClassFloat, aggmerge::CanonicalBits(v)); };
  for (double a : d)
    for (double b : d) CHECK((a < b) == (word(a) < word(b)) && (a == b) == (word(a) == word(b)));
  CHECK(word(0.0) == word(-0.0));
  for (uint64_t nb : nans) {
    const double nan = aggmerge::DoubleOf(nb);
    CHECK(word(nan) == word(aggmerge::DoubleOf(nans[0])));
    for (double a : d) CHECK(word(a) < word(nan));
    uint64_t lo, hi;
    hashgroup::FromOrderedWord(aggmerge::kClassFloat, word(nan), &lo, &hi);
    CHECK(lo == aggmerge::kCanonicalNaN && hi == 0);
  }
  for (double a : d) {
    uint64_t lo, hi;
    hashgroup::FromOrderedWord(aggmerge::kClassFloat, word(a), &lo, &hi);
    CHECK(lo == aggmerge::CanonicalBits(a) && hi == 0);
    CHECK(word(a) != 0 && word(a) != ~0ull);   // (no double's word is what MAX or MIN starts as; count tells anyway)
  }
  CHECK(hashgroup::KeyHigh(groupkey::kKeySigned, ~0ull) == ~0ull && hashgroup::KeyHigh(groupkey::kKeyUnsigned, ~0ull) == 0 && hashgroup::KeyHigh(groupkey::kKeySigned, 5) == 0);
}

static void CheckProgram() {
  using namespace aggmerge;
  const int all_ops[] = {kOpCountStar, kOpCount, kOpSum, kOpSumProduct, kOpMin, kOpMax, kOpSumExpr};
  const int all_cls[] = {kClassAny, kClassSigned, kClassUnsigned, kClassFloat, kClassWide};
  for (int op : all_ops)
    for (int cls : all_cls) {
      const bool counts = op == kOpCountStar || op == kOpCount, minmax = op == kOpMin || op == kOpMax;
      const bool integer = cls == kClassSigned || cls == kClassUnsigned;
      const bool want = counts || (minmax && (integer || cls == kClassFloat)) || (!minmax && integer);
      CHECK(hashgroup::HashProgramIsValid(groupkey::kKeySigned, 8, 1, &op, &cls) == want);
    }
  const int op = kOpCountStar, cls = kClassAny;
  for (int key_cls = 0; key_cls <= 5; key_cls++)
    for (int w : {0, 1, 2, 3, 4, 8, 16})
      CHECK(hashgroup::HashProgramIsValid(key_cls, w, 1, &op, &cls) ==
            ((key_cls == groupkey::kKeySigned || key_cls == groupkey::kKeyUnsigned) && (w == 1 || w == 2 || w == 4 || w == 8)));
  const int ops8[9] = {1, 1, 1, 1, 1, 1, 1, 1, 1}, cls8[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  CHECK(!hashgroup::HashProgramIsValid(groupkey::kKeySigned, 8, 0, ops8, cls8));
  CHECK(hashgroup::HashProgramIsValid(groupkey::kKeySigned, 8, 8, ops8, cls8));
  CHECK(!hashgroup::HashProgramIsValid(groupkey::kKeySigned, 8, 9, ops8, cls8));
  const int bad_op = 8;
  CHECK(!hashgroup::HashProgramIsValid(groupkey::kKeySigned, 8, 1, &bad_op, &cls));
}

// the serial model against std::map: sums, minima, counts, the NULL key, the empty mark as a key, collisions, the limit
static void CheckSerialTable(std::mt19937_64& rng) {
  using namespace aggmerge;
  const std::vector<int> ops = {kOpSum, kOpMin, kOpCount}, classes = {kClassSigned, kClassSigned, kClassAny};
  for (uint32_t max_groups : {1u, 2u, 31u, 32u, 33u, 500u}) {
    hashgroup::SerialTable table(max_groups, ops, classes);
    std::map<std::pair<int, uint64_t>, std::vector<Partial>> model;   // (is NULL, key word) -> partials
    const uint32_t slots = hashgroup::SlotsFor(max_groups);
    std::vector<uint64_t> pool = {hashgroup::kEmptyKey, hashgroup::kEmptyKey - 1, 0};
    for (uint64_t k = 1; pool.size() < 3 + max_groups; k++)   // keys that share the last slot: the probe wraps around the end
      if ((hashgroup::Hash(k) & (slots - 1)) == slots - 1) pool.push_back(k);
    for (int i = 0; i < 4000; i++) {
      const bool is_null = rng() % 11 == 0;
      const uint64_t key = pool[rng() % pool.size()];
      std::vector<Partial> p(3);
      for (size_t a = 0; a < 3; a++) {
        const int64_t v = static_cast<int64_t>(rng() % 2001) - 1000;
        p[a] = rng() % 5 == 0 ? Partial{0, 0, 0, 0} : Partial{static_cast<uint64_t>(v), v < 0 ? ~0ull : 0ull, 1 + rng() % 3, 0};
      }
      const std::pair<int, uint64_t> mk(is_null ? 1 : 0, is_null ? 0 : key);
      const bool known = model.count(mk) != 0;
      const bool took = table.Merge(key, is_null, p.data());
      CHECK(took == (known || model.size() < max_groups));
      if (!took) continue;
      if (!known) model[mk] = std::vector<Partial>(3, Partial{0, 0, 0, 0});
      for (size_t a = 0; a < 3; a++) Merge(ops[a], classes[a], &model[mk][a], p[a]);
    }
    CHECK(table.size() == model.size() && table.size() <= max_groups);
    std::set<std::pair<int, uint64_t>> seen;
    for (size_t g = 0; g < table.size(); g++) {
      const std::pair<int, uint64_t> mk(table.is_null(g) ? 1 : 0, table.key(g));
      CHECK(model.count(mk) == 1 && seen.insert(mk).second);
      if (!model.count(mk)) continue;
      for (size_t a = 0; a < 3; a++) {
        const Partial &x = table.partials(g)[a], &y = model[mk][a];
        CHECK(x.lo == y.lo && x.hi == y.hi && x.count == y.count && x.flags == y.flags);
      }
    }
  }
}

int main() {
  std::mt19937_64 rng(20261020);
  CheckHash(rng);
  CheckSlots();
  CheckCarry(rng);
  CheckOrderedWords(rng);
  CheckProgram();
  CheckSerialTable(rng);
  const uint64_t probe[] = {0ull, 1ull, 2ull, 63ull, 64ull, 0xFFFFFFFFull, 1ull << 32, (1ull << 63) - 1, 1ull << 63, ~0ull - 1, 0x0123456789ABCDEFull, 0xDEADBEEFCAFEF00Dull};
  for (uint64_t k : probe) printf("hash %" PRIu64 " %" PRIu64 "\n", k, hashgroup::Hash(k));
  printf("%ld checks, %ld failed\n", g_checks, g_failed);
  return g_failed == 0 ? 0 : 1;
}
