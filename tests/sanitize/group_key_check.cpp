// group_key_check.cpp -- the GROUP BY key rules of mi_scan_group_aggregate (duckdb-arrow_amd/csrc/group_key.hpp, the
// header the group kernels compile): normalisation of every class at its edges, masked padding, equality / hash / order
// against plain restatements, and the host's GroupTable against a std::map, as a program of its own for
// g++ -fsanitize=address,undefined.  No arguments; prints "<checks> checks, <failed> failed" and exits 1 on a failure.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <tuple>
#include <vector>

#include "group_key.hpp"

using namespace miarrow::groupkey;
using miarrow::aggmerge::Partial;

namespace {
long failed = 0, checks = 0;

void Expect(bool ok, const char* what, long a = 0, long b = 0) {
  checks++;
  if (!ok && failed++ < 20) std::fprintf(stderr, "FAILED: %s (%ld, %ld)\n", what, a, b);
}

typedef __int128 i128;
typedef unsigned __int128 u128;
i128 Value(uint64_t lo, uint64_t hi) { return static_cast<i128>((static_cast<u128>(hi) << 64) | lo); }

// ---- a key part written out plainly: what the normalised image must mean
struct Plain {
  bool null = false;
  bool is_string = false;
  i128 integer = 0;
  std::string bytes;
  bool operator==(const Plain& o) const { return null == o.null && (null || (is_string ? bytes == o.bytes : integer == o.integer)); }
};
// ascending, NULLS LAST; strings bytewise (unsigned), then shorter first: std::string's compare on unsigned char traits
bool PlainLess(const Plain& a, const Plain& b) {
  if (a.null || b.null) return !a.null && b.null;
  if (!a.is_string) return a.integer < b.integer;
  const size_t n = std::min(a.bytes.size(), b.bytes.size());
  const int c = std::memcmp(a.bytes.data(), b.bytes.data(), n);
  return c != 0 ? c < 0 : a.bytes.size() < b.bytes.size();
}

void SetInteger(Key* k, int part, i128 v) {
  k->lo[part] = static_cast<uint64_t>(static_cast<u128>(v));
  k->hi[part] = static_cast<uint64_t>(static_cast<u128>(v) >> 64);
}
// a string_t row with 0xFF behind the string, normalised
bool SetString(Key* k, int part, const std::string& s) {
  uint8_t row[16];
  std::memset(row, 0xFF, sizeof(row));
  const uint32_t len = static_cast<uint32_t>(s.size());
  std::memcpy(row, &len, 4);
  std::memcpy(row + 4, s.data(), std::min<size_t>(s.size(), 12));
  uint64_t lo, hi;
  std::memcpy(&lo, row, 8);
  std::memcpy(&hi, row + 8, 8);
  return NormString(lo, hi, &k->lo[part], &k->hi[part]);
}
Key Make(const std::vector<Plain>& parts) {
  Key k;
  std::memset(&k, 0, sizeof(k));
  for (size_t i = 0; i < parts.size(); i++) {
    if (parts[i].null) k.nulls |= 1u << i;
    else if (parts[i].is_string) SetString(&k, static_cast<int>(i), parts[i].bytes);
    else SetInteger(&k, static_cast<int>(i), parts[i].integer);
  }
  return k;
}

void CheckIntegers() {
  struct Case { int cls, width; uint64_t raw; i128 want; };
  const i128 one = 1;
  const Case cases[] = {
      {kKeySigned, 1, 0x80, -128}, {kKeySigned, 1, 0x7F, 127}, {kKeySigned, 1, 0xFF, -1}, {kKeySigned, 1, 0xFFFFFFFFFFFFFF80ull, -128},
      {kKeyUnsigned, 1, 0xFF, 255}, {kKeyUnsigned, 1, 0, 0}, {kKeyUnsigned, 1, 0xABCDEF80ull, 128},
      {kKeySigned, 2, 0x8000, -32768}, {kKeySigned, 2, 0x7FFF, 32767}, {kKeyUnsigned, 2, 0xFFFF, 65535},
      {kKeySigned, 4, 0x80000000ull, -(one << 31)}, {kKeySigned, 4, 0x7FFFFFFFull, (one << 31) - 1}, {kKeyUnsigned, 4, 0xFFFFFFFFull, (one << 32) - 1},
      {kKeySigned, 8, 0x8000000000000000ull, -(one << 63)}, {kKeySigned, 8, 0x7FFFFFFFFFFFFFFFull, (one << 63) - 1},
      {kKeySigned, 8, ~0ull, -1}, {kKeyUnsigned, 8, ~0ull, (one << 64) - 1}, {kKeyUnsigned, 8, 0x8000000000000000ull, one << 63},
      {kKeySigned, 8, 0, 0}, {kKeyUnsigned, 8, 0, 0}};
  for (const Case& c : cases) {
    uint64_t lo = 1, hi = 2;
    NormInteger(c.cls, c.width, c.raw, &lo, &hi);
    Expect(Value(lo, hi) == c.want, "NormInteger extends to 128 bits", c.cls, c.width);
  }
  // -1 as int8 and 255 as uint8 are different keys; 2^63 as uint64 sorts after 2^63 - 1
  uint64_t alo, ahi, blo, bhi;
  NormInteger(kKeySigned, 1, 0xFF, &alo, &ahi);
  NormInteger(kKeyUnsigned, 1, 0xFF, &blo, &bhi);
  Expect(!(alo == blo && ahi == bhi), "-1 (int8) differs from 255 (uint8)");
  Expect(ComparePart(kKindInt128, alo, ahi, blo, bhi) < 0, "-1 sorts before 255");
  NormInteger(kKeyUnsigned, 8, 0x8000000000000000ull, &alo, &ahi);
  NormInteger(kKeyUnsigned, 8, 0x7FFFFFFFFFFFFFFFull, &blo, &bhi);
  Expect(ComparePart(kKindInt128, blo, bhi, alo, ahi) < 0 && ComparePart(kKindInt128, alo, ahi, blo, bhi) > 0, "2^63 sorts after 2^63 - 1");
}

void CheckStrings() {
  for (size_t len = 0; len <= 12; len++) {
    const std::string s(len, 'x');
    Key k;
    std::memset(&k, 0, sizeof(k));
    Expect(SetString(&k, 0, s), "a string of up to 12 bytes has an inline image", static_cast<long>(len));
    uint8_t img[16];
    std::memcpy(img, &k.lo[0], 8);
    std::memcpy(img + 8, &k.hi[0], 8);
    uint32_t got_len;
    std::memcpy(&got_len, img, 4);
    Expect(got_len == len, "the length survives", static_cast<long>(len));
    bool ok = true;
    for (size_t i = 0; i < 12; i++) ok = ok && img[4 + i] == (i < len ? 'x' : 0);
    Expect(ok, "bytes kept, 0xFF padding masked to zero", static_cast<long>(len));
    for (uint32_t i = 0; i < len; i++) Expect(StringByte(k.lo[0], k.hi[0], i) == 'x', "StringByte");
  }
  for (uint32_t len : {13u, 14u, 255u, 0x7FFFFFFFu, 0xFFFFFFFFu}) {
    uint64_t lo = 7, hi = 7;
    Expect(!NormString(0xFFFFFFFF00000000ull | len, ~0ull, &lo, &hi) && lo == 0 && hi == 0, "more than 12 bytes: no inline image", static_cast<long>(len));
  }
  Key a = Make({Plain{false, true, 0, "a"}}), b = Make({Plain{false, true, 0, std::string("a\0", 2)}}), e = Make({Plain{false, true, 0, ""}}),
      n = Make({Plain{true, true, 0, ""}});
  Expect(!Equal(a, b, 1), "'a' and 'a\\0' differ");
  Expect(!Equal(e, n, 1), "'' and NULL differ");
  const int kind = kKindString;
  Expect(KeyLess(&kind, a, b, 1) && !KeyLess(&kind, b, a, 1), "shorter first");
  Expect(KeyLess(&kind, e, n, 1) && !KeyLess(&kind, n, e, 1), "NULLS LAST");
  Key hi_byte = Make({Plain{false, true, 0, "\xFF"}}), lo_byte = Make({Plain{false, true, 0, "\x01zzzzzzzzzzz"}});
  Expect(KeyLess(&kind, lo_byte, hi_byte, 1), "bytes compare unsigned");
}

std::vector<Plain> EdgeParts(bool strings) {
  std::vector<Plain> v;
  v.push_back(Plain{true, strings, 0, ""});
  if (strings) {
    for (const char* s : {"", "a", "b", "ab", "abc", "abcd", "abcde", "abcdefghijkl", "abcdefghijk", "A", "N", "O", "R", "F", "\xFF", "\x80", "\x7F"})
      v.push_back(Plain{false, true, 0, s});
    v.push_back(Plain{false, true, 0, std::string("a\0", 2)});
    v.push_back(Plain{false, true, 0, std::string("\0", 1)});
    v.push_back(Plain{false, true, 0, std::string("\0\0\0\0\0", 5)});
  } else {
    const i128 one = 1;
    for (i128 x : {i128(0), i128(1), i128(-1), i128(255), i128(-128), one << 63, (one << 63) - 1, -(one << 63), (one << 64) - 1, one << 64, -(one << 64),
                   (one << 100) + 7, -(one << 100) - 7, static_cast<i128>(~static_cast<u128>(0) >> 1), -static_cast<i128>(~static_cast<u128>(0) >> 1) - 1})
      v.push_back(Plain{false, false, x, ""});
  }
  return v;
}

void CheckOrderAndHash() {
  std::mt19937_64 rng(20261019);
  // keys of 1 .. 4 parts, kinds mixed, drawn from the edge values and random ones
  for (int n_keys = 1; n_keys <= kMaxKeys; n_keys++) {
    int kinds[kMaxKeys];
    for (int k = 0; k < kMaxKeys; k++) kinds[k] = (n_keys + k) % 2 ? kKindString : kKindInt128;
    std::vector<std::vector<Plain>> plain;
    std::vector<Key> keys;
    const int count = n_keys == 1 ? 60 : 1000;
    for (int i = 0; i < count; i++) {
      std::vector<Plain> parts;
      for (int k = 0; k < n_keys; k++) {
        const std::vector<Plain> edges = EdgeParts(kinds[k] == kKindString);
        if (rng() % 4 != 0 || n_keys == 1) {
          parts.push_back(edges[rng() % edges.size()]);
        } else if (kinds[k] == kKindString) {
          std::string s(rng() % 13, '\0');
          for (char& c : s) c = static_cast<char>(rng() % 4 == 0 ? 0 : rng());
          parts.push_back(Plain{false, true, 0, s});
        } else {
          parts.push_back(Plain{false, false, static_cast<i128>((static_cast<u128>(rng()) << 64) | rng()) >> (rng() % 128), ""});
        }
      }
      plain.push_back(parts);
      keys.push_back(Make(parts));
    }
    for (size_t a = 0; a < keys.size(); a++)
      for (size_t b = 0; b < keys.size(); b++) {
        const bool eq = plain[a] == plain[b];
        Expect(Equal(keys[a], keys[b], n_keys) == eq, "Equal agrees with the plain parts", n_keys);
        if (eq) Expect(Hash(keys[a], n_keys) == Hash(keys[b], n_keys), "equal keys, equal hashes", n_keys);
        const bool less = std::lexicographical_compare(plain[a].begin(), plain[a].end(), plain[b].begin(), plain[b].end(), PlainLess);
        Expect(KeyLess(kinds, keys[a], keys[b], n_keys) == less, "KeyLess agrees with the plain order (NULLS LAST)", n_keys);
      }
    // a strict weak order: irreflexive, asymmetric, and "neither less" is exactly equality, so sorting is total on distinct keys
    for (size_t a = 0; a < keys.size(); a++) {
      Expect(!KeyLess(kinds, keys[a], keys[a], n_keys), "irreflexive");
      const size_t b = rng() % keys.size(), c = rng() % keys.size();
      const bool ab = KeyLess(kinds, keys[a], keys[b], n_keys), ba = KeyLess(kinds, keys[b], keys[a], n_keys);
      Expect(!(ab && ba), "asymmetric");
      Expect((!ab && !ba) == Equal(keys[a], keys[b], n_keys), "incomparable means equal");
      if (ab && KeyLess(kinds, keys[b], keys[c], n_keys)) Expect(KeyLess(kinds, keys[a], keys[c], n_keys), "transitive");
    }
    std::vector<Key> sorted = keys;
    std::sort(sorted.begin(), sorted.end(), [&](const Key& x, const Key& y) { return KeyLess(kinds, x, y, n_keys); });
    Expect(std::is_sorted(sorted.begin(), sorted.end(), [&](const Key& x, const Key& y) { return KeyLess(kinds, x, y, n_keys); }), "std::sort accepts the order");
  }
}

void CheckGroupTable() {
  std::mt19937_64 rng(7);
  const std::vector<int> ops = {miarrow::aggmerge::kOpCountStar, miarrow::aggmerge::kOpSum, miarrow::aggmerge::kOpMin, miarrow::aggmerge::kOpMax};
  const std::vector<int> classes = {miarrow::aggmerge::kClassAny, miarrow::aggmerge::kClassSigned, miarrow::aggmerge::kClassSigned, miarrow::aggmerge::kClassUnsigned};
  struct Ref { long count = 0; i128 sum = 0; bool has = false; int64_t mn = 0; uint64_t mx = 0; };
  for (int distinct : {1, 2, 100, kMaxGroups}) {
    GroupTable table(2, ops, classes);
    std::map<std::tuple<int64_t, std::string>, Ref> ref;
    bool ok = true;
    for (int round = 0; round < 3; round++)            // three lists merged one after the other, as three devices' are
      for (int i = 0; i < distinct; i++) {
        const int64_t a = (i % 7 == 0) ? INT64_MIN + i : i - 50;
        const std::string b = std::to_string(i % 13);
        const bool null_a = i % 11 == 3 && i < 40;   // (NULL, '3'), (NULL, '1'), (NULL, '12'), (NULL, '10'): still distinct keys
        Key k = Make({Plain{null_a, false, a, ""}, Plain{false, true, 0, b}});
        const int64_t v = static_cast<int64_t>(rng() % 2000) - 1000;
        const bool contributes = rng() % 5 != 0;
        Partial p[4] = {{1, 0, 1, 0},
                        {static_cast<uint64_t>(v), v < 0 ? ~0ull : 0ull, contributes ? 1ull : 0ull, 0},
                        {static_cast<uint64_t>(v), v < 0 ? ~0ull : 0ull, contributes ? 1ull : 0ull, 0},
                        {static_cast<uint64_t>(v + 1000), 0, contributes ? 1ull : 0ull, 0}};
        p[0].lo = 0;
        ok = ok && table.Merge(k, p);
        Ref& r = ref[std::make_tuple(null_a ? INT64_MAX : a, (null_a ? "N" : "V") + b)];
        r.count++;
        if (contributes) {
          r.sum += v;
          r.mn = r.has ? std::min(r.mn, v) : v;
          r.mx = r.has ? std::max<uint64_t>(r.mx, static_cast<uint64_t>(v + 1000)) : static_cast<uint64_t>(v + 1000);
          r.has = true;
        }
      }
    Expect(ok, "every merge below the limit succeeds", distinct);
    Expect(table.size() == ref.size(), "as many groups as the map has", static_cast<long>(table.size()), static_cast<long>(ref.size()));
    const int kinds[2] = {kKindInt128, kKindString};
    const std::vector<uint32_t> order = table.Sorted(kinds);
    Expect(order.size() == table.size(), "Sorted lists every group");
    for (size_t i = 0; i + 1 < order.size(); i++) Expect(KeyLess(kinds, table.key(order[i]), table.key(order[i + 1]), 2), "Sorted is strictly ascending");
    for (size_t g = 0; g < table.size(); g++) {
      const Key& k = table.key(g);
      const bool null_a = k.nulls & 1u;
      const uint32_t len = static_cast<uint32_t>(k.lo[1]);
      std::string b;
      for (uint32_t i = 0; i < len; i++) b.push_back(static_cast<char>(StringByte(k.lo[1], k.hi[1], i)));
      const auto it = ref.find(std::make_tuple(null_a ? INT64_MAX : static_cast<int64_t>(k.lo[0]), (null_a ? "N" : "V") + b));
      Expect(it != ref.end(), "the group's key is one that was merged");
      if (it == ref.end()) continue;
      const Partial* p = table.partials(g);
      Expect(static_cast<long>(p[0].count) == it->second.count, "COUNT(*) per group");
      Expect((p[1].count != 0) == it->second.has && (!it->second.has || Value(p[1].lo, p[1].hi) == it->second.sum), "SUM per group");
      Expect(!it->second.has || static_cast<int64_t>(p[2].lo) == it->second.mn, "MIN per group");
      Expect(!it->second.has || p[3].lo == it->second.mx, "MAX per group");
    }
    if (distinct == kMaxGroups) {
      const Partial p[4] = {{0, 0, 1, 0}, {1, 0, 1, 0}, {1, 0, 1, 0}, {1, 0, 1, 0}};
      Expect(table.size() == static_cast<size_t>(kMaxGroups), "the table is full", static_cast<long>(table.size()));
      Expect(!table.Merge(Make({Plain{false, false, 1 << 30, ""}, Plain{false, true, 0, "new"}}), p), "one key past kMaxGroups is refused");
      Expect(table.size() == static_cast<size_t>(kMaxGroups), "... and changes nothing");
      Expect(table.Merge(table.key(17), p), "a key the full table knows still merges");
    }
  }
}
}  // namespace

int main() {
  CheckIntegers();
  CheckStrings();
  CheckOrderAndHash();
  CheckGroupTable();
  std::printf("%ld checks, %ld failed\n", checks, failed);
  return failed ? 1 : 0;
}
