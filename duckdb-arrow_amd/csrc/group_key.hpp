// group_key.hpp -- the GROUP BY keys of mi_scan_group_aggregate.  One header for hipcc and a plain C++ compiler, as
// agg_merge.hpp is: the lanes of group_windows and group_combine (kernels_group.hip), the host's merge of the per-device
// group lists (MultiDeviceScan::GroupAggregate), the final sort and the stand-alone check under tests/sanitize/ all compile
// these functions, so a key is normalised, compared, hashed and ordered by one rule wherever that happens.
//
// A group key has 1 .. kMaxKeys parts.  Every part is normalised to 16 bytes {lo, hi} plus a NULL bit:
//   integers     sign- or zero-extended to a 128-bit two's-complement integer (kKeySigned / kKeyUnsigned: width 1 / 2 / 4 /
//                8; kKeyWide: hugeint_t{uint64 lower; int64 upper} as it is)
//   strings      the inline string_t image: uint32 length, then at most 12 bytes; the bytes behind `length` are masked to
//                zero here, whatever the row held.  A string of more than 12 bytes has no inline image: NormString says so.
//   NULL         {0, 0} and the part's bit in `nulls`: the bytes under a NULL are never looked at.
// Two keys are equal exactly when all parts and all NULL bits are.  The result order (KeyLess) is ascending part by part,
// integers by value, strings bytewise and then shorter first, NULLS LAST.
#pragma once

#include <cstdint>
#include <cstring>

#include "agg_merge.hpp"

#include <algorithm>
#include <utility>
#include <vector>

namespace miarrow {
namespace groupkey {

constexpr int kMaxKeys = 4;          // == MI_MAX_GROUP_KEYS
constexpr int kWindowLimit = 256;    // == MI_GROUP_WINDOW_LIMIT: distinct keys among the selected rows of one window
constexpr int kMaxGroups = 4096;     // == MI_MAX_GROUPS: distinct keys of one scan
// what a key column's rows are (== MI_GROUP_KEY_CLASS_* of mi_arrow_ipc.h)
constexpr int kKeySigned = 1, kKeyUnsigned = 2, kKeyWide = 3, kKeyString = 4;
// what a normalised part is (== MI_GROUP_KEY_INT128 / MI_GROUP_KEY_STRING)
constexpr int kKindInt128 = 0, kKindString = 1;

MI_KEY_FN int KindOfClass(int cls) { return cls == kKeyString ? kKindString : kKindInt128; }

struct Key {
  uint64_t lo[kMaxKeys], hi[kMaxKeys];
  uint32_t nulls;   // bit k: part k is NULL (its lo / hi are 0)
};

//! the stored integer `raw` (its low `width` bytes) of a signed or unsigned column as a 128-bit integer
MI_KEY_FN void NormInteger(int cls, int width, uint64_t raw, uint64_t* lo, uint64_t* hi) {
  const int shift = 64 - 8 * width;   // width 1 / 2 / 4 / 8
  if (cls == kKeyUnsigned) {
    *lo = (raw << shift) >> shift;
    *hi = 0;
  } else {
    const int64_t s = static_cast<int64_t>(raw << shift) >> shift;
    *lo = static_cast<uint64_t>(s);
    *hi = s < 0 ? ~0ull : 0ull;
  }
}

//! the two halves of a string_t row -> its inline image with the padding masked; false: longer than 12 bytes (lo / hi are 0)
MI_KEY_FN bool NormString(uint64_t row_lo, uint64_t row_hi, uint64_t* lo, uint64_t* hi) {
  const uint32_t len = static_cast<uint32_t>(row_lo);
  if (len > 12u) {
    *lo = 0;
    *hi = 0;
    return false;
  }
  // bytes 0 .. 3 the length, 4 .. 4 + len the string: everything behind is zero
  const uint64_t keep_lo = len >= 4u ? ~0ull : ((1ull << (32u + 8u * len)) - 1ull);
  const uint64_t keep_hi = len <= 4u ? 0ull : (len >= 12u ? ~0ull : ((1ull << (8u * (len - 4u))) - 1ull));
  *lo = row_lo & keep_lo;
  *hi = row_hi & keep_hi;
  return true;
}

MI_KEY_FN bool Equal(const Key& a, const Key& b, int n_keys) {
  bool eq = a.nulls == b.nulls;
#pragma unroll
  for (int k = 0; k < kMaxKeys; k++)
    if (k < n_keys) eq = eq && a.lo[k] == b.lo[k] && a.hi[k] == b.hi[k];
  return eq;
}

MI_KEY_FN uint32_t Mix(uint32_t h, uint64_t v) {
  h = (h ^ static_cast<uint32_t>(v)) * 0x9E3779B1u;
  h = (h ^ (h >> 15) ^ static_cast<uint32_t>(v >> 32)) * 0x85EBCA77u;
  return h ^ (h >> 13);
}
//! equal keys, equal hashes: a function of the normalised parts and the NULL bits alone
MI_KEY_FN uint32_t Hash(const Key& a, int n_keys) {
  uint32_t h = 0x2545F491u + a.nulls;
#pragma unroll
  for (int k = 0; k < kMaxKeys; k++)
    if (k < n_keys) h = Mix(Mix(h, a.lo[k]), a.hi[k]);
  return h ^ (h >> 16);
}

//! byte i (0 .. 11) of a normalised string
MI_KEY_FN uint32_t StringByte(uint64_t lo, uint64_t hi, uint32_t i) {
  return i < 4u ? static_cast<uint32_t>(lo >> (32u + 8u * i)) & 255u : static_cast<uint32_t>(hi >> (8u * (i - 4u))) & 255u;
}

//! -1 / 0 / +1: part a against part b of one kind, neither NULL
MI_KEY_FN int ComparePart(int kind, uint64_t alo, uint64_t ahi, uint64_t blo, uint64_t bhi) {
  if (kind == kKindString) {
    const uint32_t la = static_cast<uint32_t>(alo), lb = static_cast<uint32_t>(blo);
    const uint32_t n = la < lb ? la : lb;
    for (uint32_t i = 0; i < n && i < 12u; i++) {
      const uint32_t x = StringByte(alo, ahi, i), y = StringByte(blo, bhi, i);
      if (x != y) return x < y ? -1 : 1;
    }
    return la == lb ? 0 : (la < lb ? -1 : 1);
  }
  if (alo == blo && ahi == bhi) return 0;
  return filterkey::WideLess(static_cast<int64_t>(ahi), alo, static_cast<int64_t>(bhi), blo) ? -1 : 1;
}

//! the result order: ascending by part 0, then part 1 ...; NULLS LAST.  kinds[k]: kKind* of part k
MI_KEY_FN bool KeyLess(const int* kinds, const Key& a, const Key& b, int n_keys) {
  for (int k = 0; k < n_keys && k < kMaxKeys; k++) {
    const bool an = (a.nulls >> k) & 1u, bn = (b.nulls >> k) & 1u;
    if (an || bn) {
      if (an != bn) return bn;   // the one that is not NULL comes first
      continue;
    }
    const int c = ComparePart(kinds[k], a.lo[k], a.hi[k], b.lo[k], b.hi[k]);
    if (c != 0) return c < 0;
  }
  return false;
}

//! The host's group table: the groups of one list merged into another with aggmerge::Merge, in the order the caller
//! merges (MultiDeviceScan: device order).  Open addressing over the entries' indices; at most kMaxGroups groups.
class GroupTable {
 public:
  GroupTable(int n_keys, std::vector<int> ops, std::vector<int> classes)
      : n_keys_(n_keys), ops_(std::move(ops)), classes_(std::move(classes)), slots_(kSlots, -1) {}

  size_t size() const { return keys_.size(); }
  size_t n_aggs() const { return ops_.size(); }
  const Key& key(size_t g) const { return keys_[g]; }
  const aggmerge::Partial* partials(size_t g) const { return &partials_[g * ops_.size()]; }

  //! merges one group's partials (n_aggs of them) into the table; false: the key is new and the table is full
  bool Merge(const Key& k, const aggmerge::Partial* p) {
    Key n = k;   // (a caller's key may carry stale bits behind its parts)
    for (int i = n_keys_; i < kMaxKeys; i++) n.lo[i] = n.hi[i] = 0;
    uint32_t h = Hash(n, n_keys_) & (kSlots - 1);
    for (uint32_t probe = 0; probe < kSlots; probe++, h = (h + 1) & (kSlots - 1)) {
      const int32_t g = slots_[h];
      if (g < 0) {
        if (keys_.size() >= static_cast<size_t>(kMaxGroups)) return false;
        slots_[h] = static_cast<int32_t>(keys_.size());
        keys_.push_back(n);
        partials_.insert(partials_.end(), p, p + ops_.size());
        return true;
      }
      if (Equal(keys_[static_cast<size_t>(g)], n, n_keys_)) {
        for (size_t a = 0; a < ops_.size(); a++) aggmerge::Merge(ops_[a], classes_[a], &partials_[static_cast<size_t>(g) * ops_.size() + a], p[a]);
        return true;
      }
    }
    return false;
  }

  //! the groups' indices in the result order
  std::vector<uint32_t> Sorted(const int* kinds) const;

 private:
  static constexpr uint32_t kSlots = 2 * kMaxGroups;
  int n_keys_;
  std::vector<int> ops_, classes_;
  std::vector<int32_t> slots_;
  std::vector<Key> keys_;
  std::vector<aggmerge::Partial> partials_;
};

inline std::vector<uint32_t> GroupTable::Sorted(const int* kinds) const {
  std::vector<uint32_t> order(keys_.size());
  for (size_t i = 0; i < order.size(); i++) order[i] = static_cast<uint32_t>(i);
  // (the keys are distinct, so the order is total: any sort gives the same list)
  struct Less {
    const GroupTable* t;
    const int* kinds;
    bool operator()(uint32_t x, uint32_t y) const { return KeyLess(kinds, t->keys_[x], t->keys_[y], t->n_keys_); }
  };
  std::sort(order.begin(), order.end(), Less{this, kinds});
  return order;
}

}  // namespace groupkey
}  // namespace miarrow
