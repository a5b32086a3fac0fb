// hash_group.hpp -- the rules of the hash GROUP BY for many groups (K11: mi_scan_hash_aggregate, mi_hash_aggregate_vectors;
// kernels_hash_group.hip).  One header for hipcc and a plain C++ compiler, as group_key.hpp is: the lanes of hash_group_rows
// and hash_group_collect, the host's merge of the per-device group lists (MultiDeviceScan::HashAggregate) and the
// stand-alone check under tests/sanitize/ all compile these functions.
//
// The key is ONE column of groupkey::kKeySigned / kKeyUnsigned, normalised by groupkey::NormInteger; its low word `lo` is the
// key word (within one column `hi` is a function of `lo`: the sign extension, or 0).  A key of one 64-bit word is claimed in
// the table by one compare-and-swap and is complete the moment it is claimed; a wider key would need a claim followed by a
// publication, and lanes that wait for it.  Nothing here waits.
//
// The table, in HBM, for max_groups groups (1 .. kMaxHashGroups) and n_aggs aggregates:
//   head      kHeadWords uint32: [kHeadGroups] the groups claimed so far, [kHeadStatus] MI_ST_* bits (atomic OR),
//             [kHeadCollected] the records hash_group_collect has handed out, [kHeadExtra + e] 1 once extra record e is in use
//   keys      SlotsFor(max_groups) = max(64, the power of two >= 2 * max_groups) key words, kEmptyKey = free
//   records   (slots + kExtraRecords) * n_aggs records of kRecordWords uint64 {lo, hi, count}: slot s owns records
//             [s * n_aggs, (s + 1) * n_aggs).  The two records behind the probed range belong to the NULL key (kExtraNull)
//             and to the key whose word IS kEmptyKey (kExtraEmptyKey); neither is ever probed for.
//   TableBytes(max_groups, n_aggs) = 4 * kHeadWords + 8 * slots + 8 * kRecordWords * (slots + 2) * n_aggs
// A record, by the operation:
//   COUNT(*) / COUNT   count alone
//   SUM (all three)    {lo, hi} the 128-bit two's-complement sum modulo 2^128: a returning add on lo, then one add on hi of
//                      the value's high word plus CarryOf(what lo held, what was added) -- every wrap of lo is counted once
//   MIN / MAX          lo = the least / greatest OrderedWord of the contributors (unsigned 64-bit order); it starts as
//                      RecordInit(op): all ones for MIN, zero for MAX.  hi is not used.
//   count == 0 is the NULL rule, as everywhere (agg_merge.hpp).
// Only merges that are exact in any order are taken (HashProgramIsValid): no floating-point sum, no 128-bit MIN / MAX.
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "agg_merge.hpp"
#include "group_key.hpp"

namespace miarrow {
namespace hashgroup {

constexpr uint32_t kMaxHashGroups = 1u << 24;   // == MI_MAX_HASH_GROUPS
constexpr uint64_t kEmptyKey = ~0ull;           // the key word of a free slot (the int64 -1: its group lives in an extra record)
constexpr uint32_t kExtraNull = 0, kExtraEmptyKey = 1, kExtraRecords = 2;
constexpr uint32_t kHeadGroups = 0, kHeadStatus = 1, kHeadCollected = 2, kHeadExtra = 4, kHeadWords = 8;
constexpr uint32_t kRecordWords = 3;            // {lo, hi, count}
constexpr uint64_t kSignBit = 0x8000000000000000ull;

//! the table's key words: a power of two, at least 64, at least twice the groups (load factor <= 1 / 2)
MI_KEY_FN uint32_t SlotsFor(uint32_t max_groups) {
  uint32_t s = 64;
  while (s < 2u * max_groups && s < (1u << 31)) s <<= 1;
  return s;
}

MI_KEY_FN size_t TableBytes(uint32_t max_groups, int n_aggs) {
  const size_t slots = SlotsFor(max_groups);
  return 4u * kHeadWords + 8u * slots + 8u * kRecordWords * (slots + kExtraRecords) * static_cast<size_t>(n_aggs);
}

//! the 64-bit hash of a key word: two rounds of xor-shift and multiplication by an odd constant (the fractional bits of
//! sqrt 2 and sqrt 3), each a bijection of the 64-bit words; the slot is the low bits, which the last shift fills from above
MI_KEY_FN uint64_t Hash(uint64_t key) {
  uint64_t x = key ^ (key >> 31);
  x *= 0x6A09E667F3BCC909ull;
  x ^= x >> 29;
  x *= 0xBB67AE8584CAA73Bull;
  x ^= x >> 32;
  return x;
}

//! what the add on `hi` takes besides the value's high word: 1 when `old + added` wrapped
MI_KEY_FN uint64_t CarryOf(uint64_t old, uint64_t added) { return old + added < old ? 1ull : 0ull; }

//! the word MIN / MAX order a contributor by, unsigned: `lo` is what the row fold hands over -- the sign- or zero-extended
//! integer, or aggmerge::CanonicalBits of a double
MI_KEY_FN uint64_t OrderedWord(int cls, uint64_t lo) {
  if (cls == aggmerge::kClassFloat) return static_cast<uint64_t>(filterkey::FloatKey(static_cast<int64_t>(lo))) ^ kSignBit;
  return cls == aggmerge::kClassUnsigned ? lo : lo ^ kSignBit;
}
//! ... and back: {lo, hi} as a Partial holds a minimum / maximum (canonical bits for a double, hi the extension otherwise)
MI_KEY_FN void FromOrderedWord(int cls, uint64_t word, uint64_t* lo, uint64_t* hi) {
  *hi = 0;
  if (cls == aggmerge::kClassFloat) {
    const int64_t k = static_cast<int64_t>(word ^ kSignBit), max = 0x7FFFFFFFFFFFFFFFll;
    *lo = k == max ? aggmerge::kCanonicalNaN : static_cast<uint64_t>(k >= 0 ? k : k ^ max);
    return;
  }
  if (cls == aggmerge::kClassUnsigned) {
    *lo = word;
    return;
  }
  *lo = word ^ kSignBit;
  *hi = (*lo >> 63) ? ~0ull : 0ull;
}
//! what a record's lo starts as
MI_KEY_FN uint64_t RecordInit(int op) { return op == aggmerge::kOpMin ? ~0ull : 0ull; }

//! the high word of a normalised key of class `key_cls` whose low word is `lo`
MI_KEY_FN uint64_t KeyHigh(int key_cls, uint64_t lo) { return key_cls == groupkey::kKeySigned && (lo >> 63) ? ~0ull : 0ull; }

//! one key column of 1 / 2 / 4 / 8 bytes, signed or unsigned; 1 .. 8 aggregates of K9's operations whose merge is exact in
//! any order: classes[a] is the class SUM / MIN / MAX read (for a product or an expression: of its factors)
MI_KEY_FN bool HashProgramIsValid(int key_cls, int key_width, int n_aggs, const int* ops, const int* classes) {
  if (key_cls != groupkey::kKeySigned && key_cls != groupkey::kKeyUnsigned) return false;
  if (key_width != 1 && key_width != 2 && key_width != 4 && key_width != 8) return false;
  if (n_aggs < 1 || n_aggs > aggmerge::kMaxAggregates) return false;
  for (int a = 0; a < n_aggs; a++) {
    const int op = ops[a], cls = classes[a];
    if (op < aggmerge::kOpCountStar || op > aggmerge::kOpSumExpr) return false;
    if (op == aggmerge::kOpCountStar || op == aggmerge::kOpCount) continue;
    if (op == aggmerge::kOpMin || op == aggmerge::kOpMax) {
      if (cls != aggmerge::kClassSigned && cls != aggmerge::kClassUnsigned && cls != aggmerge::kClassFloat) return false;
    } else if (cls != aggmerge::kClassSigned && cls != aggmerge::kClassUnsigned) {
      return false;   // a sum in arrival order: integers only
    }
  }
  return true;
}

//! The table as one thread would fill it: (key word, NULL bit, n_aggs partials) records merged with aggmerge::Merge in the
//! order the caller merges (MultiDeviceScan: device order).  Same slots, same hash, same two extra records, same limit.
//! Host code only: it has no device function.  (It is declared in both passes of hipcc, as groupkey::GroupTable is, because
//! the host translation units that use it are compiled by hipcc and their bodies are parsed in the device pass too.)
class SerialTable {
 public:
  SerialTable(uint32_t max_groups, std::vector<int> ops, std::vector<int> classes)
      : max_groups_(max_groups), mask_(SlotsFor(max_groups) - 1), ops_(std::move(ops)), classes_(std::move(classes)),
        slots_(static_cast<size_t>(mask_) + 1, kEmptyKey), group_of_(static_cast<size_t>(mask_) + 1 + kExtraRecords, -1) {}

  size_t size() const { return keys_.size(); }
  uint64_t key(size_t g) const { return keys_[g]; }
  bool is_null(size_t g) const { return nulls_[g] != 0; }
  const aggmerge::Partial* partials(size_t g) const { return &partials_[g * ops_.size()]; }

  //! false: the key is new and the table holds max_groups groups already
  bool Merge(uint64_t key, bool is_null, const aggmerge::Partial* p) {
    size_t at;
    if (is_null) {
      at = static_cast<size_t>(mask_) + 1 + kExtraNull;
      key = 0;
    } else if (key == kEmptyKey) {
      at = static_cast<size_t>(mask_) + 1 + kExtraEmptyKey;
    } else {
      uint32_t h = static_cast<uint32_t>(Hash(key)) & mask_;
      uint32_t probe = 0;
      for (; probe <= mask_ && slots_[h] != kEmptyKey && slots_[h] != key; probe++) h = (h + 1) & mask_;
      if (probe > mask_) return false;
      at = h;
    }
    int64_t g = group_of_[at];
    if (g < 0) {
      if (keys_.size() >= max_groups_) return false;
      if (at <= mask_) slots_[at] = key;
      g = static_cast<int64_t>(keys_.size());
      group_of_[at] = g;
      keys_.push_back(key);
      nulls_.push_back(is_null ? 1 : 0);
      partials_.insert(partials_.end(), ops_.size(), aggmerge::Partial{0, 0, 0, 0});
    }
    for (size_t a = 0; a < ops_.size(); a++) aggmerge::Merge(ops_[a], classes_[a], &partials_[static_cast<size_t>(g) * ops_.size() + a], p[a]);
    return true;
  }

 private:
  uint32_t max_groups_, mask_;
  std::vector<int> ops_, classes_;
  std::vector<uint64_t> slots_;
  std::vector<int64_t> group_of_;
  std::vector<uint64_t> keys_;
  std::vector<uint8_t> nulls_;
  std::vector<aggmerge::Partial> partials_;
};

}  // namespace hashgroup
}  // namespace miarrow
