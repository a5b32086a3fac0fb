// scan_dictionary.hpp -- one version of a decoded dictionary: what the scan keeps of it (DictState) and the host side of
// building it from a DictionaryBatch (scan_dictionary.cpp: plain functions over the bytes of the message, no HIP call).  The
// device sequence around them is ArrowScan::DecodeDictionary (scan_operator.cpp).
#pragma once

#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "batch_slice.hpp"
#include "engine.hpp"
#include "scan_column.hpp"

namespace miarrow {

//! What a dictionary version keeps of its values on the host, for pushed-down predicates: the dictionary is matched once,
//! on the host, the rows by index (K6, kLeafDictMap)
struct DictHostValues {
  //! string-valued dictionaries: the values themselves (empty + not valid for NULL entries)
  std::vector<std::string> host_strings;
  std::vector<char> host_valid;        // per entry (dict_len of them)
  //! FLOAT / DOUBLE / 128-bit dictionaries: the decoded values (out_width bytes each)
  std::vector<uint8_t> host_values;
};

//! One immutable version of a decoded dictionary (dict_len + 1 entries, the last one NULL).  Record batches keep the
//! version they were enqueued with, so a later replacement / delta never changes what an in-flight batch sees.
struct DictState : DictHostValues {
  DeviceBuffer d_data;           // decoded values on the device
  DeviceBuffer d_validity;
  PinnedBuffer h_data;           // pinned host copy (host consumers)
  void* h_validity = nullptr;    // == h_words for host consumers
  PinnedBuffer h_words;          // the validity words (uint64_t) as built on the host (uploaded from here)
  PinnedBuffer h_status;         // status word (uint32_t) of the decode of the values, checked with the first batch that uses them
  HipEvent uploaded;             // the dictionary body is in HBM
  std::unique_ptr<Plan> decode_plan;   // kept until the version dies: its status word is read asynchronously
  std::vector<std::shared_ptr<void>> d_heaps;      // device copies of the dictionary bodies (long string payload)
  std::vector<std::shared_ptr<void>> host_bodies;  // host bodies: long dictionary strings point into them
  int64_t dict_len = 0;
  int32_t kind = 0, out_width = 0;
  std::map<size_t, std::shared_ptr<void>> match_maps;   // filter leaf -> device byte per entry: 0 no, 1 yes, 2 NULL
};

//! The value kinds a dictionary may have: its values are decoded as ONE flat task, so value types that need more than
//! {validity, buffer 1, buffer 2} (string views: a table of variadic buffers; lists / structs: child nodes) are not among them
bool DictionaryKindIsFlat(int32_t kind);

//! binary16 -> the bits of the binary32 with the same value (exact: every half is a float)
uint32_t HalfToFloatBits(uint16_t h);

//! The host side of a dictionary version, from DictionaryBatch `b` (its one column: validity, buffer 1, buffer 2), whose values
//! decode as `kind` / `width` / `param` (ArrowField::Plan, value_only).  `old`: the version a delta extends, or NULL.
//!   words        validity of the old entries, then of the new ones, one bit each; every other bit of the `n_words` words is
//!                set -- the extra NULL entry at index dict_len included, which the caller clears
//!   out->host_valid     the same, one char per entry
//!   out->host_strings   string kinds: old values then new ones, offsets checked against the payload
//!   out->host_values    `keep_values` (the column can be compared by a filter: FLOAT / DOUBLE / 128-bit): old then new, decoded
//! Every read of the body is checked against the span it comes from; a span that is too short raises InternalException.
void BuildDictionaryHost(const DecodedBatch& b, int32_t kind, int32_t width, int64_t param, bool keep_values, const DictHostValues* old,
                         uint64_t* words, size_t n_words, DictHostValues* out);

}  // namespace miarrow
