// like_match.hpp -- contains / ends_with / %-pattern LIKE as the filter kernel (K6) and the host evaluate them.  One header
// for hipcc and a plain C++ compiler: the kernel (kLeafStrMatch), the host side of the filter (folding, dictionary match
// maps), mi_filter_like_match and the stand-alone check under tests/sanitize/ all compile these functions.  Nothing here
// allocates or touches a global.
//
// Rows and patterns are byte strings.  `%` is the only wildcard of LIKE (any run of bytes, the empty one included); `_` is
// refused, because it steps over UTF-8 characters and these are bytes; there is no escape character, so `\` is a byte.
// contains / ends_with take their constant literally.  A pattern is its literal segments -- the pattern split at `%`, empty
// pieces dropped, at most kMaxSegments -- and two anchors: at the head when it does not begin with `%`, at the tail when
// it does not end with `%`.  A row matches when
//   1. it is at least as long as all segments together,
//   2. an anchored head segment is a prefix of it,
//   3. an anchored tail segment is a suffix of it,
//   4. the remaining segments are found left to right, each at its leftmost occurrence at or behind the end of the
//      previous one, none reaching into the tail segment's bytes.
// Leftmost placement is exact for `%`-only patterns: moving a segment to an earlier occurrence never takes room from the
// ones behind it.  No byte at or behind row[row_len] is read, and every index handed to the row is below row_len.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define MI_LIKE_FN __host__ __device__ __forceinline__
#else
#define MI_LIKE_FN inline
#endif

namespace miarrow {
namespace likematch {

constexpr int kMaxSegments = 8;
// the operators, numbered as enum mi_filter_op numbers them
constexpr int32_t kOpContains = 11, kOpEndsWith = 12, kOpLike = 13, kOpNotLike = 14;
// what Compile answers
constexpr int kCompiled = 0, kUnknownOp = 1, kHasUnderscore = 2, kTooManySegments = 3;

//! A compiled pattern: the segments are stretches of the pattern's own bytes
struct Pattern {
  int32_t n_seg;
  bool head, tail;     // anchored: the first segment is a prefix / the last one a suffix of a matching row
  bool negate;         // NOT LIKE: a non-NULL row passes when it does not match
  uint32_t off[kMaxSegments], len[kMaxSegments];
};

inline int Compile(int32_t op, const uint8_t* bytes, uint32_t n, Pattern* out) {
  Pattern p = {};
  if (op == kOpContains || op == kOpEndsWith) {   // literal: one segment, or none (the empty constant matches every row)
    if (n > 0) {
      p.n_seg = 1;
      p.len[0] = n;
      p.tail = op == kOpEndsWith;
    }
    *out = p;
    return kCompiled;
  }
  if (op != kOpLike && op != kOpNotLike) return kUnknownOp;
  for (uint32_t i = 0; i < n; i++)
    if (bytes[i] == '_') return kHasUnderscore;
  p.negate = op == kOpNotLike;
  p.head = n == 0 || bytes[0] != '%';
  p.tail = n == 0 || bytes[n - 1] != '%';
  for (uint32_t i = 0; i < n;) {
    if (bytes[i] == '%') {
      i++;
      continue;
    }
    uint32_t e = i;
    while (e < n && bytes[e] != '%') e++;
    if (p.n_seg == kMaxSegments) return kTooManySegments;
    p.off[p.n_seg] = i;
    p.len[p.n_seg] = e - i;
    p.n_seg++;
    i = e;
  }
  *out = p;
  return kCompiled;
}

//! The segments of a compiled pattern over the pattern's bytes (host)
struct PatternSegments {
  const Pattern* p;
  const uint8_t* bytes;
  uint32_t len(int s) const { return p->len[s]; }
  uint8_t byte(int s, uint32_t i) const { return bytes[p->off[s] + i]; }
};

//! row[at .. at + len) equals segment s; the caller has made sure that at + len <= row_len
template <typename Segs, typename Row>
MI_LIKE_FN bool SegmentAt(const Segs& segs, int s, uint32_t len, const Row& row, uint32_t at) {
  for (uint32_t i = 0; i < len; i++)
    if (static_cast<uint8_t>(row[at + i]) != segs.byte(s, i)) return false;
  return true;
}

//! Does the row match?  `segs` gives len(s) and byte(s, i) of the n_seg segments (every len >= 1), `row` its bytes through
//! row[i], i < row_len: a plain pointer on the host, the row's registers or aligned dwords of its heap bytes in the kernel.
template <typename Segs, typename Row>
MI_LIKE_FN bool Matches(const Segs& segs, int n_seg, bool head, bool tail, const Row& row, uint32_t row_len) {
  uint64_t total = 0;
  for (int s = 0; s < n_seg; s++) total += segs.len(s);
  if (row_len < total) return false;
  if (n_seg == 0) return (head && tail) ? row_len == 0 : true;   // '' matches the empty row alone, '%' every row
  if (n_seg == 1 && head && tail && row_len != total) return false;
  uint32_t lo = 0, hi = row_len;   // the bytes [lo, hi) are still free
  int first = 0, last = n_seg;
  if (head) {
    const uint32_t l = segs.len(0);
    if (!SegmentAt(segs, 0, l, row, 0)) return false;
    lo = l;
    first = 1;
  }
  if (tail && last > first) {
    const uint32_t l = segs.len(last - 1);
    if (!SegmentAt(segs, last - 1, l, row, row_len - l)) return false;
    hi = row_len - l;
    last--;
  }
  for (int s = first; s < last; s++) {
    const uint32_t l = segs.len(s);
    if (hi - lo < l) return false;
    const uint32_t end = hi - l;   // the last place the segment can begin
    uint32_t j = lo;
    while (j <= end && !SegmentAt(segs, s, l, row, j)) j++;
    if (j > end) return false;
    lo = j + l;
  }
  return true;
}

//! Host: does the row pass the compiled pattern (NULL rows are the caller's: they pass nothing)
inline bool Passes(const Pattern& p, const uint8_t* pattern_bytes, const uint8_t* row, uint32_t row_len) {
  const PatternSegments segs = {&p, pattern_bytes};
  return Matches(segs, p.n_seg, p.head, p.tail, row, row_len) != p.negate;
}

}  // namespace likematch
}  // namespace miarrow
