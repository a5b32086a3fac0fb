// union_format.hpp -- the rules of an Arrow union column (sparse or dense) on its way to a DuckDB UNION vector.  One header
// for hipcc and a plain C++ compiler, as group_key.hpp and agg_merge.hpp are: the schema decode (ipc_format.cpp), the planner
// (batch_planner.cpp), the lanes of transcode_union (kernels_union.hip: the table look-up, the table's layout, the status
// bits) and the stand-alone check under tests/sanitize/ all compile it.  RowRule states the rule for one row in one place;
// the kernel applies it in two rounds of loads (member and offset first, the validity bit they name second) and
// tests/union_cases.py restates it in numpy.
//
// A union of m members (1 .. kMaxMembers) names them by TYPE IDS, int8 values 0 .. 127 listed in Union.typeIds (absent: id =
// index).  The tag of a DuckDB UNION row is the MEMBER INDEX 0 .. m - 1: the position of the row's type id in that list, found
// through a table of 128 entries.  (DuckDB's own conversion takes the id for the index; for the ids 0 .. m - 1 that DuckDB and
// pyarrow write by default the two agree -- DESIGN.md section 2.)
//
// A row is NULL when its type id is no member (kStBadTag), when it is dense and its offset lies outside its member array
// (kStBadOffset), when its member's value is NULL, or when a struct parent is NULL there.  A NULL row has tag 0.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MI_UNION_FN __host__ __device__ __forceinline__
#else
#define MI_UNION_FN inline
#endif

namespace miarrow {
namespace unionfmt {

constexpr int kMaxMembers = 32;          // == MI_MAX_UNION_MEMBERS
constexpr int kTableEntries = 128;       // one per type id 0 .. 127
constexpr int kTableWords = kTableEntries / 8;
constexpr int kMemberWords = 4;          // {bitmap address, length, null_count, flags} per member behind the table
constexpr uint32_t kStBadTag = 8192u;    // == MI_ST_BAD_UNION_TAG
constexpr uint32_t kStBadOffset = 16384u;  // == MI_ST_BAD_UNION_OFFSET
constexpr uint64_t kMemberNullType = 1;  // member flags bit 0: arrow null type, every row NULL

// what CheckTypeIds found
enum TypeIdDefect { kIdsOk = 0, kIdsNoMembers, kIdsTooMany, kIdsCount, kIdsRange, kIdsTwice };

MI_UNION_FN const char* DefectText(int d) {
  switch (d) {
    case kIdsNoMembers: return "a union needs at least one member";
    case kIdsTooMany: return "more than 32 union members";
    case kIdsCount: return "the number of type ids differs from the number of children";
    case kIdsRange: return "a type id outside 0 .. 127";
    case kIdsTwice: return "a type id listed twice";
    default: return "";
  }
}

//! Union.typeIds against the field's children: n_ids < 0 = the list is absent (id = index)
MI_UNION_FN int CheckTypeIds(const int32_t* ids, int n_ids, int n_children) {
  if (n_children < 1) return kIdsNoMembers;
  if (n_children > kMaxMembers) return kIdsTooMany;
  if (n_ids < 0) return kIdsOk;
  if (n_ids != n_children) return kIdsCount;
  uint64_t seen[2] = {0, 0};
  for (int k = 0; k < n_ids; k++) {
    const int32_t id = ids[k];
    if (id < 0 || id >= kTableEntries) return kIdsRange;
    const uint64_t bit = 1ull << (id & 63);
    if (seen[id >> 6] & bit) return kIdsTwice;
    seen[id >> 6] |= bit;
  }
  return kIdsOk;
}

//! The id -> member table: table[id] = member index, -1 = no member.  `ids` as CheckTypeIds accepted them.
MI_UNION_FN void BuildTable(const int32_t* ids, int n_ids, int n_children, int8_t table[kTableEntries]) {
  for (int i = 0; i < kTableEntries; i++) table[i] = -1;
  for (int k = 0; k < n_children; k++) table[n_ids < 0 ? k : ids[k]] = static_cast<int8_t>(k);
}

//! member index of a row's type id, -1 when the id is negative or no member
MI_UNION_FN int MemberOfId(const int8_t* table, int8_t id) { return id < 0 ? -1 : table[static_cast<int>(id)]; }

struct Row {
  int tag;          // member index; 0 for a NULL row
  bool valid;
  uint32_t status;  // kStBadTag / kStBadOffset / 0
};

//! The rule for one row.  member = MemberOfId(...); dense: `offset` against the member's length (sparse rows pass dense =
//! false); value_valid = the selected member's value is not NULL (looked up only when member >= 0 and the offset is in range:
//! callers pass anything otherwise); parent_valid = the struct parent's bit.  A damaged row reports its status bit whatever
//! the parent says.
MI_UNION_FN Row RowRule(int member, bool dense, int64_t offset, int64_t member_length, bool value_valid, bool parent_valid) {
  if (member < 0) return Row{0, false, kStBadTag};
  if (dense && (offset < 0 || offset >= member_length)) return Row{0, false, kStBadOffset};
  if (!value_valid || !parent_valid) return Row{0, false, 0u};
  return Row{member, true, 0u};
}

// ---------------------------------------------------------------------------------------------------- the way back
// A DuckDB UNION vector -> an Arrow SPARSE union with the type ids 0 .. m - 1 (MI_K_ENC_UNION, kernels_encode_union.hip; the
// writer's staging in chunk_staging.cpp and tests/union_encode_cases.py restate it).  The union has no bitmap of its own: a row's
// NULL lives in its member.  So the pass writes the type id of every row and, per member, an EFFECTIVE validity mask that the
// member's own encode task takes for its validity.

struct EncodedRow {
  int type_id;      // == the tag; 0 for a NULL union row (ArrowUnionData::Append) and for a tag that names no member
  int member;       // whose mask may hold the row's bit: the tag clamped into 0 .. m - 1 (0 for a tag >= m)
  bool selects;     // the union row is valid and its tag names a member: bit r of mask `member` = selects && the member's own bit
  uint32_t status;  // kStBadTag / 0
};

//! The rule for one row.  `tag` as loaded (uint8); union_valid = the union's validity bit ANDed with a struct parent's.
//! A tag >= m under a valid row is reported and the row goes to member 0 as NULL; under a NULL row the tag is not looked at.
MI_UNION_FN EncodedRow EncodeRow(int tag, int m, bool union_valid) {
  if (!union_valid) return EncodedRow{0, 0, false, 0u};
  if (tag < 0 || tag >= m) return EncodedRow{0, 0, false, kStBadTag};
  return EncodedRow{tag, tag, true, 0u};
}

//! Word j of a mask over n rows: `bits` with the pad bits (rows >= n) set
MI_UNION_FN uint64_t WithPadBits(uint64_t bits, int64_t n, int64_t j) {
  const int64_t rem = n - 64 * j;
  return rem >= 64 ? bits : rem <= 0 ? ~0ull : bits | (~0ull << rem);
}

}  // namespace unionfmt
}  // namespace miarrow
