// Stand-alone check of duckdb-arrow_amd/csrc/union_format.hpp (the rules of an Arrow union column that the schema decode, the
// planner and the lanes of transcode_union all compile), meant to be built with -fsanitize=address,undefined:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I duckdb-arrow_amd/csrc tests/sanitize/union_format_check.cpp -o union_format_check
// Every check is against a restatement written here (a linear search of the type id list), never against the header itself.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "union_format.hpp"

using namespace miarrow::unionfmt;

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                     \
    }                                                                 \
  } while (0)

// the member of a type id by the format's own words: the position of the id in the list
static int MemberByList(const std::vector<int32_t>& ids, int id) {
  for (size_t k = 0; k < ids.size(); k++)
    if (ids[k] == id) return static_cast<int>(k);
  return -1;
}

static void CheckTable(const std::vector<int32_t>& ids) {
  const int m = static_cast<int>(ids.size());
  CHECK(CheckTypeIds(ids.data(), m, m) == kIdsOk);
  int8_t* table = static_cast<int8_t*>(std::malloc(kTableEntries));  // on the heap: a write past entry 127 is ASan's to see
  BuildTable(ids.data(), m, m, table);
  for (int id = -128; id <= 127; id++) {
    const int want = id < 0 ? -1 : MemberByList(ids, id);
    CHECK(MemberOfId(table, static_cast<int8_t>(id)) == want);
  }
  std::free(table);
}

int main() {
  static_assert(kMaxMembers == 32 && kTableEntries == 128 && kTableWords == 16 && kMemberWords == 4, "the contract of MI_K_UNION");
  static_assert(kStBadTag == 8192u && kStBadOffset == 16384u, "MI_ST_BAD_UNION_TAG / MI_ST_BAD_UNION_OFFSET");
  // ---- tables: every id -128 .. 127 against the list
  CheckTable({0, 1});
  CheckTable({5, 7});
  CheckTable({127, 0, 64});
  CheckTable({0});
  CheckTable({127});
  {
    std::vector<int32_t> ids;
    for (int k = 0; k < 32; k++) ids.push_back(k);
    CheckTable(ids);
    ids.clear();
    for (int k = 0; k < 32; k++) ids.push_back(127 - 4 * k);   // descending, sparse
    CheckTable(ids);
  }
  // typeIds absent: id = index
  for (int m = 1; m <= 32; m++) {
    CHECK(CheckTypeIds(nullptr, -1, m) == kIdsOk);
    int8_t table[kTableEntries];
    BuildTable(nullptr, -1, m, table);
    for (int id = -128; id <= 127; id++) CHECK(MemberOfId(table, static_cast<int8_t>(id)) == (id >= 0 && id < m ? id : -1));
  }
  // ---- the checks of typeIds
  {
    std::vector<int32_t> ids;
    for (int k = 0; k < 33; k++) ids.push_back(k);
    CHECK(CheckTypeIds(ids.data(), 33, 33) == kIdsTooMany);
    CHECK(CheckTypeIds(nullptr, -1, 33) == kIdsTooMany);
    CHECK(CheckTypeIds(ids.data(), 32, 32) == kIdsOk);
    CHECK(CheckTypeIds(nullptr, -1, 0) == kIdsNoMembers);
    CHECK(CheckTypeIds(ids.data(), 0, 0) == kIdsNoMembers);
    CHECK(CheckTypeIds(ids.data(), 3, 2) == kIdsCount);
    CHECK(CheckTypeIds(ids.data(), 1, 2) == kIdsCount);
    CHECK(CheckTypeIds(ids.data(), 0, 2) == kIdsCount);
  }
  for (int32_t bad : {-1, -128, 128, 255, 256, 1 << 20, INT32_MIN, INT32_MAX}) {
    const int32_t ids[3] = {3, bad, 4};
    CHECK(CheckTypeIds(ids, 3, 3) == kIdsRange);
  }
  for (int a = 0; a < 128; a++) {   // every id twice, at every distance that the two 64-bit halves of `seen` can hide
    const int32_t ids[3] = {a, (a + 64) % 128, a};
    CHECK(CheckTypeIds(ids, 3, 3) == kIdsTwice);
    const int32_t ok[2] = {a, (a + 64) % 128};
    CHECK(CheckTypeIds(ok, 2, 2) == kIdsOk);
  }
  for (int d = kIdsOk; d <= kIdsTwice; d++) CHECK((DefectText(d)[0] == 0) == (d == kIdsOk));
  // ---- the row rule
  for (int member = -2; member < 3; member++)
    for (int dense = 0; dense < 2; dense++)
      for (int64_t off : {int64_t(-1), int64_t(0), int64_t(4), int64_t(5), int64_t(2147483647)})
        for (int vv = 0; vv < 2; vv++)
          for (int pv = 0; pv < 2; pv++) {
            const Row r = RowRule(member, dense != 0, off, 5, vv != 0, pv != 0);
            const bool bad_tag = member < 0;
            const bool bad_off = !bad_tag && dense && (off < 0 || off >= 5);
            const bool valid = !bad_tag && !bad_off && vv && pv;
            CHECK(r.status == (bad_tag ? kStBadTag : bad_off ? kStBadOffset : 0u));
            CHECK(r.valid == valid);
            CHECK(r.tag == (valid ? member : 0));
          }
  if (failures) {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::printf("union_format: ok\n");
  return 0;
}
