// plan_layout_check.cpp -- the kind table (duckdb-arrow_amd/csrc/task_kind.hpp) and the plan layout
// (duckdb-arrow_amd/csrc/plan_layout.cpp) without a GPU, under AddressSanitizer + UBSan (test infrastructure, never shipped).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include
//       tests/sanitize/plan_layout_check.cpp duckdb-arrow_amd/csrc/plan_layout.cpp duckdb-arrow_amd/csrc/ipc_format.cpp
//
// Every expected value below is a literal, worked out by hand from the rules of a plan: one slice per (pass, depth, slot) that
// has tasks -- pass 0 the seven classes in enum order and then the union tag passes, pass 1 run-end and then dense-union
// expansions, pass 2 string-view encode; stable inside a slice; ceil(rows / 2048) tiles per task; encode tasks at depth 0 with
// param2 = their NULL-counter slot in caller order -- and from the per-kind switches this table replaced.  Task pointers are
// made-up addresses: a layout looks at their alignment and never follows them.
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../../duckdb-arrow_amd/csrc/extension_format.hpp"
#include "../../duckdb-arrow_amd/csrc/ipc_format.hpp"
#include "../../duckdb-arrow_amd/csrc/plan_layout.hpp"

using namespace miarrow;
using namespace miarrow::device;

static_assert(kCopyTileRows == 2048 && kDecTileRows == 2048 && kVectorRows == 2048, "the tile counts below are written out for 2048-row tiles");

namespace {
int g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                    \
  do {                                      \
    g_checks++;                             \
    if (!(cond)) {                          \
      std::fprintf(stderr, "FAILED: ");     \
      std::fprintf(stderr, __VA_ARGS__);    \
      std::fprintf(stderr, "\n");           \
      g_failed++;                           \
    }                                       \
  } while (0)

// a made-up device address, 256-byte aligned; `plus` bytes further to misalign it
void* A(int n, int plus = 0) { return reinterpret_cast<void*>(static_cast<uintptr_t>(0x100000 + 0x100 * n + plus)); }

// ------------------------------------------------------------------------------------------------ kind table
struct KindRow {
  int kind, cls, slot, group;
  bool gather;
};
// every integer from 0 to one past MI_K_ENC_UUID_TEXT; class / slot -1 and gather false where the parent's switches fell to default
const KindRow kKinds[] = {
    {0, -1, -1, 2, false},
    {MI_K_COPY, 0, 0, 2, true},
    {MI_K_BOOL, 3, 3, 0, true},
    {MI_K_DEC128, 1, 1, 2, true},
    {MI_K_DATE64, 3, 3, 3, true},
    {MI_K_MUL_I32, 3, 3, 0, true},
    {MI_K_MUL_I64, 3, 3, 3, true},
    {MI_K_DIV_I64, 3, 3, 3, true},
    {MI_K_STR32, 2, 2, 2, true},
    {MI_K_STR64, 2, 2, 2, true},
    {MI_K_DICT, 3, 3, 0, true},
    {MI_K_FIXED_BINARY, 2, 2, 2, true},
    {MI_K_DURATION, 3, 3, 2, false},
    {MI_K_INTERVAL_MONTHS, 3, 3, 2, false},
    {MI_K_INTERVAL_MDN, 3, 3, 2, false},
    {MI_K_NARROW, 3, 3, 2, false},
    {MI_K_HALF_FLOAT, 3, 3, 2, false},
    {MI_K_NULL, 3, 3, 2, false},
    {MI_K_STRVIEW, 3, 3, 1, false},
    {MI_K_LIST32, 3, 3, 1, false},
    {MI_K_LIST64, 3, 3, 1, false},
    {MI_K_STRUCT, 3, 3, 1, false},
    {MI_K_RUN_END, -1, 7, 2, false},
    {MI_K_UNION, -1, 9, 2, false},
    {MI_K_UNION_DENSE, -1, 10, 2, false},
    {MI_K_UUID, 3, 3, 2, true},
    {MI_K_BOOL8, 3, 3, 2, true},
    {27, -1, -1, 2, false}, {28, -1, -1, 2, false}, {29, -1, -1, 2, false}, {30, -1, -1, 2, false}, {31, -1, -1, 2, false},
    {MI_K_ENC_COPY, 4, 4, 2, false},
    {MI_K_ENC_DEC128, 4, 4, 2, false},
    {MI_K_ENC_BOOL, 4, 4, 2, false},
    {MI_K_ENC_STR32, 5, 5, 2, false},
    {MI_K_ENC_VALIDITY, 4, 4, 2, false},
    {MI_K_ENC_LIST32, 5, 5, 2, false},
    {MI_K_ENC_STRVIEW, -1, 8, 2, false},
    {MI_K_ENC_UUID_TEXT, 4, 4, 2, false},
    {40, -1, -1, 2, false},
};

void CheckKindTable() {
  static_assert(kClassCopy == 0 && kClassDec128 == 1 && kClassString == 2 && kClassMisc == 3 && kClassEncFixed == 4 && kClassEncString == 5 &&
                    kClassGather == 6 && kNumClasses == 7 && kSlotRunEnd == 7 && kSlotEncView == 8 && kSlotUnionTags == 9 && kSlotUnionDense == 10,
                "the numbers the C ABI reports classes by");
  CHECK(sizeof(kKinds) / sizeof(kKinds[0]) == 41, "the table has %zu rows", sizeof(kKinds) / sizeof(kKinds[0]));
  int k = 0;
  for (const KindRow& r : kKinds) {
    CHECK(r.kind == k, "row %d of the table is kind %d", k, r.kind);
    k++;
    CHECK(ClassOfKind(r.kind) == r.cls, "ClassOfKind(%d) = %d, not %d", r.kind, ClassOfKind(r.kind), r.cls);
    CHECK(SlotOfKind(r.kind) == r.slot, "SlotOfKind(%d) = %d, not %d", r.kind, SlotOfKind(r.kind), r.slot);
    CHECK(MiscGroupOfKind(r.kind) == r.group, "MiscGroupOfKind(%d) = %d, not %d", r.kind, MiscGroupOfKind(r.kind), r.group);
    CHECK(KindCanGather(r.kind) == r.gather, "KindCanGather(%d) = %d", r.kind, KindCanGather(r.kind));
  }
  CHECK(ClassOfKind(-1) == -1 && SlotOfKind(-1) == -1 && !KindCanGather(-1) && OutWidth(-1, 8) == 0, "kind -1");
  // the slot table: pass, position, accounting class, tile rows
  const int slots[11][4] = {{0, 0, 0, 2048}, {0, 1, 1, 2048}, {0, 2, 2, 2048}, {0, 3, 3, 2048}, {0, 4, 4, 2048}, {0, 5, 5, 2048},
                            {0, 6, 6, 2048}, {1, 0, 3, 2048}, {2, 0, 5, 2048}, {0, 7, 3, 2048}, {1, 1, 3, 2048}};
  CHECK(kNumSlots == 11, "%d slots", static_cast<int>(kNumSlots));
  for (int s = 0; s < 11; s++)
    CHECK(kSlots[s].pass == slots[s][0] && kSlots[s].position == slots[s][1] && kSlots[s].cls == slots[s][2] && kSlots[s].tile_rows == slots[s][3],
          "slot %d is {%d, %d, %d, %d}", s, kSlots[s].pass, kSlots[s].position, kSlots[s].cls, kSlots[s].tile_rows);
  const char* names[7] = {"transcode_copy", "transcode_dec128", "transcode_string", "transcode_misc_light", "encode_fixed", "encode_string_1p", "transcode_gather"};
  for (int c = 0; c < 7; c++) CHECK(std::string(KernelNameOfClass(c)) == names[c], "class %d is named %s", c, KernelNameOfClass(c));
  CHECK(std::string(KernelNameOfClass(-1)).empty() && std::string(KernelNameOfClass(7)).empty(), "classes that do not exist have no name");

  // OutWidth over the parameters each kind admits
  for (int64_t w : {1, 2, 4, 8, 16}) {
    CHECK(OutWidth(MI_K_COPY, w) == w, "COPY %lld", (long long)w);
    CHECK(OutWidth(MI_K_UNION_DENSE, w) == w, "UNION_DENSE %lld", (long long)w);
    for (int64_t rw : {2, 4, 8}) CHECK(OutWidth(MI_K_RUN_END, rw | (w << 8)) == w, "RUN_END %lld over %lld", (long long)w, (long long)rw);
  }
  for (int64_t w : {2, 4, 8}) CHECK(OutWidth(MI_K_DEC128, w) == w, "DEC128 %lld", (long long)w);
  CHECK(OutWidth(MI_K_NARROW, 4 | (2 << 8)) == 2 && OutWidth(MI_K_NARROW, 8 | (2 << 8)) == 2 && OutWidth(MI_K_NARROW, 8 | (4 << 8)) == 4, "NARROW");
  for (int64_t iw : {1, 2, 4, 8}) CHECK(OutWidth(MI_K_DICT, iw) == 4 && OutWidth(MI_K_DICT, iw | (1 << 8)) == 4, "DICT %lld", (long long)iw);
  const int fixed[][2] = {{MI_K_BOOL, 1}, {MI_K_BOOL8, 1}, {MI_K_NULL, 1}, {MI_K_UNION, 1}, {MI_K_DATE64, 4}, {MI_K_HALF_FLOAT, 4}, {MI_K_MUL_I32, 8},
                          {MI_K_MUL_I64, 8}, {MI_K_DIV_I64, 8}, {MI_K_STR32, 16}, {MI_K_STR64, 16}, {MI_K_FIXED_BINARY, 16}, {MI_K_DURATION, 16},
                          {MI_K_INTERVAL_MONTHS, 16}, {MI_K_INTERVAL_MDN, 16}, {MI_K_STRVIEW, 16}, {MI_K_LIST32, 16}, {MI_K_LIST64, 16}, {MI_K_UUID, 16},
                          {MI_K_STRUCT, 0}, {0, 0}, {27, 0}, {31, 0}, {40, 0}, {MI_K_ENC_COPY, 0}, {MI_K_ENC_DEC128, 0}, {MI_K_ENC_BOOL, 0}, {MI_K_ENC_STR32, 0},
                          {MI_K_ENC_VALIDITY, 0}, {MI_K_ENC_LIST32, 0}, {MI_K_ENC_STRVIEW, 0}, {MI_K_ENC_UUID_TEXT, 0}};
  for (auto& f : fixed)
    for (int64_t param : {0, 1, 5, 1000, 1000000, -1000})
      CHECK(OutWidth(f[0], param) == f[1], "OutWidth(%d, %lld) = %d, not %d", f[0], (long long)param, OutWidth(f[0], param), f[1]);
}

// ------------------------------------------------------------------------------------------------ ArrowField::Plan against OutWidth
ArrowField Field(int32_t type) {
  ArrowField f;
  f.name = "f";
  f.type = type;
  return f;
}

void CheckPlanWidths() {
  std::vector<ArrowField> fields;
  auto add = [&](int32_t type, auto&& fill) {
    ArrowField f = Field(type);
    fill(f);
    fields.push_back(f);
  };
  for (int bits : {8, 16, 32, 64}) {
    add(MI_AT_INT, [&](ArrowField& f) { f.bit_width = bits; f.is_signed = true; });
    add(MI_AT_UTF8, [&](ArrowField& f) { f.has_dictionary = true; f.dict_index_bit_width = bits; });                       // dictionary indices
    add(MI_AT_INT, [&](ArrowField& f) { f.bit_width = 64; f.has_dictionary = true; f.dict_index_bit_width = bits; f.dict_index_signed = false; });
  }
  add(MI_AT_FIXED_BINARY, [](ArrowField& f) { f.byte_width = 16; f.extension = extfmt::kUuid; });
  add(MI_AT_INT, [](ArrowField& f) { f.bit_width = 8; f.is_signed = true; f.extension = extfmt::kBool8; });
  add(MI_AT_UTF8, [](ArrowField& f) { f.extension = extfmt::kJson; });   // json: a string column like any other
  add(MI_AT_NULL, [](ArrowField&) {});
  for (int p : {0, 1, 2}) add(MI_AT_FLOAT, [&](ArrowField& f) { f.precision = p; });
  add(MI_AT_BOOL, [](ArrowField&) {});
  const int decimals[][2] = {{32, 4}, {32, 9}, {64, 4}, {64, 9}, {64, 18}, {128, 4}, {128, 9}, {128, 18}, {128, 19}, {128, 38}};   // narrow, same width, 128-bit
  for (auto& d : decimals) add(MI_AT_DECIMAL, [&](ArrowField& f) { f.bit_width = d[0]; f.precision = d[1]; f.scale = 2; });
  for (int u : {0, 1}) add(MI_AT_DATE, [&](ArrowField& f) { f.unit = u; });
  for (int u : {0, 1, 2, 3}) {
    add(MI_AT_TIME, [&](ArrowField& f) { f.unit = u; });
    add(MI_AT_TIMESTAMP, [&](ArrowField& f) { f.unit = u; });
    add(MI_AT_TIMESTAMP, [&](ArrowField& f) { f.unit = u; f.timezone = "UTC"; });
    add(MI_AT_DURATION, [&](ArrowField& f) { f.unit = u; });
  }
  for (int u : {0, 2}) add(MI_AT_INTERVAL, [&](ArrowField& f) { f.unit = u; });
  for (int t : {MI_AT_UTF8, MI_AT_BINARY, MI_AT_LARGE_UTF8, MI_AT_LARGE_BINARY, MI_AT_UTF8_VIEW, MI_AT_BINARY_VIEW, MI_AT_STRUCT}) add(t, [](ArrowField&) {});
  add(MI_AT_FIXED_BINARY, [](ArrowField& f) { f.byte_width = 7; });
  ArrowField i32 = Field(MI_AT_INT), utf8 = Field(MI_AT_UTF8), i16 = Field(MI_AT_INT);
  i32.bit_width = 32;
  i32.is_signed = true;
  i16.bit_width = 16;
  i16.is_signed = true;
  for (int t : {MI_AT_LIST, MI_AT_MAP, MI_AT_LARGE_LIST}) add(t, [&](ArrowField& f) { f.children = {i32}; });
  add(MI_AT_FIXED_LIST, [&](ArrowField& f) { f.byte_width = 3; f.children = {i32}; });
  for (int bits : {16, 32, 64})
    for (const ArrowField& values : {i32, utf8, i16}) {
      ArrowField ends = Field(MI_AT_INT);
      ends.bit_width = bits;
      ends.is_signed = true;
      add(MI_AT_RUN_END, [&](ArrowField& f) { f.children = {ends, values}; });
    }
  for (int mode : {0, 1}) add(MI_AT_UNION, [&](ArrowField& f) { f.unit = mode; f.children = {i32, utf8, i16}; });

  int kinds_seen[41] = {0};
  for (const ArrowField& f : fields) {
    int32_t kind = -1, width = -1;
    int64_t param = -1;
    const bool ok = f.Plan(&kind, &param, &width);
    CHECK(ok, "Plan refuses a field of type %d", f.type);
    if (!ok) continue;
    CHECK(OutWidth(kind, param) == width, "type %d: Plan gives kind %d param %lld out_width %d, OutWidth says %d", f.type, kind, (long long)param, width,
          OutWidth(kind, param));
    if (kind >= 0 && kind <= 40) kinds_seen[kind]++;
  }
  // every decode kind Plan can name was reached (UNION_DENSE is the scan's, not Plan's)
  for (int k = MI_K_COPY; k <= MI_K_BOOL8; k++)
    if (k != MI_K_UNION_DENSE) CHECK(kinds_seen[k] > 0, "no field above plans as kind %d", k);
  // the value plan of a dictionary field is the value type's
  ArrowField d = Field(MI_AT_UTF8);
  d.has_dictionary = true;
  int32_t kind, width;
  int64_t param;
  CHECK(d.Plan(&kind, &param, &width, true) && kind == MI_K_STR32 && width == 16 && OutWidth(kind, param) == 16, "dictionary values");
}

// ------------------------------------------------------------------------------------------------ layouts
struct SliceRow {
  int slot, depth, first_task, n_tasks, tile_begin_at, tile_task_at;
  uint32_t total_tiles, kernel_mask;
};

void CheckSlices(const char* what, const PlanLayout& l, const std::vector<SliceRow>& want) {
  CHECK(l.slices.size() == want.size(), "%s: %zu slices, not %zu", what, l.slices.size(), want.size());
  for (size_t i = 0; i < want.size() && i < l.slices.size(); i++) {
    const ClassSlice& s = l.slices[i];
    const SliceRow& w = want[i];
    CHECK(s.slot == w.slot && s.depth == w.depth, "%s: slice %zu is (slot %d, depth %d), not (%d, %d)", what, i, s.slot, s.depth, w.slot, w.depth);
    CHECK(s.first_task == w.first_task && s.n_tasks == w.n_tasks, "%s: slice %zu holds tasks %d + %d, not %d + %d", what, i, s.first_task, s.n_tasks,
          w.first_task, w.n_tasks);
    CHECK(s.tile_begin_at == w.tile_begin_at && s.tile_task_at == static_cast<size_t>(w.tile_task_at), "%s: slice %zu tables at %d / %zu, not %d / %d", what, i,
          s.tile_begin_at, s.tile_task_at, w.tile_begin_at, w.tile_task_at);
    CHECK(s.total_tiles == w.total_tiles, "%s: slice %zu has %u tiles, not %u", what, i, s.total_tiles, w.total_tiles);
    CHECK(s.kernel_mask == w.kernel_mask, "%s: slice %zu has kernel_mask %u, not %u", what, i, s.kernel_mask, w.kernel_mask);
  }
}

template <typename T, typename U>
void CheckArray(const char* what, const char* name, const T* got, size_t n_got, const std::vector<U>& want) {
  CHECK(n_got == want.size(), "%s: %s has %zu entries, not %zu", what, name, n_got, want.size());
  for (size_t i = 0; i < want.size() && i < n_got; i++)
    CHECK(static_cast<long long>(got[i]) == static_cast<long long>(want[i]), "%s: %s[%zu] = %lld, not %lld", what, name, i, (long long)got[i], (long long)want[i]);
}

// caller index i carries row_offset 1000 + i (no rule and no counter depends on it)
void CheckOrder(const char* what, const PlanLayout& l, const std::vector<std::pair<int, int>>& want) {
  CHECK(l.order.size() == want.size() && l.tasks.size() == want.size(), "%s: order has %zu entries, tasks %zu", what, l.order.size(), l.tasks.size());
  for (size_t i = 0; i < want.size() && i < l.order.size(); i++) {
    CHECK(l.order[i].first == want[i].first && l.order[i].second == want[i].second, "%s: task %zu went to (%d, %d), not (%d, %d)", what, i, l.order[i].first,
          l.order[i].second, want[i].first, want[i].second);
    if (l.order[i].first < 0 || static_cast<size_t>(l.order[i].first) >= l.slices.size()) continue;
    const size_t at = static_cast<size_t>(l.slices[static_cast<size_t>(l.order[i].first)].first_task + l.order[i].second);
    CHECK(at < l.tasks.size() && l.tasks[at].row_offset == 1000 + static_cast<int64_t>(i), "%s: order[%zu] names another task", what, i);
  }
}

mi_col_task Task(int32_t kind, int32_t depth, int64_t nrows, int64_t param = 0) {
  mi_col_task t = {};
  t.kind = kind;
  t.depth = depth;
  t.nrows = nrows;
  t.param = param;
  t.buf1 = A(1);
  t.out_data = A(2);
  t.out_validity = A(3);
  return t;
}

std::vector<mi_col_task> MixedDecodeTasks() {
  std::vector<mi_col_task> v;
  mi_col_task t;
  t = Task(MI_K_UNION_DENSE, 1, 2049, 4);                         //  0: member of the dense union, 100 values in its scratch vector
  t.buf2 = A(4); t.buf2_len = 100; t.out_aux = A(5);
  v.push_back(t);
  t = Task(MI_K_STR32, 1, 2047);                                  //  1: child of the struct: needs a mask
  t.buf2 = A(4); t.buf2_len = 5000; t.out_aux = A(5);
  v.push_back(t);
  t = Task(MI_K_RUN_END, 0, 2048, 4 | (8 << 8));                  //  2: int32 run ends over 8-byte values, 10 runs
  t.param2 = 10; t.buf2 = A(4);
  v.push_back(t);
  t = Task(MI_K_COPY, 0, kCopyTileRows + 1, 8);                   //  3: with NULLs
  t.validity = A(6); t.null_count = 5;
  v.push_back(t);
  v.push_back(Task(MI_K_STRUCT, 0, 2048));                        //  4
  t = Task(MI_K_COPY, 1, 2048, 4);                                //  5: child of the struct
  t.out_aux = A(5);
  v.push_back(t);
  t = Task(MI_K_DEC128, 0, 1, 8);                                 //  6: a bitmap, but null_count 0: no mask
  t.validity = A(6);
  v.push_back(t);
  t = Task(MI_K_DEC128, 0, 2049, 4);                              //  7: NULLs
  t.validity = A(6); t.null_count = 3;
  v.push_back(t);
  v.push_back(Task(MI_K_BOOL, 0, 2047));                          //  8: misc group 0
  t = Task(MI_K_DICT, 2, 1, 2);                                   //  9: misc group 0, no validity out
  t.out_validity = nullptr;
  v.push_back(t);
  v.push_back(Task(MI_K_MUL_I32, 0, 2048, 1000));                 // 10: misc group 0
  v.push_back(Task(MI_K_DATE64, 0, 2049));                        // 11: misc group 3
  v.push_back(Task(MI_K_LIST32, 0, 2047, 100));                   // 12: misc group 1
  v.push_back(Task(MI_K_UUID, 1, 1));                             // 13: misc group 2
  t = Task(MI_K_UNION, 0, 2048, 2);                               // 14: dense, two members
  t.buf2 = A(4); t.ptr_base = 0x5000; t.param2 = 2048; t.buf2_len = 256;
  v.push_back(t);
  t = Task(MI_K_COPY, 1, 2047, 8);                                // 15: the values child of the run-end column
  t.out_validity = nullptr;
  v.push_back(t);
  t = Task(MI_K_COPY, 0, 2049, 4);                                // 16: gather
  t.sel = A(7); t.sel_count = A(8);
  v.push_back(t);
  t = Task(MI_K_STR32, 0, 0);                                     // 17: no rows, no buffers
  t.buf1 = nullptr; t.out_data = nullptr; t.out_validity = nullptr;
  v.push_back(t);
  for (size_t i = 0; i < v.size(); i++) v[i].row_offset = 1000 + static_cast<int64_t>(i);
  return v;
}

void CheckMixedDecode(const char* what, const PlanLayout& l) {
  CheckSlices(what, l,
              {{kClassCopy, 0, 0, 1, 0, 0, 2, 0},          // task 3
               {kClassDec128, 0, 1, 2, 2, 2, 3, 3},        // tasks 6, 7: one without and one with a mask
               {kClassString, 0, 3, 1, 5, 5, 0, 1},        // task 17: no rows, still a slice
               {kClassMisc, 0, 4, 5, 7, 5, 6, 11},         // tasks 4, 8, 10, 11, 12: groups 1, 0, 0, 3, 1 = bits 2 | 1 | 8
               {kClassGather, 0, 9, 1, 13, 11, 2, 0},      // task 16
               {kSlotUnionTags, 0, 10, 1, 15, 13, 1, 0},   // task 14
               {kClassCopy, 1, 11, 2, 17, 14, 2, 0},       // tasks 5, 15
               {kClassString, 1, 13, 1, 20, 16, 1, 2},     // task 1
               {kClassMisc, 1, 14, 1, 22, 17, 1, 4},       // task 13
               {kClassMisc, 2, 15, 1, 24, 18, 1, 1},       // task 9
               {kSlotRunEnd, 0, 16, 1, 26, 19, 1, 0},      // task 2
               {kSlotUnionDense, 1, 17, 1, 28, 20, 2, 0}});  // task 0
  CheckArray(what, "tile_begin", l.tile_begin.data(), l.tile_begin.size(),
             std::vector<int>{0, 2, 0, 1, 3, 0, 0, 0, 1, 2, 3, 5, 6, 0, 2, 0, 1, 0, 1, 2, 0, 1, 0, 1, 0, 1, 0, 1, 0, 2});
  CheckArray(what, "tile_task", l.tile_task.data(), l.tile_task.size(), std::vector<int>{0, 0, 0, 1, 1, 0, 1, 2, 3, 3, 4, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0});
  CheckOrder(what, l, {{11, 0}, {7, 0}, {10, 0}, {0, 0}, {3, 0}, {6, 0}, {1, 0}, {1, 1}, {3, 1}, {9, 0}, {3, 2}, {3, 3}, {3, 4}, {8, 0}, {5, 0}, {6, 1}, {4, 0}, {2, 0}});
  CHECK(l.total_tiles == 22, "%s: %u tiles", what, l.total_tiles);
  // copy, dec128, string, misc (+ run-end, union tags, dense union), enc_fixed, enc_string, gather
  CheckArray(what, "class_tiles", l.class_tiles, 7, std::vector<int>{4, 3, 1, 12, 0, 0, 2});
  CheckArray(what, "class_rows", l.class_rows, 7, std::vector<int>{6144, 2050, 2047, 16386, 0, 0, 2049});
  //   copy: (257 + 16392) + (8192 + 256) + 16376;  dec128: 16 + (257 + 32784);  string: 8192 + 5000 + 256
  //   misc: 0 + 256 + 8192 + 16392 + 8192 + 16 + 2 + union 5 x 2048 + run-end 10 x 12 + dense (8196 + 264 + 400);  gather: 8196
  CheckArray(what, "class_bytes_read", l.class_bytes_read, 7, std::vector<int>{41473, 33057, 13448, 52270, 0, 0, 8196});
  //   copy: (16392 + 264) + (8192 + 256) + 16376;  dec128: (8 + 8) + (8196 + 264);  string: 32752 + 256
  //   misc: 256 + 2303 + 16640 + 8460 + 33008 + 24 + 4 + union (2048 + 3 x 256) + run-end 16640 + dense 8460;  gather: 8196 + 264
  CheckArray(what, "class_bytes_written", l.class_bytes_written, 7, std::vector<int>{41480, 8476, 33008, 88611, 0, 0, 8460});
  CHECK(l.bytes_read == 148444 && l.bytes_written == 180035 && l.rows == 28676, "%s: totals %lld / %lld / %lld", what, (long long)l.bytes_read,
        (long long)l.bytes_written, (long long)l.rows);
  CHECK(!l.is_encode && l.n_null_counts == 0, "%s: a decode plan has no NULL counters", what);
  // decode tasks come through as they were given
  if (l.tasks.size() == 18) CHECK(l.tasks[16].kind == MI_K_RUN_END && l.tasks[16].param2 == 10 && l.tasks[15].depth == 2, "%s: tasks were altered", what);
}

std::vector<mi_col_task> EncodeTasks() {
  std::vector<mi_col_task> v;
  mi_col_task t;
  t = Task(MI_K_ENC_STRVIEW, 3, 2049);        // 0
  t.out_aux = A(5); t.validity = A(6); t.buf2_len = 700;
  v.push_back(t);
  t = Task(MI_K_ENC_COPY, 1, 2048, 4);        // 1: list offsets, no bitmap
  t.out_validity = nullptr;
  v.push_back(t);
  t = Task(MI_K_ENC_UUID_TEXT, 2, 1);         // 2
  t.out_aux = A(5); t.buf2_len = 36;
  v.push_back(t);
  t = Task(MI_K_ENC_STR32, 1, 2047);          // 3
  t.out_aux = A(5); t.buf2_len = 900;
  v.push_back(t);
  t = Task(MI_K_ENC_BOOL, 5, 1);              // 4: a bitmap at an odd byte is fine
  t.out_validity = A(3, 1);
  v.push_back(t);
  t = Task(MI_K_ENC_LIST32, 64, 2049);        // 5: int64 offsets
  t.flags = 1;
  v.push_back(t);
  for (size_t i = 0; i < v.size(); i++) v[i].row_offset = 1000 + static_cast<int64_t>(i);
  return v;
}

void CheckEncode(const char* what, const PlanLayout& l) {
  CheckSlices(what, l,
              {{kClassEncFixed, 0, 0, 3, 0, 0, 3, 3},     // tasks 1, 2, 4: encode_fixed and encode_uuid_text
               {kClassEncString, 0, 3, 2, 4, 3, 3, 2},    // tasks 3, 5: the list bit
               {kSlotEncView, 0, 5, 1, 7, 6, 2, 0}});     // task 0, last
  CheckArray(what, "tile_begin", l.tile_begin.data(), l.tile_begin.size(), std::vector<int>{0, 1, 2, 3, 0, 1, 3, 0, 2});
  CheckArray(what, "tile_task", l.tile_task.data(), l.tile_task.size(), std::vector<int>{0, 1, 2, 0, 1, 1, 0, 0});
  CheckOrder(what, l, {{2, 0}, {0, 0}, {0, 1}, {1, 0}, {0, 2}, {1, 1}});
  const int64_t slots[6] = {1, 2, 4, 3, 5, 0};   // param2 of the staged tasks = caller index
  for (size_t i = 0; i < l.tasks.size() && i < 6; i++)
    CHECK(l.tasks[i].depth == 0 && l.tasks[i].param2 == slots[i], "%s: staged task %zu has depth %d, NULL counter %lld", what, i, l.tasks[i].depth,
          (long long)l.tasks[i].param2);
  CHECK(l.is_encode && l.n_null_counts == 6 && l.total_tiles == 8, "%s: is_encode %d, %lld counters, %u tiles", what, l.is_encode, (long long)l.n_null_counts, l.total_tiles);
  CheckArray(what, "class_tiles", l.class_tiles, 7, std::vector<int>{0, 0, 0, 0, 3, 5, 0});   // views under enc_string
  CheckArray(what, "class_rows", l.class_rows, 7, std::vector<int>{0, 0, 0, 0, 2050, 6145, 0});
  //   enc_fixed: 8192 + 16 + 1;  enc_string: (32752 + 900) + 32784 + views (264 + 32784 + 700)
  CheckArray(what, "class_bytes_read", l.class_bytes_read, 7, std::vector<int>{0, 0, 0, 0, 8209, 100184, 0});
  //   enc_fixed: 8192 + (1 + 8 + 36) + (1 + 1);  enc_string: (256 + 8192 + 900) + (257 + 16400) + views (257 + 32784 + 700)
  CheckArray(what, "class_bytes_written", l.class_bytes_written, 7, std::vector<int>{0, 0, 0, 0, 8239, 59746, 0});
  CHECK(l.bytes_read == 108393 && l.bytes_written == 67985 && l.rows == 8195, "%s: totals %lld / %lld / %lld", what, (long long)l.bytes_read,
        (long long)l.bytes_written, (long long)l.rows);
  const int64_t per_slot[6] = {100, 101, 102, 103, 104, 105};
  const std::vector<int64_t> nulls = l.MapNullCounts(per_slot);
  CheckArray(what, "MapNullCounts", nulls.data(), nulls.size(), std::vector<int>{100, 101, 102, 103, 104, 105});
}

void CheckEmpty(const char* what, const PlanLayout& l) {
  CHECK(l.slices.empty() && l.tasks.empty() && l.order.empty() && l.tile_begin.empty() && l.tile_task.empty(), "%s: tables are not empty", what);
  CHECK(l.total_tiles == 0 && l.bytes_read == 0 && l.bytes_written == 0 && l.rows == 0 && l.n_null_counts == 0 && !l.is_encode, "%s: counters are not zero", what);
  for (int c = 0; c < 7; c++)
    CHECK(l.class_tiles[c] == 0 && l.class_rows[c] == 0 && l.class_bytes_read[c] == 0 && l.class_bytes_written[c] == 0, "%s: class %d is not zero", what, c);
  CHECK(l.MapNullCounts(nullptr).empty(), "%s: NULL counts of no task", what);
}

void CheckLayouts() {
  const std::vector<mi_col_task> mixed = MixedDecodeTasks(), enc = EncodeTasks();
  CheckMixedDecode("mixed decode", LayOutPlan(mixed.data(), static_cast<int32_t>(mixed.size())));
  CheckEncode("encode", LayOutPlan(enc.data(), static_cast<int32_t>(enc.size())));
  CheckEmpty("no tasks", LayOutPlan(nullptr, 0));
  // one object, filled again and again
  PlanLayout l;
  LayOutPlan(mixed.data(), static_cast<int32_t>(mixed.size()), &l);
  CheckMixedDecode("mixed decode, first use", l);
  LayOutPlan(enc.data(), static_cast<int32_t>(enc.size()), &l);
  CheckEncode("encode, reused", l);
  LayOutPlan(mixed.data(), static_cast<int32_t>(mixed.size()), &l);
  CheckMixedDecode("mixed decode, reused", l);
  LayOutPlan(nullptr, 0, &l);
  CheckEmpty("no tasks, reused", l);

  // decode and encode tasks in one plan: only the encode tasks own a counter
  mi_col_task bare = Task(MI_K_ENC_COPY, 0, 10, 8);
  bare.out_validity = nullptr;
  const mi_col_task both[4] = {Task(MI_K_COPY, 0, 10, 4), Task(MI_K_ENC_BOOL, 0, 10), Task(MI_K_COPY, 1, 10, 4), bare};
  const PlanLayout lb = LayOutPlan(both, 4);
  const int64_t per_slot[2] = {7, 9};
  const std::vector<int64_t> nulls = lb.MapNullCounts(per_slot);
  CHECK(lb.n_null_counts == 2 && lb.is_encode, "decode + encode: %lld counters", (long long)lb.n_null_counts);
  CheckArray("decode + encode", "MapNullCounts", nulls.data(), nulls.size(), std::vector<int>{0, 7, 0, 9});
  CheckSlices("decode + encode", lb, {{kClassCopy, 0, 0, 1, 0, 0, 1, 0}, {kClassEncFixed, 0, 1, 2, 2, 1, 2, 1}, {kClassCopy, 1, 3, 1, 5, 3, 1, 0}});

  // more tiles than a launch can number: refused before a tile table of that size exists
  const mi_col_task huge = Task(MI_K_COPY, 0, 0xFFFFFFF1ll * kCopyTileRows, 1);
  std::string said;
  try {
    LayOutPlan(&huge, 1, &l);
  } catch (const InvalidInputException& e) {
    said = e.what();
  }
  CHECK(said == "plan has too many tiles", "0xFFFFFFF1 tiles: '%s'", said.c_str());
  CHECK(l.tile_task.empty(), "0xFFFFFFF1 tiles: %zu tile_task entries", l.tile_task.size());
  const mi_col_task most = Task(MI_K_COPY, 0, 70000ll * kCopyTileRows, 1);   // many tiles are fine
  CHECK(LayOutPlan(&most, 1).total_tiles == 70000, "70000 tiles");
}

// ------------------------------------------------------------------------------------------------ validation
// a task of `kind` that every rule accepts (100 rows)
mi_col_task Valid(int32_t kind) {
  mi_col_task t = Task(kind, 0, 100);
  switch (kind) {
    case MI_K_COPY: case MI_K_ENC_COPY: case MI_K_DICT: case MI_K_ENC_DEC128: case MI_K_UNION_DENSE: t.param = 4; break;
    case MI_K_DEC128: t.param = 8; break;
    case MI_K_LIST32: case MI_K_LIST64: t.param = 10; break;
    case MI_K_NARROW: t.param = 8 | (4 << 8); break;
    case MI_K_FIXED_BINARY: t.param = 5; break;
    case MI_K_MUL_I32: case MI_K_MUL_I64: case MI_K_DIV_I64: case MI_K_DURATION: t.param = 1000; break;
    case MI_K_RUN_END: t.param = 4 | (8 << 8); t.param2 = 3; break;
    case MI_K_UNION: t.param = 2; t.param2 = 104; t.buf2_len = 16; break;
    default: break;
  }
  if (kind == MI_K_STR32 || kind == MI_K_STR64 || kind == MI_K_RUN_END || kind == MI_K_UNION || kind == MI_K_UNION_DENSE) t.buf2 = A(4);
  if (kind == MI_K_STR32 || kind == MI_K_STR64) t.buf2_len = 64;
  if (kind == MI_K_UNION_DENSE) t.buf2_len = 10;
  if (kind == MI_K_UNION_DENSE || kind == MI_K_ENC_STR32 || kind == MI_K_ENC_STRVIEW || kind == MI_K_ENC_UUID_TEXT) t.out_aux = A(5);
  return t;
}
mi_col_task ValidGather() {
  mi_col_task t = Valid(MI_K_COPY);
  t.sel = A(7);
  t.sel_count = A(8);
  return t;
}

// what LayOutPlan says to `t` as task 2 of a plan ("" = accepted)
std::string Said(const mi_col_task& t) {
  const mi_col_task plan[3] = {Valid(MI_K_COPY), Valid(MI_K_ENC_BOOL), t};
  try {
    LayOutPlan(plan, 3);
  } catch (const InvalidInputException& e) {
    return e.what();
  }
  return "";
}

template <typename F>
void Refused(mi_col_task t, F&& damage, const char* message) {
  CHECK(Said(t).empty(), "kind %d: the valid task is refused: %s", t.kind, Said(t).c_str());
  damage(t);
  const std::string said = Said(t), want = std::string("task 2: ") + message;
  CHECK(said == want, "kind %d: '%s', not '%s'", t.kind, said.c_str(), want.c_str());
}
#define REFUSED(TASK, DAMAGE, MESSAGE) Refused(TASK, [](mi_col_task& t) { DAMAGE; }, MESSAGE)

void CheckValidation() {
  for (const KindRow& r : kKinds)
    if (r.slot >= 0) CHECK(Said(Valid(r.kind)).empty(), "a valid task of kind %d is refused: %s", r.kind, Said(Valid(r.kind)).c_str());
  CHECK(Said(ValidGather()).empty(), "a valid gather task is refused");

  REFUSED(Valid(MI_K_COPY), t.kind = 27, "unknown kind 27");
  REFUSED(Valid(MI_K_COPY), t.kind = 0, "unknown kind 0");
  REFUSED(Valid(MI_K_COPY), t.kind = 40, "unknown kind 40");
  // gather mode
  REFUSED(ValidGather(), t.kind = MI_K_DURATION; t.param = 1000, "kind 12 cannot be decoded through a selection vector");
  REFUSED(ValidGather(), t.sel_count = nullptr, "gather tasks need sel_count (rows selected per 2048-row window)");
  REFUSED(ValidGather(), t.out_aux = A(5), "gather tasks are top-level columns");
  REFUSED(ValidGather(), t.depth = 1, "gather tasks are top-level columns");
  REFUSED(ValidGather(), t.sel = A(7, 2), "selection vector misaligned");
  REFUSED(ValidGather(), t.sel_count = A(8, 2), "selection vector misaligned");
  // every kind
  REFUSED(Valid(MI_K_COPY), t.nrows = -1, "negative row count");
  REFUSED(Valid(MI_K_COPY), t.row_offset = -1, "negative row offset");
  REFUSED(Valid(MI_K_COPY), t.depth = -1, "bad nesting depth");
  REFUSED(Valid(MI_K_COPY), t.depth = 65, "bad nesting depth");
  REFUSED(Valid(MI_K_ENC_BOOL), t.depth = 65, "bad nesting depth");   // checked before an encode task's depth is set to 0
  mi_col_task deep = Valid(MI_K_COPY);
  deep.depth = 64;
  CHECK(Said(deep).empty(), "depth 64 is refused");
  mi_col_task none = {};   // no rows: nothing else is looked at
  none.kind = MI_K_DEC128;
  CHECK(Said(none).empty(), "a task of no rows and no buffers is refused: %s", Said(none).c_str());
  REFUSED(Valid(MI_K_STRUCT), t.out_validity = nullptr, "STRUCT tasks produce validity only: out_validity is NULL");
  REFUSED(Valid(MI_K_STRUCT), t.out_validity = A(3, 4), "out_validity must be 8-byte aligned");
  mi_col_task bare_struct = Valid(MI_K_STRUCT);   // a struct needs nothing but its validity
  bare_struct.buf1 = nullptr;
  bare_struct.out_data = nullptr;
  CHECK(Said(bare_struct).empty(), "a struct without data is refused");
  REFUSED(Valid(MI_K_COPY), t.out_data = nullptr, "out_data is NULL");
  REFUSED(Valid(MI_K_COPY), t.out_data = A(2, 8), "out_data must be 16-byte aligned");
  REFUSED(Valid(MI_K_COPY), t.out_validity = A(3, 4), "out_validity must be 8-byte aligned");
  mi_col_task odd_bitmap = Valid(MI_K_ENC_BOOL);   // an Arrow bitmap is bytes
  odd_bitmap.out_validity = A(3, 1);
  CHECK(Said(odd_bitmap).empty(), "an encode bitmap at an odd byte is refused");
  REFUSED(Valid(MI_K_COPY), t.validity = A(6, 4), "validity bitmap must be 8-byte aligned");
  REFUSED(Valid(MI_K_ENC_BOOL), t.validity = A(6, 4), "validity bitmap must be 8-byte aligned");
  REFUSED(Valid(MI_K_COPY), t.buf1 = nullptr, "buf1 is NULL");
  mi_col_task null_type = Valid(MI_K_NULL);
  null_type.buf1 = nullptr;
  CHECK(Said(null_type).empty(), "a NULL column without buf1 is refused");
  // per kind
  REFUSED(Valid(MI_K_LIST32), t.buf1 = A(1, 2), "offsets buffer misaligned");
  REFUSED(Valid(MI_K_LIST64), t.buf1 = A(1, 4), "offsets buffer misaligned");
  REFUSED(Valid(MI_K_LIST32), t.param = -1, "LIST needs param = child length");
  REFUSED(Valid(MI_K_LIST64), t.buf2 = A(4); t.buf2_len = 0, "window table is empty");
  REFUSED(Valid(MI_K_STRVIEW), t.buf1 = A(1, 2), "views buffer misaligned");
  REFUSED(Valid(MI_K_STRVIEW), t.buf2_len = 1, "STRVIEW needs the variadic buffer table in buf2");
  REFUSED(Valid(MI_K_NARROW), t.param = 4 | (4 << 8), "NARROW needs src 4->2 or 8->2/4");
  REFUSED(Valid(MI_K_NARROW), t.param = 2 | (2 << 8), "NARROW needs src 4->2 or 8->2/4");
  REFUSED(Valid(MI_K_COPY), t.param = 3, "COPY width must be 1,2,4,8,16");
  REFUSED(Valid(MI_K_COPY), t.param = 32, "COPY width must be 1,2,4,8,16");
  REFUSED(Valid(MI_K_DEC128), t.param = 16, "DEC128 out width must be 2,4,8");
  REFUSED(Valid(MI_K_DEC128), t.buf1 = A(1, 4), "decimal buffer must be 8-byte aligned");
  REFUSED(Valid(MI_K_STR32), t.buf2 = nullptr, "string data buffer is NULL");
  REFUSED(Valid(MI_K_STR32), t.buf1 = A(1, 2), "offsets buffer misaligned");
  REFUSED(Valid(MI_K_STR64), t.buf1 = A(1, 4), "offsets buffer misaligned");
  REFUSED(Valid(MI_K_STR64), t.buf2 = A(4, 2), "string data buffer must be 4-byte aligned");
  REFUSED(Valid(MI_K_STR32), t.buf2_len = -1, "negative buf2_len");
  REFUSED(Valid(MI_K_FIXED_BINARY), t.param = 0, "fixed binary width must be positive");
  REFUSED(Valid(MI_K_FIXED_BINARY), t.buf1 = A(1, 2), "fixed binary buffer must be 4-byte aligned");
  REFUSED(Valid(MI_K_DICT), t.param = 3, "dictionary index width must be 1,2,4,8");
  REFUSED(Valid(MI_K_MUL_I32), t.param = 0, "multiplier must be positive");
  REFUSED(Valid(MI_K_MUL_I64), t.param = -1000, "multiplier must be positive");
  REFUSED(Valid(MI_K_DIV_I64), t.param = 0, "divisor must be positive");
  REFUSED(Valid(MI_K_DURATION), t.param = 0, "duration factor must be non-zero");
  mi_col_task nanos = Valid(MI_K_DURATION);
  nanos.param = -1000;
  CHECK(Said(nanos).empty(), "a duration divisor is refused");
  REFUSED(Valid(MI_K_UUID), t.buf1 = A(1, 2), "uuid buffer must be 4-byte aligned");
  REFUSED(Valid(MI_K_RUN_END), t.param = 1 | (8 << 8), "RUN_END run-end width must be 2,4,8");
  REFUSED(Valid(MI_K_RUN_END), t.param = 4 | (3 << 8), "RUN_END out width must be 1,2,4,8,16");
  REFUSED(Valid(MI_K_RUN_END), t.buf1 = A(1, 2), "run ends misaligned");
  REFUSED(Valid(MI_K_RUN_END), t.param2 = 0, "RUN_END needs param2 = number of runs > 0");
  REFUSED(Valid(MI_K_RUN_END), t.buf2 = nullptr, "RUN_END needs the decoded values (16-byte aligned) in buf2");
  REFUSED(Valid(MI_K_RUN_END), t.buf2 = A(4, 8), "RUN_END needs the decoded values (16-byte aligned) in buf2");
  REFUSED(Valid(MI_K_RUN_END), t.flags = 2, "RUN_END parents are structs (flags 0 or 1)");
  REFUSED(Valid(MI_K_UNION), t.param = 0, "UNION needs param = number of members, 1 .. 32");
  REFUSED(Valid(MI_K_UNION), t.param = 33, "UNION needs param = number of members, 1 .. 32");
  REFUSED(Valid(MI_K_UNION), t.buf2 = nullptr, "UNION needs the union table (8-byte aligned) in buf2");
  REFUSED(Valid(MI_K_UNION), t.buf2 = A(4, 4), "UNION needs the union table (8-byte aligned) in buf2");
  REFUSED(Valid(MI_K_UNION), t.ptr_base = 0x5002, "UNION dense offsets misaligned");
  REFUSED(Valid(MI_K_UNION), t.param2 = 0, "UNION needs param2 = distance from out_data to mask 0: a multiple of 8 behind the tags");
  REFUSED(Valid(MI_K_UNION), t.param2 = 108, "UNION needs param2 = distance from out_data to mask 0: a multiple of 8 behind the tags");
  REFUSED(Valid(MI_K_UNION), t.param2 = 96, "UNION needs param2 = distance from out_data to mask 0: a multiple of 8 behind the tags");
  REFUSED(Valid(MI_K_UNION), t.buf2_len = 20, "UNION needs buf2_len = distance between masks: a multiple of 8, at least 8 ceil(nrows / 64)");
  REFUSED(Valid(MI_K_UNION), t.buf2_len = 8, "UNION needs buf2_len = distance between masks: a multiple of 8, at least 8 ceil(nrows / 64)");
  REFUSED(Valid(MI_K_UNION), t.flags = 2, "UNION parents are structs (flags 0 or 1)");
  REFUSED(Valid(MI_K_UNION_DENSE), t.param = 3, "UNION_DENSE width must be 1,2,4,8,16");
  REFUSED(Valid(MI_K_UNION_DENSE), t.buf1 = A(1, 2), "UNION_DENSE offsets misaligned");
  REFUSED(Valid(MI_K_UNION_DENSE), t.buf2 = nullptr, "UNION_DENSE needs the member's decoded vector (16-byte aligned) in buf2");
  REFUSED(Valid(MI_K_UNION_DENSE), t.buf2 = A(4, 8), "UNION_DENSE needs the member's decoded vector (16-byte aligned) in buf2");
  REFUSED(Valid(MI_K_UNION_DENSE), t.buf2_len = -1, "UNION_DENSE needs buf2_len = rows of the member's vector");
  REFUSED(Valid(MI_K_UNION_DENSE), t.out_aux = nullptr, "UNION_DENSE needs the member's mask (8-byte aligned) in out_aux");
  REFUSED(Valid(MI_K_UNION_DENSE), t.out_aux = A(5, 4), "UNION_DENSE needs the member's mask (8-byte aligned) in out_aux");
  REFUSED(Valid(MI_K_UNION_DENSE), t.flags = 2, "UNION_DENSE masks have the union's row numbering (flags 0 or 1)");
  // the two union kinds' own selection-vector rules cannot be reached: the gather rule above them speaks first
  REFUSED(Valid(MI_K_UNION), t.sel = A(7); t.sel_count = A(8), "kind 23 cannot be decoded through a selection vector");
  REFUSED(Valid(MI_K_UNION_DENSE), t.sel = A(7); t.sel_count = A(8), "kind 24 cannot be decoded through a selection vector");
  REFUSED(Valid(MI_K_ENC_COPY), t.param = 3, "ENC_COPY width must be 1,2,4,8,16");
  REFUSED(Valid(MI_K_ENC_DEC128), t.param = 16, "ENC_DEC128 in width must be 2,4,8");
  REFUSED(Valid(MI_K_ENC_STR32), t.out_aux = nullptr, "out_aux (string data) is NULL");
  REFUSED(Valid(MI_K_ENC_STRVIEW), t.out_aux = nullptr, "out_aux (string data) is NULL");
  REFUSED(Valid(MI_K_ENC_STR32), t.buf1 = A(1, 8), "string_t vector must be 16-byte aligned");
  REFUSED(Valid(MI_K_ENC_STRVIEW), t.buf1 = A(1, 8), "string_t vector must be 16-byte aligned");
  REFUSED(Valid(MI_K_ENC_LIST32), t.buf1 = A(1, 8), "list_entry_t vector must be 16-byte aligned");
  REFUSED(Valid(MI_K_ENC_UUID_TEXT), t.out_aux = nullptr, "out_aux (string data) is NULL");
  REFUSED(Valid(MI_K_ENC_UUID_TEXT), t.buf1 = A(1, 8), "UUID vector must be 16-byte aligned");
  REFUSED(Valid(MI_K_ENC_UUID_TEXT), t.out_aux = A(5, 8), "string data buffer must be 16-byte aligned");
  // (its "offsets buffer misaligned" asks for 8 bytes of out_data, of which every task must have 16: it cannot be reached either)
  REFUSED(Valid(MI_K_ENC_UUID_TEXT), t.out_data = A(2, 4), "out_data must be 16-byte aligned");
  REFUSED(Valid(MI_K_ENC_UUID_TEXT), t.nrows = 0x80000000ll, "more than INT32_MAX rows");
  mi_col_task many = Valid(MI_K_ENC_UUID_TEXT);
  many.nrows = 0x7FFFFFFFll;
  CHECK(Said(many).empty(), "INT32_MAX rows of UUID text are refused");
  for (int32_t kind : {MI_K_ENC_DEC128, MI_K_ENC_BOOL, MI_K_ENC_STR32, MI_K_ENC_VALIDITY, MI_K_ENC_LIST32, MI_K_ENC_STRVIEW, MI_K_ENC_UUID_TEXT})
    REFUSED(Valid(kind), t.out_validity = nullptr,
            "encode tasks need out_validity (the bitmap is always emitted; only a bare ENC_COPY of list offsets has none)");
  mi_col_task bare = Valid(MI_K_ENC_COPY);
  bare.out_validity = nullptr;
  CHECK(Said(bare).empty(), "a bare ENC_COPY is refused");
  // the index in the message is the task's place in the caller's table
  mi_col_task first = Valid(MI_K_COPY);
  first.nrows = -1;
  std::string said;
  try {
    LayOutPlan(&first, 1);
  } catch (const InvalidInputException& e) {
    said = e.what();
  }
  CHECK(said == "task 0: negative row count", "'%s'", said.c_str());
}

}  // namespace

int main() {
  CheckKindTable();
  CheckPlanWidths();
  CheckLayouts();
  CheckValidation();
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed == 0 ? 0 : 1;
}
