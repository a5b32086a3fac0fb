// chunk_staging_check.cpp -- the writer's chunk staging (duckdb-arrow_amd/csrc/chunk_staging.cpp: ChunkCollection) and the
// device staging layout (writer_plan.cpp: LayOutStaging) without a GPU, under AddressSanitizer + UBSan (test infrastructure,
// never shipped).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -Wextra -I include
//       tests/sanitize/chunk_staging_check.cpp duckdb-arrow_amd/csrc/chunk_staging.cpp duckdb-arrow_amd/csrc/writer_plan.cpp
//       duckdb-arrow_amd/csrc/ipc_format.cpp -o chunk_staging_check
//
// Staging memory comes from malloc, exactly the bytes the collection asks for, and every source array (vector data, validity
// words, string payloads, declared heaps) is a malloc of its exact size: a read or write one byte outside any of them is a
// report.  Expected values are written out here from the rules in chunk_staging.hpp, the Arrow format and what DuckDB's
// ArrowAppender stages -- not computed by the code under test.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include <vector>

#include "../../duckdb-arrow_amd/csrc/chunk_staging.hpp"
#include "../../duckdb-arrow_amd/csrc/extension_format.hpp"
#include "../../duckdb-arrow_amd/csrc/writer_plan.hpp"

using namespace miarrow;

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

// ---- staging memory: exactly the bytes asked, calls counted
int g_allocs = 0;
void* CountingAlloc(void* cookie, size_t bytes) {
  ++*static_cast<int*>(cookie);
  void* p = std::malloc(bytes);
  if (!p) throw std::bad_alloc();
  return p;
}
const StagingAllocator kAlloc{CountingAlloc, std::free, &g_allocs};

// ---- source arrays: a malloc of exactly their size, freed at the end of main
std::vector<void*> g_owned;
template <typename T>
T* Exact(const std::vector<T>& v) {
  T* p = static_cast<T*>(std::malloc(v.size() * sizeof(T)));
  std::memcpy(p, v.data(), v.size() * sizeof(T));
  g_owned.push_back(p);
  return p;
}
char* ExactText(const std::string& s) { return Exact(std::vector<char>(s.begin(), s.end())); }
std::string Text(size_t n, char first) {   // n letters that differ from their neighbours
  std::string s(n, ' ');
  for (size_t i = 0; i < n; i++) s[i] = static_cast<char>('a' + (static_cast<size_t>(first - 'a') + i) % 26);
  return s;
}

mi_string_t Short(const std::string& s) {   // <= 12 bytes, inlined
  mi_string_t r;
  std::memset(&r, 0, sizeof(r));
  r.value.inlined.length = static_cast<uint32_t>(s.size());
  std::memcpy(r.value.inlined.inlined, s.data(), s.size());
  return r;
}
mi_string_t Long(const char* p, uint32_t len) {   // > 12 bytes at p
  mi_string_t r;
  std::memset(&r, 0, sizeof(r));
  r.value.pointer.length = len;
  std::memcpy(r.value.pointer.prefix, p, 4);
  r.value.pointer.ptr = reinterpret_cast<uint64_t>(p);
  return r;
}
mi_string_t Garbage() {   // what a NULL row may hold: must never be followed
  mi_string_t r;
  std::memset(&r, 0, sizeof(r));
  r.value.pointer.length = 1000;
  r.value.pointer.ptr = 1;
  return r;
}

mi_vector Vec(const void* data, const uint64_t* validity = nullptr, int32_t shift = 0) {
  mi_vector v;
  std::memset(&v, 0, sizeof(v));
  v.data = const_cast<void*>(data);
  v.validity = const_cast<uint64_t*>(validity);
  v.validity_shift = shift;
  return v;
}
mi_vector Nested(const void* data, const uint64_t* validity, const mi_vector* children, int32_t n_children) {
  mi_vector v = Vec(data, validity);
  v.children = children;
  v.n_children = n_children;
  return v;
}
void AppendChunk(ChunkCollection& cc, const mi_vector* columns, int32_t n_columns, int64_t size) {
  mi_data_chunk chunk;
  std::memset(&chunk, 0, sizeof(chunk));
  chunk.columns = columns;
  chunk.n_columns = n_columns;
  chunk.size = size;
  cc.Append(chunk);
}

// ---- fields as FieldFromDuckType would make them
ArrowField Int(int bits) {
  ArrowField f;
  f.type = MI_AT_INT;
  f.bit_width = bits;
  f.is_signed = true;
  return f;
}
ArrowField Typed(int32_t type) {
  ArrowField f;
  f.type = type;
  return f;
}
ArrowField Parent(int32_t type, std::vector<ArrowField> children, int32_t byte_width = 0) {
  ArrowField f;
  f.type = type;
  f.children = std::move(children);
  f.byte_width = byte_width;
  return f;
}

bool Bit(const ChunkCollection::Column& c, int64_t i) { return (c.validity.get<uint64_t>()[i >> 6] >> (i & 63)) & 1; }
const mi_string_t* Rows(const ChunkCollection::Column& c) { return c.data.get<mi_string_t>(); }

// `f` throws an Exception of type E whose text is exactly `text`
template <typename E>
void CheckThrows(const char* what, const std::function<void()>& f, const std::string& text) {
  try {
    f();
    CHECK(false, "%s: no exception", what);
  } catch (const E& e) {
    CHECK(text == e.what(), "%s: message is \"%s\"", what, e.what());
  } catch (const std::exception& e) {
    CHECK(false, "%s: another exception type: %s", what, e.what());
  }
}

// ------------------------------------------------------------------------------------------------ fixed width, validity
// list<int32>: a list row (o, l) hands the child vector's rows [o, o + l) to the child node, so three chunks of one list each
// append child slices with start 5, 70, 100 and lengths 63, 1, 65: destination bits 0..62, 63, 64..128.  Child row r is valid
// unless r % 7 == 3; its bit is bit shift + r of the child's words.
void CheckSlicesAndShifts(int32_t shift) {
  std::vector<int32_t> values(165);
  for (size_t r = 0; r < values.size(); r++) values[r] = static_cast<int32_t>(3 * r + 1);
  std::vector<uint64_t> words(static_cast<size_t>((shift + 165 + 63) / 64), 0);
  for (int64_t r = 0; r < 165; r++)
    if (r % 7 != 3) words[static_cast<size_t>((shift + r) >> 6)] |= 1ull << ((shift + r) & 63);
  const mi_vector child = Vec(Exact(values), Exact(words), shift);
  ChunkCollection cc(kAlloc, {Parent(MI_AT_LIST, {Int(32)})});
  const int64_t slices[3][2] = {{5, 63}, {70, 1}, {100, 65}};
  for (auto& sl : slices) {
    const mi_vector list = Nested(Exact(std::vector<uint64_t>{static_cast<uint64_t>(sl[0]), static_cast<uint64_t>(sl[1])}), nullptr, &child, 1);
    AppendChunk(cc, &list, 1, 1);
  }
  const auto& c = cc.columns[1];
  CHECK(cc.Count() == 3 && cc.columns[0].count == 3 && c.count == 129, "shift %d: %lld lists, %lld child rows", shift, (long long)cc.Count(), (long long)c.count);
  CHECK(cc.columns[0].payload_bytes == 129 && !cc.columns[0].has_nulls && c.has_nulls, "shift %d: list payload %lld", shift, (long long)cc.columns[0].payload_bytes);
  CHECK(cc.SizeInBytes() == 3 * 16 + 129 * 4, "shift %d: SizeInBytes %lld", shift, (long long)cc.SizeInBytes());
  for (int64_t k = 0; k < 129; k++) {
    const int64_t r = k < 63 ? 5 + k : k == 63 ? 70 : 100 + (k - 64);   // the source row of staged row k
    CHECK(c.data.get<int32_t>()[k] == 3 * r + 1, "shift %d: staged row %lld holds %d", shift, (long long)k, c.data.get<int32_t>()[k]);
    CHECK(Bit(c, k) == (r % 7 != 3), "shift %d: validity bit %lld", shift, (long long)k);
  }
  CHECK((c.validity.get<uint64_t>()[2] >> 1) == (~0ull >> 1), "shift %d: bits behind the last row are not all ones", shift);
}

// data bytes land at count * width; validity NULL = all valid, and the first NULL flips has_nulls and leaves earlier bits 1
void CheckWidths() {
  ArrowField dec38 = Typed(MI_AT_DECIMAL);
  dec38.precision = 38;
  dec38.bit_width = 128;
  const std::vector<ArrowField> fields = {Int(8), Int(16), Int(32), Int(64), dec38};
  const int widths[5] = {1, 2, 4, 8, 16};
  ChunkCollection cc(kAlloc, fields);
  const uint8_t* src[5][2];
  mi_vector first[5], second[5];
  const uint64_t* one_null = Exact(std::vector<uint64_t>{~0ull & ~2ull});   // row 1 of the second chunk is NULL
  for (int k = 0; k < 5; k++) {
    std::vector<uint8_t> a(static_cast<size_t>(3 * widths[k])), b(static_cast<size_t>(2 * widths[k]));
    for (size_t i = 0; i < a.size(); i++) a[i] = static_cast<uint8_t>(17 * k + i + 1);
    for (size_t i = 0; i < b.size(); i++) b[i] = static_cast<uint8_t>(200 - 9 * k - i);
    first[k] = Vec(src[k][0] = Exact(a));
    second[k] = Vec(src[k][1] = Exact(b), k == 2 ? one_null : nullptr);
  }
  AppendChunk(cc, first, 5, 3);
  for (int k = 0; k < 5; k++) CHECK(!cc.columns[static_cast<size_t>(k)].has_nulls, "width %d: has_nulls after an all-valid chunk", widths[k]);
  AppendChunk(cc, second, 5, 2);
  CHECK(cc.Count() == 5 && cc.SizeInBytes() == 5 * (1 + 2 + 4 + 8 + 16), "widths: %lld rows, %lld bytes", (long long)cc.Count(), (long long)cc.SizeInBytes());
  for (int k = 0; k < 5; k++) {
    const auto& c = cc.columns[static_cast<size_t>(k)];
    CHECK(c.width == widths[k] && c.count == 5, "width %d: node says %d, %lld rows", widths[k], c.width, (long long)c.count);
    CHECK(std::memcmp(c.data.get(), src[k][0], static_cast<size_t>(3 * widths[k])) == 0, "width %d: first chunk's bytes", widths[k]);
    CHECK(std::memcmp(c.data.get() + 3 * widths[k], src[k][1], static_cast<size_t>(2 * widths[k])) == 0, "width %d: second chunk's bytes", widths[k]);
    CHECK(c.has_nulls == (k == 2), "width %d: has_nulls", widths[k]);
    CHECK(c.validity.get<uint64_t>()[0] == (k == 2 ? ~0ull & ~(1ull << 4) : ~0ull), "width %d: validity word %llx", widths[k], (unsigned long long)c.validity.get<uint64_t>()[0]);
  }
}

// a slice whose last bit is the last bit of the source's last word: 63 rows from bit 1 of ONE word (no word behind it is read),
// then the same rows again, which now end at destination bit 125
void CheckSliceEndsWithItsWord() {
  std::vector<uint8_t> values(63);
  for (size_t r = 0; r < values.size(); r++) values[r] = static_cast<uint8_t>(r + 100);
  const mi_vector v = Vec(Exact(values), Exact(std::vector<uint64_t>{0xAAAAAAAAAAAAAAABull}), 1);   // row r is valid when r is even
  ChunkCollection cc(kAlloc, {Int(8)});
  AppendChunk(cc, &v, 1, 63);
  AppendChunk(cc, &v, 1, 63);
  const auto& c = cc.columns[0];
  CHECK(c.count == 126 && c.has_nulls, "word end: %lld rows", (long long)c.count);
  CHECK(c.validity.get<uint64_t>()[0] == 0xD555555555555555ull && c.validity.get<uint64_t>()[1] == 0xEAAAAAAAAAAAAAAAull, "word end: validity %llx %llx",
        (unsigned long long)c.validity.get<uint64_t>()[0], (unsigned long long)c.validity.get<uint64_t>()[1]);
  CHECK(c.data.get()[62] == 162 && c.data.get()[63] == 100 && c.data.get()[125] == 162, "word end: staged rows");
}

void CheckEncodePlans() {
  struct Want { int32_t kind; int64_t param; int32_t width; };
  auto plan_is = [](const char* what, const ArrowField& f, Want w) {
    int32_t kind = -1, width = -1;
    int64_t param = -1;
    EncodePlanFor(f, &kind, &param, &width);
    CHECK(kind == w.kind && param == w.param && width == w.width, "%s: plan {%d, %lld, %d}", what, kind, (long long)param, width);
  };
  plan_is("BOOLEAN", Typed(MI_AT_BOOL), {MI_K_ENC_BOOL, 1, 1});
  const int precisions[] = {1, 4, 5, 9, 10, 18, 19, 38};
  const Want decimals[] = {{MI_K_ENC_DEC128, 2, 2}, {MI_K_ENC_DEC128, 2, 2}, {MI_K_ENC_DEC128, 4, 4}, {MI_K_ENC_DEC128, 4, 4},
                           {MI_K_ENC_DEC128, 8, 8}, {MI_K_ENC_DEC128, 8, 8}, {MI_K_ENC_COPY, 16, 16}, {MI_K_ENC_COPY, 16, 16}};
  for (int i = 0; i < 8; i++) {
    ArrowField d = Typed(MI_AT_DECIMAL);
    d.precision = precisions[i];
    d.bit_width = 128;
    plan_is(("DECIMAL(" + std::to_string(precisions[i]) + ")").c_str(), d, decimals[i]);
  }
  plan_is("SMALLINT", Int(16), {MI_K_ENC_COPY, 2, 2});
  plan_is("DATE", Typed(MI_AT_DATE), {MI_K_ENC_COPY, 4, 4});
  plan_is("TIMESTAMP", Typed(MI_AT_TIMESTAMP), {MI_K_ENC_COPY, 8, 8});
  plan_is("VARCHAR", Typed(MI_AT_UTF8), {MI_K_ENC_STR32, 0, 16});
  plan_is("VARCHAR as views", Typed(MI_AT_UTF8_VIEW), {MI_K_ENC_STRVIEW, 0, 16});
  ArrowField uuid = Typed(MI_AT_UTF8);
  uuid.extension = extfmt::kUuid;
  plan_is("UUID", uuid, {MI_K_ENC_UUID_TEXT, 16, 16});
  ArrowField interval = Typed(MI_AT_INTERVAL);
  interval.unit = 2;
  plan_is("INTERVAL", interval, {MI_K_ENC_INTERVAL, 16, 16});
  interval.unit = 0;
  CheckThrows<NotImplementedException>("interval of months", [&] { ChunkCollection cc(kAlloc, {interval}); },
                                       "Arrow type tiM is not encoded by the MI355X writer path");
  interval.unit = 1;
  CheckThrows<NotImplementedException>("interval of days", [&] { ChunkCollection cc(kAlloc, {interval}); },
                                       "Arrow type tiD is not encoded by the MI355X writer path");
  ArrowField fixed = Typed(MI_AT_FIXED_BINARY);
  fixed.byte_width = 16;
  CheckThrows<NotImplementedException>("fixed_size_binary", [&] { ChunkCollection cc(kAlloc, {fixed}); },
                                       "Arrow type w:16 is not encoded by the MI355X writer path");
}

// ------------------------------------------------------------------------------------------------ growth and reset
// TINYINT: 100 rows (row 5 NULL), then 524200 all-valid rows in one chunk.  Buffers start as one 64 KiB granule; 524300 rows
// need 524364 data bytes and 8193 validity words + 16 bytes = 65560: both grow once, to 720896 (need and a quarter, in
// granules) and to 131072 (half again the old capacity).
void CheckGrowthAndReset() {
  std::vector<uint8_t> a(100), b(524200);
  for (size_t i = 0; i < a.size(); i++) a[i] = static_cast<uint8_t>(i + 1);
  for (size_t i = 0; i < b.size(); i++) b[i] = static_cast<uint8_t>(i % 251);
  const mi_vector first = Vec(Exact(a), Exact(std::vector<uint64_t>{~0ull & ~(1ull << 5), ~0ull}));
  const mi_vector second = Vec(Exact(b));
  ChunkCollection cc(kAlloc, {Int(8)});
  const int allocs0 = g_allocs;
  AppendChunk(cc, &first, 1, 100);
  const auto& c = cc.columns[0];
  CHECK(g_allocs - allocs0 == 2, "growth: %d allocations for the first chunk of an integer column", g_allocs - allocs0);
  CHECK(c.data.size() == 65536 && c.validity.size() == 65536 && !c.heap, "growth: first capacities %zu, %zu", c.data.size(), c.validity.size());
  bool ones = true;
  for (size_t w = 2; w < 8192; w++) ones &= c.validity.get<uint64_t>()[w] == ~0ull;
  CHECK(ones, "growth: fresh validity words are not 0xFF");
  AppendChunk(cc, &second, 1, 524200);
  CHECK(g_allocs - allocs0 == 4, "growth: %d allocations after both buffers grew once", g_allocs - allocs0);
  CHECK(c.data.size() == 720896 && c.validity.size() == 131072, "growth: grown capacities %zu, %zu", c.data.size(), c.validity.size());
  CHECK(c.count == 524300 && cc.Count() == 524300 && cc.SizeInBytes() == 524300, "growth: %lld rows", (long long)c.count);
  CHECK(std::memcmp(c.data.get(), a.data(), 100) == 0 && std::memcmp(c.data.get() + 100, b.data(), b.size()) == 0, "growth: staged bytes");
  CHECK(c.validity.get<uint64_t>()[0] == (~0ull & ~(1ull << 5)), "growth: the NULL staged before the growth");
  ones = true;
  for (size_t w = 1; w < 16384; w++) ones &= c.validity.get<uint64_t>()[w] == ~0ull;
  CHECK(ones && c.has_nulls, "growth: validity words behind the first are not all ones");

  cc.Reset();
  CHECK(cc.Count() == 0 && cc.SizeInBytes() == 0, "reset: %lld rows, %lld bytes", (long long)cc.Count(), (long long)cc.SizeInBytes());
  CHECK(c.count == 0 && c.heap_used == 0 && c.payload_bytes == 0 && !c.has_nulls, "reset: node counters");
  ones = true;
  for (size_t w = 0; w < 16384; w++) ones &= c.validity.get<uint64_t>()[w] == ~0ull;
  CHECK(ones, "reset: validity is not all ones");
  AppendChunk(cc, &first, 1, 100);
  AppendChunk(cc, &second, 1, 524200);
  CHECK(g_allocs - allocs0 == 4, "reset: the same rows again took %d more allocations", g_allocs - allocs0 - 4);
  CHECK(c.count == 524300 && c.has_nulls && !Bit(c, 5) && Bit(c, 4) && std::memcmp(c.data.get() + 100, b.data(), b.size()) == 0, "reset: rows appended again");
}

// ------------------------------------------------------------------------------------------------ strings
// lengths 0, 12, 13, 200 and a NULL row of garbage; no declared heap, every long string an allocation of its own
void CheckStringLengths(int32_t type) {
  const bool views = type == MI_AT_UTF8_VIEW;
  const std::string s12 = Text(12, 'c'), s13 = Text(13, 'k'), s200 = Text(200, 'q');
  const char* p13 = ExactText(s13);
  const char* p200 = ExactText(s200);
  const std::vector<mi_string_t> rows = {Short(""), Short(s12), Long(p13, 13), Garbage(), Long(p200, 200)};
  const mi_vector v = Vec(Exact(rows), Exact(std::vector<uint64_t>{0x17}));   // row 3 is NULL
  ChunkCollection cc(kAlloc, {Typed(type)});
  const int allocs0 = g_allocs;
  AppendChunk(cc, &v, 1, 5);
  const auto& c = cc.columns[0];
  CHECK(g_allocs - allocs0 == 3, "strings %d: %d allocations", type, g_allocs - allocs0);
  CHECK(c.count == 5 && c.has_nulls && c.validity.get<uint64_t>()[0] == (~0ull & ~8ull), "strings %d: rows and validity", type);
  CHECK(c.payload_bytes == (views ? 213 : 225), "strings %d: payload_bytes %lld", type, (long long)c.payload_bytes);
  CHECK(c.heap_used == 213 && cc.SizeInBytes() == 213 + 5 * 16, "strings %d: heap_used %lld, SizeInBytes %lld", type, (long long)c.heap_used, (long long)cc.SizeInBytes());
  CHECK(std::memcmp(c.heap.get(), s13.data(), 13) == 0 && std::memcmp(c.heap.get() + 13, s200.data(), 200) == 0, "strings %d: staged payloads", type);
  const mi_string_t* got = Rows(c);
  CHECK(std::memcmp(&got[0], &rows[0], 16) == 0 && std::memcmp(&got[1], &rows[1], 16) == 0, "strings %d: inlined rows are staged as they are", type);
  CHECK(got[2].value.pointer.length == 13 && got[2].value.pointer.ptr == 0 && std::memcmp(got[2].value.pointer.prefix, "klmn", 4) == 0, "strings %d: the 13-byte row", type);
  CHECK(std::memcmp(&got[3], &rows[3], 16) == 0, "strings %d: the NULL row was touched", type);
  CHECK(got[4].value.pointer.length == 200 && got[4].value.pointer.ptr == 13, "strings %d: the 200-byte row points at %llu", type, (unsigned long long)got[4].value.pointer.ptr);

  cc.Reset();
  CHECK(c.count == 0 && c.heap_used == 0 && c.payload_bytes == 0 && !c.has_nulls && cc.SizeInBytes() == 0, "strings %d: reset", type);
  AppendChunk(cc, &v, 1, 5);
  CHECK(g_allocs - allocs0 == 3 && c.heap_used == 213 && Rows(c)[4].value.pointer.ptr == 13, "strings %d: the same rows after a reset", type);
}

// A declared heap of `heap_bytes` bytes (declared as `declared` bytes); row 0 is the 13 bytes at offset `at0`, row 1 a short
// string when `with_short`, the last row the 13 bytes at offset `at1`.  One copy stages [first long string, end of the last)
// and is told from staging string by string by heap_used: the range against 26.
struct HeapCase {
  const char* what;
  size_t heap_bytes;
  int64_t declared;
  size_t at0, at1;
  int64_t want_heap_used;   // after one append
  uint64_t want_ptr0, want_ptr1;
};
void CheckDeclaredHeap(const HeapCase& hc, int32_t type) {
  std::vector<char> heap(hc.heap_bytes);
  for (size_t i = 0; i < heap.size(); i++) heap[i] = static_cast<char>('A' + i % 23);
  const char* h = Exact(heap);
  const std::vector<mi_string_t> rows = {Long(h + hc.at0, 13), Long(h + hc.at1, 13)};
  mi_vector v = Vec(Exact(rows));
  v.heap = h;
  v.heap_size = hc.declared;
  ChunkCollection cc(kAlloc, {Typed(type)});
  AppendChunk(cc, &v, 1, 2);
  const auto& c = cc.columns[0];
  CHECK(c.heap_used == hc.want_heap_used, "%s: heap_used %lld", hc.what, (long long)c.heap_used);
  CHECK(c.payload_bytes == 26 && cc.SizeInBytes() == hc.want_heap_used + 32, "%s: payload %lld, SizeInBytes %lld", hc.what, (long long)c.payload_bytes, (long long)cc.SizeInBytes());
  CHECK(Rows(c)[0].value.pointer.ptr == hc.want_ptr0 && Rows(c)[1].value.pointer.ptr == hc.want_ptr1, "%s: rows point at %llu, %llu", hc.what,
        (unsigned long long)Rows(c)[0].value.pointer.ptr, (unsigned long long)Rows(c)[1].value.pointer.ptr);
  CHECK(std::memcmp(c.heap.get() + hc.want_ptr0, h + hc.at0, 13) == 0 && std::memcmp(c.heap.get() + hc.want_ptr1, h + hc.at1, 13) == 0, "%s: staged payloads", hc.what);
  // the same slice again lands behind the first: heap_used + (p - first long pointer)
  AppendChunk(cc, &v, 1, 2);
  CHECK(c.heap_used == 2 * hc.want_heap_used && Rows(c)[2].value.pointer.ptr == static_cast<uint64_t>(hc.want_heap_used) + hc.want_ptr0 &&
            Rows(c)[3].value.pointer.ptr == static_cast<uint64_t>(hc.want_heap_used) + hc.want_ptr1,
        "%s: second append points at %llu, %llu", hc.what, (unsigned long long)Rows(c)[2].value.pointer.ptr, (unsigned long long)Rows(c)[3].value.pointer.ptr);
}

void CheckStrings() {
  for (int32_t type : {MI_AT_UTF8, MI_AT_LARGE_UTF8, MI_AT_UTF8_VIEW}) CheckStringLengths(type);
  for (int32_t type : {MI_AT_UTF8, MI_AT_UTF8_VIEW}) {
    // two long strings of 13 bytes in 2 rows: one copy while the range is at most 26 + 16 * 2 = 58 bytes
    CheckDeclaredHeap({"ascending, a gap of 6", 40, 40, 4, 23, 32, 0, 19}, type);
    CheckDeclaredHeap({"range of exactly long bytes + 16 n, ending at the heap's end", 58, 58, 0, 45, 58, 0, 45}, type);
    CheckDeclaredHeap({"range one byte more", 59, 59, 0, 46, 26, 0, 13}, type);
    CheckDeclaredHeap({"last string ends one byte behind the declared heap", 58, 57, 0, 45, 26, 0, 13}, type);
    CheckDeclaredHeap({"descending pointers", 58, 58, 45, 0, 26, 0, 13}, type);
  }
  {   // a short row and a NULL row of garbage between two long strings of a declared heap: still one copy, and the second
      // append's pointers continue at heap_used
    std::vector<char> heap(50);
    for (size_t i = 0; i < heap.size(); i++) heap[i] = static_cast<char>('a' + i % 26);
    const char* h = Exact(heap);
    const std::vector<mi_string_t> rows = {Long(h + 4, 20), Short("xy"), Garbage(), Long(h + 30, 15)};
    mi_vector v = Vec(Exact(rows), Exact(std::vector<uint64_t>{0xB}));
    v.heap = h;
    v.heap_size = 50;
    ChunkCollection cc(kAlloc, {Typed(MI_AT_UTF8)});
    AppendChunk(cc, &v, 1, 4);
    AppendChunk(cc, &v, 1, 4);
    const auto& c = cc.columns[0];
    CHECK(c.heap_used == 82 && c.payload_bytes == 2 * 37 && cc.SizeInBytes() == 82 + 8 * 16, "mixed rows over a heap: heap_used %lld, payload %lld", (long long)c.heap_used, (long long)c.payload_bytes);
    CHECK(Rows(c)[0].value.pointer.ptr == 0 && Rows(c)[3].value.pointer.ptr == 26 && Rows(c)[4].value.pointer.ptr == 41 && Rows(c)[7].value.pointer.ptr == 67, "mixed rows over a heap: pointers");
    CHECK(std::memcmp(c.heap.get(), h + 4, 41) == 0 && std::memcmp(c.heap.get() + 41, h + 4, 41) == 0, "mixed rows over a heap: the copied range");
    CHECK(Rows(c)[2].value.pointer.ptr == 1 && Rows(c)[6].value.pointer.length == 1000, "mixed rows over a heap: the NULL row was touched");
  }
  {   // UUID: hugeint_t rows, 36 bytes of text per valid row
    ArrowField uuid = Typed(MI_AT_UTF8);
    uuid.extension = extfmt::kUuid;
    std::vector<mi_hugeint_t> rows(5);
    for (size_t i = 0; i < rows.size(); i++) rows[i] = mi_hugeint_t{0x1111111111111111ull * (i + 1), static_cast<int64_t>(i) - 2};
    const mi_hugeint_t* src = Exact(rows);
    const mi_vector nulls = Vec(src, Exact(std::vector<uint64_t>{0x15})), none = Vec(src);   // rows 1 and 3 are NULL
    ChunkCollection cc(kAlloc, {uuid});
    AppendChunk(cc, &nulls, 1, 5);
    CHECK(cc.columns[0].payload_bytes == 108 && cc.SizeInBytes() == 80, "uuid: payload %lld", (long long)cc.columns[0].payload_bytes);
    AppendChunk(cc, &none, 1, 5);
    CHECK(cc.columns[0].payload_bytes == 288 && cc.SizeInBytes() == 160 && !cc.columns[0].heap, "uuid: payload %lld after 5 valid rows more", (long long)cc.columns[0].payload_bytes);
    CHECK(std::memcmp(cc.columns[0].data.get() + 80, src, 80) == 0, "uuid: staged rows");
  }
}

// ------------------------------------------------------------------------------------------------ lists
void CheckLists() {
  {   // list<varchar>, child rows 1 and 3 long strings of a declared heap at offsets 0 and 20: gathered as ONE run of 5 rows they
      // are staged with one copy of 33 bytes, as two runs string by string
    std::vector<char> heap(33);
    for (size_t i = 0; i < heap.size(); i++) heap[i] = static_cast<char>('a' + i % 26);
    const char* h = Exact(heap);
    const std::vector<mi_string_t> rows = {Short("r0"), Long(h, 13), Short("r2"), Long(h + 20, 13), Short("r4")};
    mi_vector child = Vec(Exact(rows));
    child.heap = h;
    child.heap_size = 33;
    const ArrowField field = Parent(MI_AT_LIST, {Typed(MI_AT_UTF8)});
    {
      const mi_vector lists = Nested(Exact(std::vector<uint64_t>{0, 2, 2, 3}), nullptr, &child, 1);
      ChunkCollection cc(kAlloc, {field});
      AppendChunk(cc, &lists, 1, 2);
      CHECK(cc.columns[1].count == 5 && cc.columns[1].heap_used == 33 && cc.columns[0].payload_bytes == 5, "adjacent lists: %lld child rows, heap_used %lld",
            (long long)cc.columns[1].count, (long long)cc.columns[1].heap_used);
      CHECK(Rows(cc.columns[1])[3].value.pointer.ptr == 20, "adjacent lists: row 3 points at %llu", (unsigned long long)Rows(cc.columns[1])[3].value.pointer.ptr);
    }
    {
      const mi_vector lists = Nested(Exact(std::vector<uint64_t>{0, 2, 3, 1}), nullptr, &child, 1);
      ChunkCollection cc(kAlloc, {field});
      AppendChunk(cc, &lists, 1, 2);
      CHECK(cc.columns[1].count == 3 && cc.columns[1].heap_used == 26 && cc.columns[0].payload_bytes == 3, "lists one row apart: %lld child rows, heap_used %lld",
            (long long)cc.columns[1].count, (long long)cc.columns[1].heap_used);
      CHECK(Rows(cc.columns[1])[2].value.pointer.ptr == 13, "lists one row apart: row 2 points at %llu", (unsigned long long)Rows(cc.columns[1])[2].value.pointer.ptr);
    }
  }
  {   // list order, a NULL list with a garbage entry, an empty list
    std::vector<int32_t> values = {10, 11, 12, 13, 14, 15, 16};
    const mi_vector child = Vec(Exact(values));
    const std::vector<uint64_t> entries = {5, 2, 1ull << 40, 1ull << 40, 3, 0, 0, 3};
    const mi_vector lists = Nested(Exact(entries), Exact(std::vector<uint64_t>{0xD}), &child, 1);   // list 1 is NULL
    ChunkCollection cc(kAlloc, {Parent(MI_AT_LIST, {Int(32)})});
    AppendChunk(cc, &lists, 1, 4);
    const auto& l = cc.columns[0];
    const auto& c = cc.columns[1];
    const int32_t want[5] = {15, 16, 10, 11, 12};
    CHECK(l.count == 4 && l.has_nulls && l.payload_bytes == 5 && c.count == 5, "list order: %lld lists, %lld child rows", (long long)l.count, (long long)c.count);
    CHECK(std::memcmp(c.data.get(), want, sizeof(want)) == 0, "list order: child rows %d %d %d ..", c.data.get<int32_t>()[0], c.data.get<int32_t>()[1], c.data.get<int32_t>()[2]);
    CHECK(std::memcmp(l.data.get(), entries.data(), 64) == 0, "list order: the list_entry_t rows are staged as they are");
    CHECK(cc.SizeInBytes() == 4 * 16 + 5 * 4 && !l.large_offsets, "list order: SizeInBytes %lld", (long long)cc.SizeInBytes());
  }
  {   // list<null>: nothing is staged below, so 2^31 child rows cost nothing -- and are one more than int32 offsets can say
    const mi_vector child = Vec(nullptr);
    const mi_vector most = Nested(Exact(std::vector<uint64_t>{0, 0x7FFFFFFFull}), nullptr, &child, 1);
    const mi_vector one = Nested(Exact(std::vector<uint64_t>{0, 1}), nullptr, &child, 1);
    ChunkCollection cc(kAlloc, {Parent(MI_AT_LIST, {Typed(MI_AT_NULL)})});
    AppendChunk(cc, &most, 1, 1);
    CHECK(cc.columns[0].payload_bytes == 0x7FFFFFFFll && cc.columns[1].count == 0x7FFFFFFFll && !cc.columns[1].data && !cc.columns[1].validity, "list<null>: 2^31 - 1 child rows");
    CheckThrows<InvalidInputException>("list<null> past int32 offsets", [&] { AppendChunk(cc, &one, 1, 1); },
                                       "Arrow Appender: The maximum combined list offset for regular list buffers is 2147483647 but the offset of 2147483648 "
                                       "exceeds this.\n* SET arrow_large_buffer_size=true to use large list buffers");
    ChunkCollection large(kAlloc, {Parent(MI_AT_LARGE_LIST, {Typed(MI_AT_NULL)})});
    AppendChunk(large, &most, 1, 1);
    AppendChunk(large, &one, 1, 1);
    CHECK(large.columns[0].large_offsets && large.columns[0].payload_bytes == 0x80000000ll && large.columns[1].count == 0x80000000ll, "large list<null>: 2^31 child rows");
  }
  {   // a map is a list of struct<key, value>
    const mi_vector kv[2] = {Vec(Exact(std::vector<int32_t>{1, 2, 3})), Vec(Exact(std::vector<int64_t>{-1, -2, -3}))};
    const mi_vector entries = Nested(nullptr, nullptr, kv, 2);
    const mi_vector maps = Nested(Exact(std::vector<uint64_t>{1, 2}), nullptr, &entries, 1);
    ChunkCollection cc(kAlloc, {Parent(MI_AT_MAP, {Parent(MI_AT_STRUCT, {Int(32), Int(64)})})});
    AppendChunk(cc, &maps, 1, 1);
    CHECK(cc.columns[0].enc_kind == MI_K_ENC_LIST32 && !cc.columns[0].large_offsets && cc.columns[0].payload_bytes == 2 && cc.columns[1].count == 2, "map: staged as a list");
    CHECK(cc.columns[2].data.get<int32_t>()[0] == 2 && cc.columns[2].data.get<int32_t>()[1] == 3 && cc.columns[3].data.get<int64_t>()[0] == -2 && cc.columns[3].data.get<int64_t>()[1] == -3,
          "map: keys and values of the entries 1 and 2");
  }
}

// ------------------------------------------------------------------------------------------------ groups
void CheckGroups() {
  const std::vector<int32_t> a = {0, 1, 2, 3, 4, 5};
  const std::vector<int64_t> b = {0, 10, 20, 30, 40, 50};
  {   // list<struct<a, b>>, list (3, 2): the struct gets rows [3, 5) and passes them to both children
    const mi_vector ab[2] = {Vec(Exact(a)), Vec(Exact(b), Exact(std::vector<uint64_t>{~0ull & ~(1ull << 4)}))};
    const mi_vector st = Nested(nullptr, Exact(std::vector<uint64_t>{~0ull & ~(1ull << 3)}), ab, 2);
    const mi_vector lists = Nested(Exact(std::vector<uint64_t>{3, 2}), nullptr, &st, 1);
    ChunkCollection cc(kAlloc, {Parent(MI_AT_LIST, {Parent(MI_AT_STRUCT, {Int(32), Int(64)})})});
    AppendChunk(cc, &lists, 1, 1);
    const auto& s = cc.columns[1];
    CHECK(s.count == 2 && s.has_nulls && !Bit(s, 0) && Bit(s, 1) && !s.data && s.width == 0, "struct: its own rows and validity");
    CHECK(cc.columns[2].count == 2 && cc.columns[2].data.get<int32_t>()[0] == 3 && cc.columns[2].data.get<int32_t>()[1] == 4 && !cc.columns[2].has_nulls, "struct: child a");
    CHECK(cc.columns[3].count == 2 && cc.columns[3].data.get<int64_t>()[0] == 30 && cc.columns[3].data.get<int64_t>()[1] == 40 && Bit(cc.columns[3], 0) && !Bit(cc.columns[3], 1), "struct: child b");
    CHECK(cc.SizeInBytes() == 16 + 2 * 4 + 2 * 8, "struct: SizeInBytes %lld", (long long)cc.SizeInBytes());
  }
  {   // list<int32[3]>, list (1, 1): the fixed-size list gets row [1, 2) and passes rows [3, 6) to its child
    const mi_vector values = Vec(Exact(a));
    const mi_vector fsl = Nested(nullptr, nullptr, &values, 1);
    const mi_vector lists = Nested(Exact(std::vector<uint64_t>{1, 1}), nullptr, &fsl, 1);
    ChunkCollection cc(kAlloc, {Parent(MI_AT_LIST, {Parent(MI_AT_FIXED_LIST, {Int(32)}, 3)})});
    AppendChunk(cc, &lists, 1, 1);
    CHECK(cc.columns[1].count == 1 && cc.columns[1].param == 3 && cc.columns[2].count == 3, "fixed-size list: %lld rows, %lld child rows", (long long)cc.columns[1].count, (long long)cc.columns[2].count);
    CHECK(std::memcmp(cc.columns[2].data.get(), a.data() + 3, 12) == 0, "fixed-size list: child rows 3 .. 5");
  }
  {   // top level fixed_size_list(3) over two chunks
    const mi_vector values = Vec(Exact(a));
    const mi_vector fsl = Nested(nullptr, nullptr, &values, 1);
    ChunkCollection cc(kAlloc, {Parent(MI_AT_FIXED_LIST, {Int(32)}, 3)});
    AppendChunk(cc, &fsl, 1, 2);
    AppendChunk(cc, &fsl, 1, 1);
    CHECK(cc.Count() == 3 && cc.columns[1].count == 9 && cc.columns[1].data.get<int32_t>()[5] == 5 && cc.columns[1].data.get<int32_t>()[8] == 2, "fixed-size list: 3 rows are 9 child rows");
  }
  {
    const mi_vector only_a = Vec(Exact(a));
    const mi_vector few = Nested(nullptr, nullptr, &only_a, 1), none = Nested(nullptr, nullptr, nullptr, 2);
    ChunkCollection cc(kAlloc, {Parent(MI_AT_STRUCT, {Int(32), Int(64)})});
    CheckThrows<InvalidInputException>("struct vector with one child", [&] { AppendChunk(cc, &few, 1, 2); }, "nested vector without child vectors");
    CheckThrows<InvalidInputException>("struct vector without children", [&] { AppendChunk(cc, &none, 1, 2); }, "nested vector without child vectors");
    ChunkCollection lists(kAlloc, {Parent(MI_AT_LIST, {Int(32)})});
    const mi_vector childless = Vec(Exact(std::vector<uint64_t>{0, 1}));
    CheckThrows<InvalidInputException>("list vector without children", [&] { AppendChunk(lists, &childless, 1, 1); }, "nested vector without child vectors");
  }
}

// ------------------------------------------------------------------------------------------------ unions
void CheckUnions() {
  const ArrowField field = Parent(MI_AT_UNION, {Int(32), Typed(MI_AT_UTF8)});
  {   // list<union<int32, varchar>>, list (2, 4): union rows 2 .. 5 of 8.
      //   row        2      3      4      5
      //   tag        0      1      1      0
      //   union      valid  NULL   valid  valid
      //   member 0   valid  .      .      NULL     (own bits; its words start at bit 0)
      //   member 1   .      valid  valid  .        (own bits; its words start at bit 3: validity_shift 3)
      // -> member 0 is staged with the mask 1 0 0 0, member 1 with 0 0 1 0, and only row 4's string is staged
    const std::vector<uint8_t> tags = {7, 7, 0, 1, 1, 0, 7, 7};
    const std::vector<int32_t> ints = {100, 101, 102, 103, 104, 105, 106, 107};
    const std::string s3 = Text(14, 'd'), s4 = Text(17, 'm');
    const char* p4 = ExactText(s4);
    const std::vector<mi_string_t> strs = {Garbage(), Garbage(), Garbage(), Long(ExactText(s3), 14), Long(p4, 17), Garbage(), Garbage(), Garbage()};
    const uint8_t* tag_data = Exact(tags);
    const mi_vector members[3] = {Vec(tag_data), Vec(Exact(ints), Exact(std::vector<uint64_t>{0xFFull & ~(1ull << 5)})),
                                  Vec(Exact(strs), Exact(std::vector<uint64_t>{(1ull << (3 + 3)) | (1ull << (3 + 4))}), 3)};
    const mi_vector un = Nested(tag_data, Exact(std::vector<uint64_t>{0xFFull & ~(1ull << 3)}), members, 3);
    const mi_vector lists = Nested(Exact(std::vector<uint64_t>{2, 4}), nullptr, &un, 1);
    ChunkCollection cc(kAlloc, {Parent(MI_AT_LIST, {field})});
    AppendChunk(cc, &lists, 1, 1);
    const auto& u = cc.columns[1];
    const auto& m0 = cc.columns[2];
    const auto& m1 = cc.columns[3];
    const uint8_t want_tags[4] = {0, 1, 1, 0};
    CHECK(u.count == 4 && u.width == 1 && u.param == 2 && std::memcmp(u.data.get(), want_tags, 4) == 0, "union slice: the tags of rows 2 .. 5");
    CHECK(u.has_nulls && (u.validity.get<uint64_t>()[0] & 0xF) == 0xD, "union slice: the union's own validity %llx", (unsigned long long)(u.validity.get<uint64_t>()[0] & 0xF));
    CHECK(m0.count == 4 && m0.has_nulls && (m0.validity.get<uint64_t>()[0] & 0xF) == 0x1, "union slice: member 0's mask %llx", (unsigned long long)(m0.validity.get<uint64_t>()[0] & 0xF));
    CHECK(m0.data.get<int32_t>()[0] == 102 && m0.data.get<int32_t>()[3] == 105, "union slice: member 0's rows");
    CHECK(m1.count == 4 && m1.has_nulls && (m1.validity.get<uint64_t>()[0] & 0xF) == 0x4, "union slice: member 1's mask %llx", (unsigned long long)(m1.validity.get<uint64_t>()[0] & 0xF));
    CHECK(m1.payload_bytes == 17 && m1.heap_used == 17 && std::memcmp(m1.heap.get(), s4.data(), 17) == 0 && Rows(m1)[2].value.pointer.ptr == 0, "union slice: only the selected string is staged (%lld bytes)",
          (long long)m1.heap_used);
    CHECK(Rows(m1)[1].value.pointer.ptr == strs[3].value.pointer.ptr && Rows(m1)[0].value.pointer.ptr == 1, "union slice: a string that is not selected was touched");
    CHECK(cc.SizeInBytes() == 16 + 4 + 4 * 4 + 4 * 16 + 17, "union slice: SizeInBytes %lld", (long long)cc.SizeInBytes());
  }
  {   // top level, the tags in child 0 alone; a tag that names no member selects none
    const uint8_t* tag_data = Exact(std::vector<uint8_t>{1, 0, 2});
    const std::string s0 = Text(13, 'a');
    const std::vector<mi_string_t> strs = {Long(ExactText(s0), 13), Garbage(), Garbage()};
    const mi_vector members[3] = {Vec(tag_data), Vec(Exact(std::vector<int32_t>{7, 8, 9})), Vec(Exact(strs))};
    const mi_vector un = Nested(nullptr, nullptr, members, 3);
    ChunkCollection cc(kAlloc, {field});
    AppendChunk(cc, &un, 1, 3);
    const uint8_t want_tags[3] = {1, 0, 2};
    CHECK(cc.columns[0].count == 3 && !cc.columns[0].has_nulls && std::memcmp(cc.columns[0].data.get(), want_tags, 3) == 0, "union: tags from child 0");
    CHECK((cc.columns[1].validity.get<uint64_t>()[0] & 7) == 2 && (cc.columns[2].validity.get<uint64_t>()[0] & 7) == 1 && cc.columns[2].heap_used == 13, "union: member masks %llx, %llx",
          (unsigned long long)(cc.columns[1].validity.get<uint64_t>()[0] & 7), (unsigned long long)(cc.columns[2].validity.get<uint64_t>()[0] & 7));
    const mi_vector two = Nested(tag_data, nullptr, members, 2);
    CheckThrows<InvalidInputException>("union vector with a member missing", [&] { AppendChunk(cc, &two, 1, 3); },
                                       "union vector with 2 child vectors, the writer expects the tags and 2 members");
    const mi_vector no_tags[3] = {Vec(nullptr), members[1], members[2]};
    const mi_vector tagless = Nested(nullptr, nullptr, no_tags, 3);
    CheckThrows<InvalidInputException>("union vector without tags", [&] { AppendChunk(cc, &tagless, 1, 3); }, "union vector without tags");
  }
  ArrowField wide = Parent(MI_AT_UNION, std::vector<ArrowField>(33, Int(32)));
  wide.name = "u";
  const std::string refusal = "Column 'u': only sparse unions of 1 .. 32 members are encoded by the MI355X writer path";
  CheckThrows<NotImplementedException>("union of 33 members", [&] { ChunkCollection cc(kAlloc, {wide}); }, refusal);
  wide.children.resize(32);
  { ChunkCollection cc(kAlloc, {wide}); CHECK(cc.columns.size() == 33 && cc.columns[0].param == 32, "union of 32 members"); }
  wide.children.resize(2);
  wide.unit = 1;
  CheckThrows<NotImplementedException>("dense union", [&] { ChunkCollection cc(kAlloc, {wide}); }, refusal);
  wide.unit = 0;
  wide.children.clear();
  CheckThrows<NotImplementedException>("union without members", [&] { ChunkCollection cc(kAlloc, {wide}); }, refusal);
}

// ------------------------------------------------------------------------------------------------ null node, chunk checks
void CheckNullNodeAndChunks() {
  const mi_vector nothing = Vec(nullptr);
  const int allocs0 = g_allocs;
  ChunkCollection nulls(kAlloc, {Typed(MI_AT_NULL)});
  AppendChunk(nulls, &nothing, 1, 2048);
  AppendChunk(nulls, &nothing, 1, 7);
  CHECK(nulls.Count() == 2055 && nulls.columns[0].count == 2055 && nulls.SizeInBytes() == 0 && g_allocs == allocs0, "null node: %lld rows, %d allocations", (long long)nulls.columns[0].count, g_allocs - allocs0);
  CHECK(!nulls.columns[0].data && !nulls.columns[0].validity && !nulls.columns[0].heap && !nulls.columns[0].has_nulls, "null node: staged a buffer");

  ChunkCollection cc(kAlloc, {Int(32)});
  const mi_vector two[2] = {Vec(Exact(std::vector<int32_t>{1, 2})), Vec(Exact(std::vector<int32_t>{3, 4}))};
  CheckThrows<InvalidInputException>("two columns for one", [&] { AppendChunk(cc, two, 2, 2); }, "DataChunk has 2 columns, the writer expects 1");
  AppendChunk(cc, two, 1, 0);
  AppendChunk(cc, two, 1, -5);
  CHECK(cc.Count() == 0 && g_allocs == allocs0 && !cc.columns[0].data, "a chunk of no rows staged something");
  CheckThrows<InvalidInputException>("a chunk of 2048 * 1024 + 1 rows", [&] { AppendChunk(cc, two, 1, 2048 * 1024 + 1); }, "DataChunk too large");
  CheckThrows<InvalidInputException>("a vector without data", [&] { AppendChunk(cc, &nothing, 1, 2); }, "DataChunk column 0 has no data");
  CHECK(cc.Count() == 0, "a refused chunk was counted");
  AppendChunk(cc, two, 1, 2);
  CHECK(cc.Count() == 2 && cc.columns[0].data.get<int32_t>()[1] == 2, "the chunk after the refused ones");
}

// ------------------------------------------------------------------------------------------------ device staging layout
void CheckStagingLayout() {
  StagingLayout lay;
  LayOutStaging({StagingNode{100, 4, 0, false, 0}}, &lay);
  CHECK(lay.nodes.size() == 1 && lay.nodes[0].data == 0 && lay.nodes[0].validity == 512 && lay.nodes[0].heap == 768 && lay.total == 1024, "one node: %zu %zu %zu, total %zu",
        lay.nodes[0].data, lay.nodes[0].validity, lay.nodes[0].heap, lay.total);
  CHECK(lay.nodes[0].members == 0 && lay.nodes[0].masks == 0 && lay.nodes[0].mask_stride == 0, "one node: union extras of a node that is none");
  // 1000 rows of 16 bytes and 5000 heap bytes: 16016 -> 16128, 16 words + 8 -> 256, 5016 -> 5120
  LayOutStaging({StagingNode{100, 4, 0, false, 0}, StagingNode{1000, 16, 5000, false, 0}}, &lay);
  CHECK(lay.nodes.size() == 2 && lay.nodes[0].validity == 512 && lay.nodes[1].data == 1024 && lay.nodes[1].validity == 17152 && lay.nodes[1].heap == 17408 && lay.total == 22528,
        "two nodes: %zu %zu %zu, total %zu", lay.nodes[1].data, lay.nodes[1].validity, lay.nodes[1].heap, lay.total);
  // a union of 3 members over 100 rows, then its first member: 116 -> 256, 24 -> 256, 16 -> 256, 32 addresses = 256, 3 masks of 256
  LayOutStaging({StagingNode{100, 1, 0, true, 3}, StagingNode{100, 4, 0, false, 0}}, &lay);
  CHECK(lay.nodes[0].data == 0 && lay.nodes[0].validity == 256 && lay.nodes[0].heap == 512 && lay.nodes[0].members == 768 && lay.nodes[0].masks == 1024 && lay.nodes[0].mask_stride == 256,
        "union: %zu %zu %zu %zu %zu, stride %zu", lay.nodes[0].data, lay.nodes[0].validity, lay.nodes[0].heap, lay.nodes[0].members, lay.nodes[0].masks, lay.nodes[0].mask_stride);
  CHECK(lay.nodes[1].data == 1792 && lay.total == 1792 + 1024, "union: the node behind it starts at %zu, total %zu", lay.nodes[1].data, lay.total);
  // 15873 rows of 1 byte: 15889 -> 16128; 249 words + 8 = 2000 -> 2048 for the validity and for each of the 2 masks
  LayOutStaging({StagingNode{15873, 1, 0, true, 2}}, &lay);
  CHECK(lay.nodes[0].validity == 16128 && lay.nodes[0].heap == 18176 && lay.nodes[0].members == 18432 && lay.nodes[0].masks == 18688 && lay.nodes[0].mask_stride == 2048 && lay.total == 22784, "union of 15873 rows: stride %zu", lay.nodes[0].mask_stride);
  LayOutStaging({StagingNode{0, 4, 0, false, 0}}, &lay);
  CHECK(lay.nodes[0].data == 0 && lay.nodes[0].validity == 256 && lay.nodes[0].heap == 512 && lay.total == 768, "no rows: %zu %zu %zu, total %zu", lay.nodes[0].data, lay.nodes[0].validity, lay.nodes[0].heap, lay.total);
  LayOutStaging({}, &lay);
  CHECK(lay.nodes.empty() && lay.total == 0, "no nodes: total %zu", lay.total);
}

}  // namespace

int main() {
  for (int32_t shift : {0, 1, 63}) CheckSlicesAndShifts(shift);
  CheckWidths();
  CheckSliceEndsWithItsWord();
  CheckEncodePlans();
  CheckGrowthAndReset();
  CheckStrings();
  CheckLists();
  CheckGroups();
  CheckUnions();
  CheckNullNodeAndChunks();
  CheckStagingLayout();
  for (void* p : g_owned) std::free(p);
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
