// writer_view_plan_check.cpp -- the body layout and the encode task of a string-view node (MI_K_ENC_STRVIEW,
// duckdb-arrow_amd/csrc/writer_plan.cpp) without a GPU, under AddressSanitizer + UBSan (test infrastructure, never shipped).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I include tests/sanitize/writer_view_plan_check.cpp
//       duckdb-arrow_amd/csrc/writer_plan.cpp -lpthread -o writer_view_plan_check
//
// A view node has three buffers -- bitmap, 16 bytes of view per row, ONE data buffer of the long bytes, present with length
// 0 when there are none -- ascending, apart and on multiples of 64, at 0, 1, 64 and 2049 rows, alone, under a list and
// beside other kinds; arrow_large_buffer_size does not touch it; its long bytes end at INT32_MAX (the device's
// MI_ST_OFFSET_OVERFLOW takes 2 GiB of output to reach: this is the tested refusal); the compressor's blocks follow the spans.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

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

// buffer lengths of a node as the Arrow columnar format lists them ("Variable-size Binary View Layout": validity, views, and
// here exactly one variadic data buffer)
std::vector<int64_t> FormatLengths(const EncodeNode& c) {
  const int64_t n = c.rows, bitmap = (n + 7) / 8, offsets = (n + 1) * (c.large_offsets ? 8 : 4);
  switch (c.kind) {
    case MI_K_ENC_STRVIEW: return {bitmap, 16 * n, c.payload_bytes};
    case MI_K_ENC_STR32: return {bitmap, offsets, c.payload_bytes};
    case MI_K_ENC_LIST32: return {bitmap, offsets};
    case MI_K_ENC_COPY: return {bitmap, n * c.param};
    default: return {bitmap};
  }
}

void CheckLayout(const char* what, const std::vector<EncodeNode>& nodes) {
  BodyLayout lay;
  LayOutBody(nodes, &lay);
  std::vector<int64_t> want;
  CHECK(lay.first_span.size() == nodes.size(), "%s: first_span has %zu entries", what, lay.first_span.size());
  for (size_t i = 0; i < nodes.size(); i++) {
    CHECK(lay.first_span[i] == static_cast<int32_t>(want.size()), "%s: node %zu starts at span %d, not %zu", what, i, lay.first_span[i], want.size());
    for (int64_t len : FormatLengths(nodes[i])) want.push_back(len);
  }
  CHECK(lay.spans.size() == want.size(), "%s: %zu spans, the format has %zu", what, lay.spans.size(), want.size());
  if (lay.spans.size() != want.size()) return;
  int64_t end = 0, blocks = 0;
  for (size_t k = 0; k < want.size(); k++) {
    const mi_buffer_span& s = lay.spans[k];
    CHECK(s.length == want[k], "%s: span %zu is %lld bytes, not %lld", what, k, (long long)s.length, (long long)want[k]);
    CHECK(s.offset % 64 == 0, "%s: span %zu starts at %lld", what, k, (long long)s.offset);
    CHECK(s.offset >= end, "%s: span %zu at %lld overlaps the one before (ends %lld)", what, k, (long long)s.offset, (long long)end);
    end = s.offset + s.length;
    blocks += (s.length + lz4enc::kBlockSize - 1) / lz4enc::kBlockSize;
  }
  CHECK(lay.body_size == (end + 63) / 64 * 64, "%s: body of %lld bytes, last span ends at %lld", what, (long long)lay.body_size, (long long)end);
  // COMPRESSION lz4 cuts the spans, whatever node they belong to: an empty data buffer has no block
  const std::vector<lz4enc::BlockIn> cut = BlocksOfBody(lay);
  CHECK(static_cast<int64_t>(cut.size()) == blocks, "%s: %zu compressor blocks for spans that take %lld", what, cut.size(), (long long)blocks);
}

void CheckTask(const EncodeNode& node, const std::vector<EncodeNode>& before) {
  std::vector<EncodeNode> nodes = before;
  nodes.push_back(node);
  BodyLayout lay;
  LayOutBody(nodes, &lay);
  uint8_t* body = reinterpret_cast<uint8_t*>(uintptr_t{1} << 40);
  const uint8_t in[4] = {0, 0, 0, 0};
  const mi_buffer_span* sp = &lay.spans[static_cast<size_t>(lay.first_span.back())];
  const mi_col_task t = EncodeTask(node, sp, EncodeInput{in, in + 1, in + 2, 0x1234}, body);
  CHECK(t.kind == MI_K_ENC_STRVIEW && t.nrows == node.rows && t.flags == 0, "view task: kind %d, %lld rows, flags %d", t.kind, (long long)t.nrows, t.flags);
  CHECK(t.buf1 == in && t.validity == in + 1 && t.buf2 == in + 2 && t.ptr_base == 0x1234, "view task: inputs");
  CHECK(t.out_validity == body + sp[0].offset && t.out_data == body + sp[1].offset && t.out_aux == body + sp[2].offset, "view task: outputs follow the spans");
  CHECK(t.buf2_len == node.payload_bytes, "view task: buf2_len %lld", (long long)t.buf2_len);
  CHECK(reinterpret_cast<uintptr_t>(t.out_data) % 16 == 0, "view task: views are 16-byte aligned");
}

std::string Refusal(const std::vector<EncodeNode>& nodes) {
  BodyLayout lay;
  try {
    LayOutBody(nodes, &lay);
  } catch (const InvalidInputException& e) {
    return e.what();
  }
  return "";
}
}  // namespace

int main() {
  for (int64_t n : {0, 1, 64, 2049}) {
    const std::string rows = " of " + std::to_string(n) + " rows";
    for (bool large : {false, true}) {   // large_offsets is the LIST's and the BLOB's business
      CheckLayout(("view without long bytes" + rows).c_str(), {EncodeNode{MI_K_ENC_STRVIEW, 0, large, n, 0}});
      CheckLayout(("view" + rows).c_str(), {EncodeNode{MI_K_ENC_STRVIEW, 0, large, n, n * 29}});
      // list<varchar>: 3 child rows per list
      CheckLayout(("list<view>" + rows).c_str(), {EncodeNode{MI_K_ENC_LIST32, 0, large, n, 3 * n}, EncodeNode{MI_K_ENC_STRVIEW, 0, false, 3 * n, 40 * n}});
      CheckLayout(("view, blob, int" + rows).c_str(),
                  {EncodeNode{MI_K_ENC_STRVIEW, 0, false, n, 13 * n}, EncodeNode{MI_K_ENC_STR32, 0, large, n, 5 * n}, EncodeNode{MI_K_ENC_COPY, 4, false, n, 0}});
      CheckTask(EncodeNode{MI_K_ENC_STRVIEW, 0, large, n, 13 * n}, {EncodeNode{MI_K_ENC_COPY, 8, false, n, 0}});
    }
    BodyLayout lay;
    LayOutBody({EncodeNode{MI_K_ENC_STRVIEW, 0, false, n, 0}}, &lay);
    CHECK(lay.spans.size() == 3 && lay.spans[2].length == 0, "the data buffer is present with length 0%s", rows.c_str());
  }
  // view offsets are int32 and there is no large variant (no buffer of that size is made: the layout is arithmetic)
  const int64_t big = 2147483648ll;
  for (bool large : {false, true}) {
    const std::string message = Refusal({EncodeNode{MI_K_ENC_STRVIEW, 0, large, 10, big}});
    CHECK(message.find("The maximum total string size for a string view buffer is 2147483647") != std::string::npos &&
              message.find("2147483648") != std::string::npos && message.find("produce_arrow_string_view=false") != std::string::npos,
          "INT32_MAX + 1 long bytes: \"%s\"", message.c_str());
    CHECK(Refusal({EncodeNode{MI_K_ENC_STRVIEW, 0, large, 10, big - 1}}).empty(), "INT32_MAX long bytes fit");
    BodyLayout lay;
    LayOutBody({EncodeNode{MI_K_ENC_STRVIEW, 0, large, 10, big - 1}}, &lay);
    CHECK(lay.spans.size() == 3 && lay.spans[1].length == 160 && lay.spans[2].length == big - 1, "INT32_MAX long bytes: spans");
  }
  CHECK(!Refusal({EncodeNode{MI_K_ENC_LIST32, 0, true, 5, 10}, EncodeNode{MI_K_ENC_STRVIEW, 0, false, 10, big}}).empty(), "the limit holds under a large list");
  std::printf("writer_view_plan_check: %d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
