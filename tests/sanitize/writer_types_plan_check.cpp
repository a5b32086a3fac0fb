// writer_types_plan_check.cpp -- the body layout and the encode tasks of union, interval and null nodes (MI_K_ENC_UNION,
// MI_K_ENC_INTERVAL, kEncNodeNull; duckdb-arrow_amd/csrc/writer_plan.cpp) without a GPU, under AddressSanitizer + UBSan
// (test infrastructure, never shipped).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I include tests/sanitize/writer_types_plan_check.cpp
//       duckdb-arrow_amd/csrc/writer_plan.cpp -lpthread -o writer_types_plan_check
//
// A union node has ONE buffer, its int8 type ids, and no bitmap; an interval node a bitmap and 16 bytes per row; a null node
// no buffer at all, wherever it stands -- first, last, between others, as a union's member.  Spans ascend, lie apart and start
// on multiples of 64; the compressor's blocks follow the spans, so a node without buffers and an empty batch cost none.
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

// buffer lengths of a node as the Arrow columnar format lists them (V5 metadata: a union has no validity buffer)
std::vector<int64_t> FormatLengths(const EncodeNode& c) {
  const int64_t n = c.rows, bitmap = (n + 7) / 8, offsets = (n + 1) * (c.large_offsets ? 8 : 4);
  switch (c.kind) {
    case kEncNodeNull: return {};
    case MI_K_ENC_UNION: return {n};
    case MI_K_ENC_INTERVAL: return {bitmap, 16 * n};
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
  const std::vector<lz4enc::BlockIn> cut = BlocksOfBody(lay);
  CHECK(static_cast<int64_t>(cut.size()) == blocks, "%s: %zu compressor blocks for spans that take %lld", what, cut.size(), (long long)blocks);
  // the compressed layout of that body, every block stored: as many spans, none for the nodes without buffers
  std::vector<uint32_t> words;
  for (const auto& b : cut) words.push_back(b.n | lz4enc::kStoredFlag);
  CompressedBodyLayout packed;
  LayOutCompressedBody(lay, words, &packed);
  CHECK(packed.spans.size() == lay.spans.size(), "%s: %zu compressed spans", what, packed.spans.size());
}

void CheckTasks(int64_t n) {
  const std::vector<EncodeNode> nodes = {EncodeNode{MI_K_ENC_COPY, 8, false, n, 0}, EncodeNode{kEncNodeNull, 0, false, n, 0},
                                         EncodeNode{MI_K_ENC_UNION, 3, false, n, 0}, EncodeNode{MI_K_ENC_COPY, 4, false, n, 0},
                                         EncodeNode{kEncNodeNull, 0, false, n, 0}, EncodeNode{MI_K_ENC_INTERVAL, 16, false, n, 0}};
  BodyLayout lay;
  LayOutBody(nodes, &lay);
  uint8_t* body = reinterpret_cast<uint8_t*>(uintptr_t{1} << 40);
  const uint8_t in[8] = {0};
  uint8_t scratch[8];
  EncodeInput ui{in, in + 1, nullptr, 0};
  ui.member_validity = in + 2;
  ui.masks = scratch;
  ui.mask_stride = 512;
  ui.parent_validity = in + 3;
  const mi_buffer_span* sp = &lay.spans[static_cast<size_t>(lay.first_span[2])];
  const mi_col_task u = EncodeTask(nodes[2], sp, ui, body);
  CHECK(u.kind == MI_K_ENC_UNION && u.nrows == n && u.param == 3 && u.flags == 0, "union task: kind %d, %lld rows, %lld members", u.kind, (long long)u.nrows, (long long)u.param);
  CHECK(u.buf1 == in && u.validity == in + 1 && u.buf2 == in + 2 && u.buf2_len == 512 && u.ptr_base == reinterpret_cast<uint64_t>(in + 3), "union task: inputs");
  CHECK(u.out_data == body + sp[0].offset && u.out_aux == scratch && u.out_validity == nullptr, "union task: type ids into the body, masks into scratch, no bitmap");
  CHECK(lay.first_span[1] == lay.first_span[2] && lay.first_span[4] == lay.first_span[5], "a null node takes no span: the next node starts where it would have");
  sp = &lay.spans[static_cast<size_t>(lay.first_span[5])];
  const mi_col_task iv = EncodeTask(nodes[5], sp, EncodeInput{in, in + 1, nullptr, 0}, body);
  CHECK(iv.kind == MI_K_ENC_INTERVAL && iv.nrows == n && iv.param == 16 && iv.buf1 == in && iv.validity == in + 1, "interval task: inputs");
  CHECK(iv.out_validity == body + sp[0].offset && iv.out_data == body + sp[1].offset && iv.out_aux == nullptr, "interval task: outputs follow the spans");
  CHECK(reinterpret_cast<uintptr_t>(iv.out_data) % 16 == 0 && reinterpret_cast<uintptr_t>(u.out_data) % 16 == 0, "16-byte aligned outputs");
}
}  // namespace

int main() {
  for (int64_t n : {0, 1, 64, 2049, 122880}) {
    const std::string rows = " of " + std::to_string(n) + " rows";
    CheckLayout(("null alone" + rows).c_str(), {EncodeNode{kEncNodeNull, 0, false, n, 0}});
    CheckLayout(("interval alone" + rows).c_str(), {EncodeNode{MI_K_ENC_INTERVAL, 16, false, n, 0}});
    CheckLayout(("union(int, varchar)" + rows).c_str(),
                {EncodeNode{MI_K_ENC_UNION, 2, false, n, 0}, EncodeNode{MI_K_ENC_COPY, 4, false, n, 0}, EncodeNode{MI_K_ENC_STR32, 0, false, n, 7 * n}});
    CheckLayout(("null first, between and last" + rows).c_str(),
                {EncodeNode{kEncNodeNull, 0, false, n, 0}, EncodeNode{MI_K_ENC_COPY, 8, false, n, 0}, EncodeNode{kEncNodeNull, 0, false, n, 0},
                 EncodeNode{MI_K_ENC_INTERVAL, 16, false, n, 0}, EncodeNode{kEncNodeNull, 0, false, n, 0}});
    // struct(k, union(struct(p), list<int>, null, interval)): the members are nodes of their own, depth first
    CheckLayout(("a union under a struct with nested members" + rows).c_str(),
                {EncodeNode{MI_K_ENC_VALIDITY, 0, false, n, 0}, EncodeNode{MI_K_ENC_COPY, 8, false, n, 0}, EncodeNode{MI_K_ENC_UNION, 4, false, n, 0},
                 EncodeNode{MI_K_ENC_VALIDITY, 0, false, n, 0}, EncodeNode{MI_K_ENC_COPY, 4, false, n, 0}, EncodeNode{MI_K_ENC_LIST32, 0, true, n, 2 * n},
                 EncodeNode{MI_K_ENC_COPY, 4, false, 2 * n, 0}, EncodeNode{kEncNodeNull, 0, false, n, 0}, EncodeNode{MI_K_ENC_INTERVAL, 16, false, n, 0}});
    if (n > 0) CheckTasks(n);
  }
  BodyLayout lay;
  LayOutBody({EncodeNode{kEncNodeNull, 0, false, 5000, 0}}, &lay);
  CHECK(lay.spans.empty() && lay.body_size == 0 && BlocksOfBody(lay).empty(), "a batch of one null column has an empty body");
  std::printf("writer_types_plan_check: %d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
