// writer_plan.cpp -- see writer_plan.hpp.
#include "writer_plan.hpp"

#include <algorithm>
#include <cstring>

#include "union_format.hpp"

namespace miarrow {

void LayOutBody(const std::vector<EncodeNode>& nodes, BodyLayout* out) {
  out->spans.clear();
  out->first_span.assign(nodes.size(), 0);
  size_t body_off = 0;
  auto add_span = [&](int64_t len) {
    out->spans.push_back(mi_buffer_span{static_cast<int64_t>(body_off), len});
    body_off += RoundUp(static_cast<size_t>(len), kBufferAlign);
  };
  for (size_t i = 0; i < nodes.size(); i++) {
    const EncodeNode& c = nodes[i];
    const int64_t n = c.rows;
    if (n > 0x7FFFFFFFll) throw InvalidInputException("record batch too large");
    out->first_span[i] = static_cast<int32_t>(out->spans.size());
    if (c.kind == kEncNodeNull) continue;   // no buffers
    if (c.kind == MI_K_ENC_UNION) {         // type ids alone
      add_span(n);
      continue;
    }
    add_span((n + 7) / 8);
    const int64_t off_width = c.large_offsets ? 8 : 4;
    switch (c.kind) {
      case MI_K_ENC_LIST32: add_span((n + 1) * off_width); break;
      case MI_K_ENC_COPY: add_span(n * c.param); break;
      case MI_K_ENC_DEC128: case MI_K_ENC_INTERVAL: add_span(n * 16); break;
      case MI_K_ENC_BOOL: add_span((n + 7) / 8); break;
      case MI_K_ENC_STR32: case MI_K_ENC_UUID_TEXT:
        if (c.payload_bytes > 0x7FFFFFFFll && !c.large_offsets) {
          throw InvalidInputException(
              "Arrow Appender: The maximum total string size for regular string buffers is 2147483647 but the offset of " +
              std::to_string(c.payload_bytes) + " exceeds this.\n* SET arrow_large_buffer_size=true to use large string buffers");
        }
        add_span((n + 1) * off_width);
        add_span(c.payload_bytes);
        break;
      case MI_K_ENC_STRVIEW:   // views, then the one data buffer: present (length 0) even when no row is longer than 12 bytes
        if (c.payload_bytes > 0x7FFFFFFFll) {
          throw InvalidInputException(
              "Arrow Appender: The maximum total string size for a string view buffer is 2147483647 but the strings of more than 12 "
              "bytes of this record batch take " + std::to_string(c.payload_bytes) +
              " bytes.\n* Write smaller row groups, or SET produce_arrow_string_view=false and arrow_large_buffer_size=true");
        }
        add_span(n * 16);
        add_span(c.payload_bytes);
        break;
      default: break;   // struct / fixed-size list: the bitmap alone
    }
  }
  out->body_size = static_cast<int64_t>(body_off);
}

void LayOutStaging(const std::vector<StagingNode>& nodes, StagingLayout* out) {
  out->nodes.assign(nodes.size(), StagingLayout::Node{0, 0, 0, 0, 0, 0});
  size_t at = 0;
  for (size_t i = 0; i < nodes.size(); i++) {
    const StagingNode& c = nodes[i];
    StagingLayout::Node& o = out->nodes[i];
    const size_t validity_bytes = static_cast<size_t>((c.rows + 63) / 64) * 8;
    o.data = at;
    at += RoundUp(static_cast<size_t>(c.rows) * static_cast<size_t>(c.width) + 16, 256);
    o.validity = at;
    at += RoundUp(validity_bytes + 8, 256);
    o.heap = at;
    at += RoundUp(static_cast<size_t>(c.heap_used) + 16, 256);
    if (c.is_union) {
      o.members = at;
      at += RoundUp(static_cast<size_t>(unionfmt::kMaxMembers) * 8, 256);
      o.mask_stride = RoundUp(validity_bytes + 8, 256);
      o.masks = at;
      at += o.mask_stride * static_cast<size_t>(c.n_members);
    }
  }
  out->total = at;
}

mi_col_task EncodeTask(const EncodeNode& node, const mi_buffer_span* spans, const EncodeInput& in, uint8_t* body) {
  mi_col_task t;
  std::memset(&t, 0, sizeof(t));
  t.nrows = node.rows;
  t.kind = node.kind;
  t.validity = in.validity;
  t.buf1 = in.data;
  if (node.kind == MI_K_ENC_UNION) {   // type ids into the body, the members' masks into scratch; no bitmap
    t.param = node.param;
    t.buf2 = in.member_validity;
    t.buf2_len = in.mask_stride;
    t.ptr_base = reinterpret_cast<uint64_t>(in.parent_validity);
    t.out_data = body + spans[0].offset;
    t.out_aux = in.masks;
    return t;
  }
  t.out_validity = body + spans[0].offset;
  if (node.kind == MI_K_ENC_VALIDITY) {   // the node's own bitmap + NULL count
    t.out_data = body + spans[0].offset;
    return t;
  }
  t.flags = node.large_offsets && node.kind != MI_K_ENC_STRVIEW ? 1 : 0;
  t.out_data = body + spans[1].offset;
  if (node.kind == MI_K_ENC_LIST32) return t;   // bitmap + int32 (or int64) offsets from the staged list_entry_t rows
  t.param = node.param;
  if (node.kind == MI_K_ENC_UUID_TEXT) {   // no heap: the text is made from the rows
    t.buf2_len = node.payload_bytes;
    t.out_aux = body + spans[2].offset;
  }
  if (node.kind == MI_K_ENC_STR32 || node.kind == MI_K_ENC_STRVIEW) {
    t.buf2 = in.heap;
    t.buf2_len = node.payload_bytes;
    t.ptr_base = in.ptr_base;
    t.out_aux = body + spans[2].offset;
  }
  return t;
}

std::vector<lz4enc::BlockIn> BlocksOfBody(const BodyLayout& plain) {
  std::vector<lz4enc::BlockIn> blocks;
  for (const mi_buffer_span& sp : plain.spans)
    for (int64_t at = 0; at < sp.length; at += lz4enc::kBlockSize)
      blocks.push_back(lz4enc::BlockIn{static_cast<uint64_t>(sp.offset + at),
                                       static_cast<uint32_t>(std::min<int64_t>(lz4enc::kBlockSize, sp.length - at)), 0});
  return blocks;
}

void LayOutCompressedBody(const BodyLayout& plain, const std::vector<uint32_t>& words, CompressedBodyLayout* out) {
  using namespace lz4enc;
  out->spans.clear();
  out->copies.clear();
  int64_t at = 0;
  size_t block = 0;
  auto immediate = [&](uint64_t bytes, uint32_t len) {
    out->copies.push_back(BodyCopy{at, 0, len, kFromImmediate, bytes});
    at += len;
  };
  for (const mi_buffer_span& sp : plain.spans) {
    const int64_t n = sp.length, n_blocks = BlocksOf(n);
    if (block + static_cast<size_t>(n_blocks) > words.size()) throw InternalException("compressed body: fewer size words than blocks");
    if (n == 0) {
      out->spans.push_back(mi_buffer_span{at, 0});
      continue;
    }
    const int64_t start = at;
    const bool framed = FrameWins(FrameSize(words.data() + block, n_blocks), n);
    immediate(framed ? static_cast<uint64_t>(n) : ~0ull, 8);
    if (framed) immediate(kFrameHeader, kFrameHeaderSize);
    for (int64_t b = 0; b < n_blocks; b++, block++) {
      const uint32_t word = words[block], size = word & ~kStoredFlag;
      const int64_t in_block = std::min<int64_t>(kBlockSize, n - b * kBlockSize);
      const bool stored = (word & kStoredFlag) != 0;
      if (size == 0 || size > in_block || (stored && size != in_block)) throw InternalException("compressed body: impossible block size word");
      if (framed) immediate(word, 4);
      if (!framed || stored) out->copies.push_back(BodyCopy{at, sp.offset + b * kBlockSize, static_cast<uint32_t>(in_block), kFromBody, 0});
      else out->copies.push_back(BodyCopy{at, static_cast<int64_t>(block) * kSlotStride, size, kFromSlots, 0});
      at += framed ? size : in_block;
    }
    if (framed) immediate(0, kFrameEndSize);
    out->spans.push_back(mi_buffer_span{start, at - start});
    at = static_cast<int64_t>(RoundUp(static_cast<size_t>(at), 8));
  }
  if (block != words.size()) throw InternalException("compressed body: more size words than blocks");
  out->body_size = at;
}

std::vector<CutPiece> RowGroupCutter::Cut(int64_t rows) {
  std::vector<CutPiece> pieces;
  const int32_t n_windows = static_cast<int32_t>((rows + MI_VECTOR_SIZE - 1) / MI_VECTOR_SIZE);
  int32_t w0 = 0;
  bool fresh = open_rows == 0;
  for (int32_t wi = 0; wi < n_windows; wi++) {
    open_rows += std::min<int64_t>(MI_VECTOR_SIZE, rows - static_cast<int64_t>(wi) * MI_VECTOR_SIZE);
    const bool full = open_rows >= rows_per_group;
    if (!full && wi + 1 < n_windows) continue;
    pieces.push_back(CutPiece{w0, wi + 1, fresh, full});
    w0 = wi + 1;
    if (full) {
      open_rows = 0;
      fresh = true;
    }
  }
  return pieces;
}

}  // namespace miarrow
