// batch_slice.cpp -- see batch_slice.hpp.
#include "batch_slice.hpp"

#include <algorithm>
#include <cstring>
#include <string>

#include "io_pool.hpp"

namespace miarrow {

// ------------------------------------------------------------------------------------------------ record-batch walk
namespace {
//! One field node of a record batch, in the depth-first order of RecordBatch.nodes
struct WalkNode {
  const ArrowField* field;
  bool value_only;                  // the values of a dictionary batch
  int32_t column;                   // the top-level column it belongs to
  int32_t depth;
  int64_t parent;                   // node index of its parent, -1 at the top
  size_t node;                      // index into RecordBatch.nodes: may lie past its end
  size_t first_buffer, n_buffers;   // its RecordBatch.buffers entries, layout.n then the variadic ones: may run past the end
  FieldLayout layout;
  const char* defect;               // its variadicBufferCounts entry is missing (counted as 0) or out of range (clamped)
};

struct WalkEnd {
  size_t nodes = 0, buffers = 0, variadic = 0;  // entries the walk consumed
  bool defect = false;                          // some node has a WalkNode::defect
  bool unknown_dictionary = false;              // a DictionaryBatch whose id no field carries: nothing was visited
};

const ArrowField* FindDictionary(const ArrowField& f, int64_t id) {
  if (f.has_dictionary && f.dict_id == id) return &f;
  for (auto& c : f.children)
    if (const ArrowField* hit = FindDictionary(c, id)) return hit;
  return nullptr;
}

template <class Visit>
void WalkField(const ArrowField& f, const RecordBatchMeta& meta, int32_t column, int64_t parent, int32_t depth, bool value_only,
               WalkEnd* end, Visit& visit) {
  WalkNode v{&f, value_only, column, depth, parent, end->nodes++, end->buffers, 0, f.Layout(value_only), nullptr};
  v.n_buffers = static_cast<size_t>(v.layout.n);
  if (v.layout.variadic) {
    if (end->variadic >= meta.variadic_counts.size()) {
      v.defect = "RecordBatch has too few variadicBufferCounts";
    } else {
      const int64_t vc = meta.variadic_counts[end->variadic++];
      if (vc < 0 || vc > (1 << 20)) v.defect = "Invalid variadic buffer count";
      v.n_buffers += static_cast<size_t>(std::min<int64_t>(std::max<int64_t>(vc, 0), 1 << 20));
    }
    end->defect |= v.defect != nullptr;
  }
  end->buffers += v.n_buffers;
  visit(v);
  if (f.has_dictionary && !value_only) return;  // its values and their children live in the dictionary batch
  for (auto& c : f.children) WalkField(c, meta, column, static_cast<int64_t>(v.node), depth + 1, false, end, visit);
}

//! Visits every field node a RecordBatch (all columns) or a DictionaryBatch (the values of the field that carries its id,
//! at any depth) covers, and keeps the cursors of RecordBatch.{nodes, buffers, variadicBufferCounts} in step.  It never
//! throws: what the metadata lacks shows as an index past the end or as WalkNode::defect, and each caller decides --
//! SliceBatch refuses the batch, the bound / swap / projection helpers fall back to what is safe.
template <class Visit>
WalkEnd WalkBatch(const std::vector<ArrowField>& fields, const RecordBatchMeta& meta, Visit&& visit) {
  WalkEnd end;
  for (size_t i = 0; i < fields.size(); i++) {
    if (!meta.is_dictionary) {
      WalkField(fields[i], meta, static_cast<int32_t>(i), -1, 0, false, &end, visit);
    } else if (const ArrowField* owner = FindDictionary(fields[i], meta.dict_id)) {
      WalkField(*owner, meta, static_cast<int32_t>(i), -1, 0, true, &end, visit);
      return end;
    }
  }
  end.unknown_dictionary = meta.is_dictionary;
  return end;
}

// Upper bound of the UNCOMPRESSED size of buffer k of a node of n <= 2^40 rows: a compressed buffer declares its own
// uncompressed length, and that number sizes an allocation (pinned, for scans) before a byte is decoded -- a few damaged
// bytes must not be able to ask for terabytes.  Bitmaps, values and offsets are bounded by the row count, string data by
// the offset width (2 GiB for int32 offsets); what is not known keeps 2^40.
constexpr int64_t kLooseBound = int64_t(1) << 40;
int64_t BufferBound(const FieldLayout& l, int32_t k, int64_t n) {
  auto rows = [&](int64_t extra_rows) {
    int64_t b = 0;
    const int64_t per_row = l.buffers[k].width;
    if (per_row <= 0 || __builtin_mul_overflow(n + extra_rows, per_row, &b) || b > kLooseBound) return kLooseBound;
    return b + 64;
  };
  switch (l.buffers[k].role) {
    case BufferRole::VALIDITY: case BufferRole::BITS: return (n + 7) / 8 + 64;
    case BufferRole::FIXED: return rows(0);
    case BufferRole::OFFSETS: return rows(1);
    case BufferRole::PAYLOAD: return l.buffers[k - 1].width == 4 ? (int64_t(1) << 31) + 64 : kLooseBound;
  }
  return kLooseBound;
}
}  // namespace

// Per RecordBatch.buffers entry: does a projected column own it?  Empty = all of them (no projection, dictionary batch,
// or metadata the walk cannot follow -- the full validation reports that).
std::vector<char> NeededBuffers(const ArrowSchemaModel& schema, const std::vector<int32_t>& projected_columns, const RecordBatchMeta& meta) {
  std::vector<char> need;
  if (projected_columns.empty() || meta.is_dictionary) return need;
  std::vector<char> wanted(schema.fields.size(), 0);
  for (int32_t c : projected_columns) wanted[static_cast<size_t>(c)] = 1;
  need.assign(meta.buffers.size(), 0);
  const WalkEnd walked = WalkBatch(schema.fields, meta, [&](const WalkNode& v) {
    if (wanted[static_cast<size_t>(v.column)])
      for (size_t k = v.first_buffer; k < v.first_buffer + v.n_buffers && k < need.size(); k++) need[k] = 1;
  });
  if (walked.defect || walked.buffers > meta.buffers.size()) return {};
  return need;
}

std::vector<std::pair<int64_t, int64_t>> ProjectedBodyRanges(const ArrowSchemaModel& schema, const std::vector<int32_t>& projected_columns,
                                                             const RecordBatchMeta& meta, int64_t body_length, int64_t gap) {
  std::vector<std::pair<int64_t, int64_t>> ranges;
  const std::vector<char> needed = NeededBuffers(schema, projected_columns, meta);
  if (needed.empty()) return ranges;
  std::vector<std::pair<int64_t, int64_t>> need;
  for (size_t k = 0; k < meta.buffers.size(); k++) {
    if (!needed[k]) continue;
    const mi_buffer_span& b = meta.buffers[k];
    if (b.length <= 0) continue;
    if (!SpanInside(b.offset, b.length, body_length)) return {};  // malformed: read everything, validation reports it
    need.emplace_back(b.offset, b.offset + ((b.length + 7) & ~int64_t(7)));  // + the 8-byte padding kernels may touch
  }
  std::sort(need.begin(), need.end());
  for (auto& r : need) {
    const int64_t hi = std::min(r.second, body_length);
    if (!ranges.empty() && r.first <= ranges.back().second + gap) ranges.back().second = std::max(ranges.back().second, hi);
    else ranges.emplace_back(r.first, hi);
  }
  if (ranges.empty()) ranges.emplace_back(0, 0);  // nothing to read at all (projection of empty buffers)
  return ranges;
}

// Pass 1 over a compressed body: uncompressed sizes -> layout of the new body (every buffer 64-byte aligned); buffers of
// columns outside the projection are neither read (DecodeBody) nor decompressed: their length becomes 0 in `meta`.
DecompressedLayout LayOutDecompressedBody(const ArrowSchemaModel& schema, const std::vector<int32_t>& projected_columns,
                                          RecordBatchMeta* meta, const uint8_t* body, int64_t body_size,
                                          FrameContentSize frame_content_size) {
  const std::vector<char> needed = NeededBuffers(schema, projected_columns, *meta);
  const size_t nbuf = meta->buffers.size();
  std::vector<int64_t> bound(nbuf, kLooseBound);
  const WalkEnd walked = WalkBatch(schema.fields, *meta, [&](const WalkNode& v) {
    const int64_t n = v.node < meta->nodes.size() ? std::max<int64_t>(0, std::min(meta->nodes[v.node].first, kLooseBound)) : kLooseBound;
    for (int32_t k = 0; k < v.layout.n && v.first_buffer + k < nbuf; k++) bound[v.first_buffer + k] = BufferBound(v.layout, k, n);
  });
  if (walked.buffers != nbuf) bound.assign(nbuf, kLooseBound);  // metadata the walk cannot follow: validation reports it
  DecompressedLayout lay;
  lay.ulen.assign(nbuf, 0);
  lay.opos.assign(nbuf, 0);
  for (size_t i = 0; i < nbuf; i++) {
    mi_buffer_span& b = meta->buffers[i];
    lay.opos[i] = lay.total;
    if (!needed.empty() && !needed[i]) {
      b.length = 0;
      continue;
    }
    if (b.length == 0) continue;
    if (b.length < 8 || !SpanInside(b.offset, b.length, body_size))
      throw InternalException("Compressed buffer " + std::to_string(i) + " lies outside the message body");
    int64_t declared;
    std::memcpy(&declared, body + b.offset, 8);
    const int64_t n = declared == -1 ? b.length - 8 : declared;
    if (n < 0) throw IOException("Compressed buffer " + std::to_string(i) + " declares a negative uncompressed length");
    if (n > bound[i] || lay.total > (int64_t(1) << 41))
      throw IOException("Compressed buffer " + std::to_string(i) + " declares an uncompressed length of " + std::to_string(n) +
                        " bytes, more than its field node (" + std::to_string(bound[i]) + " bytes at most) can hold");
    // a frame header that carries the content size too (ZSTD): a length prefix that disagrees with it is rejected before
    // anything is allocated for it (the reference finds out after decompressing: base_stream_reader.cpp:24-29)
    uint64_t fcs = 0;
    if (frame_content_size && declared != -1 && frame_content_size(body + b.offset + 8, b.length - 8, &fcs) && fcs != static_cast<uint64_t>(n))
      throw IOException("Expected decompressed size of " + std::to_string(n) + " bytes but got " + std::to_string(fcs) + " bytes");
    lay.ulen[i] = n;
    lay.total += (n + 63) & ~static_cast<int64_t>(63);
  }
  return lay;
}

// list / map columns: the planner samples their offsets on the host (child windows of every chunk), so their record batches
// need the decompressed body in host memory
static bool HasListField(const ArrowField& f) {
  if (f.type == MI_AT_LIST || f.type == MI_AT_LARGE_LIST || f.type == MI_AT_MAP) return true;
  for (auto& c : f.children)
    if (HasListField(c)) return true;
  return false;
}

// GPU consumers (SetDeferLz4 / SetDeferZstd): the body may stay compressed and go out with the frame / block tables instead
bool MayStayCompressed(const ArrowSchemaModel& schema, const std::vector<int32_t>& projected_columns, const RecordBatchMeta& meta,
                       int64_t decompressed_size, int64_t body_size) {
  constexpr int64_t kLimit = (int64_t(1) << 31) - 64;   // the kernels' tables hold 32-bit positions
  if (meta.is_dictionary || schema.endianness != 0 || decompressed_size >= kLimit || body_size >= kLimit) return false;
  if (projected_columns.empty()) return std::none_of(schema.fields.begin(), schema.fields.end(), HasListField);
  return std::none_of(projected_columns.begin(), projected_columns.end(), [&](int32_t c) { return HasListField(schema.fields[static_cast<size_t>(c)]); });
}

// ------------------------------------------------------------------------------------------------ big-endian bodies
namespace {
void SwapElements(uint8_t* p, int64_t bytes, ByteSwap how) {
  switch (how) {
    case ByteSwap::NONE: return;
    case ByteSwap::W2: { uint16_t* v = reinterpret_cast<uint16_t*>(p); for (int64_t i = 0; i < bytes / 2; i++) v[i] = __builtin_bswap16(v[i]); return; }
    case ByteSwap::W4: { uint32_t* v = reinterpret_cast<uint32_t*>(p); for (int64_t i = 0; i < bytes / 4; i++) v[i] = __builtin_bswap32(v[i]); return; }
    case ByteSwap::W8: { uint64_t* v = reinterpret_cast<uint64_t*>(p); for (int64_t i = 0; i < bytes / 8; i++) v[i] = __builtin_bswap64(v[i]); return; }
    case ByteSwap::W16: case ByteSwap::W32: {  // one wide integer: the whole value is reversed
      const int w = static_cast<int>(how);
      for (int64_t i = 0; i + w <= bytes; i += w) std::reverse(p + i, p + i + w);
      return;
    }
    case ByteSwap::MONTH_DAY_NANO:  // {int32 months, int32 days, int64 nanoseconds}
      for (int64_t i = 0; i + 16 <= bytes; i += 16) {
        uint32_t a, b;
        uint64_t c;
        std::memcpy(&a, p + i, 4);
        std::memcpy(&b, p + i + 4, 4);
        std::memcpy(&c, p + i + 8, 8);
        a = __builtin_bswap32(a);
        b = __builtin_bswap32(b);
        c = __builtin_bswap64(c);
        std::memcpy(p + i, &a, 4);
        std::memcpy(p + i + 4, &b, 4);
        std::memcpy(p + i + 8, &c, 8);
      }
      return;
    case ByteSwap::VIEW:  // {int32 length, 12 inline bytes} or {int32 length, 4 prefix bytes, int32 buffer, int32 offset}
      for (int64_t i = 0; i + 16 <= bytes; i += 16) {
        uint32_t len;
        std::memcpy(&len, p + i, 4);
        len = __builtin_bswap32(len);
        std::memcpy(p + i, &len, 4);
        if (static_cast<int32_t>(len) > 12) {
          uint32_t bi, bo;
          std::memcpy(&bi, p + i + 8, 4);
          std::memcpy(&bo, p + i + 12, 4);
          bi = __builtin_bswap32(bi);
          bo = __builtin_bswap32(bo);
          std::memcpy(p + i + 8, &bi, 4);
          std::memcpy(p + i + 12, &bo, 4);
        }
      }
      return;
  }
}
}  // namespace

// Only multi-byte numbers are affected (FieldLayout's swap rules): bitmaps, boolean data, string / binary payloads and
// fixed_size_binary values are byte sequences.
void SwapBody(const ArrowSchemaModel& schema, const RecordBatchMeta& meta, const std::vector<char>& needed, uint8_t* body, int64_t body_size) {
  std::vector<ByteSwap> how(meta.buffers.size(), ByteSwap::NONE);
  const WalkEnd walked = WalkBatch(schema.fields, meta, [&](const WalkNode& v) {
    for (int32_t k = 0; k < v.layout.n && v.first_buffer + k < how.size(); k++) how[v.first_buffer + k] = v.layout.buffers[k].swap;
  });
  if (walked.buffers != how.size()) return;  // metadata the walk cannot follow: the full validation reports it
  ParallelFor(static_cast<int>(how.size()), [&](int i) {
    const mi_buffer_span& b = meta.buffers[static_cast<size_t>(i)];
    if (how[static_cast<size_t>(i)] == ByteSwap::NONE || b.length <= 0) return;
    if (!needed.empty() && !needed[static_cast<size_t>(i)]) return;    // never read from the file: nothing there to swap
    if (!SpanInside(b.offset, b.length, body_size)) return;             // reported by SliceBatch
    SwapElements(body + b.offset, b.length, how[static_cast<size_t>(i)]);
  });
}

static std::string BufferSizeError(const std::string& column, int buffer, int64_t need, int64_t have) {
  return "Expected " + column + " buffer " + std::to_string(buffer) + " to have size >= " + std::to_string(need) +
         " bytes but found buffer with " + std::to_string(have) + " bytes";
}

void SliceBatch(const ArrowSchemaModel& schema, const std::vector<int32_t>& projected_columns, const RecordBatchMeta& meta, const uint8_t* body,
                int64_t body_size, int64_t body_file_offset, const std::shared_ptr<void>& owner, DecodedBatch* out) {
  const bool projected = !projected_columns.empty() && !meta.is_dictionary;
  out->length = meta.length;
  out->body = body;
  out->body_size = body_size;
  out->body_file_offset = body_file_offset;
  out->is_dictionary = meta.is_dictionary;
  out->dict_id = meta.dict_id;
  out->is_delta = meta.is_delta;
  out->compression = meta.compression;
  out->owner = owner;
  out->column_field.clear();
  out->null_count.clear();
  out->column_length.clear();
  out->buffers.clear();
  if (meta.compression != -1 && body_size > 0) throw InternalException("compressed body reached SliceBatch");

  auto check_span = [&](const mi_buffer_span& s) {
    if (!SpanInside(s.offset, s.length, body_size)) {
      throw InternalException("Buffer requires body offsets [" + std::to_string(s.offset) + ", " + std::to_string(s.offset) + " + " +
                              std::to_string(s.length) + ") but body has size " + std::to_string(body_size));
    }
    if (s.offset % 8 != 0) throw InternalException("Buffer offset " + std::to_string(s.offset) + " is not 8-byte aligned");
  };

  auto add_column = [&](int32_t top_index, int32_t node_idx) {
    const DecodedNode& nd = out->nodes[static_cast<size_t>(node_idx)];
    out->column_field.push_back(top_index);
    out->column_node.push_back(node_idx);
    out->null_count.push_back(nd.null_count);
    out->column_length.push_back(nd.length);
    for (size_t k = 0; k < 3; k++) out->buffers.push_back(k < nd.spans.size() ? nd.spans[k] : mi_buffer_span{0, 0});
  };
  out->nodes.clear();
  out->column_node.clear();

  // Nodes are materialised only for the projected columns and their descendants (all of a dictionary batch), in walk
  // order: a kept node's index is its column root's plus its distance from that root in RecordBatch.nodes.
  std::vector<int32_t> node_of_field(schema.fields.size(), -1);
  std::vector<char> wanted(schema.fields.size(), projected ? 0 : 1);
  if (!meta.is_dictionary)
    for (int32_t c : projected_columns) wanted[static_cast<size_t>(c)] = 1;
  int32_t root = 0;
  size_t root_node = 0;
  const WalkEnd walked = WalkBatch(schema.fields, meta, [&](const WalkNode& v) {
    const ArrowField& f = *v.field;
    if (v.node >= meta.nodes.size()) throw InternalException("RecordBatch has too few field nodes");
    const int64_t n = meta.nodes[v.node].first;
    const int64_t nulls = meta.nodes[v.node].second;
    if (n < 0) throw InternalException("Field node length is negative");
    // lengths come from the file: bound them before anything is multiplied by them (ArrowArrayViewValidate checks the
    // same relations), so a damaged RecordBatch cannot overflow a size computation and slip past the buffer checks
    if (n > (int64_t(1) << 40)) throw InternalException("Field node length " + std::to_string(n) + " is implausible");
    if (nulls < -1 || nulls > n) throw InternalException("Field node null_count " + std::to_string(nulls) + " is outside [0, length]");
    if (v.depth == 0 && !v.value_only && n != meta.length)
      throw InternalException("Expected array length " + std::to_string(meta.length) + " for column " + f.name + " but found " + std::to_string(n));
    const bool keep = wanted[static_cast<size_t>(v.column)] != 0;
    if (keep && v.depth == 0) {
      root = static_cast<int32_t>(out->nodes.size());
      root_node = v.node;
    }
    const int32_t parent = v.parent < 0 ? -1 : root + static_cast<int32_t>(static_cast<size_t>(v.parent) - root_node);
    if (keep && f.type == MI_AT_RUN_END && !(f.has_dictionary && !v.value_only)) {
      // structural checks that need only the metadata (the run ends themselves are checked on the device / by the exporter)
      if (nulls != 0) throw InternalException("Run-end encoded column " + f.name + " has null_count " + std::to_string(nulls) + ", expected 0");
      if (f.children.size() != 2)
        throw InternalException("Run-end encoded column " + f.name + " has " + std::to_string(f.children.size()) + " children, expected 2 (run_ends, values)");
      if (v.node + 2 >= meta.nodes.size()) throw InternalException("RecordBatch has too few field nodes");
      // the children's nodes follow right away: run_ends is always a leaf (an integer), values comes after it
      const int64_t re_len = meta.nodes[v.node + 1].first, re_nulls = meta.nodes[v.node + 1].second;
      const int64_t v_len = meta.nodes[v.node + 2].first;
      if (re_nulls != 0) throw InternalException("Run ends of column " + f.name + " have null_count " + std::to_string(re_nulls) + ", expected 0");
      if (re_len != v_len)
        throw InternalException("Run-end encoded column " + f.name + " has " + std::to_string(re_len) + " run ends but " + std::to_string(v_len) + " values");
      if ((re_len == 0) != (n == 0))
        throw InternalException("Run-end encoded column " + f.name + " of length " + std::to_string(n) + " has " + std::to_string(re_len) + " runs");
    }
    if (keep && parent >= 0) {
      const DecodedNode& pn = out->nodes[static_cast<size_t>(parent)];
      const int32_t pt = pn.field->type;
      if (pt == MI_AT_STRUCT && n != pn.length)
        throw InternalException("Struct child " + f.name + " has length " + std::to_string(n) + ", its parent " + std::to_string(pn.length));
      if (pt == MI_AT_UNION && pn.field->unit == 0 && !pn.field->has_dictionary && n != pn.length)
        throw InternalException("Sparse union member " + f.name + " has length " + std::to_string(n) + ", its parent " + std::to_string(pn.length));
      if (pt == MI_AT_FIXED_LIST) {
        int64_t expect = 0;  // length <= 2^40 and listSize < 2^31: checked anyway, the product sizes buffers
        if (__builtin_mul_overflow(pn.length, static_cast<int64_t>(pn.field->byte_width), &expect) || n != expect)
          throw InternalException("Fixed-size list child " + f.name + " has length " + std::to_string(n) + ", expected " +
                                  std::to_string(pn.length) + " x " + std::to_string(pn.field->byte_width));
      }
    }
    if (v.defect) throw InternalException(v.defect);
    if (v.first_buffer + v.n_buffers > meta.buffers.size()) throw InternalException("RecordBatch has too few buffers");
    if (!keep) return;
    DecodedNode nd;
    nd.field = &f;
    nd.parent = parent;
    nd.depth = v.depth;
    nd.length = n;
    nd.null_count = nulls;
    nd.value_only = v.value_only;
    for (size_t k = 0; k < v.n_buffers; k++) {
      nd.spans.push_back(meta.buffers[v.first_buffer + k]);
      check_span(nd.spans.back());
    }
    // size checks of ArrowArrayViewValidate (FULL), minus the data-dependent offsets walk (done on the device)
    int32_t kind, w;
    int64_t param;
    if (f.Plan(&kind, &param, &w, v.value_only)) {
      const size_t own = v.n_buffers;
      const mi_buffer_span none{0, 0};
      const mi_buffer_span& s0 = own > 0 ? nd.spans[0] : none;
      const mi_buffer_span& s1 = own > 1 ? nd.spans[1] : none;
      if (kind == MI_K_UNION && s0.length < n) throw InternalException(BufferSizeError(f.name, 0, n, s0.length));  // type ids, no validity
      if (s0.length != 0 && s0.length < (n + 7) / 8) throw InternalException(BufferSizeError(f.name, 0, (n + 7) / 8, s0.length));
      if (kind != MI_K_NULL && s0.length == 0 && n > 0 && nulls > 0)
        throw InternalException("Column " + f.name + " has null_count " + std::to_string(nulls) + " but no validity buffer");
      int64_t need1 = 0, per_row = 0, rows = n;
      if (v.layout.n > 1) {
        const BufferLayout& b1 = v.layout.buffers[1];
        if (b1.role == BufferRole::BITS) need1 = (n + 7) / 8;
        else per_row = b1.width;
        if (b1.role == BufferRole::OFFSETS) rows = n > 0 ? n + 1 : 0;
      }
      // rows <= 2^40 + 1 and widths come from the schema (validated, but up to 2^31 for fixed_size_binary): the
      // product is formed with an overflow check so that a wrapped size can never pass for a small one
      if (per_row < 0 || (per_row > 0 && __builtin_mul_overflow(rows, per_row, &need1)))
        throw InternalException("Column " + f.name + " needs more bytes than a buffer can hold (" + std::to_string(rows) + " x " + std::to_string(per_row) + ")");
      if (s1.length < need1) throw InternalException(BufferSizeError(f.name, 1, need1, s1.length));
    }
    const int32_t idx = static_cast<int32_t>(out->nodes.size());
    if (parent >= 0) out->nodes[static_cast<size_t>(parent)].children.push_back(idx);
    else node_of_field[static_cast<size_t>(v.column)] = idx;
    out->nodes.push_back(std::move(nd));
  });
  if (walked.unknown_dictionary) throw IOException("DictionaryBatch refers to unknown dictionary id " + std::to_string(meta.dict_id));
  if (!meta.is_dictionary && walked.nodes != meta.nodes.size()) {
    throw InternalException("Expected " + std::to_string(walked.nodes) + " field nodes in message but found " +
                            std::to_string(meta.nodes.size()));
  }
  if (projected) {
    for (int32_t c : projected_columns) add_column(c, node_of_field[static_cast<size_t>(c)]);
  } else {
    for (size_t i = 0; i < schema.fields.size(); i++)
      if (node_of_field[i] >= 0) add_column(static_cast<int32_t>(i), node_of_field[i]);
  }
}

}  // namespace miarrow
