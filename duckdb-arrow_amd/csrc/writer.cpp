// writer.cpp -- see writer.hpp.
#include "writer.hpp"
#include "writer_internal.hpp"
#include "extension_format.hpp"
#include "union_format.hpp"
#include "writer_plan.hpp"

#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cctype>
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <functional>

namespace miarrow {

int WrapC(const std::function<void()>& f);  // c_api.cpp

SinkTimers& Timers() {
  static SinkTimers t;
  return t;
}

namespace {
struct ScopedTimer {
  double* acc;
  std::chrono::steady_clock::time_point t0;
  explicit ScopedTimer(double* a) : acc(Timers().on ? a : nullptr) { if (acc) t0 = std::chrono::steady_clock::now(); }
  ~ScopedTimer() {
    if (!acc) return;
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::lock_guard<std::mutex> lk(Timers().mu);
    *acc += dt;
  }
};

// DuckDB logical type -> how the vector is laid out and which K7 kernel encodes it
void EncodePlanFor(const ArrowField& f, int32_t* enc_kind, int64_t* param, int32_t* width) {
  switch (f.type) {
    case MI_AT_BOOL: *enc_kind = MI_K_ENC_BOOL; *param = 1; *width = 1; return;
    case MI_AT_INT: *enc_kind = MI_K_ENC_COPY; *param = f.bit_width / 8; *width = f.bit_width / 8; return;
    case MI_AT_FLOAT: *enc_kind = MI_K_ENC_COPY; *param = f.precision == 1 ? 4 : 8; *width = static_cast<int32_t>(*param); return;
    case MI_AT_DATE: *enc_kind = MI_K_ENC_COPY; *param = 4; *width = 4; return;
    case MI_AT_TIME: case MI_AT_TIMESTAMP: *enc_kind = MI_K_ENC_COPY; *param = 8; *width = 8; return;
    case MI_AT_DECIMAL:
      if (f.precision <= 4) { *enc_kind = MI_K_ENC_DEC128; *param = 2; *width = 2; }
      else if (f.precision <= 9) { *enc_kind = MI_K_ENC_DEC128; *param = 4; *width = 4; }
      else if (f.precision <= 18) { *enc_kind = MI_K_ENC_DEC128; *param = 8; *width = 8; }
      else { *enc_kind = MI_K_ENC_COPY; *param = 16; *width = 16; }
      return;
    case MI_AT_UTF8: case MI_AT_BINARY: case MI_AT_LARGE_UTF8: case MI_AT_LARGE_BINARY:
      if (f.extension == extfmt::kUuid) { *enc_kind = MI_K_ENC_UUID_TEXT; *param = 16; *width = 16; return; }   // hugeint_t rows -> their text
      *enc_kind = MI_K_ENC_STR32; *param = 0; *width = 16; return;
    case MI_AT_UTF8_VIEW: *enc_kind = MI_K_ENC_STRVIEW; *param = 0; *width = 16; return;   // produce_arrow_string_view
    case MI_AT_INTERVAL:   // interval_t rows -> month_day_nano, the one interval DuckDB exports
      if (f.unit != 2) break;
      *enc_kind = MI_K_ENC_INTERVAL; *param = 16; *width = 16; return;
    default: break;
  }
  throw NotImplementedException("Arrow type " + f.Format() + " is not encoded by the MI355X writer path");
}

// append `n` bits of `src` starting at bit `spos` (src NULL = all ones) to `dst` at bit position `pos`
void AppendBits(uint64_t* dst, int64_t pos, const uint64_t* src, int64_t spos, int64_t n) {
  for (int64_t i = 0; i < n;) {
    const int64_t dw = (pos + i) >> 6;
    const int dsh = static_cast<int>((pos + i) & 63);
    const int64_t take = std::min<int64_t>(64 - dsh, n - i);
    uint64_t bits;
    if (!src) {
      bits = ~0ull;
    } else {
      const int64_t sw = (spos + i) >> 6;
      const int ssh = static_cast<int>((spos + i) & 63);
      bits = src[sw] >> ssh;
      if (ssh && ssh + take > 64) bits |= src[sw + 1] << (64 - ssh);
    }
    const uint64_t mask = take == 64 ? ~0ull : ((1ull << take) - 1ull);
    dst[dw] = (dst[dw] & ~(mask << dsh)) | ((bits & mask) << dsh);
    i += take;
  }
}
inline bool BitAt(const uint64_t* v, int64_t i) { return !v || ((v[i >> 6] >> (i & 63)) & 1); }
}  // namespace

// ------------------------------------------------------------------------------------------------ collection
ChunkCollection::ChunkCollection(Context* ctx_p, const std::vector<ArrowField>& fields) : ctx(ctx_p) {
  for (auto& f : fields) roots.push_back(AddField(f, 0));
}

int32_t ChunkCollection::AddField(const ArrowField& f, int32_t depth) {
  const int32_t idx = static_cast<int32_t>(columns.size());
  columns.emplace_back();
  {
    Column& c = columns.back();
    c.arrow_type = f.type;
    c.depth = depth;
    switch (f.type) {
      case MI_AT_STRUCT: case MI_AT_NULL: break;   // (a null node stages its count alone)
      case MI_AT_FIXED_LIST: c.param = f.byte_width; break;
      case MI_AT_UNION:   // the tag bytes; the members are nodes of their own, appended row for row like a struct's children
        if (f.unit != 0 || f.children.empty() || f.children.size() > static_cast<size_t>(unionfmt::kMaxMembers))
          throw NotImplementedException("Column '" + f.name + "': only sparse unions of 1 .. 32 members are encoded by the MI355X writer path");
        c.enc_kind = MI_K_ENC_UNION;
        c.param = static_cast<int64_t>(f.children.size());
        c.width = 1;
        break;
      case MI_AT_LIST: case MI_AT_LARGE_LIST: case MI_AT_MAP: c.enc_kind = MI_K_ENC_LIST32; c.param = 0; c.width = 16; break;
      default: EncodePlanFor(f, &c.enc_kind, &c.param, &c.width); break;
    }
    c.large_offsets = f.type == MI_AT_LARGE_UTF8 || f.type == MI_AT_LARGE_BINARY || f.type == MI_AT_LARGE_LIST;
  }
  for (auto& ch : f.children) {
    const int32_t k = AddField(ch, depth + 1);
    columns[static_cast<size_t>(idx)].children.push_back(k);
  }
  return idx;
}

void ChunkCollection::Reserve(Column& c, int64_t rows, int64_t extra_heap) {
  ctx->Bind();
  if (c.width > 0)
    Fit(c.data, static_cast<size_t>(rows) * static_cast<size_t>(c.width) + 64, static_cast<size_t>(c.count) * static_cast<size_t>(c.width));
  const size_t old_vcap = c.validity.size();
  const size_t used = static_cast<size_t>((c.count + 63) / 64) * 8;
  Fit(c.validity, static_cast<size_t>((rows + 63) / 64) * 8 + 16, used);
  if (c.validity.size() != old_vcap) std::memset(c.validity.get() + used, 0xFF, c.validity.size() - used);
  if (extra_heap > 0) Fit(c.heap, static_cast<size_t>(c.heap_used + extra_heap) + 64, static_cast<size_t>(c.heap_used));
}

void ChunkCollection::Append(const mi_data_chunk& chunk) {
  ScopedTimer timer(&Timers().append);
  if (chunk.n_columns != static_cast<int32_t>(roots.size()))
    throw InvalidInputException("DataChunk has " + std::to_string(chunk.n_columns) + " columns, the writer expects " + std::to_string(roots.size()));
  const int64_t n = chunk.size;
  if (n <= 0) return;
  if (n > MI_VECTOR_SIZE * 1024) throw InvalidInputException("DataChunk too large");
  for (size_t ci = 0; ci < roots.size(); ci++) AppendNode(roots[ci], chunk.columns[ci], 0, n);
  count += n;
}

// rows [start, start + n) of vector `v` -> node `ni` (and, for nested types, the rows they own in the child nodes)
void ChunkCollection::AppendNode(int32_t ni, const mi_vector& v, int64_t start, int64_t n) {
  if (n <= 0) return;
  const int64_t vbit = static_cast<int64_t>(v.validity_shift) + start;  // bit of v.validity that belongs to row `start`
  {
    Column& c = columns[static_cast<size_t>(ni)];
    if (c.IsNull()) {   // nothing to stage: every row is NULL
      c.count += n;
      return;
    }
    if (c.IsUnion()) {
      AppendUnion(ni, v, start, n);
      return;
    }
    if (!c.IsGroup() && !v.data) throw InvalidInputException("DataChunk column " + std::to_string(ni) + " has no data");
    if ((c.IsList() || c.IsGroup()) && (v.n_children < (c.arrow_type == MI_AT_STRUCT ? static_cast<int32_t>(c.children.size()) : 1) || !v.children))
      throw InvalidInputException("nested vector without child vectors");
  }
  // strings: one pass over the rows decides how the long-string payloads of this slice are staged
  int64_t extra_heap = 0, payload = 0;
  bool one_copy = false;
  uint64_t region_lo = 0, region_hi = 0;
  const bool as_views = columns[static_cast<size_t>(ni)].enc_kind == MI_K_ENC_STRVIEW;
  if (columns[static_cast<size_t>(ni)].enc_kind == MI_K_ENC_STR32 || as_views) {
    const mi_string_t* s = static_cast<const mi_string_t*>(v.data) + start;
    const uint64_t heap_lo = reinterpret_cast<uint64_t>(v.heap), heap_hi = heap_lo + static_cast<uint64_t>(v.heap_size > 0 ? v.heap_size : 0);
    bool ascending_inside = v.heap != nullptr;
    int64_t long_bytes = 0;
    uint64_t prev_end = 0;
    for (int64_t i = 0; i < n; i++) {
      if (!BitAt(v.validity, vbit + i)) continue;
      const uint32_t len = s[i].value.inlined.length;
      payload += len;
      if (len <= 12) continue;
      const uint64_t p = s[i].value.pointer.ptr;
      long_bytes += len;
      if (region_lo == 0) region_lo = p;
      if (p < prev_end || p < heap_lo || p > heap_hi || len > heap_hi - p) ascending_inside = false;
      prev_end = p + len;
    }
    region_hi = prev_end;
    if (long_bytes > 0) {
      // one copy of [first long string, end of the last) when that range is known to be one allocation and is not much
      // larger than what it is needed for (short and NULL rows in between own at most 12 bytes each there)
      one_copy = ascending_inside && region_hi - region_lo <= static_cast<uint64_t>(long_bytes) + 16ull * static_cast<uint64_t>(n);
      extra_heap = one_copy ? static_cast<int64_t>(region_hi - region_lo) : long_bytes;
    }
    if (as_views) payload = long_bytes;   // the data buffer of a view column holds the long strings alone
  }
  Reserve(columns[static_cast<size_t>(ni)], columns[static_cast<size_t>(ni)].count + n, extra_heap);
  Column& c = columns[static_cast<size_t>(ni)];  // (children are appended after this block: `columns` never grows here)
  AppendBits(c.validity.get<uint64_t>(), c.count, v.validity, vbit, n);
  if (v.validity && !c.has_nulls) {
    for (int64_t i = 0; i < n; i++)
      if (!BitAt(v.validity, vbit + i)) { c.has_nulls = true; break; }
  }
  if (c.IsGroup()) {
    const int64_t mult = c.arrow_type == MI_AT_FIXED_LIST ? c.param : 1;
    c.count += n;
    for (size_t k = 0; k < c.children.size(); k++) AppendNode(c.children[k], v.children[k], start * mult, n * mult);
    return;
  }
  if (c.IsList()) {
    // the list_entry_t rows are staged as they are (the GPU turns the lengths of the valid rows into Arrow offsets);
    // the child rows of every valid list are gathered here, in list order (ArrowListData::Append)
    const uint64_t* ent = static_cast<const uint64_t*>(v.data) + 2 * start;
    std::memcpy(c.data.get() + static_cast<size_t>(c.count) * 16, ent, static_cast<size_t>(n) * 16);
    int64_t run_start = 0, run_len = 0;
    const int32_t child = c.children[0];
    c.count += n;
    size_in_bytes += n * 16;
    for (int64_t i = 0; i < n; i++) {
      if (!BitAt(v.validity, vbit + i)) continue;
      const int64_t o = static_cast<int64_t>(ent[2 * i]), l = static_cast<int64_t>(ent[2 * i + 1]);
      if (l <= 0) continue;
      if (run_len > 0 && o == run_start + run_len) {
        run_len += l;
      } else {
        if (run_len > 0) AppendNode(child, v.children[0], run_start, run_len);
        run_start = o;
        run_len = l;
      }
      columns[static_cast<size_t>(ni)].payload_bytes += l;   // child rows so far = the last Arrow offset
      if (columns[static_cast<size_t>(ni)].payload_bytes > 0x7FFFFFFFll && !columns[static_cast<size_t>(ni)].large_offsets)
        throw InvalidInputException("Arrow Appender: The maximum combined list offset for regular list buffers is 2147483647 but the offset of " +
                                    std::to_string(columns[static_cast<size_t>(ni)].payload_bytes) +
                                    " exceeds this.\n* SET arrow_large_buffer_size=true to use large list buffers");
    }
    if (run_len > 0) AppendNode(child, v.children[0], run_start, run_len);
    return;
  }
  std::memcpy(c.data.get() + static_cast<size_t>(c.count) * static_cast<size_t>(c.width),
              static_cast<const uint8_t*>(v.data) + static_cast<size_t>(start) * static_cast<size_t>(c.width),
              static_cast<size_t>(n) * static_cast<size_t>(c.width));
  if (c.enc_kind == MI_K_ENC_UUID_TEXT) {   // 36 bytes of text per valid row, none per NULL row
    int64_t valid = n;
    if (v.validity)
      for (int64_t i = 0; i < n; i++) valid -= BitAt(v.validity, vbit + i) ? 0 : 1;
    c.payload_bytes += valid * extfmt::kUuidTextBytes;
  }
  if (c.enc_kind == MI_K_ENC_STR32 || c.enc_kind == MI_K_ENC_STRVIEW) {
    c.payload_bytes += payload;
    if (extra_heap > 0) {
      mi_string_t* dst = reinterpret_cast<mi_string_t*>(c.data.get()) + c.count;
      if (one_copy) std::memcpy(c.heap.get() + c.heap_used, reinterpret_cast<const void*>(static_cast<uintptr_t>(region_lo)), static_cast<size_t>(extra_heap));
      int64_t at = c.heap_used;
      for (int64_t i = 0; i < n; i++) {   // the staged rows point at heap offsets
        if (!BitAt(v.validity, vbit + i)) continue;
        const uint32_t len = dst[i].value.inlined.length;
        if (len <= 12) continue;
        const uint64_t p = dst[i].value.pointer.ptr;
        if (one_copy) {
          dst[i].value.pointer.ptr = static_cast<uint64_t>(c.heap_used) + (p - region_lo);
        } else {
          std::memcpy(c.heap.get() + at, reinterpret_cast<const void*>(static_cast<uintptr_t>(p)), len);
          dst[i].value.pointer.ptr = static_cast<uint64_t>(at);
          at += len;
        }
      }
      c.heap_used += extra_heap;
    }
    size_in_bytes += extra_heap;
  }
  size_in_bytes += n * c.width;
  c.count += n;
}

// A union node: its tag bytes and validity words as they are, and under them the member vectors row for row, each with the
// EFFECTIVE validity the union's pass will give it on the GPU (union_format.hpp: EncodeRow) -- the row is valid, its tag names
// the member, the member's own bit is set -- so that what is staged for a member (the bytes of its valid strings, the child
// rows of its valid lists) is what its encode task will write.
void ChunkCollection::AppendUnion(int32_t ni, const mi_vector& v, int64_t start, int64_t n) {
  const int32_t m = static_cast<int32_t>(columns[static_cast<size_t>(ni)].children.size());
  if (v.n_children != m + 1 || !v.children)
    throw InvalidInputException("union vector with " + std::to_string(v.n_children) + " child vectors, the writer expects the tags and " +
                                std::to_string(m) + " members");
  const uint8_t* tags = static_cast<const uint8_t*>(v.data ? v.data : v.children[0].data);
  if (!tags) throw InvalidInputException("union vector without tags");
  const int64_t vbit = static_cast<int64_t>(v.validity_shift) + start;
  Reserve(columns[static_cast<size_t>(ni)], columns[static_cast<size_t>(ni)].count + n, 0);
  {
    Column& c = columns[static_cast<size_t>(ni)];
    AppendBits(c.validity.get<uint64_t>(), c.count, v.validity, vbit, n);
    if (v.validity && !c.has_nulls) {
      for (int64_t i = 0; i < n; i++)
        if (!BitAt(v.validity, vbit + i)) { c.has_nulls = true; break; }
    }
    std::memcpy(c.data.get() + c.count, tags + start, static_cast<size_t>(n));
    c.count += n;
    size_in_bytes += n;
  }
  // bit start + i of a member's mask = row i of the slice
  std::vector<uint64_t> mask(static_cast<size_t>((start + n + 63) / 64));
  for (int32_t k = 0; k < m; k++) {
    const mi_vector& mv = v.children[1 + k];
    const int64_t mbit = static_cast<int64_t>(mv.validity_shift) + start;
    std::fill(mask.begin(), mask.end(), 0ull);
    for (int64_t i = 0; i < n; i++) {
      const unionfmt::EncodedRow row = unionfmt::EncodeRow(tags[start + i], m, BitAt(v.validity, vbit + i));
      if (row.selects && row.member == k && BitAt(mv.validity, mbit + i)) mask[static_cast<size_t>((start + i) >> 6)] |= 1ull << ((start + i) & 63);
    }
    mi_vector masked = mv;
    masked.validity = mask.data();
    masked.validity_shift = 0;
    AppendNode(columns[static_cast<size_t>(ni)].children[static_cast<size_t>(k)], masked, start, n);
  }
}

void ChunkCollection::Reset() {
  for (auto& c : columns) {
    c.count = 0;
    c.heap_used = 0;
    c.payload_bytes = 0;
    c.has_nulls = false;
    if (c.validity) std::memset(c.validity.get(), 0xFF, c.validity.size());
  }
  count = 0;
  size_in_bytes = 0;
}

// ------------------------------------------------------------------------------------------------ serializer
ColumnDataCollectionSerializer::ColumnDataCollectionSerializer(Context* ctx_p, bool own_stream) : ctx(ctx_p) {
  stream = ctx->stream;
  if (own_stream) {
    ctx->Bind();
    stream = owned_stream = HipStream::Create();
  }
}

void ColumnDataCollectionSerializer::Init(const ArrowSchemaModel* schema_p, int32_t compression_p) {
  schema = schema_p;
  compression = compression_p;
}

void ColumnDataCollectionSerializer::SerializeSchema() {
  header = EncodeSchemaMessage(*schema);
  body_size = 0;
}

idx_t ColumnDataCollectionSerializer::Serialize(ChunkCollection& buffer) {
  ScopedTimer timer(&Timers().serialize);
  header.clear();
  body_size = 0;
  const int64_t n_top = buffer.Count();
  if (n_top == 0) return 0;
  ctx->Bind();
  if (!plan) plan = std::make_unique<Plan>(ctx);
  if (n_top > 0x7FFFFFFFll) throw InvalidInputException("record batch too large");

  // the body layout, and the device staging layout beside it
  const size_t n_nodes = buffer.columns.size();
  std::vector<EncodeNode> nodes(n_nodes);
  struct InOff { size_t data, validity, heap, members, masks, mask_stride; };   // members, masks: union nodes
  std::vector<InOff> in_off(n_nodes);
  size_t in_bytes = 0, n_unions = 0;
  for (size_t ci = 0; ci < n_nodes; ci++) {
    auto& c = buffer.columns[ci];
    nodes[ci] = EncodeNode{c.IsGroup() ? MI_K_ENC_VALIDITY : c.IsNull() ? kEncNodeNull : c.enc_kind, c.param, c.large_offsets, c.count, c.payload_bytes};
    in_off[ci].data = in_bytes;
    in_bytes += RoundUp(static_cast<size_t>(c.count) * static_cast<size_t>(c.width) + 16, 256);
    in_off[ci].validity = in_bytes;
    in_bytes += RoundUp(static_cast<size_t>((c.count + 63) / 64) * 8 + 8, 256);
    in_off[ci].heap = in_bytes;
    in_bytes += RoundUp(static_cast<size_t>(c.heap_used) + 16, 256);
    if (c.IsUnion()) {   // the addresses of its members' validity words, and the scratch its pass leaves their masks in
      in_off[ci].members = in_bytes;
      in_bytes += RoundUp(static_cast<size_t>(unionfmt::kMaxMembers) * 8, 256);
      in_off[ci].mask_stride = RoundUp(static_cast<size_t>((c.count + 63) / 64) * 8 + 8, 256);
      in_off[ci].masks = in_bytes;
      in_bytes += in_off[ci].mask_stride * c.children.size();
      n_unions++;
    }
  }
  BodyLayout layout;
  LayOutBody(nodes, &layout);
  const size_t body_bytes = static_cast<size_t>(layout.body_size);
  Fit(d_in, in_bytes + 256);
  Fit(d_body, body_bytes + 256);
  PinnedBuffer& h_body = bodies[cur_body];

  hipStream_t s = stream;
  MI_HIP_CHECK(hipMemsetAsync(d_body.get(), 0, body_bytes, s));  // the padding bytes of every buffer are zero
  std::vector<mi_col_task> tasks;
  std::vector<int32_t> validity_task(n_nodes, -1);  // task whose NULL counter belongs to node ci
  // a union member's task reads the mask the union's pass makes for it in place of its staged validity words (the same bits)
  std::vector<const uint8_t*> member_mask(n_nodes, nullptr);
  if (n_unions) Fit(h_union, n_unions * static_cast<size_t>(unionfmt::kMaxMembers) * 8);
  size_t unions_done = 0;
  for (size_t ci = 0; ci < n_nodes; ci++) {
    auto& c = buffer.columns[ci];
    const int64_t n = c.count;
    if (n == 0) continue;  // zero-length buffers, no work
    if (c.IsNull()) continue;  // no buffers either
    const uint8_t* d_data = d_in.get() + in_off[ci].data;
    const uint8_t* d_validity = d_in.get() + in_off[ci].validity;
    const uint8_t* d_heap = d_in.get() + in_off[ci].heap;
    if (c.width > 0)
      MI_HIP_CHECK(hipMemcpyAsync(d_in.get() + in_off[ci].data, c.data.get(), static_cast<size_t>(n) * static_cast<size_t>(c.width), hipMemcpyHostToDevice, s));
    if (c.has_nulls)
      MI_HIP_CHECK(hipMemcpyAsync(d_in.get() + in_off[ci].validity, c.validity.get(), static_cast<size_t>((n + 63) / 64) * 8, hipMemcpyHostToDevice, s));
    if (c.heap_used)
      MI_HIP_CHECK(hipMemcpyAsync(d_in.get() + in_off[ci].heap, c.heap.get(), static_cast<size_t>(c.heap_used), hipMemcpyHostToDevice, s));
    // a struct / fixed-size list reads its own validity words; the staged string_t rows point at heap offsets (ptr_base 0)
    EncodeInput in{c.IsGroup() ? d_validity : d_data, c.has_nulls ? d_validity : nullptr, d_heap, 0};
    if (member_mask[ci]) {
      in.validity = member_mask[ci];
      if (c.IsGroup()) in.data = member_mask[ci];
    }
    if (c.IsUnion()) {
      uint64_t* table = h_union.get<uint64_t>() + unions_done++ * static_cast<size_t>(unionfmt::kMaxMembers);
      for (size_t k = 0; k < c.children.size(); k++) {
        const size_t child = static_cast<size_t>(c.children[k]);
        table[k] = buffer.columns[child].has_nulls ? reinterpret_cast<uint64_t>(d_in.get() + in_off[child].validity) : 0;
        member_mask[child] = d_in.get() + in_off[ci].masks + k * in_off[ci].mask_stride;
      }
      MI_HIP_CHECK(hipMemcpyAsync(d_in.get() + in_off[ci].members, table, c.children.size() * 8, hipMemcpyHostToDevice, s));
      in.member_validity = d_in.get() + in_off[ci].members;
      in.masks = d_in.get() + in_off[ci].masks;
      in.mask_stride = static_cast<int64_t>(in_off[ci].mask_stride);
    }
    validity_task[ci] = static_cast<int32_t>(tasks.size());
    tasks.push_back(EncodeTask(nodes[ci], &layout.spans[static_cast<size_t>(layout.first_span[ci])], in, d_body.get()));
  }
  plan->Set(tasks.data(), static_cast<int32_t>(tasks.size()), s);
  plan->Launch(s);
  // what goes to the file: the encoded body, or (COMPRESSION lz4) the body the compressor makes of it in HBM
  const uint8_t* d_final = d_body.get();
  const std::vector<mi_buffer_span>* spans = &layout.spans;
  body_size = layout.body_size;
  if (compression == MI_WRITE_COMPRESSION_LZ4_FRAME) {
    compressor.Run(layout, d_body.get(), s);
    d_final = compressor.Body();
    spans = &compressor.Layout().spans;
    body_size = compressor.Layout().body_size;
  }
  Fit(h_body, static_cast<size_t>(body_size) + 256);
  MI_HIP_CHECK(hipMemcpyAsync(h_body.get(), d_final, static_cast<size_t>(body_size), hipMemcpyDeviceToHost, s));
  ThrowForStatus(plan->Status());  // synchronises the stream
  std::vector<int64_t> null_counts = plan->NullCounts(/*reset*/ true);
  std::vector<std::pair<int64_t, int64_t>> node_counts;
  for (size_t ci = 0; ci < n_nodes; ci++) {   // (a union's counter stays 0: it has no bitmap; every row of a null node is NULL)
    const auto& c = buffer.columns[ci];
    node_counts.emplace_back(c.count, c.IsNull() ? c.count : validity_task[ci] >= 0 ? null_counts[static_cast<size_t>(validity_task[ci])] : 0);
  }
  int64_t n_view_fields = 0;   // RecordBatch.variadicBufferCounts: one data buffer per view field, rows or not
  for (auto& c : buffer.columns) n_view_fields += c.enc_kind == MI_K_ENC_STRVIEW;
  header = EncodeRecordBatchMessage(n_top, node_counts, *spans, body_size, compression == MI_WRITE_COMPRESSION_LZ4_FRAME ? 0 : -1, n_view_fields);
  return 1;
}

// ------------------------------------------------------------------------------------------------ stream writer
ArrowStreamWriter::ArrowStreamWriter(Context* ctx_p, const std::string& file_path, const std::vector<ArrowField>& fields,
                                     const std::vector<std::pair<std::string, std::string>>& metadata, int32_t compression)
    : ctx(ctx_p), serializer(ctx_p), file_name(file_path) {
  InitSchema(fields, metadata, compression);
  if (!file_path.empty()) InitOutputFile(file_path);
}

ArrowStreamWriter::~ArrowStreamWriter() {
  {
    std::lock_guard<std::mutex> lk(io_mu);
    io_stop = true;
  }
  io_cv.notify_all();
  if (io_thread.joinable()) io_thread.join();  // queued batches are still written
  if (fd >= 0) ::close(fd);
}

void ArrowStreamWriter::InitSchema(const std::vector<ArrowField>& fields,
                                   const std::vector<std::pair<std::string, std::string>>& metadata, int32_t compression) {
  schema.fields = fields;
  schema.metadata = metadata;  // kv_metadata COPY option (arrow_stream_writer.cpp:26-44)
  serializer.Init(&schema, compression);
}

void ArrowStreamWriter::InitOutputFile(const std::string& file_path) {
  // FILE_FLAGS_WRITE | FILE_FLAGS_FILE_CREATE_NEW (arrow_stream_writer.cpp:49-53): always a fresh file
  fd = ::open(file_path.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0644);
  if (fd < 0) throw IOException("Cannot open file \"" + file_path + "\": " + std::strerror(errno));
  // Record batches are pwritten at claimed offsets by whichever thread serialized them.  (On tmpfs the page cache IS the
  // file and every new page is allocated, charged and zeroed under the write: measured on the MI355X box ~5-6 GB/s into one
  // file whether 1, 2, 4 or 6 threads pwrite and whether they write() or store through a shared mapping -- the end-to-end
  // COPY of SF10 is bound by that, not by staging or the K7 kernels: tools/copy_bench.py)
}

void ArrowStreamWriter::WriteAt(int64_t offset, const uint8_t* p, size_t n) {
  ScopedTimer timer(&Timers().write);
  size_t done = 0;
  while (done < n) {
    ssize_t w = ::pwrite(fd, p + done, n - done, static_cast<off_t>(offset + static_cast<int64_t>(done)));
    if (w < 0) {
      if (errno == EINTR) continue;
      throw IOException("Could not write to file \"" + file_name + "\": " + std::strerror(errno));
    }
    done += static_cast<size_t>(w);
  }
}

int64_t ArrowStreamWriter::ReserveRowGroup(size_t bytes) {
  std::lock_guard<std::mutex> lk(io_mu);
  const int64_t at = static_cast<int64_t>(total_written);
  total_written += bytes;
  ++row_group_count;
  return at;
}

void ArrowStreamWriter::WriteMessageAt(int64_t offset, const uint8_t* header, size_t header_size, const uint8_t* body, size_t body_size) {
  WriteAt(offset, header, header_size);
  WriteAt(offset + static_cast<int64_t>(header_size), body, body_size);
}

int64_t ArrowStreamWriter::WriteMessage(const uint8_t* header, size_t header_size, const uint8_t* body, size_t body_size) {
  const int64_t at = ReserveRowGroup(header_size + body_size);
  WriteMessageAt(at, header, header_size, body, body_size);
  return at;
}

void ArrowStreamWriter::WriteData(const uint8_t* p, size_t n) {
  int64_t at;
  {
    std::lock_guard<std::mutex> lk(io_mu);
    at = static_cast<int64_t>(total_written);
    total_written += n;
  }
  WriteAt(at, p, n);
}

void ArrowStreamWriter::WriteSchema() {
  serializer.SerializeSchema();
  WriteData(serializer.GetHeader().data(), serializer.GetHeader().size());
}

void ArrowStreamWriter::IoLoop() {
  while (true) {
    WriteJob job;
    {
      std::unique_lock<std::mutex> lk(io_mu);
      io_cv.wait(lk, [&] { return io_stop || !io_jobs.empty(); });
      if (io_jobs.empty()) return;  // stop requested and nothing left
      job = std::move(io_jobs.front());
      io_jobs.pop_front();
    }
    try {
      if (!io_error) WriteMessageAt(job.offset, job.header.data(), job.header.size(), job.body, job.body_size);
    } catch (...) {
      std::lock_guard<std::mutex> lk(io_mu);
      if (!io_error) io_error = std::current_exception();
    }
    {
      std::lock_guard<std::mutex> lk(io_mu);
      if (job.buffer >= 0) buffer_busy[job.buffer] = false;
    }
    io_cv.notify_all();
  }
}

void ArrowStreamWriter::WaitBufferFree(int buffer) {
  std::unique_lock<std::mutex> lk(io_mu);
  io_cv.wait(lk, [&] { return !buffer_busy[buffer]; });
  if (io_error) std::rethrow_exception(io_error);
}

void ArrowStreamWriter::DrainIo() {
  std::unique_lock<std::mutex> lk(io_mu);
  io_cv.wait(lk, [&] { return io_jobs.empty() && !buffer_busy[0] && !buffer_busy[1]; });
  if (io_error) std::rethrow_exception(io_error);
}

void ArrowStreamWriter::Flush(ChunkCollection& buffer) {
  // Serialize() writes into the serializer's current body buffer: it must not be in the I/O thread's hands any more
  WaitBufferFree(serializer.CurrentBody());
  if (serializer.Serialize(buffer) == 0) {
    buffer.Reset();
    CountEmptyFlush();  // the reference counts the flush even when the collection was empty (arrow_stream_writer.cpp:66-71)
    return;
  }
  buffer.Reset();
  WriteJob job;
  job.header = serializer.GetHeader();
  job.body = serializer.GetBody();
  job.body_size = static_cast<size_t>(serializer.GetBodySize());
  job.offset = ReserveRowGroup(job.header.size() + job.body_size);
  {
    std::lock_guard<std::mutex> lk(io_mu);
    job.buffer = serializer.SwapBody();
    buffer_busy[job.buffer] = true;
    io_jobs.push_back(std::move(job));
    if (!io_thread.joinable()) io_thread = std::thread([this] { IoLoop(); });
  }
  io_cv.notify_all();
}

void ArrowStreamWriter::Finalize() {
  if (finalized) return;
  DrainIo();
  const uint8_t end_of_stream[] = {0xFF, 0xFF, 0xFF, 0xFF, 0x00, 0x00, 0x00, 0x00};
  WriteData(end_of_stream, sizeof(end_of_stream));
  ::close(fd);
  fd = -1;
  finalized = true;
  if (Timers().on)
    std::fprintf(stderr, "[mi_writer] append %.3f s, serialize (H2D + K7 + D2H) %.3f s, write (I/O thread) %.3f s\n", Timers().append,
                 Timers().serialize, Timers().write);
  if (Timers().on && Timers().view_sizing > 0)
    std::fprintf(stderr, "[mi_writer] view sizing (host pass over the offsets, pump thread) %.3f s\n", Timers().view_sizing);
}

std::unique_ptr<mi_writer_local> MakeLocal(mi_writer* w) {
  auto l = std::make_unique<mi_writer_local>();
  l->w = w;
  l->buffer = std::make_unique<ChunkCollection>(w->ctx, w->fields);
  l->serializer = std::make_unique<ColumnDataCollectionSerializer>(w->ctx, /*own_stream*/ true);
  l->serializer->Init(&w->writer->Schema(), w->opts.compression);
  return l;
}

}  // namespace miarrow

void mi_writer_local::FlushRowGroup(const std::function<void()>& before_claim, const std::function<void()>& after_claim) {
  miarrow::ArrowStreamWriter& out = *w->writer;
  if (serializer->Serialize(*buffer) == 0) {
    buffer->Reset();
    if (before_claim) before_claim();
    out.CountEmptyFlush();
    if (after_claim) after_claim();
    return;
  }
  buffer->Reset();
  const auto& header = serializer->GetHeader();
  const size_t body = static_cast<size_t>(serializer->GetBodySize());
  if (before_claim) before_claim();
  const int64_t at = out.ReserveRowGroup(header.size() + body);
  if (after_claim) after_claim();
  out.WriteMessageAt(at, header.data(), header.size(), serializer->GetBody(), body);
}


// ------------------------------------------------------------------------------------------------ C ABI
using namespace miarrow;

namespace miarrow {
Context* ContextOf(mi_ctx* c);
}

namespace {
std::string LowerStr(std::string s) {
  for (auto& c : s) c = static_cast<char>(std::tolower(static_cast<unsigned char>(c)));
  return s;
}
std::string UpperStr(std::string s) {
  for (auto& c : s) c = static_cast<char>(std::toupper(static_cast<unsigned char>(c)));
  return s;
}

// DBConfig::ParseMemoryLimit-style sizes: "100", "1KB", "2 MiB", "1gb"
int64_t ParseMemory(const std::string& v) {
  char* end = nullptr;
  double num = std::strtod(v.c_str(), &end);
  if (end == v.c_str() || num < 0) throw InvalidInputException("Could not parse memory size '" + v + "'");
  std::string unit;
  for (const char* p = end; *p; p++)
    if (!std::isspace(static_cast<unsigned char>(*p))) unit += static_cast<char>(std::tolower(static_cast<unsigned char>(*p)));
  double mult = 1;
  if (unit.empty() || unit == "b" || unit == "byte" || unit == "bytes") mult = 1;
  else if (unit == "kb" || unit == "k") mult = 1000.0;
  else if (unit == "mb" || unit == "m") mult = 1000.0 * 1000;
  else if (unit == "gb" || unit == "g") mult = 1000.0 * 1000 * 1000;
  else if (unit == "tb" || unit == "t") mult = 1000.0 * 1000 * 1000 * 1000;
  else if (unit == "kib") mult = 1024.0;
  else if (unit == "mib") mult = 1024.0 * 1024;
  else if (unit == "gib") mult = 1024.0 * 1024 * 1024;
  else if (unit == "tib") mult = 1024.0 * 1024 * 1024 * 1024;
  else throw InvalidInputException("Unknown unit for memory size: '" + unit + "'");
  return static_cast<int64_t>(num * mult);
}

uint64_t ParseU64(const std::string& name, const std::string& v) {
  char* end = nullptr;
  errno = 0;
  unsigned long long x = std::strtoull(v.c_str(), &end, 10);
  if (end == v.c_str() || *end != 0 || errno != 0 || (!v.empty() && v[0] == '-'))
    throw InvalidInputException("Could not convert string '" + v + "' to UINT64 for option " + UpperStr(name));
  return x;
}

// arrow_large_buffer_size: VARCHAR / BLOB / LIST export with 64-bit offsets (ArrowConverter::ToArrowSchema with
// ArrowOffsetSize::LARGE); MAP keeps int32 offsets (the Arrow format has no large map)
void MakeLarge(ArrowField& f) {
  if (f.type == MI_AT_UTF8) f.type = MI_AT_LARGE_UTF8;
  else if (f.type == MI_AT_BINARY) f.type = MI_AT_LARGE_BINARY;
  else if (f.type == MI_AT_LIST) f.type = MI_AT_LARGE_LIST;
  for (auto& c : f.children) MakeLarge(c);
}

// produce_arrow_string_view: VARCHAR at any depth exports as Utf8View, whatever arrow_large_buffer_size says (ArrowConverter::
// ToArrowSchema asks for the view property first); BLOB is not touched (DuckDB writes no binary views)
void MakeView(ArrowField& f) {
  // (a UUID column stays utf8 / large_utf8: DuckDB's switch for UUID looks at the offset size alone)
  if (f.type == MI_AT_UTF8 && f.extension != extfmt::kUuid) f.type = MI_AT_UTF8_VIEW;
  for (auto& c : f.children) MakeView(c);
}

std::vector<ArrowField> FieldsFromC(const mi_field* fields, int32_t n_fields, bool large = false, bool views = false) {
  if (!fields || n_fields <= 0) throw InvalidInputException("writer needs at least one column");
  std::vector<ArrowField> out;
  for (int32_t i = 0; i < n_fields; i++) {
    out.push_back(FieldFromDuckType(fields[i].name, fields[i].duck_type));
    if (views) MakeView(out.back());
    if (large) MakeLarge(out.back());
  }
  return out;
}
}  // namespace

extern "C" {

int mi_write_options_init(mi_write_options* o) {
  return WrapC([&] {
    if (!o) throw InvalidInputException("mi_write_options_init: NULL");
    std::memset(o, 0, sizeof(*o));
    o->row_group_size = 122880;
    o->preserve_insertion_order = 1;
  });
}

int mi_write_options_set(mi_write_options* o, const char* name, const char* value) {
  return WrapC([&] {
    if (!o || !name) throw InvalidInputException("mi_write_options_set: NULL");
    const std::string loption = LowerStr(name);
    if (!value) throw BinderException(UpperStr(loption) + " requires exactly one argument");
    if (loption == "row_group_size" || loption == "chunk_size") {
      if (o->row_group_size_set) throw BinderException("ROW_GROUP_SIZE and ROW_GROUP_SIZE_BYTES are mutually exclusive");
      o->row_group_size = static_cast<int64_t>(ParseU64(loption, value));
      o->row_group_size_set = 1;
    } else if (loption == "row_group_size_bytes") {
      o->row_group_size_bytes = ParseMemory(value);
      o->row_group_size_bytes_set = 1;
    } else if (loption == "row_groups_per_file") {
      o->row_groups_per_file = static_cast<int64_t>(ParseU64(loption, value));
    } else if (loption == "compression" || loption == "codec") {
      const std::string codec = LowerStr(value);
      if (codec == "uncompressed" || codec == "none") o->compression = MI_WRITE_COMPRESSION_NONE;
      else if (codec == "lz4" || codec == "lz4_frame") o->compression = MI_WRITE_COMPRESSION_LZ4_FRAME;
      else if (codec == "zstd") throw NotImplementedException("COMPRESSION zstd: ZSTD bodies are read but not written by this path (use lz4 or uncompressed)");
      else throw BinderException("Unknown COMPRESSION '" + std::string(value) + "' for FORMAT ARROWS: expected uncompressed, none, lz4 or lz4_frame");
    }
    // other options are not ours: the bind loop ignores them (write_arrow_stream.cpp:62-105) -- produce_arrow_string_view and
    // arrow_large_buffer_size among them: those are settings, which reach the struct's fields from the client's properties
  });
}

int mi_write_options_add_kv(mi_write_options* o, const char* key, const char* value, int32_t value_len) {
  return WrapC([&] {
    if (!o || !key || !value) throw InvalidInputException("mi_write_options_add_kv: NULL");
    if (o->n_kv_metadata >= MI_MAX_KV_METADATA) throw InvalidInputException("too many kv_metadata entries");
    if (value_len < 0) value_len = static_cast<int32_t>(std::strlen(value));
    if (std::strlen(key) >= sizeof(o->kv_keys[0]) || static_cast<size_t>(value_len) > sizeof(o->kv_values[0]))
      throw InvalidInputException("kv_metadata entry too long");
    std::snprintf(o->kv_keys[o->n_kv_metadata], sizeof(o->kv_keys[0]), "%s", key);
    std::memcpy(o->kv_values[o->n_kv_metadata], value, static_cast<size_t>(value_len));
    o->kv_value_lens[o->n_kv_metadata] = value_len;
    o->n_kv_metadata++;
  });
}

int mi_write_options_finalize(mi_write_options* o) {
  return WrapC([&] {
    if (!o) throw InvalidInputException("mi_write_options_finalize: NULL");
    if (o->row_group_size_bytes_set) {
      if (o->preserve_insertion_order) {
        throw BinderException(
            "ROW_GROUP_SIZE_BYTES does not work while preserving insertion order. Use \"SET "
            "preserve_insertion_order=false;\" to disable preserving insertion order.");
      }
    } else {
      // We always set a max row group size bytes so we don't use too much memory
      o->row_group_size_bytes = o->row_group_size * 1024;
    }
  });
}

int mi_encode_schema(const mi_field* fields, int32_t n_fields, uint8_t* out, int64_t cap, int64_t* size) {
  return WrapC([&] {
    if (!size) throw InvalidInputException("mi_encode_schema: NULL argument");
    ArrowSchemaModel schema;
    schema.fields = FieldsFromC(fields, n_fields);
    const std::vector<uint8_t> msg = EncodeSchemaMessage(schema);
    *size = static_cast<int64_t>(msg.size());
    if (out && cap >= *size) std::memcpy(out, msg.data(), msg.size());
  });
}

int mi_writer_open(mi_ctx* ctx, const char* path, const mi_field* fields, int32_t n_fields, const mi_write_options* opts,
                   mi_writer** out) {
  return WrapC([&] {
    if (!ctx || !path || !out) throw InvalidInputException("mi_writer_open: NULL argument");
    auto w = std::make_unique<mi_writer>();
    w->ctx = ContextOf(ctx);
    if (opts) {
      w->opts = *opts;
    } else {
      mi_write_options_init(&w->opts);
      mi_write_options_finalize(&w->opts);
    }
    if (w->opts.row_group_size_bytes <= 0) w->opts.row_group_size_bytes = w->opts.row_group_size * 1024;
    w->fields = FieldsFromC(fields, n_fields, w->opts.arrow_large_buffer_size != 0, w->opts.produce_arrow_string_view != 0);
    std::vector<std::pair<std::string, std::string>> kv;
    for (int32_t i = 0; i < w->opts.n_kv_metadata; i++)
      kv.emplace_back(w->opts.kv_keys[i], std::string(w->opts.kv_values[i], static_cast<size_t>(w->opts.kv_value_lens[i])));
    w->buffer = std::make_unique<ChunkCollection>(w->ctx, w->fields);
    if (w->opts.compression != MI_WRITE_COMPRESSION_NONE && w->opts.compression != MI_WRITE_COMPRESSION_LZ4_FRAME)
      throw InvalidInputException("mi_write_options.compression " + std::to_string(w->opts.compression) + " is not a codec of this writer");
    w->writer = std::make_unique<ArrowStreamWriter>(w->ctx, path, w->fields, kv, w->opts.compression);
    w->writer->WriteSchema();
    *out = w.release();
  });
}

int mi_writer_sink(mi_writer* w, const mi_data_chunk* chunk) {
  return WrapC([&] {
    if (!w || !chunk || !w->writer) throw InvalidInputException("mi_writer_sink: bad argument");
    // append data to the local (buffered) chunk collection; flush when it exceeds the row / byte budget
    w->buffer->Append(*chunk);
    if (w->buffer->Count() >= w->opts.row_group_size || w->buffer->SizeInBytes() >= w->opts.row_group_size_bytes) {
      w->writer->Flush(*w->buffer);
    }
  });
}

int mi_writer_local_create(mi_writer* w, mi_writer_local** out) {
  return WrapC([&] {
    if (!w || !w->writer || !out) throw InvalidInputException("mi_writer_local_create: bad argument");
    *out = MakeLocal(w).release();
  });
}

int mi_writer_local_sink(mi_writer_local* l, const mi_data_chunk* chunk) {
  return WrapC([&] {
    if (!l || !chunk) throw InvalidInputException("mi_writer_local_sink: bad argument");
    l->buffer->Append(*chunk);
    if (l->buffer->Count() >= l->w->opts.row_group_size || l->buffer->SizeInBytes() >= l->w->opts.row_group_size_bytes) l->FlushRowGroup();
  });
}

int mi_writer_local_combine(mi_writer_local* l) {
  return WrapC([&] {
    if (!l) throw InvalidInputException("mi_writer_local_combine: NULL");
    if (l->buffer->Count() > 0) l->FlushRowGroup();
  });
}

void mi_writer_local_destroy(mi_writer_local* l) { delete l; }

int mi_writer_finalize(mi_writer* w) {
  return WrapC([&] {
    if (!w || !w->writer) throw InvalidInputException("mi_writer_finalize: bad argument");
    if (w->buffer->Count() > 0) w->writer->Flush(*w->buffer);  // ArrowWriteCombine
    w->writer->Finalize();                                     // ArrowWriteFinalize
  });
}

void mi_writer_close(mi_writer* w) { delete w; }

int64_t mi_writer_row_groups(const mi_writer* w) { return (w && w->writer) ? static_cast<int64_t>(w->writer->NumberOfRowGroups()) : 0; }
int64_t mi_writer_file_size(const mi_writer* w) { return (w && w->writer) ? static_cast<int64_t>(w->writer->FileSize()) : 0; }

int mi_writer_rotate_next_file(const mi_writer* w, int64_t file_size_bytes) {
  if (!w || !w->writer) return 0;
  if (file_size_bytes >= 0 && static_cast<int64_t>(w->writer->FileSize()) > file_size_bytes) return 1;
  if (w->opts.row_groups_per_file > 0 && static_cast<int64_t>(w->writer->NumberOfRowGroups()) >= w->opts.row_groups_per_file) return 1;
  return 0;
}

int mi_ipc_serializer_create(mi_ctx* ctx, const mi_field* fields, int32_t n_fields, mi_writer** out) {
  return WrapC([&] {
    if (!ctx || !out) throw InvalidInputException("mi_ipc_serializer_create: NULL argument");
    auto w = std::make_unique<mi_writer>();
    w->ctx = ContextOf(ctx);
    mi_write_options_init(&w->opts);
    w->fields = FieldsFromC(fields, n_fields);
    w->schema.fields = w->fields;
    w->buffer = std::make_unique<ChunkCollection>(w->ctx, w->fields);
    w->serializer = std::make_unique<ColumnDataCollectionSerializer>(w->ctx);
    w->serializer->Init(&w->schema);
    *out = w.release();
  });
}

int mi_ipc_serialize_schema(mi_writer* w, const uint8_t** blob, int64_t* size) {
  return WrapC([&] {
    if (!w || !w->serializer || !blob || !size) throw InvalidInputException("mi_ipc_serialize_schema: bad argument");
    w->serializer->SerializeSchema();
    w->blob = w->serializer->GetHeader();
    *blob = w->blob.data();
    *size = static_cast<int64_t>(w->blob.size());
  });
}

int mi_writer_append_message(mi_writer* w, const uint8_t* blob, int64_t size) {
  return WrapC([&] {
    if (!w || !w->writer || (!blob && size) || size < 0) throw InvalidInputException("mi_writer_append_message: bad argument");
    if (size == 0) {   // an empty collection still counts as a flushed row group (ArrowStreamWriter::Flush)
      w->writer->CountEmptyFlush();
      return;
    }
    w->writer->WriteMessage(blob, static_cast<size_t>(size), nullptr, 0);
  });
}

int mi_ipc_serialize_chunks(mi_writer* w, const mi_data_chunk* chunks, int32_t n_chunks, const uint8_t** blob, int64_t* size) {
  return WrapC([&] {
    if (!w || !w->serializer || !blob || !size || (!chunks && n_chunks)) throw InvalidInputException("mi_ipc_serialize_chunks: bad argument");
    w->buffer->Reset();
    for (int32_t i = 0; i < n_chunks; i++) w->buffer->Append(chunks[i]);
    w->blob.clear();
    if (w->serializer->Serialize(*w->buffer)) {
      // header || body concatenated, like SerializeArray (to_arrow_ipc.cpp:72-87)
      const auto& h = w->serializer->GetHeader();
      w->blob.resize(h.size() + static_cast<size_t>(w->serializer->GetBodySize()));
      std::memcpy(w->blob.data(), h.data(), h.size());
      std::memcpy(w->blob.data() + h.size(), w->serializer->GetBody(), static_cast<size_t>(w->serializer->GetBodySize()));
    }
    w->buffer->Reset();
    *blob = w->blob.data();
    *size = static_cast<int64_t>(w->blob.size());
  });
}

}  // extern "C"
