// chunk_staging.cpp -- see chunk_staging.hpp.
#include "chunk_staging.hpp"

#include <algorithm>
#include <cstring>
#include <string>

#include "extension_format.hpp"
#include "union_format.hpp"

namespace miarrow {

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

ChunkCollection::ChunkCollection(const StagingAllocator& alloc_p, const std::vector<ArrowField>& fields) : alloc(alloc_p) {
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

// The buffers grow by GrownCapacity -- a quarter of headroom, in 64 KiB granules -- and the new one starts with the first
// `keep_bytes` of the old.  The allocator is called only here, and only when `buf` is too small.
void ChunkCollection::Fit(StagingBuffer& buf, size_t need, size_t keep_bytes) {
  if (buf && need <= buf.size()) return;
  StagingBuffer grown(alloc, GrownCapacity(need, buf.size(), 1 << 16));
  if (buf && keep_bytes) std::memcpy(grown.get(), buf.get(), std::min(keep_bytes, buf.size()));
  buf = std::move(grown);
}

void ChunkCollection::Reserve(Column& c, int64_t rows, int64_t extra_heap) {
  if (c.width > 0)
    Fit(c.data, static_cast<size_t>(rows) * static_cast<size_t>(c.width) + 64, static_cast<size_t>(c.count) * static_cast<size_t>(c.width));
  const size_t old_vcap = c.validity.size();
  const size_t used = static_cast<size_t>((c.count + 63) / 64) * 8;
  Fit(c.validity, static_cast<size_t>((rows + 63) / 64) * 8 + 16, used);
  if (c.validity.size() != old_vcap) std::memset(c.validity.get() + used, 0xFF, c.validity.size() - used);
  if (extra_heap > 0) Fit(c.heap, static_cast<size_t>(c.heap_used + extra_heap) + 64, static_cast<size_t>(c.heap_used));
}

void ChunkCollection::Append(const mi_data_chunk& chunk) {
  if (chunk.n_columns != static_cast<int32_t>(roots.size()))
    throw InvalidInputException("DataChunk has " + std::to_string(chunk.n_columns) + " columns, the writer expects " + std::to_string(roots.size()));
  const int64_t n = chunk.size;
  if (n <= 0) return;
  if (n > MI_VECTOR_SIZE * 1024) throw InvalidInputException("DataChunk too large");
  for (size_t ci = 0; ci < roots.size(); ci++) AppendNode(roots[ci], chunk.columns[ci], 0, n);
  count += n;
}

// bit of v.validity that belongs to row `start`
static int64_t FirstBit(const mi_vector& v, int64_t start) { return static_cast<int64_t>(v.validity_shift) + start; }

// the validity bits of rows [vbit, vbit + n) of `v` behind the node's, and whether the node has seen a NULL
void ChunkCollection::AppendValidity(Column& c, const mi_vector& v, int64_t vbit, int64_t n) {
  AppendBits(c.validity.get<uint64_t>(), c.count, v.validity, vbit, n);
  if (v.validity && !c.has_nulls) {
    for (int64_t i = 0; i < n; i++)
      if (!BitAt(v.validity, vbit + i)) { c.has_nulls = true; break; }
  }
}

// rows [start, start + n) of vector `v` -> node `ni` (and, for nested types, the rows they own in the child nodes).
// A node that has children is handed on by its index: its function takes `columns[ni]` anew for every step of its own,
// and holds no reference to it across the append of a child.
void ChunkCollection::AppendNode(int32_t ni, const mi_vector& v, int64_t start, int64_t n) {
  if (n <= 0) return;
  Column& c = columns[static_cast<size_t>(ni)];
  if (c.IsNull()) {   // nothing to stage: every row is NULL
    c.count += n;
    return;
  }
  if (c.IsUnion()) return AppendUnion(ni, v, start, n);
  if (!c.IsGroup() && !v.data) throw InvalidInputException("DataChunk column " + std::to_string(ni) + " has no data");
  if ((c.IsList() || c.IsGroup()) && (v.n_children < (c.arrow_type == MI_AT_STRUCT ? static_cast<int32_t>(c.children.size()) : 1) || !v.children))
    throw InvalidInputException("nested vector without child vectors");
  if (c.IsGroup()) return AppendGroup(ni, v, start, n);
  if (c.IsList()) return AppendList(ni, v, start, n);
  if (c.enc_kind == MI_K_ENC_STR32 || c.enc_kind == MI_K_ENC_STRVIEW) return AppendStrings(c, v, start, n);
  AppendFixed(c, v, start, n);
}

// A struct / fixed-size list: its own validity words, and every row (every `param` rows) of each child
void ChunkCollection::AppendGroup(int32_t ni, const mi_vector& v, int64_t start, int64_t n) {
  int64_t mult;
  size_t n_children;
  {
    Column& c = columns[static_cast<size_t>(ni)];  // (children are appended after this block: `columns` never grows here)
    Reserve(c, c.count + n, 0);
    AppendValidity(c, v, FirstBit(v, start), n);
    c.count += n;
    mult = c.arrow_type == MI_AT_FIXED_LIST ? c.param : 1;
    n_children = c.children.size();
  }
  for (size_t k = 0; k < n_children; k++) AppendNode(columns[static_cast<size_t>(ni)].children[k], v.children[k], start * mult, n * mult);
}

// A list / map: the list_entry_t rows are staged as they are (the GPU turns the lengths of the valid rows into Arrow
// offsets); the child rows of every valid list are gathered here, in list order (ArrowListData::Append), adjacent lists
// as one run
void ChunkCollection::AppendList(int32_t ni, const mi_vector& v, int64_t start, int64_t n) {
  const int64_t vbit = FirstBit(v, start);
  const uint64_t* ent = static_cast<const uint64_t*>(v.data) + 2 * start;
  int32_t child;
  {
    Column& c = columns[static_cast<size_t>(ni)];
    Reserve(c, c.count + n, 0);
    AppendValidity(c, v, vbit, n);
    std::memcpy(c.data.get() + static_cast<size_t>(c.count) * 16, ent, static_cast<size_t>(n) * 16);
    c.count += n;
    size_in_bytes += n * 16;
    child = c.children[0];
  }
  int64_t run_start = 0, run_len = 0;
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
    Column& c = columns[static_cast<size_t>(ni)];
    c.payload_bytes += l;   // child rows so far = the last Arrow offset
    if (c.payload_bytes > 0x7FFFFFFFll && !c.large_offsets)
      throw InvalidInputException("Arrow Appender: The maximum combined list offset for regular list buffers is 2147483647 but the offset of " +
                                  std::to_string(c.payload_bytes) +
                                  " exceeds this.\n* SET arrow_large_buffer_size=true to use large list buffers");
  }
  if (run_len > 0) AppendNode(child, v.children[0], run_start, run_len);
}

// A fixed-width leaf: the rows as they are
void ChunkCollection::AppendFixed(Column& c, const mi_vector& v, int64_t start, int64_t n) {
  const int64_t vbit = FirstBit(v, start);
  Reserve(c, c.count + n, 0);
  AppendValidity(c, v, vbit, n);
  std::memcpy(c.data.get() + static_cast<size_t>(c.count) * static_cast<size_t>(c.width),
              static_cast<const uint8_t*>(v.data) + static_cast<size_t>(start) * static_cast<size_t>(c.width),
              static_cast<size_t>(n) * static_cast<size_t>(c.width));
  if (c.enc_kind == MI_K_ENC_UUID_TEXT) {   // 36 bytes of text per valid row, none per NULL row
    int64_t valid = n;
    if (v.validity)
      for (int64_t i = 0; i < n; i++) valid -= BitAt(v.validity, vbit + i) ? 0 : 1;
    c.payload_bytes += valid * extfmt::kUuidTextBytes;
  }
  size_in_bytes += n * c.width;
  c.count += n;
}

// A string leaf (MI_K_ENC_STR32 / MI_K_ENC_STRVIEW): the string_t rows, and the bytes of the long ones in `heap`
void ChunkCollection::AppendStrings(Column& c, const mi_vector& v, int64_t start, int64_t n) {
  const int64_t vbit = FirstBit(v, start);
  const mi_string_t* s = static_cast<const mi_string_t*>(v.data) + start;
  // one pass over the rows decides how the long-string payloads of this slice are staged
  int64_t payload = 0, long_bytes = 0, extra_heap = 0;
  bool one_copy = false;
  uint64_t region_lo = 0, region_hi = 0;
  {
    const uint64_t heap_lo = reinterpret_cast<uint64_t>(v.heap), heap_hi = heap_lo + static_cast<uint64_t>(v.heap_size > 0 ? v.heap_size : 0);
    bool ascending_inside = v.heap != nullptr;
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
  }
  Reserve(c, c.count + n, extra_heap);
  AppendValidity(c, v, vbit, n);
  mi_string_t* dst = c.data.get<mi_string_t>() + c.count;
  std::memcpy(dst, s, static_cast<size_t>(n) * sizeof(mi_string_t));
  if (extra_heap > 0) {
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
  // the data buffer of a view column holds the long strings alone
  c.payload_bytes += c.enc_kind == MI_K_ENC_STRVIEW ? long_bytes : payload;
  size_in_bytes += extra_heap + n * c.width;
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
  const int64_t vbit = FirstBit(v, start);
  {
    Column& c = columns[static_cast<size_t>(ni)];
    Reserve(c, c.count + n, 0);
    AppendValidity(c, v, vbit, n);
    std::memcpy(c.data.get() + c.count, tags + start, static_cast<size_t>(n));
    c.count += n;
    size_in_bytes += n;
  }
  // bit start + i of a member's mask = row i of the slice
  std::vector<uint64_t> mask(static_cast<size_t>((start + n + 63) / 64));
  for (int32_t k = 0; k < m; k++) {
    const mi_vector& mv = v.children[1 + k];
    const int64_t mbit = FirstBit(mv, start);
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

}  // namespace miarrow
