// chunk_staging.hpp -- the buffered rows of one future record batch, in DuckDB layout, ready for the encode kernels.
// Host code only: no GPU header and no engine type, so tests/sanitize/chunk_staging_check.cpp runs it under
// AddressSanitizer + UBSan with malloc for staging memory.  Where the staging memory comes from is the caller's business
// (StagingAllocator): the writer passes pinned memory of its context (writer.cpp: PinnedStaging).
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "ipc_format.hpp"

namespace miarrow {

//! Where staging memory comes from.  `alloc` returns `bytes` bytes or throws; it is called only when a buffer grows.
struct StagingAllocator {
  void* (*alloc)(void* cookie, size_t bytes);
  void (*free)(void* p);
  void* cookie;
};

//! One allocation of a StagingAllocator, size() bytes.  Move-only; an empty one holds nothing and frees nothing.
class StagingBuffer {
 public:
  StagingBuffer() = default;
  StagingBuffer(const StagingAllocator& a, size_t bytes) : p_(a.alloc(a.cookie, bytes)), bytes_(bytes), free_(a.free) {}
  StagingBuffer(StagingBuffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)), free_(o.free_) {}
  StagingBuffer& operator=(StagingBuffer o) noexcept {   // the allocation held before goes with `o`
    std::swap(p_, o.p_);
    std::swap(bytes_, o.bytes_);
    std::swap(free_, o.free_);
    return *this;
  }
  ~StagingBuffer() {
    if (p_) free_(p_);
  }
  template <typename T = uint8_t>
  T* get() const { return static_cast<T*>(p_); }
  size_t size() const { return bytes_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  void* p_ = nullptr;
  size_t bytes_ = 0;
  void (*free_)(void*) = nullptr;
};

//! The buffered rows of one future record batch (the reference's local ColumnDataCollection,
//! write_arrow_stream.cpp:43-52): per FIELD NODE (depth first; a flat column is one node) a staging array in
//! DuckDB layout.  Nested vectors are flattened while they are appended, the way ArrowAppender walks them: struct and
//! fixed-size-list children take every parent row, a list's child rows are gathered in list order (NULL lists add none)
//! and the list node itself stages its list_entry_t rows (the GPU turns their lengths into the int32 Arrow offsets).
class ChunkCollection {
 public:
  //! fields as exported (LargeUtf8 / LargeBinary / LargeList nodes get int64 offsets)
  ChunkCollection(const StagingAllocator& alloc, const std::vector<ArrowField>& fields);
  void Append(const mi_data_chunk& chunk);
  void Reset();
  int64_t Count() const { return count; }
  int64_t SizeInBytes() const { return size_in_bytes; }

  struct Column {
    int32_t enc_kind = 0;    // MI_K_ENC_* of a leaf; MI_K_ENC_LIST32 for a list / map; 0 for struct / fixed-size list
    int32_t arrow_type = 0;  // MI_AT_*
    int64_t param = 0;       // vector element width (or decimal physical width); fixed_size_list: list size
    int32_t width = 0;       // bytes per staged row (list: 16 = one list_entry_t)
    int32_t depth = 0;
    int64_t count = 0;       // rows buffered in this node
    StagingBuffer data;
    StagingBuffer validity;       // uint64_t words
    StagingBuffer heap;           // payload of long strings (pointer = heap offset)
    int64_t heap_used = 0;
    int64_t payload_bytes = 0;    // sum of valid string lengths = size of the Arrow data buffer (list: child rows gathered)
    bool has_nulls = false;
    bool large_offsets = false;   // int64 Arrow offsets (arrow_large_buffer_size)
    // long-string payloads are staged in `heap` and the staged string_t rows point at heap offsets.  When the
    // source vector declares the allocation its long strings live in (mi_vector.heap: the Arrow data buffer of a scanned
    // record batch) and they ascend inside it, the bytes from the first to the last long string of an appended slice are
    // staged with ONE copy; otherwise string by string.  Nothing outside a declared allocation or a string is ever read.
    std::vector<int32_t> children;
    bool IsList() const { return arrow_type == MI_AT_LIST || arrow_type == MI_AT_LARGE_LIST || arrow_type == MI_AT_MAP; }
    bool IsGroup() const { return arrow_type == MI_AT_STRUCT || arrow_type == MI_AT_FIXED_LIST; }
    bool IsUnion() const { return arrow_type == MI_AT_UNION; }   // stages its tags (width 1); children = the members
    bool IsNull() const { return arrow_type == MI_AT_NULL; }     // stages nothing but `count`
  };
  std::vector<Column> columns;     // every field node, depth first
  std::vector<int32_t> roots;      // node of top-level column c

 private:
  int32_t AddField(const ArrowField& f, int32_t depth);
  // rows [start, start + n) of vector `v` -> node `ni`: the dispatcher, and one function per sort of node
  void AppendNode(int32_t ni, const mi_vector& v, int64_t start, int64_t n);
  void AppendGroup(int32_t ni, const mi_vector& v, int64_t start, int64_t n);
  void AppendList(int32_t ni, const mi_vector& v, int64_t start, int64_t n);
  void AppendUnion(int32_t ni, const mi_vector& v, int64_t start, int64_t n);
  void AppendFixed(Column& c, const mi_vector& v, int64_t start, int64_t n);
  void AppendStrings(Column& c, const mi_vector& v, int64_t start, int64_t n);
  void AppendValidity(Column& c, const mi_vector& v, int64_t vbit, int64_t n);
  void Reserve(Column& c, int64_t rows, int64_t extra_heap);
  void Fit(StagingBuffer& buf, size_t need, size_t keep_bytes);
  StagingAllocator alloc;
  int64_t count = 0;
  int64_t size_in_bytes = 0;
};

//! DuckDB logical type of a leaf -> how its vector is laid out and which K7 kernel encodes it
void EncodePlanFor(const ArrowField& f, int32_t* enc_kind, int64_t* param, int32_t* width);
//! append `n` bits of `src` starting at bit `spos` (src NULL = all ones) to `dst` at bit position `pos`
void AppendBits(uint64_t* dst, int64_t pos, const uint64_t* src, int64_t spos, int64_t n);
inline bool BitAt(const uint64_t* v, int64_t i) { return !v || ((v[i >> 6] >> (i & 63)) & 1); }

}  // namespace miarrow
