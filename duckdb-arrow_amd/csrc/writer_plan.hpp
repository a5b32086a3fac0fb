// writer_plan.hpp -- what the encode direction decides without a GPU, one definition each: where the buffers of a record
// batch lie in its IPC body, where its staged arrays lie in the device buffer the kernels read, the encode task of a field
// node, where the COPY pumps end a row group, and which record batches of the scan a pump still holds.  Host code only (no
// HIP header), so tests/sanitize/writer_plan_check.cpp runs it under AddressSanitizer and ThreadSanitizer.  writer.cpp
// (serializer) and copy_pump.cpp (both pumps) call it.
#pragma once

#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <exception>
#include <functional>
#include <mutex>
#include <vector>

#include "ipc_format.hpp"
#include "lz4_encode_format.hpp"

namespace miarrow {

constexpr size_t kBufferAlign = 64;  // Arrow's recommended buffer alignment; any multiple of 8 is valid IPC
inline size_t RoundUp(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ------------------------------------------------------------------------------------------------ body layout
//! EncodeNode::kind of an Arrow null node: no buffers, no task; its field node is {length = rows, null_count = rows}
constexpr int32_t kEncNodeNull = -1;
//! One field node of a record batch to encode
struct EncodeNode {
  int32_t kind = 0;             // MI_K_ENC_* of a leaf; MI_K_ENC_LIST32: list / map; MI_K_ENC_VALIDITY: struct / fixed-size list;
                                // MI_K_ENC_UNION: a union (its members are nodes of their own); kEncNodeNull
  int64_t param = 0;            // leaf: vector element width (or decimal physical width)
  bool large_offsets = false;   // int64 Arrow offsets
  int64_t rows = 0;
  int64_t payload_bytes = 0;    // size of the Arrow data buffer: MI_K_ENC_STR32 the bytes of the valid rows, MI_K_ENC_STRVIEW of
                                // those among them that are longer than 12 bytes, MI_K_ENC_UUID_TEXT 36 per valid row
};
struct BodyLayout {
  std::vector<mi_buffer_span> spans;   // RecordBatch.buffers
  std::vector<int32_t> first_span;     // per node: its validity span; offsets / data and string data follow it.  A union's one
                                       // span is its type ids (it has no validity), a null node has none
  int64_t body_size = 0;
};
//! Field nodes depth first, per node validity (always emitted, ArrowAppender::FinalizeChild), then offsets / data -- the
//! order ArrowIpcEncoderEncodeSimpleRecordBatch walks the ArrowArray tree; every buffer starts on a multiple of
//! kBufferAlign.  A string-view node (MI_K_ENC_STRVIEW) has three: bitmap, 16 bytes of view per row, one data buffer.
//! A union node (MI_K_ENC_UNION) has ONE, its int8 type ids (sparse: no offsets, and a union never has a bitmap); an
//! interval node (MI_K_ENC_INTERVAL) bitmap + 16 bytes per row; a null node (kEncNodeNull) none at all.
//! Throws when a node has more than INT32_MAX rows or int32 offsets cannot address its string bytes.
void LayOutBody(const std::vector<EncodeNode>& nodes, BodyLayout* out);

//! What one field node has staged for the device
struct StagingNode {
  int64_t rows = 0;
  int32_t width = 0;        // bytes per staged row
  int64_t heap_used = 0;    // bytes of long strings
  bool is_union = false;
  int32_t n_members = 0;    // union: its members
};
struct StagingLayout {
  struct Node {
    size_t data, validity, heap;
    size_t members, masks, mask_stride;   // union nodes: the addresses of its members' validity words (kMaxMembers of them),
                                          // and the scratch its pass leaves their masks in, mask k at masks + k * mask_stride
  };
  std::vector<Node> nodes;
  size_t total = 0;
};
//! Where the staged arrays of every node lie in the one device buffer the serializer copies them into: nodes depth first,
//! per node data, validity, heap, then a union's two extras; every array starts on a multiple of 256 and has a few bytes
//! of slack behind it (the kernels load whole words)
void LayOutStaging(const std::vector<StagingNode>& nodes, StagingLayout* out);

//! Where the K7 kernels read one node (device addresses)
struct EncodeInput {
  const void* data = nullptr;       // DuckDB vector data; list: list_entry_t rows; struct / fixed-size list: its validity words
  const void* validity = nullptr;   // validity words, NULL when every row is valid
  const void* heap = nullptr;       // MI_K_ENC_STR32 / MI_K_ENC_STRVIEW: the bytes long string_t rows point into ...
  uint64_t ptr_base = 0;            // ... and the pointer value its byte 0 has inside them
  // MI_K_ENC_UNION (data = the tags, validity = the union's words):
  const void* member_validity = nullptr;   // m words: the address of every member's own validity words, 0 = all valid
  void* masks = nullptr;                   // where the pass leaves the members' effective masks, mask k at k * mask_stride
  int64_t mask_stride = 0;                 // bytes, a multiple of 8
  const void* parent_validity = nullptr;   // a struct parent's words, NULL = none
};
//! The encode task of `node` (not a kEncNodeNull one: it has none): `spans` are the node's own (BodyLayout::first_span), `body` is where the body starts in HBM
mi_col_task EncodeTask(const EncodeNode& node, const mi_buffer_span* spans, const EncodeInput& in, uint8_t* body);

// ------------------------------------------------------------------------------------------------ compressed body
// BodyCompression{LZ4_FRAME, BUFFER}: every buffer of the encoded body is cut into 64 KiB blocks, the compress kernel leaves
// block b in slot b of its scratch buffer and reports a size word for it (lz4_encode_format.hpp), and the body that goes to
// the file is put together from those.  Blocks are numbered in span order; an empty buffer has none.

//! The blocks of `plain`'s buffers, in the order of their size words
std::vector<lz4enc::BlockIn> BlocksOfBody(const BodyLayout& plain);

struct CompressedBodyLayout {
  std::vector<mi_buffer_span> spans;     // RecordBatch.buffers: {offset, int64 prefix + frame (or + raw bytes), unpadded}
  int64_t body_size = 0;                 // a multiple of 8
  std::vector<lz4enc::BodyCopy> copies;  // what the compaction kernel copies into the (zeroed) body
};
//! Buffers start on multiples of 8.  A buffer whose frame is smaller than its bytes becomes {its length, the frame}, any
//! other {-1, its bytes}, an empty one stays empty.  `words`: one size word per block of BlocksOfBody(plain).
void LayOutCompressedBody(const BodyLayout& plain, const std::vector<uint32_t>& words, CompressedBodyLayout* out);

// ------------------------------------------------------------------------------------------------ cut rule
// The COPY pumps end a row group after the 2048-row chunk with which its rows reach row_group_size, or its rows x the
// staged row width reach row_group_size_bytes.  The one-thread sink (mi_writer_sink) compares ChunkCollection::
// SizeInBytes() with row_group_size_bytes instead -- the bytes really staged, string heap included -- so a pump writes
// the one-thread file only when row_group_size is the limit that binds.

//! Bytes a row of the scan's output takes in the sink's staging arrays (strings, nested and constant columns: 16)
template <typename ScanColumns>
int64_t StagedRowBytes(const ScanColumns& columns) {
  int64_t b = 0;
  for (auto& c : columns) {
    int32_t kind, wd;
    int64_t param;
    b += (!c.is_constant() && c.field.Plan(&kind, &param, &wd)) ? wd : 16;
  }
  return std::max<int64_t>(1, b);
}
//! Rows with which a row group is full
inline int64_t RowsPerGroup(const mi_write_options& o, int64_t row_bytes) {
  return std::max<int64_t>(1, std::min(o.row_group_size, (o.row_group_size_bytes + row_bytes - 1) / row_bytes));
}

//! Chunks [window0, window1) of one record batch that go to the same row group
struct CutPiece {
  int32_t window0 = 0, window1 = 0;
  bool starts_group = false;   // no earlier piece belongs to its row group
  bool closes_group = false;   // the row group is full with it (else it ends with the batch and the group goes on)
};
class RowGroupCutter {
 public:
  explicit RowGroupCutter(int64_t rows_per_group_p) : rows_per_group(rows_per_group_p) {}
  //! the next record batch of the stream, `rows` long: its pieces in order (none when it is empty)
  std::vector<CutPiece> Cut(int64_t rows);
  int64_t OpenRows() const { return open_rows; }   // rows of the row group that is not full yet

 private:
  const int64_t rows_per_group;
  int64_t open_rows = 0;
};

// ------------------------------------------------------------------------------------------------ batch ledger
//! The record batches a pump has acquired from the scan and not given back: a batch goes back once it is fully cut into
//! pieces and every piece is closed (appended by a sink thread, or read by the GPU).  Pieces are closed on any thread; the
//! scan belongs to the pump thread, so only that thread releases.  Shares the pump's mutex, condition variable and error.
template <typename Ref>
class BatchLedger {
 public:
  BatchLedger(std::mutex& mu_p, std::condition_variable& cv_p, const std::exception_ptr& error_p, std::function<void(const Ref&)> release_p)
      : mu(mu_p), cv(cv_p), error(error_p), release(std::move(release_p)) {}
  //! pump thread: a newly acquired batch -> its token
  int Hold(const Ref& ref) {
    std::lock_guard<std::mutex> lk(mu);
    held.push_back(Entry{ref, 0, false, false});
    return static_cast<int>(held.size() - 1);
  }
  Ref RefOf(int tok) {
    std::lock_guard<std::mutex> lk(mu);
    return held[static_cast<size_t>(tok)].ref;
  }
  void OpenPiece(int tok) {
    std::lock_guard<std::mutex> lk(mu);
    held[static_cast<size_t>(tok)].open++;
  }
  void ClosePiece(int tok) {
    std::lock_guard<std::mutex> lk(mu);
    Entry& e = held[static_cast<size_t>(tok)];
    if (--e.open == 0 && e.fully_cut) Queue(tok);
  }
  //! pump thread: no piece of this batch will be opened any more
  void MarkFullyCut(int tok) {
    std::lock_guard<std::mutex> lk(mu);
    Entry& e = held[static_cast<size_t>(tok)];
    e.fully_cut = true;
    if (e.open == 0) Queue(tok);
  }
  //! pump thread: gives back what is ready (wait: blocks until something is, or the pump has failed -- which it rethrows)
  void ReleaseReady(bool wait) {
    std::unique_lock<std::mutex> lk(mu);
    if (wait) cv.wait(lk, [&] { return error || !to_release.empty(); });
    if (error) std::rethrow_exception(error);
    while (!to_release.empty()) {
      Entry& e = held[static_cast<size_t>(to_release.front())];
      to_release.pop_front();
      e.released = true;
      n_released++;
      const Ref ref = e.ref;
      lk.unlock();
      release(ref);
      lk.lock();
    }
  }
  //! pump thread, on the way out (no other thread touches the ledger any more): gives back every batch still held
  void ReleaseAll() {
    std::unique_lock<std::mutex> lk(mu);
    to_release.clear();
    for (size_t tok = 0; tok < held.size(); tok++) {
      if (held[tok].released) continue;
      held[tok].released = true;
      n_released++;
      const Ref ref = held[tok].ref;
      lk.unlock();
      release(ref);
      lk.lock();
    }
  }
  //! batches held and not given back yet
  int64_t Unreleased() {
    std::lock_guard<std::mutex> lk(mu);
    return static_cast<int64_t>(held.size()) - n_released;
  }

 private:
  struct Entry { Ref ref; int open; bool fully_cut, released; };
  void Queue(int tok) {   // under mu
    to_release.push_back(tok);
    cv.notify_all();
  }
  std::mutex& mu;
  std::condition_variable& cv;
  const std::exception_ptr& error;
  const std::function<void(const Ref&)> release;
  std::vector<Entry> held;      // index = token
  std::deque<int> to_release;   // tokens ready to go back
  int64_t n_released = 0;
};

}  // namespace miarrow
