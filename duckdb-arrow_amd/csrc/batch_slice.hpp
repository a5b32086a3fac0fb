// batch_slice.hpp -- what the metadata of a record batch says about its body: which buffers a projection needs, where
// they go once decompressed, how a big-endian body is swapped, and the per-column buffer table (DecodedBatch) with the size
// checks of NANOARROW_VALIDATION_LEVEL_FULL.  Free functions of (schema, projection, RecordBatchMeta, body span): no I/O, no
// reader state.  `projected_columns` = top-level field index per projected column, empty = no projection.
#pragma once

#include <cstdint>
#include <memory>
#include <utility>
#include <vector>

#include "frame_walk.hpp"
#include "ipc_format.hpp"

namespace miarrow {

//! One field node of a record batch (depth-first), with every buffer it owns.
struct DecodedNode {
  const ArrowField* field = nullptr;
  int32_t parent = -1;
  int32_t depth = 0;
  int64_t length = 0;
  int64_t null_count = 0;
  bool value_only = false;               // dictionary batch: decode with the value type, not as indices
  std::vector<mi_buffer_span> spans;     // validity, buffer 1, buffer 2, ... (views: + variadic data buffers)
  std::vector<int32_t> children;         // indices into DecodedBatch::nodes
};

//! What GetNextBatch produces: the buffers of every (projected) top-level column of one message.
struct DecodedBatch {
  int64_t length = 0;
  const uint8_t* body = nullptr;
  int64_t body_size = 0;
  int64_t body_file_offset = 0;
  bool is_dictionary = false;
  int64_t dict_id = -1;
  bool is_delta = false;
  int32_t compression = -1;
  std::vector<int32_t> column_field;     // top-level field index per output column
  std::vector<int64_t> null_count;       // per output column
  std::vector<int64_t> column_length;    // per output column (== length for top-level fields)
  std::vector<mi_buffer_span> buffers;   // 3 per output column: validity, buf1, buf2
  std::vector<DecodedNode> nodes;        // the projected columns with their descendants, depth-first
  std::vector<int32_t> column_node;      // per output column: its node
  //! Keeps the body alive (file reader: shared ownership like shared_ptr<AllocatedData>, base_stream_reader.cpp:286-294)
  std::shared_ptr<void> owner;
  //! set: `body` is NULL, body_size and every span describe the DECOMPRESSED layout, the bytes are still compressed
  std::shared_ptr<const DeferredBody> deferred;
};

//! Per RecordBatch.buffers entry: does a projected column own it?  Empty = all of them (no projection, dictionary batch,
//! or metadata the walk cannot follow -- the full validation reports that).
std::vector<char> NeededBuffers(const ArrowSchemaModel& schema, const std::vector<int32_t>& projected_columns, const RecordBatchMeta& meta);
//! Byte ranges of a record-batch body that hold the buffers of the projected columns (merged when closer than
//! `gap`); empty = everything (no projection, compressed body, or malformed metadata: the full validation decides).
std::vector<std::pair<int64_t, int64_t>> ProjectedBodyRanges(const ArrowSchemaModel& schema, const std::vector<int32_t>& projected_columns,
                                                             const RecordBatchMeta& meta, int64_t body_length, int64_t gap);

//! Where the buffers of a compressed body lie once decompressed: length and position (64-byte aligned) per
//! RecordBatch.buffers entry, and the size of the whole.
struct DecompressedLayout {
  std::vector<int64_t> ulen, opos;
  int64_t total = 0;
};
//! "the content size the frame's own header declares, if that can be told" (host_codec.hpp: ZstdFrameContentSize)
using FrameContentSize = bool (*)(const uint8_t* frame, int64_t frame_len, uint64_t* content_size);
//! Reads the length prefix of every needed buffer and bounds it by what its field node can hold; throws on a buffer outside
//! the body, a negative length, a length past the bound, or (frame_content_size given) one the frame header contradicts.
DecompressedLayout LayOutDecompressedBody(const ArrowSchemaModel& schema, const std::vector<int32_t>& projected_columns,
                                          RecordBatchMeta* meta, const uint8_t* body, int64_t body_size,
                                          FrameContentSize frame_content_size);
//! A record batch the K8 kernels can expand: little-endian, no list / map among the scanned columns (the planner samples
//! their offsets on the host), compressed and decompressed body below 2 GiB.
bool MayStayCompressed(const ArrowSchemaModel& schema, const std::vector<int32_t>& projected_columns, const RecordBatchMeta& meta,
                       int64_t decompressed_size, int64_t body_size);

//! A big-endian body: every multi-byte number of the needed buffers is swapped in place (on the I/O pool), so the rest of the
//! path sees little-endian buffers (what nanoarrow's decoder does for the reference, base_stream_reader.cpp:68-69)
void SwapBody(const ArrowSchemaModel& schema, const RecordBatchMeta& meta, const std::vector<char>& needed, uint8_t* body, int64_t body_size);

//! Slices body / body_size into per-column buffers, with the size checks of NANOARROW_VALIDATION_LEVEL_FULL that do not
//! need the data (offset monotonicity is checked on the device by the string kernel)
void SliceBatch(const ArrowSchemaModel& schema, const std::vector<int32_t>& projected_columns, const RecordBatchMeta& meta, const uint8_t* body,
                int64_t body_size, int64_t body_file_offset, const std::shared_ptr<void>& owner, DecodedBatch* out);

}  // namespace miarrow
