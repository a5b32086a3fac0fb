// ipc_stream_reader.hpp -- host half of the scan path: Arrow IPC message framing.
//
// Takes the place of the reference's reader classes (same class names, same error strings):
//   IPCStreamReader        src/include/ipc/stream_reader/base_stream_reader.hpp:44-126, base_stream_reader.cpp
//   IPCFileStreamReader    src/ipc/stream_reader/ipc_file_stream_reader.cpp
//   IPCBufferStreamReader  src/ipc/stream_reader/ipc_buffer_stream_reader.cpp
// What differs by design: metadata is parsed by ipc_format.cpp instead of nanoarrow, GetNextBatch yields a flat
// buffer table (DecodedBatch) instead of an ArrowArray, and the file reader can read message bodies straight into
// caller-provided (pinned) memory so the body is copied exactly once on its way to HBM.
// The units around it: io_pool (threads the bodies are read and decompressed on), host_codec (libzstd / liblz4),
// frame_walk (tables for the GPU decompressors), batch_slice (everything the metadata says about a body: DecodedBatch).
#pragma once

#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "batch_slice.hpp"

namespace miarrow {

struct ArrowIpcMessagePrefix {  // base_stream_reader.hpp:39-42
  uint32_t continuation_token;
  int32_t metadata_size;
};

//! == ArrowIPCBuffer (src/include/table_function/scan_arrow_ipc.hpp:19-23)
struct ArrowIPCBuffer {
  ArrowIPCBuffer(uint64_t ptr_p, uint64_t size_p) : ptr(ptr_p), size(size_p) {}
  uint64_t ptr;
  uint64_t size;
};

struct BatchIndexEntry {
  int64_t prefix_offset;
  int32_t meta_len;
  int32_t type;
  int64_t body_offset;
  int64_t body_len;
  int64_t n_rows;
};

//! Base IPC Reader
class IPCStreamReader {
 public:
  virtual ~IPCStreamReader() = default;

  //! Gets the output schema, which is the file schema with projection pushdown being considered
  const ArrowSchemaModel& GetOutputSchema();
  //! Gets the base schema with no projection pushdown
  const ArrowSchemaModel& GetBaseSchema();
  //! Gets the next batch; false at end of stream.  accept_dictionaries: also return DictionaryBatch messages
  //! (the reference accepts RecordBatch only, base_stream_reader.cpp:86-96)
  bool GetNextBatch(DecodedBatch* out, bool accept_dictionaries = false, bool skip_record_batch_body = false);
  //! Sets the projection pushdown for this reader
  void SetColumnProjection(const std::vector<std::string>& column_names);
  bool HasProjection() const { return !projected_columns.empty(); }
  //! Drops the reader's own reference to the body of the message it returned last (the DecodedBatch keeps its own);
  //! a caller that recycles body buffers needs this when it stops pulling from a reader
  void ReleaseCurrentBody() {
    cur_owner.reset();
    compressed_owner.reset();
    cur_ptr = nullptr;
    cur_size = 0;
  }

  MessageType ReadNextMessage(std::vector<MessageType> expected_types, bool end_of_stream_ok = true);
  virtual MessageType ReadNextMessage() = 0;
  virtual double GetProgress() { return 0; }
  //! Header-only walk of the remaining input: batch boundaries for record-batch sharding
  virtual const std::vector<BatchIndexEntry>& BuildIndex() = 0;

  //! Where message bodies are placed (file reader only). Default: an internal 64-byte aligned heap block per message.
  using BodyAllocator = std::function<std::shared_ptr<void>(size_t bytes, MessageType type, uint8_t** ptr)>;
  void SetBodyAllocator(BodyAllocator a) { body_allocator = std::move(a); }

  //! LZ4_FRAME record batches (not dictionary batches, not big-endian streams) are handed out still compressed, with the
  //! frame / block tables a GPU decompressor needs (DecodedBatch::deferred); everything else is decompressed here as before
  void SetDeferLz4(bool on) { defer_lz4 = on; }
  //! the same for ZSTD record batches (frames with a dictionary id or a content checksum stay with the host library)
  void SetDeferZstd(bool on) { defer_zstd = on; }

  static constexpr uint32_t kContinuationToken = 0xFFFFFFFF;

 protected:
  //! With the prefix in message_prefix: checks the metadata size, then header and body through the two virtual seams
  //! below (what the reference does in DecodeMetadata + DecodeMessage, base_stream_reader.cpp:214-236)
  MessageType FinishMessage();
  //! Reads and parses the flatbuffer header (message_header_size = prefix + metadata); true = end-of-stream marker
  virtual bool DecodeHeader(idx_t message_header_size) = 0;
  //! Makes the message body available at cur_ptr / cur_size
  virtual void DecodeBody() = 0;

  //! Parses the current header into `message` (ENODATA == metadata_size 0 => returns false)
  bool ParseHeader(const uint8_t* header_with_prefix, idx_t size);
  //! Rewrites meta->buffers to the decompressed layout.  Either the body stays compressed and the frame / block tables
  //! are returned (SetDeferLz4 / SetDeferZstd; cur_size becomes the decompressed size, cur_ptr stays), or cur_ptr/cur_size
  //! become the body decompressed on the host (per buffer; the CPU step the reference performs in DuckDBDecompressZstd,
  //! base_stream_reader.cpp:11-32) and nullptr is returned
  std::shared_ptr<const DeferredBody> DecompressBody(RecordBatchMeta* meta);
  //! Big-endian stream: refuses run-end encoded columns, then swaps the body in place (after decompression); a
  //! caller-owned body is copied first
  void SwapBodyEndianness(const RecordBatchMeta& meta);
  //! The first projected top-level field (any, without a projection) for which `has` holds, or nullptr
  const ArrowField* WantedFieldWith(bool (*has)(const ArrowField&)) const;
  bool defer_lz4 = false, defer_zstd = false;
  std::shared_ptr<void> compressed_owner;

  MessageHeader message;               // the decoder's message_type / body_size_bytes
  const uint8_t* message_meta = nullptr;  // flatbuffer of the current message
  int64_t message_meta_len = 0;

  std::vector<int32_t> projected_columns;  // top-level field index per projected column
  ArrowSchemaModel projected_schema;
  ArrowSchemaModel base_schema;
  bool have_base_schema = false;

  //! Information on current buffer
  const uint8_t* cur_ptr = nullptr;
  int64_t cur_size = 0;
  int64_t cur_body_offset = 0;
  std::shared_ptr<void> cur_owner;

  bool finished = false;
  bool skip_record_batch_body = false;  // sharded scans: batches owned by another rank are stepped over unread
  ArrowIpcMessagePrefix message_prefix{};
  BodyAllocator body_allocator;
  std::vector<BatchIndexEntry> index;
  bool index_built = false;
};

//! Reads from a file (stream format, or the stream embedded in the file format)
class IPCFileStreamReader : public IPCStreamReader {
 public:
  explicit IPCFileStreamReader(const std::string& path);
  ~IPCFileStreamReader() override;

  MessageType ReadNextMessage() override;
  double GetProgress() override;
  const std::vector<BatchIndexEntry>& BuildIndex() override;
  //! Positions the reader on a message found by BuildIndex (record-batch sharding)
  void Seek(int64_t prefix_offset);

 protected:
  const uint8_t* ReadData(uint8_t* ptr, idx_t size);
  bool DecodeHeader(idx_t message_header_size) override;
  void DecodeBody() override;
  bool ReadPrefix();
  void SkipBodyPadding();
  bool IndexFromFooter();

 private:
  int fd = -1;
  std::string path;
  int64_t file_size = 0;
  int64_t offset = 0;  // BufferedFileReader::CurrentOffset
  std::vector<uint8_t> message_header;
};

//! Reads from caller-owned memory, zero copy
class IPCBufferStreamReader : public IPCStreamReader {
 public:
  explicit IPCBufferStreamReader(std::vector<ArrowIPCBuffer> buffers);

  MessageType ReadNextMessage() override;
  const std::vector<BatchIndexEntry>& BuildIndex() override;
  double GetProgress() override;

 protected:
  const uint8_t* ReadData(idx_t size);
  bool DecodeHeader(idx_t message_header_size) override;
  void DecodeBody() override;

 private:
  //! positions `view` on the next byte of the buffer list nobody has read yet; false when there is none
  bool SeekUnreadByte();
  struct View {
    const uint8_t* ptr = nullptr;
    bool opened = false;            // false until the first buffer is opened
    int64_t size = 0;
    int64_t pos = 0;
  };
  std::vector<ArrowIPCBuffer> buffers;
  View view;
  idx_t view_index = 0;             // which buffer `view` is a window of
  const uint8_t* prefix_at = nullptr;  // where the current message's prefix lies in the caller's memory
};

}  // namespace miarrow
