// writer.hpp -- the encode direction: DuckDB vectors -> Arrow IPC messages.
//
// Mirrors the reference's writer classes (same names and call structure):
//   ColumnDataCollectionSerializer   src/writer/column_data_collection_serializer.cpp  (Init / SerializeSchema /
//                                    Serialize / Flush / GetHeader / GetBody)
//   ArrowStreamWriter                src/writer/arrow_stream_writer.cpp (InitSchema / InitOutputFile / WriteSchema /
//                                    Flush / Finalize / NumberOfRowGroups / FileSize)
//   COPY ... (FORMAT ARROWS) sink    src/writer/write_arrow_stream.cpp:141-174 (ArrowWriteSink / Combine / Finalize)
// ArrowConverter::ToArrowArray / ArrowAppender (DuckDB core; call site column_data_collection_serializer.cpp:85) is the
// part that runs on the GPU: the buffered chunks are staged in pinned memory, DMA'd to HBM, encoded by the K7 kernels
// straight into the IPC body layout (every buffer padded to 8 bytes, column_data_collection_serializer.cpp:86-92 ->
// ArrowIpcEncoderEncodeSimpleRecordBatch) and DMA'd back as one body.
// The units of this direction:
//   chunk_staging.{hpp,cpp} ChunkCollection: the buffered rows of a row group in DuckDB layout (host code only)
//   writer.{hpp,cpp}        the serializer, the stream writer
//   writer_api.cpp          the C API with its option parser
//   writer_plan.{hpp,cpp}   body layout, device staging layout, compressed body layout, encode tasks, the pumps' cut rule
//                           and batch ledger (host code only)
//   writer_compress.cpp     BodyCompressor: the encoded body in HBM -> the LZ4_FRAME body in HBM (COMPRESSION lz4)
//   copy_pump.cpp           mi_writer_sink_scan: the sink-thread pump and the fused pump of COPY (FROM read_arrow(..))
//   writer_internal.hpp     struct mi_writer / mi_writer_local, shared by writer.cpp, writer_api.cpp and copy_pump.cpp
#pragma once

#include <hip/hip_runtime_api.h>

#include <condition_variable>
#include <cstdint>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "chunk_staging.hpp"
#include "engine.hpp"
#include "ipc_format.hpp"
#include "writer_plan.hpp"

namespace miarrow {

//! COPY ... (COMPRESSION lz4): turns the body the K7 kernels left in HBM into the body BodyCompression{LZ4_FRAME, BUFFER}
//! describes, still in HBM.  One per serializer / fused encoder.  Its buffers grow with a quarter of headroom and an
//! outgrown one is kept until the compressor goes: nothing is freed while row groups are in flight.
class BodyCompressor {
 public:
  //! `d_body` holds plain.body_size encoded bytes once the work queued on `s` is done.  Compresses every 64 KiB block,
  //! fetches the size words (synchronises `s` once), lays the compressed body out and queues its compaction on `s`.
  //! Afterwards Layout() describes the body and Body() holds it as soon as `s` has run.
  void Run(const BodyLayout& plain, const uint8_t* d_body, hipStream_t s);
  const CompressedBodyLayout& Layout() const { return layout; }
  const uint8_t* Body() const { return d_out.get(); }

 private:
  template <typename Buffer>
  void Keep(Buffer& buf, std::vector<Buffer>& retired, size_t need);
  DeviceBuffer d_tables, d_slots, d_out;   // d_tables: blocks | size words | copies
  PinnedBuffer h_tables;
  std::vector<DeviceBuffer> retired_device;
  std::vector<PinnedBuffer> retired_pinned;
  CompressedBodyLayout layout;
};

class ColumnDataCollectionSerializer {
 public:
  //! own_stream: the encode runs on a stream of its own (one serializer per sink thread: their H2D / K7 / D2H overlap)
  explicit ColumnDataCollectionSerializer(Context* ctx, bool own_stream = false);
  //! compression: mi_write_options::compression (0 none, 1 LZ4_FRAME bodies)
  void Init(const ArrowSchemaModel* schema, int32_t compression = 0);
  void SerializeSchema();
  //! Serializes the collection as ONE record batch (header + body). Returns the number of messages (0 when empty).
  idx_t Serialize(ChunkCollection& buffer);
  const std::vector<uint8_t>& GetHeader() const { return header; }
  const uint8_t* GetBody() const { return bodies[cur_body].get(); }
  int CurrentBody() const { return cur_body; }
  //! The next Serialize() writes its body into the other pinned buffer (the stream writer hands the current one to its
  //! I/O thread); returns the index of the buffer that was current
  int SwapBody() {
    cur_body ^= 1;
    return cur_body ^ 1;
  }
  int64_t GetBodySize() const { return body_size; }
  int64_t LastBytesRead() const { return plan ? plan->bytes_read : 0; }

 private:
  Context* ctx;
  HipStream owned_stream;         // own_stream: the encode runs here, otherwise
  hipStream_t stream = nullptr;   // on the context's compute stream
  const ArrowSchemaModel* schema = nullptr;
  int32_t compression = 0;
  BodyCompressor compressor;
  std::vector<uint8_t> header;
  PinnedBuffer bodies[2];         // the current one is bodies[cur_body]
  int cur_body = 0;
  DeviceBuffer d_body, d_in;
  PinnedBuffer h_union;   // per union node of the batch: the device addresses of its members' validity words
  int64_t body_size = 0;
  std::unique_ptr<Plan> plan;
};

class ArrowStreamWriter {
 public:
  ArrowStreamWriter(Context* ctx, const std::string& file_path, const std::vector<ArrowField>& fields,
                    const std::vector<std::pair<std::string, std::string>>& metadata, int32_t compression = 0);
  ~ArrowStreamWriter();
  void WriteSchema();
  void Flush(ChunkCollection& buffer);
  void Finalize();
  // ---- thread-safe half, for sink threads that serialize their own row groups (write_arrow_stream.cpp:141-159: every
  // DuckDB thread has a local state; here each also owns a serializer) ----
  //! Claims the next `bytes` of the file for one record-batch message and counts the row group
  int64_t ReserveRowGroup(size_t bytes);
  //! pwrite of a claimed range (any thread, no lock)
  void WriteAt(int64_t offset, const uint8_t* p, size_t n);
  //! One record-batch message: claims its range (ReserveRowGroup), writes header and body there, returns the offset
  int64_t WriteMessage(const uint8_t* header, size_t header_size, const uint8_t* body, size_t body_size);
  //! The writing half, for callers whose claim happens elsewhere: Flush claims on the sink's thread and the I/O thread
  //! writes; an ordered sink claims when its turn has come (mi_writer_local::FlushRowGroup)
  void WriteMessageAt(int64_t offset, const uint8_t* header, size_t header_size, const uint8_t* body, size_t body_size);
  void CountEmptyFlush() { std::lock_guard<std::mutex> lk(io_mu); ++row_group_count; }
  Context* GetContext() const { return ctx; }
  idx_t NumberOfRowGroups() const { return row_group_count; }
  idx_t FileSize() const { return total_written; }
  const ArrowSchemaModel& Schema() const { return schema; }

 private:
  void InitSchema(const std::vector<ArrowField>& fields, const std::vector<std::pair<std::string, std::string>>& metadata, int32_t compression);
  void InitOutputFile(const std::string& file_path);
  void WriteData(const uint8_t* p, size_t n);   // appends at the end of what has been claimed so far

  // record-batch messages are written by an I/O thread while the sink stages the next row group; two body buffers
  // alternate (the reference writes synchronously inside Flush, arrow_stream_writer.cpp:66-77)
  struct WriteJob {
    std::vector<uint8_t> header;
    const uint8_t* body = nullptr;
    size_t body_size = 0;
    int buffer = -1;
    int64_t offset = 0;   // claimed position of the message in the file
  };
  void IoLoop();
  void WaitBufferFree(int buffer);
  void DrainIo();
  std::thread io_thread;
  std::mutex io_mu;
  std::condition_variable io_cv;
  std::deque<WriteJob> io_jobs;
  bool buffer_busy[2] = {false, false};
  bool io_stop = false;
  std::exception_ptr io_error;

  Context* ctx;
  ArrowSchemaModel schema;
  ColumnDataCollectionSerializer serializer;
  std::string file_name;
  int fd = -1;
  idx_t row_group_count = 0;
  idx_t total_written = 0;      // bytes handed to the file (queued writes included: rotation decisions see them at once)
  bool finalized = false;
};

}  // namespace miarrow
