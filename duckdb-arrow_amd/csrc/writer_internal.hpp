// writer_internal.hpp -- what writer.cpp, writer_api.cpp (C API) and copy_pump.cpp (COPY pumps) share behind
// include/mi_arrow_ipc.h.
#pragma once

#include <functional>
#include <memory>
#include <mutex>

#include "writer.hpp"

namespace miarrow {

// MI_WRITER_TIMING=1: cumulative seconds per stage of the COPY sink, printed when a writer is finalized
struct SinkTimers {
  double append = 0, serialize = 0, write = 0;
  double view_sizing = 0;   // fused pump, produce_arrow_string_view: the host pass over the Arrow offsets that sizes the data buffers
  bool on = std::getenv("MI_WRITER_TIMING") != nullptr;
  std::mutex mu;  // several sink threads add their stage times
};
SinkTimers& Timers();  // writer.cpp
//! buffer.Append(chunk) under the `append` timer
void TimedAppend(ChunkCollection& buffer, const mi_data_chunk& chunk);   // writer.cpp
//! Staging memory of a writer: pinned memory allocated with `ctx`'s device bound
StagingAllocator PinnedStaging(Context* ctx);   // writer.cpp

// The sink's buffers grow by GrownCapacity -- a quarter of headroom: row groups of one table differ by a few percent, and
// the outgrown buffer is freed at once, which waits for the device to go idle (with the other sink threads' row groups in
// flight a stall of milliseconds).  `keep_bytes`: what the new buffer starts with (pinned buffers).
template <typename Buffer>
void Fit(Buffer& buf, size_t need, size_t keep_bytes = 0) {
  Grow(buf, need, GrownCapacity(need, buf.size(), 1 << 16), keep_bytes);
}

}  // namespace miarrow

struct mi_writer {
  miarrow::Context* ctx = nullptr;
  mi_write_options opts;
  std::vector<miarrow::ArrowField> fields;
  std::unique_ptr<miarrow::ArrowStreamWriter> writer;        // COPY TO file
  std::unique_ptr<miarrow::ChunkCollection> buffer;
  // to_arrow_ipc mode
  miarrow::ArrowSchemaModel schema;
  std::unique_ptr<miarrow::ColumnDataCollectionSerializer> serializer;
  std::vector<uint8_t> blob;
};

// ---- per-thread sink state (ArrowWriteInitializeLocal / Sink / Combine, write_arrow_stream.cpp:141-174): every sink
// thread buffers its own chunks AND serializes its own row groups (H2D + K7 + D2H on a stream of its own), so staging,
// encoding and writing of different row groups overlap; only the claim of the file range is serialised.
struct mi_writer_local {
  mi_writer* w = nullptr;
  std::unique_ptr<miarrow::ChunkCollection> buffer;
  std::unique_ptr<miarrow::ColumnDataCollectionSerializer> serializer;
  //! serializes the buffered rows as one record batch and writes it at the next free position of the file; ordered sinks
  //! wait for their turn in `before_claim` and pass it on in `after_claim`
  void FlushRowGroup(const std::function<void()>& before_claim = nullptr, const std::function<void()>& after_claim = nullptr);
};

namespace miarrow {
std::unique_ptr<mi_writer_local> MakeLocal(mi_writer* w);   // writer.cpp
}
