// writer.cpp -- see writer.hpp.
#include "writer.hpp"
#include "writer_internal.hpp"
#include "union_format.hpp"
#include "writer_plan.hpp"

#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>

namespace miarrow {

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
}  // namespace

void TimedAppend(ChunkCollection& buffer, const mi_data_chunk& chunk) {
  ScopedTimer timer(&Timers().append);
  buffer.Append(chunk);
}

StagingAllocator PinnedStaging(Context* ctx) {
  return StagingAllocator{
      [](void* cookie, size_t bytes) {
        static_cast<Context*>(cookie)->Bind();
        void* p = nullptr;
        MI_HIP_CHECK(hipHostMalloc(&p, bytes, hipHostMallocDefault));
        return p;
      },
      [](void* p) { (void)hipHostFree(p); }, ctx};
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

  // the body layout, and the device staging layout beside it (writer_plan.hpp)
  const size_t n_nodes = buffer.columns.size();
  std::vector<EncodeNode> nodes(n_nodes);
  std::vector<StagingNode> staged(n_nodes);
  size_t n_unions = 0;
  for (size_t ci = 0; ci < n_nodes; ci++) {
    auto& c = buffer.columns[ci];
    nodes[ci] = EncodeNode{c.IsGroup() ? MI_K_ENC_VALIDITY : c.IsNull() ? kEncNodeNull : c.enc_kind, c.param, c.large_offsets, c.count, c.payload_bytes};
    staged[ci] = StagingNode{c.count, c.width, c.heap_used, c.IsUnion(), static_cast<int32_t>(c.children.size())};
    n_unions += c.IsUnion();
  }
  BodyLayout layout;
  LayOutBody(nodes, &layout);
  StagingLayout staging;
  LayOutStaging(staged, &staging);
  const std::vector<StagingLayout::Node>& in_off = staging.nodes;
  const size_t body_bytes = static_cast<size_t>(layout.body_size);
  Fit(d_in, staging.total + 256);
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
  l->buffer = std::make_unique<ChunkCollection>(PinnedStaging(w->ctx), w->fields);
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
