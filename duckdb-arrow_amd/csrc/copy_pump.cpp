// copy_pump.cpp -- mi_writer_sink_scan: COPY (FROM read_arrow(...)) TO 'file', the pump DuckDB's executor is between a scan
// and a copy sink, with the batch copy's re-partitioning (PhysicalBatchCopyToFile hands prepare_batch collections of
// desired_batch_size = row_group_size rows, write_arrow_stream.cpp:225-245).  Two pumps pull whole record batches from the
// scan; both cut them into row groups with RowGroupCutter and keep them with BatchLedger (writer_plan.hpp), so both write
// the same file -- the file of the one-thread sink where writer_plan.hpp says so.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "scan_operator.hpp"
#include "writer_internal.hpp"
#include "extension_format.hpp"
#include "writer_plan.hpp"

namespace miarrow {

int WrapC(const std::function<void()>& f);  // c_api.cpp
ArrowScan* SingleScanOf(mi_scan* s);        // scan_operator.cpp

namespace {

int SinkThreads() {
  const char* v = std::getenv("MI_WRITER_THREADS");
  if (v) return std::max(1, std::min(16, std::atoi(v)));
  const int hw = static_cast<int>(std::thread::hardware_concurrency());
  return std::max(1, std::min(6, hw / 3));
}

//! What the pump thread of either pump shares with its other threads (under `mu`), and its own view of the stream
struct PumpBase {
  PumpBase(mi_writer* w_p, ArrowScan* scan_p, int64_t rows_per_group)
      : w(w_p), scan(scan_p), ledger(mu, cv, error, [scan_p](const BatchRef& ref) { scan_p->ReleaseBatch(ref); }), cutter(rows_per_group) {}
  void Fail(std::exception_ptr e) {
    std::lock_guard<std::mutex> lk(mu);
    if (!error) error = e;
    cv.notify_all();
  }
  mi_writer* const w;
  ArrowScan* const scan;
  std::mutex mu;
  std::condition_variable cv;
  std::exception_ptr error;        // the first failure of any thread
  BatchLedger<BatchRef> ledger;
  // pump thread only
  RowGroupCutter cutter;
  int64_t rows = 0;
};

// ---- the sink-thread pump: each row group goes to one of T sink threads which appends its chunks, encodes it and writes
// it -- claims of the file range happen in row-group order.
class ParallelPump : PumpBase {
 public:
  ParallelPump(mi_writer* w_p, ArrowScan* scan_p, int threads_p, int64_t rows_per_group) : PumpBase(w_p, scan_p, rows_per_group), threads(threads_p) {}
  int64_t Run(const BatchRef& first);

 private:
  struct Piece { int batch; int32_t w0, w1; };        // windows [w0, w1) of held batch `batch`
  // `spilled`: rows of this row group the pump has already staged itself (see SpillCurrent); the worker that takes the
  // job appends the remaining pieces to it and flushes it instead of its own state
  struct Job { std::vector<Piece> pieces; int64_t seq = 0; std::unique_ptr<mi_writer_local> spilled; };
  void WorkerLoop();
  void AppendPieces(mi_writer_local* sink, const std::vector<Piece>& pieces, ChunkStorage* storage, mi_data_chunk* chunk);
  void Pump(const BatchRef& first);
  void Dispatch();
  void MakeRoom();
  void SpillCurrent();

  const int threads;
  std::deque<Job> jobs;
  int64_t next_claim = 0;             // sequence number of the row group that may claim its file range next
  bool done = false;
  // pump thread only
  Job cur;                            // the row group being cut
  int64_t seq = 0;
  ChunkStorage spill_storage;
  mi_data_chunk spill_chunk;
};

void ParallelPump::AppendPieces(mi_writer_local* sink, const std::vector<Piece>& pieces, ChunkStorage* storage, mi_data_chunk* chunk) {
  for (const Piece& pc : pieces) {
    const BatchRef ref = ledger.RefOf(pc.batch);
    for (int32_t wi = pc.w0; wi < pc.w1; wi++) {
      scan->BuildChunk(ref, wi, storage, chunk);
      TimedAppend(*sink->buffer, *chunk);
    }
    ledger.ClosePiece(pc.batch);
  }
}

void ParallelPump::WorkerLoop() {
  try {
    auto local = MakeLocal(w);
    ChunkStorage storage;
    mi_data_chunk chunk;
    while (true) {
      Job job;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return error || done || !jobs.empty(); });
        if (error || jobs.empty()) return;
        job = std::move(jobs.front());
        jobs.pop_front();
      }
      mi_writer_local* sink = job.spilled ? job.spilled.get() : local.get();
      AppendPieces(sink, job.pieces, &storage, &chunk);
      sink->FlushRowGroup(
          [&] {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return error || next_claim == job.seq; });
          },
          [&] {
            std::lock_guard<std::mutex> lk(mu);
            next_claim = job.seq + 1;
            cv.notify_all();
          });
    }
  } catch (...) {
    Fail(std::current_exception());
  }
}

void ParallelPump::Dispatch() {
  if (cur.pieces.empty() && !cur.spilled) return;
  cur.seq = seq++;
  {
    std::lock_guard<std::mutex> lk(mu);
    jobs.push_back(std::move(cur));
  }
  cv.notify_all();
  cur = Job();
}

// A row group that spans more record batches than the scan has slots: every slot is held by a piece of the row group
// still being cut, which no sink thread will see before it is full.  The pump then stages those rows itself (a sink
// state of its own that travels with the job), which closes their pieces; the worker that gets the job appends the rest.
void ParallelPump::SpillCurrent() {
  if (!cur.spilled) cur.spilled = MakeLocal(w);
  AppendPieces(cur.spilled.get(), cur.pieces, &spill_storage, &spill_chunk);
  cur.pieces.clear();
}

// Every slot of the scan is held.  Batches whose pieces all went to sink threads come back by themselves; the ones that
// only the undispatched row group refers to never would.
void ParallelPump::MakeRoom() {
  std::vector<int> cur_toks;
  for (const Piece& pc : cur.pieces)
    if (std::find(cur_toks.begin(), cur_toks.end(), pc.batch) == cur_toks.end()) cur_toks.push_back(pc.batch);
  if (ledger.Unreleased() - static_cast<int64_t>(cur_toks.size()) > 0) ledger.ReleaseReady(true);
  else if (!cur.pieces.empty()) SpillCurrent();
  else throw InternalException("COPY pump: no record batch can be acquired and none is held");
}

void ParallelPump::Pump(const BatchRef& first) {
  bool have_first = true;
  while (true) {
    ledger.ReleaseReady(false);
    BatchRef ref;
    if (have_first) {
      ref = first;
      have_first = false;
    } else if (!scan->AcquireBatch(&ref)) {
      if (scan->Exhausted()) break;
      MakeRoom();
      continue;
    }
    scan->EnsureHostVectors(ref);
    rows += ref.chunk_rows;
    const int tok = ledger.Hold(ref);
    for (const CutPiece& pc : cutter.Cut(ref.chunk_rows)) {
      ledger.OpenPiece(tok);
      cur.pieces.push_back(Piece{tok, pc.window0, pc.window1});
      if (pc.closes_group) Dispatch();
    }
    ledger.MarkFullyCut(tok);
  }
  Dispatch();   // the tail row group (ArrowWriteCombine)
}

int64_t ParallelPump::Run(const BatchRef& first) {
  std::vector<std::thread> workers;
  for (int t = 0; t < threads; t++) workers.emplace_back([this] { WorkerLoop(); });
  try {
    Pump(first);
  } catch (...) {
    Fail(std::current_exception());
  }
  {
    std::lock_guard<std::mutex> lk(mu);
    done = true;
  }
  cv.notify_all();
  for (auto& t : workers) t.join();
  if (Timers().on)
    std::fprintf(stderr, "[mi_writer] pump with %d sink threads (thread-seconds): append %.3f, serialize (H2D + K7 + D2H) %.3f, write %.3f\n", threads,
                 Timers().append, Timers().serialize, Timers().write);
  ledger.ReleaseAll();   // give every batch back before reporting
  if (error) std::rethrow_exception(error);
  return rows;
}

// ---- the fused pump: decode and encode both run on the GPU, so the decoded vectors never have to leave HBM.  For every row
// group that lies inside one record batch of the scan the K7 kernels read the scan slot's vectors where the K1-K4 kernels
// wrote them (string payloads: the HBM copy of the Arrow data buffer the string_t rows point into) and write the IPC body;
// only that body travels back (one D2H) and is written by an I/O thread.  Per row this takes the host out of the loop
// except for pread -> H2D and D2H -> pwrite: no D2H of the vectors, no staging copy, no H2D of the staged rows (DESIGN.md
// section 10 has the byte counts).  Rows of a row group that straddles two record batches take the host path
// (EnsureHostVectors + ChunkCollection) on the pump thread, so the file is that of the sink-thread pump in every case.
struct FusedEncoder {
  DeviceBuffer d_body;
  PinnedBuffer h_body;
  PinnedBuffer h_nulls;     // int64_t: copy of the plan's NULL counters
  PinnedBuffer h_status;    // uint32_t
  std::unique_ptr<Plan> plan;
  HipEvent encoded, done;
  bool busy = false;
  // the row group in flight
  int64_t nrows = 0;
  BodyLayout layout;
  BodyCompressor compressor;                 // COMPRESSION lz4: d_body -> the body that goes to the file
  std::vector<mi_buffer_span> file_spans;    // of the body that goes to the file
  int64_t file_body_size = 0;
};

bool FusedSinkPossible(mi_writer* w, ArrowScan* scan) {
  if (std::getenv("MI_WRITER_NO_FUSED")) return false;
  if (scan->HasFilter() || w->buffer->Count() != 0) return false;
  const auto& cols = scan->OutputColumns();
  if (cols.size() != w->buffer->roots.size() || w->buffer->columns.size() != cols.size()) return false;   // flat schema only
  for (size_t c = 0; c < cols.size(); c++) {
    if (cols[c].is_constant()) return false;
    const auto& wc = w->buffer->columns[static_cast<size_t>(w->buffer->roots[c])];
    if (!wc.children.empty()) return false;
    if (wc.enc_kind != MI_K_ENC_COPY && wc.enc_kind != MI_K_ENC_DEC128 && wc.enc_kind != MI_K_ENC_BOOL && wc.enc_kind != MI_K_ENC_STR32 &&
        wc.enc_kind != MI_K_ENC_STRVIEW && wc.enc_kind != MI_K_ENC_UUID_TEXT)
      return false;
  }
  return true;
}

class FusedPump : PumpBase {
 public:
  FusedPump(mi_writer* w_p, ArrowScan* scan_p, int64_t rows_per_group);
  //! whatever ends the pump, the GPU is done with the encoders' buffers before they go
  ~FusedPump() {
    (void)hipStreamSynchronize(enc_stream);
    (void)hipStreamSynchronize(back_stream);
  }
  int64_t Run(const BatchRef& first);

 private:
  static constexpr int kEncoders = 4;   // row groups between the kernels and the file at most
  struct WriteJob {
    int enc = -1;                        // fused encoder; -1: `header` / `body` are ready (host-serialized row group)
    int tok = -1;                        // batch token whose piece closes once the GPU has read it
    std::vector<uint8_t> header;
    const uint8_t* body = nullptr;
    size_t body_size = 0;
  };
  const ChunkCollection::Column& WriterColumn(size_t c) const { return w->buffer->columns[static_cast<size_t>(w->buffer->roots[c])]; }
  void IoLoop();
  void FinishEncoded(WriteJob* job);
  void QueueJob(WriteJob&& job);
  bool ViewsOf(const BatchRef& ref, std::vector<DeviceColumnView>* views);
  int ClaimEncoder();
  void EncodeOnGpu(int tok, const std::vector<DeviceColumnView>& views, int64_t r0, int64_t m);
  void FlushHost();
  void Pump(const BatchRef& first);

  const size_t n_cols;
  const bool compressed;                    // COMPRESSION lz4
  std::unique_ptr<mi_writer_local> local;   // host path of row groups that straddle record batches
  HipStream enc_stream, back_stream;
  std::vector<FusedEncoder> enc;
  std::deque<WriteJob> jobs;
  bool stop = false;
  int64_t jobs_written = 0, jobs_queued = 0;
  // pump thread only
  ChunkStorage storage;
  mi_data_chunk chunk;
};

FusedPump::FusedPump(mi_writer* w_p, ArrowScan* scan_p, int64_t rows_per_group)
    : PumpBase(w_p, scan_p, rows_per_group), n_cols(scan_p->NumOutputColumns()),
      compressed(w_p->opts.compression == MI_WRITE_COMPRESSION_LZ4_FRAME) {
  w->ctx->Bind();
  local = MakeLocal(w);
  enc_stream = HipStream::Create();
  back_stream = HipStream::Create();
  enc = std::vector<FusedEncoder>(kEncoders);
  for (auto& e : enc) {
    e.plan = std::make_unique<Plan>(w->ctx);
    e.encoded = HipEvent::Create();
    e.done = HipEvent::Create();
    e.h_status = PinnedBuffer(64);
  }
}

// the GPU is done with the scan slot and the body is in pinned memory: header from the NULL counts that came with it
void FusedPump::FinishEncoded(WriteJob* job) {
  FusedEncoder& e = enc[static_cast<size_t>(job->enc)];
  MI_HIP_CHECK(hipEventSynchronize(e.done));
  ledger.ClosePiece(job->tok);
  ThrowForStatus(e.h_status.get<uint32_t>()[0]);
  const std::vector<int64_t> nulls = e.plan->MapNullCounts(e.h_nulls.get<int64_t>());
  std::vector<std::pair<int64_t, int64_t>> nodes;
  for (size_t c = 0; c < n_cols; c++) nodes.emplace_back(e.nrows, nulls[c]);
  int64_t n_view_fields = 0;
  for (size_t c = 0; c < n_cols; c++) n_view_fields += WriterColumn(c).enc_kind == MI_K_ENC_STRVIEW;
  job->header = EncodeRecordBatchMessage(e.nrows, nodes, e.file_spans, e.file_body_size, compressed ? 0 : -1, n_view_fields);
  job->body = e.h_body.get();
  job->body_size = static_cast<size_t>(e.file_body_size);
}

void FusedPump::IoLoop() {
  try {
    w->ctx->Bind();
    while (true) {
      WriteJob job;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return stop || error || !jobs.empty(); });
        if (error || jobs.empty()) return;
        job = std::move(jobs.front());
        jobs.pop_front();
      }
      if (job.enc >= 0) FinishEncoded(&job);
      w->writer->WriteMessage(job.header.data(), job.header.size(), job.body, job.body_size);
      {
        std::lock_guard<std::mutex> lk(mu);
        if (job.enc >= 0) enc[static_cast<size_t>(job.enc)].busy = false;
        ++jobs_written;
      }
      cv.notify_all();
    }
  } catch (...) {
    Fail(std::current_exception());
  }
}

void FusedPump::QueueJob(WriteJob&& job) {
  {
    std::lock_guard<std::mutex> lk(mu);
    jobs.push_back(std::move(job));
    ++jobs_queued;
  }
  cv.notify_all();
}

// valid string bytes of rows [r0, r0 + m): the size of the Arrow data buffer the encoder will fill
int64_t PayloadOf(const DeviceColumnView& v, int64_t r0, int64_t m) {
  auto off = [&](int64_t i) -> int64_t {
    if (v.offset_width == 8) { int64_t x; std::memcpy(&x, v.h_offsets + i * 8, 8); return x; }
    int32_t x; std::memcpy(&x, v.h_offsets + i * 4, 4); return x;
  };
  if (v.null_count == 0 || !v.h_validity) return off(r0 + m) - off(r0);
  int64_t total = 0;
  for (int64_t i = r0; i < r0 + m; i++)
    if ((v.h_validity[i >> 3] >> (i & 7)) & 1) total += off(i + 1) - off(i);
  return total;
}

// text bytes of a UUID column's rows [r0, r0 + m): 36 per valid row
int64_t UuidTextPayloadOf(const DeviceColumnView& v, int64_t r0, int64_t m) {
  int64_t valid = m;
  if (v.null_count != 0 && v.h_validity)
    for (int64_t i = r0; i < r0 + m; i++) valid -= ((v.h_validity[i >> 3] >> (i & 7)) & 1) ? 0 : 1;
  return valid * extfmt::kUuidTextBytes;
}

// row groups the fused pump has encoded where they lay in HBM, and string-view columns among them (mi_writer_fused_counts)
std::atomic<int64_t> g_fused_row_groups{0}, g_fused_view_columns{0};

// bytes of the valid strings of more than 12 bytes among rows [r0, r0 + m): the size of a view column's data buffer.  Always a
// pass over the offsets (timed: MI_WRITER_TIMING reports it as "view sizing").
int64_t LongPayloadOf(const DeviceColumnView& v, int64_t r0, int64_t m) {
  const auto t0 = std::chrono::steady_clock::now();
  const bool nulls = v.null_count != 0 && v.h_validity;
  int64_t total = 0;
  auto sum = [&](auto zero) {
    using T = decltype(zero);
    T prev;
    std::memcpy(&prev, v.h_offsets + r0 * static_cast<int64_t>(sizeof(T)), sizeof(T));
    for (int64_t i = r0; i < r0 + m; i++) {
      T next;
      std::memcpy(&next, v.h_offsets + (i + 1) * static_cast<int64_t>(sizeof(T)), sizeof(T));
      const int64_t len = static_cast<int64_t>(next) - static_cast<int64_t>(prev);
      prev = next;
      if (len > 12 && (!nulls || ((v.h_validity[i >> 3] >> (i & 7)) & 1))) total += len;
    }
  };
  if (v.offset_width == 8) sum(int64_t{0});
  else sum(int32_t{0});
  if (Timers().on) {
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::lock_guard<std::mutex> lk(Timers().mu);
    Timers().view_sizing += dt;
  }
  return total;
}

// can rows of this batch be encoded where they lie?
bool FusedPump::ViewsOf(const BatchRef& ref, std::vector<DeviceColumnView>* views) {
  views->resize(n_cols);
  for (size_t c = 0; c < n_cols; c++) {
    DeviceColumnView& v = (*views)[c];
    scan->DeviceColumn(ref, c, &v);
    if (!v.flat) return false;
    const auto& wc = WriterColumn(c);
    const bool is_string = v.kind == MI_K_STR32 || v.kind == MI_K_STR64;
    if (wc.enc_kind == MI_K_ENC_UUID_TEXT) {   // the decoded hugeint_t rows, NULLs by the Arrow bitmap on the host
      if (v.kind != MI_K_UUID || (v.null_count != 0 && !v.h_validity)) return false;
    } else if (wc.enc_kind == MI_K_ENC_STR32 || wc.enc_kind == MI_K_ENC_STRVIEW) {
      if (!is_string) return false;
    } else if (is_string || v.width != wc.width || v.kind == MI_K_STRVIEW || v.kind == MI_K_FIXED_BINARY) {
      return false;
    }
  }
  return true;
}

int FusedPump::ClaimEncoder() {
  int ei = -1;
  std::unique_lock<std::mutex> lk(mu);
  cv.wait(lk, [&] {
    if (error) return true;
    for (int i = 0; i < kEncoders; i++)
      if (!enc[static_cast<size_t>(i)].busy) { ei = i; return true; }
    return false;
  });
  if (error) std::rethrow_exception(error);
  enc[static_cast<size_t>(ei)].busy = true;
  return ei;
}

// rows [r0, r0 + m) of held batch `tok` (r0 a multiple of 2048) as one row group, read where the scan decoded them
void FusedPump::EncodeOnGpu(int tok, const std::vector<DeviceColumnView>& views, int64_t r0, int64_t m) {
  const int ei = ClaimEncoder();
  ledger.OpenPiece(tok);
  FusedEncoder& e = enc[static_cast<size_t>(ei)];
  e.nrows = m;
  std::vector<EncodeNode> nodes(n_cols);
  for (size_t c = 0; c < n_cols; c++) {
    const auto& wc = WriterColumn(c);
    const int64_t payload = wc.enc_kind == MI_K_ENC_STR32 ? PayloadOf(views[c], r0, m) : wc.enc_kind == MI_K_ENC_STRVIEW ? LongPayloadOf(views[c], r0, m)
                            : wc.enc_kind == MI_K_ENC_UUID_TEXT ? UuidTextPayloadOf(views[c], r0, m) : 0;
    nodes[c] = EncodeNode{wc.enc_kind, wc.param, wc.large_offsets, m, payload};
  }
  g_fused_row_groups++;
  for (size_t c = 0; c < n_cols; c++) g_fused_view_columns += nodes[c].kind == MI_K_ENC_STRVIEW;
  LayOutBody(nodes, &e.layout);
  const size_t body_bytes = static_cast<size_t>(e.layout.body_size);
  Fit(e.d_body, body_bytes + 256);
  MI_HIP_CHECK(hipMemsetAsync(e.d_body.get(), 0, body_bytes, enc_stream));
  std::vector<mi_col_task> tasks(n_cols);
  for (size_t c = 0; c < n_cols; c++) {
    const DeviceColumnView& v = views[c];
    const EncodeInput in{v.d_data + static_cast<size_t>(r0) * static_cast<size_t>(v.width),
                         v.d_validity ? v.d_validity + static_cast<size_t>(r0 / 64) * 8 : nullptr, v.d_heap, v.ptr_base};
    tasks[c] = EncodeTask(nodes[c], &e.layout.spans[static_cast<size_t>(e.layout.first_span[c])], in, e.d_body.get());
  }
  e.plan->Set(tasks.data(), static_cast<int32_t>(tasks.size()), enc_stream);
  e.plan->ResetCounters(enc_stream);
  e.plan->Launch(enc_stream);
  const uint8_t* d_final = e.d_body.get();
  e.file_spans = e.layout.spans;
  e.file_body_size = e.layout.body_size;
  if (compressed) {   // waits for the size words of this row group's blocks (and so for the kernels queued before them)
    e.compressor.Run(e.layout, e.d_body.get(), enc_stream);
    d_final = e.compressor.Body();
    e.file_spans = e.compressor.Layout().spans;
    e.file_body_size = e.compressor.Layout().body_size;
  }
  Fit(e.h_body, static_cast<size_t>(e.file_body_size) + 256);
  MI_HIP_CHECK(hipEventRecord(e.encoded, enc_stream));
  MI_HIP_CHECK(hipStreamWaitEvent(back_stream, e.encoded, 0));
  MI_HIP_CHECK(hipMemcpyAsync(e.h_body.get(), d_final, static_cast<size_t>(e.file_body_size), hipMemcpyDeviceToHost, back_stream));
  Fit(e.h_nulls, static_cast<size_t>(e.plan->n_null_counts + 1) * 8);
  if (e.plan->n_null_counts)
    MI_HIP_CHECK(hipMemcpyAsync(e.h_nulls.get(), e.plan->d_null_counts.get(), static_cast<size_t>(e.plan->n_null_counts) * 8, hipMemcpyDeviceToHost, back_stream));
  MI_HIP_CHECK(hipMemcpyAsync(e.h_status.get(), e.plan->d_status.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, back_stream));
  MI_HIP_CHECK(hipEventRecord(e.done, back_stream));
  WriteJob job;
  job.enc = ei;
  job.tok = tok;
  QueueJob(std::move(job));
}

// the host path: serialise the rows buffered in `local` and hand them to the I/O thread; its body buffer is reused by
// the next host-path row group, so wait until it is written (row groups that straddle batches are the exception)
void FusedPump::FlushHost() {
  const bool empty = local->serializer->Serialize(*local->buffer) == 0;
  local->buffer->Reset();
  if (!empty) {
    WriteJob job;
    job.header = local->serializer->GetHeader();
    job.body = local->serializer->GetBody();
    job.body_size = static_cast<size_t>(local->serializer->GetBodySize());
    QueueJob(std::move(job));
  }
  std::unique_lock<std::mutex> lk(mu);
  cv.wait(lk, [&] { return error || jobs_written == jobs_queued; });
  if (empty) w->writer->CountEmptyFlush();
  else if (error) std::rethrow_exception(error);
}

// A piece that starts a row group and closes it lies inside one record batch: it is encoded where it lies in HBM when the
// batch's columns allow it.  Every other piece takes the host path.
void FusedPump::Pump(const BatchRef& first) {
  bool have_first = true;
  std::vector<DeviceColumnView> views;
  while (true) {
    ledger.ReleaseReady(false);
    BatchRef ref;
    if (have_first) {
      ref = first;
      have_first = false;
    } else if (!scan->AcquireBatch(&ref)) {
      if (scan->Exhausted()) break;
      ledger.ReleaseReady(true);
      continue;
    }
    const int64_t n = ref.chunk_rows;
    rows += n;
    const int tok = ledger.Hold(ref);
    const bool on_gpu = n > 0 && ViewsOf(ref, &views);
    for (const CutPiece& pc : cutter.Cut(n)) {
      if (on_gpu && pc.starts_group && pc.closes_group) {
        const int64_t r0 = static_cast<int64_t>(pc.window0) * MI_VECTOR_SIZE;
        EncodeOnGpu(tok, views, r0, std::min<int64_t>(static_cast<int64_t>(pc.window1) * MI_VECTOR_SIZE, n) - r0);
        continue;
      }
      scan->EnsureHostVectors(ref);
      for (int32_t wi = pc.window0; wi < pc.window1; wi++) {
        scan->BuildChunk(ref, wi, &storage, &chunk);
        TimedAppend(*local->buffer, chunk);
      }
      if (pc.closes_group) FlushHost();
    }
    ledger.MarkFullyCut(tok);
  }
  if (cutter.OpenRows() > 0) FlushHost();   // the tail row group (ArrowWriteCombine)
}

int64_t FusedPump::Run(const BatchRef& first) {
  std::thread io([this] { IoLoop(); });
  try {
    Pump(first);
  } catch (...) {
    Fail(std::current_exception());
  }
  {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return error || jobs_written == jobs_queued; });
    stop = true;
  }
  cv.notify_all();
  io.join();
  (void)hipStreamSynchronize(enc_stream);   // the GPU is done with every scan slot before the batches go back
  (void)hipStreamSynchronize(back_stream);
  ledger.ReleaseAll();
  if (error) std::rethrow_exception(error);
  return rows;
}

// Which pump: record batches at least one row group long are encoded where they lie in HBM; smaller ones go through the
// sink threads.  Decided on the first batch (the scan keeps its vectors on the device until then).
void PumpScan(mi_writer* w, ArrowScan* scan, int threads, int64_t* rows) {
  const int64_t rows_per_group = RowsPerGroup(w->opts, StagedRowBytes(scan->OutputColumns()));
  const bool fused = FusedSinkPossible(w, scan);
  scan->EnsurePipelineDepth(std::max(1, threads) + 4);
  // whatever happens below, the scan hands out host vectors again afterwards
  struct Restore { ArrowScan* s; ~Restore() { s->KeepVectorsOnDevice(false); } } restore{scan};
  scan->KeepVectorsOnDevice(fused);
  BatchRef first;
  int64_t n = 0;
  if (scan->AcquireBatch(&first)) {
    if (fused && first.chunk_rows >= rows_per_group) {
      n = FusedPump(w, scan, rows_per_group).Run(first);
    } else {
      scan->KeepVectorsOnDevice(false);
      n = ParallelPump(w, scan, std::max(1, threads), rows_per_group).Run(first);
    }
  }
  if (rows) *rows = n;
}

}  // namespace
}  // namespace miarrow

using namespace miarrow;

extern "C" int mi_writer_sink_scan(mi_writer* w, mi_scan* scan, int64_t* rows) {
  if (!w || !w->writer || !scan) return WrapC([] { throw InvalidInputException("mi_writer_sink_scan: bad argument"); });
  ArrowScan* single = SingleScanOf(scan);
  const int threads = SinkThreads();
  if (single && single->HostConsumer() && w->buffer->Count() == 0 && !single->Initialized()) single->Init({});
  if (single && single->HostConsumer() && w->buffer->Count() == 0 && (threads > 1 || FusedSinkPossible(w, single)))
    return WrapC([&] { PumpScan(w, single, threads, rows); });
  int64_t n = 0;
  mi_data_chunk ch;
  while (true) {
    int rc = mi_scan_next(scan, &ch);
    if (rc != MI_OK) return rc;
    if (ch.size == 0) break;
    rc = mi_writer_sink(w, &ch);
    if (rc != MI_OK) return rc;
    n += ch.size;
  }
  if (rows) *rows = n;
  return MI_OK;
}

extern "C" int mi_writer_fused_counts(int64_t* row_groups, int64_t* view_columns) {
  if (!row_groups || !view_columns) return WrapC([] { throw InvalidInputException("mi_writer_fused_counts: NULL argument"); });
  *row_groups = g_fused_row_groups.load();
  *view_columns = g_fused_view_columns.load();
  return MI_OK;
}
