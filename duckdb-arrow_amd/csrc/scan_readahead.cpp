// scan_readahead.cpp -- see scan_readahead.hpp.
#include "scan_readahead.hpp"

#include <algorithm>
#include <cstdlib>

namespace miarrow {

int HardwareQueues() {
  const char* v = std::getenv("GPU_MAX_HW_QUEUES");
  return v != nullptr ? std::atoi(v) : 0;
}
bool DeferLz4(const mi_scan_options& o) { return o.host_decompress < 0 || (o.host_decompress == 0 && o.device_resident != 0); }
// ZSTD bodies in HBM pay only with many record batches side by side, and those need hardware queues of their own
// (where LZ4 bodies go there: when asked for, host_decompress = -1, or with the queues)
bool DeferZstd(const mi_scan_options& o) { return DeferLz4(o) && (o.host_decompress != 0 || HardwareQueues() >= 12); }

ReadAhead::ReadAhead(std::vector<std::string> paths, std::vector<ArrowIPCBuffer> buffers_p, const mi_scan_options& o, int max_in_flight, Hooks h)
    : opts(o), hooks(std::move(h)), buffers(std::move(buffers_p)), is_buffers(paths.empty()), sources(std::max<size_t>(paths.size(), 1)) {
  for (size_t i = 0; i < paths.size(); i++) sources[i].path = std::move(paths[i]);
  staging.resize(static_cast<size_t>(max_in_flight + 2 * kMaxProducers + 2));   // the deepest pipeline's slots + queues + the bodies being read + a decompressed copy (buffers are allocated on first use)
}

ReadAhead::~ReadAhead() {
  Stop();
  // what may hold a staging lease goes before the staging buffers and the lock its release takes (the members, after this body)
  fetched.clear();
  extra_readers.clear();
  for (auto& s : sources) s.reader.reset();
}

void ReadAhead::ConfigureReader(IPCStreamReader* reader) {
  reader->SetDeferLz4(DeferLz4(opts));
  reader->SetDeferZstd(DeferZstd(opts));
  reader->GetBaseSchema();
}

void ReadAhead::Open(size_t i) {
  Source& s = sources[i];
  if (s.opened) return;
  if (is_buffers) s.reader = std::make_unique<IPCBufferStreamReader>(buffers);
  else s.reader = std::make_unique<IPCFileStreamReader>(s.path);
  ConfigureReader(s.reader.get());
  s.opened = true;
}

const ArrowSchemaModel& ReadAhead::Schema(size_t i) {
  Open(i);
  return sources[i].reader->GetBaseSchema();
}

// reader projection of a file, settled by the scan (Hooks::project) on producer 0
void ReadAhead::Prepare(size_t si) {
  Open(si);
  Source& src = sources[si];
  if (src.prepared) return;
  std::vector<std::string> wanted = hooks.project(si, src.reader->GetBaseSchema());
  if (!wanted.empty()) src.reader->SetColumnProjection(wanted);
  {
    std::lock_guard<std::mutex> lk(mu);   // the other producers wait for this before they open their own reader of the file
    src.wanted = std::move(wanted);
    src.prepared = true;
  }
  cv.notify_all();
}

// A pinned staging buffer for one record-batch body; the returned handle gives it back when the batch is released.
std::shared_ptr<void> ReadAhead::LeaseStaging(size_t bytes, uint8_t** ptr) {
  Staging* st = nullptr;
  {
    std::unique_lock<std::mutex> lk(mu);
    const int64_t t0 = trace ? TraceNow() : 0;
    cv.wait(lk, [&] {
      if (stop) return true;
      for (auto& x : staging)
        if (!x.leased) return true;
      return false;
    });
    if (trace) tr_lease_wait_ns += TraceNow() - t0;
    if (stop) throw IOException("scan closed while reading");
    // prefer a free buffer that is already large enough
    for (auto& x : staging)
      if (!x.leased && x.size >= bytes + 64) { st = &x; break; }
    if (!st)
      for (auto& x : staging)
        if (!x.leased) { st = &x; break; }
    st->leased = true;
  }
  if (bytes + 64 > st->size) {
    const size_t grown = GrownCapacity(bytes + 64, st->size, 1 << 16);
    uint8_t* at = nullptr;
    std::shared_ptr<void> buf = hooks.alloc(grown, &at);
    std::swap(st->buf, buf);
    st->size = grown;
    if (buf) {
      std::lock_guard<std::mutex> lk(mu);
      outgrown.push_back(std::move(buf));
    }
  }
  *ptr = static_cast<uint8_t*>(st->buf.get());
  return std::shared_ptr<void>(st->buf.get(), [this, st](void*) {
    {
      std::lock_guard<std::mutex> lk(mu);
      st->leased = false;
    }
    cv.notify_all();
  });
}

void ReadAhead::ProducerLoop(int p) {
  size_t cap = n_producers > 1 ? 2 : static_cast<size_t>(kReadAhead);
  if (const char* v = std::getenv("MI_SCAN_READAHEAD")) cap = static_cast<size_t>(std::max(1, std::min(4, std::atoi(v))));   // fetched batches a producer holds (A/B)
  auto push = [&](Fetched&& f) {
    std::unique_lock<std::mutex> lk(mu);
    const int64_t t0 = trace ? TraceNow() : 0;
    cv.wait(lk, [&] { return stop || fetched[static_cast<size_t>(p)].size() < cap; });
    if (trace) tr_push_wait_ns += TraceNow() - t0;
    if (stop) return false;
    fetched[static_cast<size_t>(p)].push_back(std::move(f));
    lk.unlock();
    cv.notify_all();
    return true;
  };
  try {
    hooks.thread_start();   // the GPU's NUMA node: this thread's preads (and the I/O pool's, for it) and its pinned staging buffers
    size_t si = 0;
    int64_t ordinal = 0, share = 0;   // record batches of the file list; of those, this scan's (rank / world)
    while (si < sources.size()) {
      {
        std::lock_guard<std::mutex> lk(mu);
        if (stop) return;
      }
      IPCStreamReader* reader = nullptr;
      if (p == 0) {
        Prepare(si);
        reader = sources[si].reader.get();
      } else {
        // a reader of its own over the same file, with the projection producer 0 settled on
        auto& mine = extra_readers[static_cast<size_t>(p - 1)];
        if (mine.size() <= si) mine.resize(sources.size());
        if (!mine[si]) {
          std::vector<std::string> wanted;
          {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return stop || producer_error || sources[si].prepared; });
            if (stop) return;
            // producer 0 could not prepare the file: same error here.  A file it did prepare is still read: the error belongs
            // to a later one, and this producer's batches in front of it are due first
            if (!sources[si].prepared) std::rethrow_exception(producer_error);
            wanted = sources[si].wanted;
          }
          mine[si] = std::make_unique<IPCFileStreamReader>(sources[si].path);
          ConfigureReader(mine[si].get());
          if (!wanted.empty()) mine[si]->SetColumnProjection(wanted);
        }
        reader = mine[si].get();
      }
      reader->SetBodyAllocator([this](size_t bytes, MessageType type, uint8_t** ptr) -> std::shared_ptr<void> {
        if (type == MessageType::DICTIONARY_BATCH) return hooks.alloc(bytes + 64, ptr);  // lives as long as the dictionary version that points into it
        return LeaseStaging(bytes, ptr);
      });
      Fetched f;
      const bool in_share = opts.world <= 1 || (ordinal % opts.world) == opts.rank;
      const bool mine = in_share && (share % n_producers) == p;
      const int64_t t_read = trace ? TraceNow() : 0;
      const bool got = reader->GetNextBatch(&f.batch, opts.accept_dictionaries != 0, /*skip_body*/ !mine);
      if (trace) tr_read_ns += TraceNow() - t_read;
      reader->ReleaseCurrentBody();  // the lease belongs to the batch alone
      if (!got) {
        si++;
        continue;
      }
      f.source = static_cast<int32_t>(si);
      if (!f.batch.is_dictionary) {
        f.ordinal = ordinal++;
        if (in_share) share++;
        if (!mine) continue;
      }
      if (!push(std::move(f))) return;
    }
    Fetched end;
    end.end = true;
    push(std::move(end));
  } catch (...) {
    Fetched err;
    err.error = std::current_exception();
    {
      std::lock_guard<std::mutex> lk(mu);   // producers waiting for this one (a file it was to prepare) fail with it
      if (!producer_error) producer_error = err.error;
    }
    cv.notify_all();
    push(std::move(err));
  }
}

void ReadAhead::Start(bool trace_p) {
  if (started) return;
  started = true;
  trace = trace_p;
  // several producers only where record batches are independent of what came before them in the stream (no dictionary
  // batches, which every later batch of the file depends on) and where there is a pread to overlap (files, not caller buffers)
  // How many: ONE when the bodies only have to be read (plain bodies, and compressed ones that are expanded in HBM) -- its preads
  // already run on the whole I/O pool, and with a CPU quota of 16 more threads only throttle one another (SF10 host consumer:
  // 0.18 s with one producer, 0.20 with three) -- THREE when the reader's host threads decompress them (a producer then spends
  // most of its time waiting for its own body's decompression: LZ4 0.29 against 0.60 s, ZSTD 0.61 against 1.27 s).  Which it
  // is shows in the first record batch's header.
  n_producers = 1;
  if (!is_buffers && !opts.accept_dictionaries) {
    int wanted = 1;
    try {
      IPCFileStreamReader peek(sources[0].path);
      peek.GetBaseSchema();
      DecodedBatch first;
      if (peek.GetNextBatch(&first, /*accept_dictionaries*/ false, /*skip_body*/ true) && first.compression >= 0) {
        const bool in_hbm = first.compression == 1 ? DeferZstd(opts) : DeferLz4(opts);
        if (!in_hbm) wanted = 3;
      }
    } catch (...) {   // whatever is wrong with the file, the scan itself will say
    }
    const char* v = std::getenv("MI_SCAN_PRODUCERS");
    n_producers = std::max(1, std::min(kMaxProducers, v ? std::atoi(v) : wanted));
  }
  fetched.assign(static_cast<size_t>(n_producers), {});
  extra_readers.resize(static_cast<size_t>(n_producers - 1));
  next_fetch = 0;
  for (int p = 0; p < n_producers; p++) producers.emplace_back([this, p] { ProducerLoop(p); });
}

void ReadAhead::Stop() {
  if (!started) return;
  {
    std::lock_guard<std::mutex> lk(mu);
    stop = true;
  }
  cv.notify_all();
  for (auto& t : producers)
    if (t.joinable()) t.join();
}

bool ReadAhead::Take(Fetched* out, bool may_block) {
  {
    // in order: batch j of this scan's share comes from producer j mod P (a dictionary batch -- single producer only --
    // does not count)
    std::unique_lock<std::mutex> lk(mu);
    auto& q = fetched[static_cast<size_t>(next_fetch % n_producers)];
    if (q.empty()) {
      if (!may_block) return false;
      cv.wait(lk, [&] { return !q.empty(); });
    }
    *out = std::move(q.front());
    q.pop_front();
    if (!out->error && !out->end) {
      cur_source = static_cast<size_t>(out->source);
      if (!out->batch.is_dictionary) next_fetch++;
    }
  }
  cv.notify_all();
  return true;
}

void ReadAhead::WaitReady(std::chrono::microseconds patience) {
  std::unique_lock<std::mutex> lk(mu);
  auto& ready = fetched[static_cast<size_t>(next_fetch % n_producers)];
  cv.wait_for(lk, patience, [&] { return !ready.empty(); });
}

double ReadAhead::Progress() {
  if (sources.empty()) return 100;
  double done = static_cast<double>(std::min(cur_source, sources.size()));
  if (cur_source < sources.size() && sources[cur_source].reader) done += sources[cur_source].reader->GetProgress() / 100.0;
  return std::min(100.0, 100.0 * done / static_cast<double>(sources.size()));
}

}  // namespace miarrow
