// scan_readahead.hpp -- the read-ahead of a scan: producer threads walk the sources (open, reader projection, sharding,
// pread into pinned staging buffers) a few record batches ahead of the consumer, so file I/O overlaps whatever the
// consumer does between two Next() calls; the reference reads synchronously inside the scan call
// (ipc_file_stream_reader.cpp:71-94).  Host code only: the two things it needs of the GPU -- pinned memory and the
// device's context / NUMA node on its threads -- come in as hooks, so the unit builds and runs without one.
#pragma once

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "ipc_stream_reader.hpp"

namespace miarrow {

// LZ4_FRAME bodies stay compressed until they are in HBM (K8) when the consumer is on the device too.  A host consumer can
// ask for it (host_decompress = -1: the string payloads come back beside the vectors, Slot::h_mirror), but by default its
// bodies are decompressed by the reader's host threads: on this platform D2H copies run as copy kernels, which then
// queue up with the K8 kernels instead of overlapping them (SF10: 0.85 s against 0.68 s, tools/lz4_bench.py)
bool DeferLz4(const mi_scan_options& o);
// ZSTD likewise, when the process has hardware queues for many record batches side by side (its entropy stage is one serial
// chain per 128 KiB block: with the runtime's default of 4 queues the reader's host threads are faster)
bool DeferZstd(const mi_scan_options& o);
//! GPU_MAX_HW_QUEUES as the process was started with, 0 when it is not set: the GPU runtime reads it once, at its first
//! call (default 4; the library asks for 24 when it is loaded, c_api.cpp)
int HardwareQueues();

inline int64_t TraceNow() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Fetched {
  DecodedBatch batch;
  int32_t source = 0;
  int64_t ordinal = 0;
  bool end = false;                 // every source is exhausted
  std::exception_ptr error;         // raised where the consumer reaches it, after the batches read before it
};

class ReadAhead {
 public:
  struct Hooks {
    //! `bytes` of pinned memory at *ptr, freed when the last reference goes (the reader's SetBodyAllocator, without the
    //! message type); called on the producer threads
    std::function<std::shared_ptr<void>(size_t bytes, uint8_t** ptr)> alloc;
    //! first thing on every producer thread: device context, NUMA binding
    std::function<void()> thread_start;
    //! The columns to read of file `source`, given its schema (empty: all).  Runs on producer 0 when it first opens the
    //! file, before any other producer opens it; what it throws reaches the consumer in stream order and fails the
    //! other producers.
    std::function<std::vector<std::string>(size_t source, const ArrowSchemaModel& schema)> project;
  };
  //! Files (`paths`) or, without any, one source over caller memory (`buffers`).  max_in_flight: record batches the
  //! consumer holds on to at most (each keeps its staging buffer until it is released).
  ReadAhead(std::vector<std::string> paths, std::vector<ArrowIPCBuffer> buffers, const mi_scan_options& opts, int max_in_flight, Hooks hooks);
  //! Stop() + the queues and readers; the caller has released every batch it took (their leases point into this object)
  ~ReadAhead();

  size_t NumSources() const { return sources.size(); }
  const std::string& Path(size_t source) const { return sources[source].path; }   // empty for buffers
  //! opens the source on first use
  const ArrowSchemaModel& Schema(size_t source);
  bool Started() const { return started; }
  void Start(bool trace);
  //! The next message of this scan's share (rank / world) in stream order: a record batch, a dictionary batch in front
  //! of the batches that use it, the end, or a producer's failure.  false: nothing fetched yet and `may_block` is false.
  bool Take(Fetched* out, bool may_block);
  //! waits up to `patience` for Take(.., false) to have something
  void WaitReady(std::chrono::microseconds patience);
  //! ends the producer threads (those blocked on a full queue or for a staging buffer included); idempotent
  void Stop();
  double Progress();

  // MI_SCAN_TRACE: where the producers' time went (summed over them)
  int Producers() const { return n_producers; }
  double ReadSeconds() const { return tr_read_ns.load() * 1e-9; }
  double PushWaitSeconds() const { return tr_push_wait_ns.load() * 1e-9; }
  double LeaseWaitSeconds() const { return tr_lease_wait_ns.load() * 1e-9; }

  static constexpr int kReadAhead = 3;              // fetched batches waiting for a slot (per producer: 2 when there are several)
  static constexpr int kMaxProducers = 4;

 private:
  struct Source {
    std::string path;
    std::unique_ptr<IPCStreamReader> reader;   // producer 0's
    bool opened = false, prepared = false;
    std::vector<std::string> wanted;           // the reader projection Prepare settled on (the extra producers' readers take it too)
  };
  struct Staging {                    // pinned body buffers, leased to one record batch at a time
    std::shared_ptr<void> buf;
    size_t size = 0;
    bool leased = false;
  };
  void Open(size_t source);
  void Prepare(size_t source);
  void ConfigureReader(IPCStreamReader* reader);
  void ProducerLoop(int p);
  std::shared_ptr<void> LeaseStaging(size_t bytes, uint8_t** ptr);

  const mi_scan_options opts;
  const Hooks hooks;
  const std::vector<ArrowIPCBuffer> buffers;
  const bool is_buffers;
  // Everything below is shared between the consumer and the producers and guarded by `mu` -- except a source's reader,
  // which belongs to producer 0 once the threads run (the consumer only asks it for its progress).
  std::mutex mu;
  std::condition_variable cv;
  std::vector<Source> sources;
  std::vector<Staging> staging;                     // in flight on the GPU + waiting + the one being read
  // Staging buffers a body has outgrown.  Freeing pinned memory waits for the device to go idle -- with record batches in
  // flight that is a pipeline stall of milliseconds -- so they are kept until the scan closes (growth is geometric: at
  // most twice the final sizes in all).
  std::vector<std::shared_ptr<void>> outgrown;
  //! Several read-ahead threads for file scans without dictionaries: producer p reads the record batches j of this scan's
  //! share with j mod P == p (every producer walks every header, bodies that are not its own are stepped over unread -- the
  //! rank / world rule once more, inside the process), so the pread of one body overlaps the header walk, staging lease and
  //! pread of the next ones.  The consumer takes them back in order: batch j from queue j mod P.
  int n_producers = 1;
  std::vector<std::thread> producers;
  std::vector<std::deque<Fetched>> fetched;         // one queue per producer
  int64_t next_fetch = 0;                           // j of the batch the consumer takes next
  size_t cur_source = 0;                            // source of the message the consumer took last
  std::exception_ptr producer_error;                // the first failure of any producer
  std::vector<std::vector<std::unique_ptr<IPCStreamReader>>> extra_readers;   // [producer - 1][source]
  bool started = false, stop = false, trace = false;
  std::atomic<int64_t> tr_read_ns{0}, tr_push_wait_ns{0}, tr_lease_wait_ns{0};
};

}  // namespace miarrow
