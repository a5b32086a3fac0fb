// readahead_check.cpp -- the scan's read-ahead (duckdb-arrow_amd/csrc/scan_readahead.cpp) without a GPU, under
// ThreadSanitizer (test infrastructure, never shipped).  Pinned memory is plain malloc behind the allocation hook.
//
//   g++ -std=c++17 -O1 -g -fsanitize=thread -I include tests/sanitize/readahead_check.cpp
//       duckdb-arrow_amd/csrc/{scan_readahead,ipc_format,io_pool,host_codec,frame_walk,batch_slice,ipc_stream_reader}.cpp -ldl -lpthread -o readahead_check
//   readahead_check [--dict] <stream file> ...
//
// Every file is read once on this thread with IPCFileStreamReader; then, for 1 to 4 producers (MI_SCAN_PRODUCERS) and for
// world 1 and ranks 0..2 of world 3, a ReadAhead over the same files must hand out exactly the messages of that share --
// record batches with ordinal % world == rank, and with --dict every dictionary batch in front of them -- in stream order,
// bodies byte-equal.  A file list with a missing file in the middle must fail after the batches before it, and Stop() must
// return while the producers are blocked (queue full; no free staging buffer).
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../duckdb-arrow_amd/csrc/scan_readahead.hpp"

using namespace miarrow;

namespace {
struct Message {
  bool is_dictionary = false;
  int32_t source = 0;
  int64_t ordinal = -1;   // record batches: position in the file list
  int64_t length = 0;
  std::vector<uint8_t> body;
};

int g_failed = 0;
#define CHECK(cond, ...)                    \
  do {                                      \
    if (!(cond)) {                          \
      std::fprintf(stderr, "FAILED: ");     \
      std::fprintf(stderr, __VA_ARGS__);    \
      std::fprintf(stderr, "\n");           \
      g_failed++;                           \
      return;                               \
    }                                       \
  } while (0)

std::atomic<int> g_threads_started{0};

ReadAhead::Hooks Hooks() {
  ReadAhead::Hooks h;
  h.alloc = [](size_t bytes, uint8_t** ptr) {
    std::shared_ptr<void> mem(std::malloc(bytes), std::free);
    *ptr = static_cast<uint8_t*>(mem.get());
    return mem;
  };
  h.thread_start = [] { g_threads_started++; };
  h.project = [](size_t, const ArrowSchemaModel&) { return std::vector<std::string>(); };   // every column
  return h;
}

std::vector<Message> ReadSingleThreaded(const std::vector<std::string>& paths, bool dict) {
  std::vector<Message> all;
  int64_t ordinal = 0;
  for (size_t si = 0; si < paths.size(); si++) {
    IPCFileStreamReader reader(paths[si]);
    reader.GetBaseSchema();
    DecodedBatch b;
    while (reader.GetNextBatch(&b, dict)) {
      Message m;
      m.is_dictionary = b.is_dictionary;
      m.source = static_cast<int32_t>(si);
      if (!b.is_dictionary) m.ordinal = ordinal++;
      m.length = b.length;
      m.body.assign(b.body, b.body + b.body_size);
      all.push_back(std::move(m));
    }
  }
  return all;
}

mi_scan_options Options(bool dict, int world, int rank) {
  mi_scan_options o;
  std::memset(&o, 0, sizeof(o));   // host consumer: compressed bodies are decompressed by the reader's host threads
  o.accept_dictionaries = dict;
  o.world = world;
  o.rank = rank;
  return o;
}

// the messages of `expect` that belong to (world, rank), then the end -- or, when `fails`, an error instead of the end
void CheckShare(const std::vector<std::string>& paths, const std::vector<Message>& expect, bool dict, int world, int rank, bool fails, int* producers) {
  g_threads_started = 0;
  ReadAhead ra(paths, {}, Options(dict, world, rank), /*max_in_flight*/ 3, Hooks());
  CHECK(!ra.Started(), "started before Start()");
  ra.Start(/*trace*/ false);
  *producers = ra.Producers();
  size_t at = 0;
  for (;;) {
    Fetched f;
    CHECK(ra.Take(&f, /*may_block*/ true), "a blocking Take returned nothing");
    while (at < expect.size() && !expect[at].is_dictionary && world > 1 && expect[at].ordinal % world != rank) at++;
    if (f.end || f.error) {
      CHECK(at == expect.size(), "world %d rank %d, %d producers: the stream ended at message %zu of %zu", world, rank, *producers, at, expect.size());
      CHECK(fails == static_cast<bool>(f.error), "world %d rank %d, %d producers: %s", world, rank, *producers, fails ? "no error for the missing file" : "unexpected error");
      break;
    }
    CHECK(at < expect.size(), "more messages than the files hold");
    const Message& m = expect[at++];
    CHECK(f.batch.is_dictionary == m.is_dictionary && f.source == m.source && (m.is_dictionary || f.ordinal == m.ordinal),
          "world %d rank %d, %d producers: got %s %lld of file %d where %s %lld of file %d was due", world, rank, *producers,
          f.batch.is_dictionary ? "a dictionary before batch" : "batch", static_cast<long long>(f.ordinal), f.source,
          m.is_dictionary ? "a dictionary before batch" : "batch", static_cast<long long>(m.ordinal), m.source);
    CHECK(f.batch.body != nullptr && f.batch.length == m.length && static_cast<size_t>(f.batch.body_size) == m.body.size() &&
              std::memcmp(f.batch.body, m.body.data(), m.body.size()) == 0,
          "batch %lld: body differs from the single-threaded read", static_cast<long long>(m.ordinal));
  }
  CHECK(g_threads_started.load() == *producers, "thread_start ran %d times for %d producers", g_threads_started.load(), *producers);
}

void CheckStopWhileQueuesAreFull(const std::vector<std::string>& paths, bool dict) {
  ReadAhead ra(paths, {}, Options(dict, 1, 0), 3, Hooks());
  ra.Start(false);
  std::this_thread::sleep_for(std::chrono::milliseconds(100));   // nobody takes: every producer fills its queue and waits
  ra.Stop();
}

void CheckStopWithoutStagingBuffers(const std::vector<std::string>& paths, bool dict) {
  ReadAhead ra(paths, {}, Options(dict, 1, 0), /*max_in_flight*/ 2, Hooks());
  std::vector<Fetched> held;   // declared second: the batches give their staging buffers back before the read-ahead goes
  ra.Start(false);
  // hold every batch: once all staging buffers are leased the producers wait for one and nothing more arrives
  int idle_ms = 0;
  while (idle_ms < 300) {
    Fetched f;
    if (!ra.Take(&f, /*may_block*/ false)) {
      // (not ReadAhead::WaitReady: libstdc++ waits on the steady clock through pthread_cond_clockwait, which the libtsan of
      // GCC 11 does not intercept -- it misses the unlock inside the wait and reports everything the mutex guards)
      std::this_thread::sleep_for(std::chrono::milliseconds(1));
      idle_ms++;
      continue;
    }
    idle_ms = 0;
    CHECK(!f.error, "unexpected error");
    CHECK(!f.end, "the files are too short for this check: every body found a staging buffer");
    held.push_back(std::move(f));
  }
  ra.Stop();
}
}  // namespace

int main(int argc, char** argv) {
  bool dict = false;
  std::vector<std::string> paths;
  for (int i = 1; i < argc; i++) {
    if (std::string(argv[i]) == "--dict") dict = true;
    else paths.emplace_back(argv[i]);
  }
  if (paths.size() < 3) {
    std::fprintf(stderr, "usage: readahead_check [--dict] <stream file> <stream file> <stream file> ...\n");
    return 2;
  }
  const std::vector<Message> expect = ReadSingleThreaded(paths, dict);
  // the same list with a file that does not exist in the middle: what comes before it is still delivered
  const size_t cut = paths.size() / 2;
  std::vector<std::string> broken = paths;
  broken.insert(broken.begin() + static_cast<long>(cut), paths[0] + ".does-not-exist");
  std::vector<Message> before;
  for (auto& m : expect)
    if (static_cast<size_t>(m.source) < cut) before.push_back(m);

  int runs = 0, producers = 0;
  unsetenv("MI_SCAN_PRODUCERS");
  CheckShare(paths, expect, dict, 1, 0, false, &producers);
  std::printf("%d producers by default\n", producers);
  for (int p = 1; p <= 4; p++) {
    setenv("MI_SCAN_PRODUCERS", std::to_string(p).c_str(), 1);
    for (int k = 0; k < 4; k++) {
      const int world = k == 0 ? 1 : 3, rank = k == 0 ? 0 : k - 1;
      CheckShare(paths, expect, dict, world, rank, false, &producers);
      CheckShare(broken, before, dict, world, rank, true, &producers);
      runs += 2;
    }
    CheckStopWhileQueuesAreFull(paths, dict);
    CheckStopWithoutStagingBuffers(paths, dict);
  }
  std::printf("%zu messages, %d runs, %d failed\n", expect.size(), runs, g_failed);
  return g_failed ? 1 : 0;
}
