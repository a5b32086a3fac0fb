// io_pool_check.cpp -- the process-wide I/O pool and the NUMA binding on their own (test infrastructure, never shipped).
//
// duckdb-arrow_amd/csrc/io_pool.cpp includes no other header of the project, so this program builds from that one source and
// runs under ThreadSanitizer and under ASan + UBSan.  The pool reads MI_IO_THREADS once, so each setting is a process:
//   g++ -std=c++17 -O1 -g -fsanitize=thread tests/sanitize/io_pool_check.cpp duckdb-arrow_amd/csrc/io_pool.cpp -lpthread -o io_pool_check
//   MI_IO_THREADS=1 ./io_pool_check serial && MI_IO_THREADS=4 ./io_pool_check pool
// Prints "N checks, 0 failed".  Nothing is asserted about where threads or pages end up: the machine may have one NUMA node.
#include <sched.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../duckdb-arrow_amd/csrc/io_pool.hpp"

using namespace miarrow;

static int g_checks = 0, g_failed = 0;
static void Check(bool ok, const char* what) {
  g_checks++;
  if (!ok) {
    g_failed++;
    std::fprintf(stderr, "FAILED %s\n", what);
  }
}

// One ParallelFor whose every index is counted: true when each of the n ran exactly once and all were done on return.
static bool RunCounted(int n) {
  std::unique_ptr<std::atomic<int>[]> runs(new std::atomic<int>[static_cast<size_t>(std::max(n, 1))]);
  for (int i = 0; i < n; i++) runs[i].store(0);
  std::atomic<int> done{0};
  ParallelFor(n, [&](int i) {
    if (i % 5 == 0) std::this_thread::yield();   // let the batches of other callers in between
    runs[i].fetch_add(1);
    done.fetch_add(1);
  });
  bool ok = done.load() == n;   // read right after the return: no index may still be running
  for (int i = 0; i < n; i++) ok = ok && runs[i].load() == 1;
  return ok;
}

// Every i in order on the calling thread (what n <= 1, or a pool of one thread, promises)
static bool RunsInOrderOnCaller(int n) {
  const std::thread::id me = std::this_thread::get_id();
  std::vector<int> order;
  bool same_thread = true;
  ParallelFor(n, [&](int i) {
    order.push_back(i);   // unsynchronised on purpose: TSan reports it if a second thread ever gets here
    same_thread = same_thread && std::this_thread::get_id() == me;
  });
  bool ok = same_thread && static_cast<int>(order.size()) == n;
  for (int i = 0; ok && i < n; i++) ok = order[static_cast<size_t>(i)] == i;
  return ok;
}

// The CPUs this process gets, restated from the documentation of the pool: the hardware's, or the cgroup quota when smaller
static int CpuBudget() {
  long long hw = std::max(1u, std::thread::hardware_concurrency());
  long long quota = -1, period = 0;
  if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[32] = {0};
    if (std::fscanf(f, "%31s %lld", q, &period) == 2 && std::strcmp(q, "max") != 0) quota = std::atoll(q);
    std::fclose(f);
  } else if (FILE* g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
    if (std::fscanf(g, "%lld", &quota) != 1) quota = -1;
    std::fclose(g);
    if (FILE* h = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
      if (std::fscanf(h, "%lld", &period) != 1) period = 0;
      std::fclose(h);
    }
  }
  if (quota > 0 && period > 0) hw = std::min(hw, std::max(1ll, quota / period));
  return static_cast<int>(hw);
}

static void Serial() {
  Check(IoThreads() == 1, "MI_IO_THREADS=1 gives a pool of the calling thread alone");
  for (int n : {0, 1, 2, 50}) Check(RunsInOrderOnCaller(n), "one thread: every index once, in order, on the caller");
}

static void ConcurrentCallers() {
  constexpr int kCallers = 6, kCalls = 200;
  std::atomic<int> bad{0};
  std::vector<std::thread> callers;
  for (int t = 0; t < kCallers; t++)
    callers.emplace_back([&, t] {
      for (int c = 0; c < kCalls; c++)
        if (!RunCounted(1 + (c * 7 + t * 13) % 64)) bad.fetch_add(1);   // n takes every value from 1 to 64
    });
  for (auto& th : callers) th.join();
  Check(bad.load() == 0, "six callers x 200 calls: every index of every call exactly once, none left when the call returns");
}

static void OneTaskThrows() {
  std::atomic<int> ran{0};
  std::string got;
  try {
    ParallelFor(32, [&](int i) {
      if (i == 7) throw std::runtime_error("seven");
      ran.fetch_add(1);
    });
  } catch (const std::runtime_error& e) {
    got = e.what();
  }
  Check(got == "seven", "the caller gets the task's exception");
  Check(ran.load() == 31, "every other index of that call still ran");
  Check(RunCounted(16), "a later call on the same pool works");
}

static void Nested() {
  std::atomic<int> inner{0};
  ParallelFor(8, [&](int) { ParallelFor(8, [&](int) { inner.fetch_add(1); }); });
  Check(inner.load() == 64, "a task that calls ParallelFor itself completes (the caller works on its own batch)");
}

static void Ensure() {
  const int cap = std::max(CpuBudget() / 2, 8);
  const int before = IoThreads();
  EnsureIoThreads(1);
  Check(IoThreads() == before, "EnsureIoThreads below the size changes nothing");
  EnsureIoThreads(before + 2);
  Check(IoThreads() == std::max(before, std::min(before + 2, cap)), "EnsureIoThreads grows to what was asked, within the cap");
  const int grown = IoThreads();
  EnsureIoThreads(1 << 20);
  Check(IoThreads() == std::max(grown, cap), "EnsureIoThreads never goes past max(budget / 2, 8)");
  EnsureIoThreads(2);
  Check(IoThreads() == std::max(grown, cap), "... and never lowers");
  Check(RunCounted(64), "the grown pool runs every index");
}

static void Binding() {
  cpu_set_t before, after, allowed;
  CPU_ZERO(&before);
  CPU_ZERO(&after);
  CPU_ZERO(&allowed);
  Check(sched_getaffinity(0, sizeof(before), &before) == 0, "sched_getaffinity");
  BindThisThreadToNode(-1, {});
  BindThisThreadToNode(0, {});
  Check(sched_getaffinity(0, sizeof(after), &after) == 0 && CPU_EQUAL(&before, &after), "no node or no CPUs: nothing is bound");
  std::vector<int> cpus;
  if (sched_getaffinity(getpid(), sizeof(allowed), &allowed) == 0)
    for (int c = 0; c < CPU_SETSIZE; c++)
      if (CPU_ISSET(c, &allowed)) cpus.push_back(c);
  Check(!cpus.empty(), "the process may run somewhere");
  BindThisThreadToNode(0, cpus);
  Check(RunCounted(64), "bound to the CPUs the process may use: every index still runs");
  Check(RunCounted(3), "... and again, from workers that have adopted the binding");
  PreferNode(-1);
  Check(true, "PreferNode(-1) returns");
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "serial") {
    Serial();
  } else if (mode == "pool") {
    Check(IoThreads() == 4, "MI_IO_THREADS=4");
    for (int n : {0, 1}) Check(RunsInOrderOnCaller(n), "n <= 1: on the caller, whatever the pool's size");
    ConcurrentCallers();
    OneTaskThrows();
    Nested();
    Binding();
    Ensure();
  } else {
    std::fprintf(stderr, "usage: MI_IO_THREADS=1 io_pool_check serial | MI_IO_THREADS=4 io_pool_check pool\n");
    return 2;
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
