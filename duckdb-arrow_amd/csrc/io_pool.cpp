// io_pool.cpp -- see io_pool.hpp.
#include "io_pool.hpp"

#include <sched.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <exception>
#include <map>
#include <memory>
#include <mutex>
#include <thread>

namespace miarrow {

// Large bodies are read with several concurrent pread()s: one thread copies out of the page cache at ~10 GB/s, far below
// what the H2D link takes, so the body is cut into slices read in parallel.  The pool is process wide (MI_IO_THREADS,
// default 8, grown by multi-device scans to 8 per device) and serves any number of callers at once: a Run() is a batch of
// tasks in one shared queue, the caller works on its own batch while it waits.
namespace {
struct IoAffinity {
  cpu_set_t cpus;
  int node = -1;
};
thread_local const IoAffinity* tls_io_affinity = nullptr;   // what this thread is bound to; its pool jobs ask the same of the workers
constexpr int kMpolDefault = 0, kMpolPreferred = 1;          // <linux/mempolicy.h>
void SetPreferredNode(int node) {
  if (node < 0) {
    (void)syscall(SYS_set_mempolicy, kMpolDefault, nullptr, 0);
    return;
  }
  unsigned long mask[16] = {0};
  if (node >= static_cast<int>(sizeof(mask) * 8)) return;
  mask[static_cast<size_t>(node) / (8 * sizeof(unsigned long))] |= 1ul << (static_cast<size_t>(node) % (8 * sizeof(unsigned long)));
  (void)syscall(SYS_set_mempolicy, kMpolPreferred, mask, sizeof(mask) * 8);
}
void ApplyIoAffinity(const IoAffinity* a) {
  cpu_set_t allowed, want;
  CPU_ZERO(&allowed);
  CPU_ZERO(&want);
  // a thread that was narrowed to another node before may widen again: ask for the process's CPUs first
  if (sched_getaffinity(getpid(), sizeof(allowed), &allowed) != 0) return;
  int n = 0;
  for (int c = 0; c < CPU_SETSIZE; c++)
    if (CPU_ISSET(c, &a->cpus) && CPU_ISSET(c, &allowed)) {
      CPU_SET(c, &want);
      n++;
    }
  if (n == 0) return;   // the process may not run on that node at all: stay
  (void)sched_setaffinity(0, sizeof(want), &want);
  SetPreferredNode(a->node);
  tls_io_affinity = a;
}
const IoAffinity* IoAffinityOf(int node, const std::vector<int>& cpus) {
  static std::mutex mu;
  static std::map<int, std::unique_ptr<IoAffinity>> by_node;   // a node's CPUs do not change: one object per node, never freed
  std::lock_guard<std::mutex> lk(mu);
  auto& slot = by_node[node];
  if (!slot) {
    slot = std::make_unique<IoAffinity>();
    CPU_ZERO(&slot->cpus);
    for (int c : cpus)
      if (c >= 0 && c < CPU_SETSIZE) CPU_SET(c, &slot->cpus);
    slot->node = node;
  }
  return slot.get();
}

class IoPool {
 public:
  static IoPool& Get() {
    static IoPool pool;
    return pool;
  }
  int Threads() {
    std::lock_guard<std::mutex> lk(mu);
    return n_threads;
  }
  // CPUs the process may really use: the hardware's, or the cgroup's CPU quota when there is one (a container sees all 256
  // CPUs of the box and gets 16 CPUs' worth of time: threads beyond the quota only throttle one another -- with 12 and 16
  // I/O threads the SF10 host-consumer scan took 0.204 s, with 8 0.18 s)
  static int CpuBudget() {
    int hw = std::max(1, static_cast<int>(std::thread::hardware_concurrency()));
    long long quota = -1, period = 0;
    if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {   // cgroup v2: "<quota|max> <period>"
      char q[32] = {0};
      if (std::fscanf(f, "%31s %lld", q, &period) == 2 && std::strcmp(q, "max") != 0) quota = std::atoll(q);
      std::fclose(f);
    } else if (FILE* g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {   // cgroup v1
      if (std::fscanf(g, "%lld", &quota) != 1) quota = -1;
      std::fclose(g);
      if (FILE* h = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
        if (std::fscanf(h, "%lld", &period) != 1) period = 0;
        std::fclose(h);
      }
    }
    if (quota > 0 && period > 0) hw = std::min<long long>(hw, std::max<long long>(1, quota / period));
    return hw;
  }
  void Ensure(int n) {
    std::lock_guard<std::mutex> lk(mu);
    const int cap = CpuBudget();
    n = std::min(n, std::max(cap / 2, 8));   // half of the budget: the pipeline threads, the HIP runtime's and the caller's need the rest
    while (n_threads < n) {
      workers.emplace_back([this] { Loop(); });
      n_threads++;
    }
  }
  // runs fn(i) for i in [0, n) on the pool + the calling thread; rethrows the first failure
  void Run(int n, const std::function<void(int)>& fn) {
    if (n <= 1 || Threads() <= 1) {
      for (int i = 0; i < n; i++) fn(i);
      return;
    }
    Job job;
    job.fn = &fn;
    job.n = n;
    job.pending = n;
    job.affinity = tls_io_affinity;   // the caller's binding, if it has one
    {
      std::lock_guard<std::mutex> lk(mu);
      jobs.push_back(&job);
    }
    cv.notify_all();
    Work(&job);  // the caller takes tasks of its own batch
    std::unique_lock<std::mutex> lk(mu);
    job.done_cv.wait(lk, [&] { return job.pending == 0; });
    if (job.error) std::rethrow_exception(job.error);
  }

 private:
  struct Job {
    const std::function<void(int)>* fn = nullptr;
    const IoAffinity* affinity = nullptr;
    int n = 0, next = 0, pending = 0;
    std::exception_ptr error;
    std::condition_variable done_cv;
  };
  IoPool() {
    const char* v = std::getenv("MI_IO_THREADS");
    const int n = v ? std::max(1, std::atoi(v)) : 8;
    n_threads = 1;  // the calling thread
    for (int i = 1; i < n; i++) {
      workers.emplace_back([this] { Loop(); });
      n_threads++;
    }
  }
  ~IoPool() {
    {
      std::lock_guard<std::mutex> lk(mu);
      stop = true;
    }
    cv.notify_all();
    for (auto& t : workers) t.join();
  }
  // takes tasks of `only` (or of the oldest batch with tasks left when NULL) until none is left
  void Work(Job* only) {
    while (true) {
      Job* job = nullptr;
      int i = 0;
      {
        std::lock_guard<std::mutex> lk(mu);
        if (only) {
          if (only->next < only->n) job = only;
        } else {
          for (Job* j : jobs)
            if (j->next < j->n) { job = j; break; }
        }
        if (!job) return;
        i = job->next++;
        if (job->next >= job->n) jobs.erase(std::find(jobs.begin(), jobs.end(), job));  // nothing left to hand out
      }
      if (job->affinity && job->affinity != tls_io_affinity) ApplyIoAffinity(job->affinity);   // ~2 us, once per change of caller
      std::exception_ptr err;
      try {
        (*job->fn)(i);
      } catch (...) {
        err = std::current_exception();
      }
      std::lock_guard<std::mutex> lk(mu);
      if (err && !job->error) job->error = err;
      if (--job->pending == 0) job->done_cv.notify_all();
    }
  }
  void Loop() {
    while (true) {
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return stop || !jobs.empty(); });
        if (stop) return;
      }
      Work(nullptr);
    }
  }
  std::mutex mu;
  std::condition_variable cv;
  std::vector<std::thread> workers;
  std::deque<Job*> jobs;  // batches that still have tasks to hand out
  int n_threads = 1;
  bool stop = false;
};
}  // namespace

void ParallelFor(int n, const std::function<void(int)>& fn) { IoPool::Get().Run(n, fn); }
int IoThreads() { return IoPool::Get().Threads(); }
void EnsureIoThreads(int n) { IoPool::Get().Ensure(n); }

void BindThisThreadToNode(int node, const std::vector<int>& cpus) {
  if (node < 0 || cpus.empty()) return;
  ApplyIoAffinity(IoAffinityOf(node, cpus));
}
void PreferNode(int node) { SetPreferredNode(node); }

}  // namespace miarrow
