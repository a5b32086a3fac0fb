// io_pool.hpp -- the process-wide I/O thread pool and the NUMA binding of the threads that feed it.  Shared by every scan,
// every device and the host decompressors; includes no other header of the project.
#pragma once

#include <functional>
#include <vector>

namespace miarrow {

//! Runs fn(i), i in [0, n), on the process-wide I/O pool (MI_IO_THREADS, default 8) + the calling thread; rethrows the
//! first failure.  Callers on different threads share the pool.
void ParallelFor(int n, const std::function<void(int)>& fn);
int IoThreads();
//! Grows the pool to at least n threads (bounded by the host's cores); multi-device scans ask for 8 per device
void EnsureIoThreads(int n);
// NUMA locality of the host side (engine.hpp, Context::BindThisThread).  BindThisThreadToNode pins the calling thread to
// `cpus` (within what it may use) and makes its allocations prefer `node`; from then on the tasks it gives the I/O pool
// (parallel preads of a body, host decompression) run under the same binding: a pool worker adopts the binding of the batch
// of tasks it takes.  PreferNode(node) / PreferNode(-1): only the allocation policy of the calling thread.
void BindThisThreadToNode(int node, const std::vector<int>& cpus);
void PreferNode(int node);

}  // namespace miarrow
