// engine.hpp -- device context and transcode plans (host side of the fused kernel launch).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <string>
#include <vector>

#include "hip_resources.hpp"
#include "ipc_format.hpp"
#include "kernels.hpp"
#include "plan_layout.hpp"

namespace miarrow {

struct Context {
  int device = 0;
  int num_cus = 256;
  HipStream stream;       // compute
  HipStream h2d_stream;   // pinned host -> HBM
  HipStream d2h_stream;   // HBM -> pinned host

  // Where the device hangs in the host: its NUMA node and that node's CPUs (/sys/bus/pci/devices/<bus id>/numa_node and
  // local_cpulist; -1 / empty when the platform does not say).  The library's OWN host threads -- read-ahead producers, the
  // I/O pool while it works for this context -- run there and allocate their pinned buffers there (BindThisThread): a pread
  // into pinned memory followed by a DMA to the device crosses the socket interconnect twice when it happens on the other
  // socket (two-socket boxes: 199 against 300 M rows/s for the same host-consumer scan, by where the threads happened to
  // run).  The caller's threads are never touched.  MI_NUMA_BIND=0 turns it off.
  int numa_node = -1;
  std::vector<int> local_cpus;
  std::string local_cpulist;            // as the kernel prints it ("0-63,128-191")
  void BindThisThread() const;          // affinity = local_cpus (within what the thread may use), allocations prefer numa_node
  // RAII: allocations of the calling thread prefer the device's node inside the scope (pinned buffers the caller's thread makes)
  struct PreferNode {
    explicit PreferNode(const Context* c);
    ~PreferNode();
    bool on = false;
    int saved_mode = 0;                 // the caller's own policy, put back when the scope ends
    unsigned long saved_mask[16] = {0};
  };

  explicit Context(int device_id);
  void Bind() const;  // hipSetDevice
};

// The device side of a plan: the layout's tables in HBM, and the launches.  What is launched, and in which order, is the
// layout's (plan_layout.hpp); its members are read through the plan.
struct Plan : PlanLayout {
  Context* ctx;
  // device tables (mi_col_task / uint32_t / int64_t elements) and the pinned mirrors they are uploaded from (reusable plans)
  DeviceBuffer d_tasks, d_tile_begin;
  DeviceBuffer d_tile_task;          // per class slice: task index (within the slice) of every tile
  DeviceBuffer d_status;             // uint32_t status word
  DeviceBuffer d_tile_sums;          // encode plans with string columns
  DeviceBuffer d_gather_bases;       // gather plans: first output row of every window (indexed like tile_task)
  DeviceBuffer d_null_counts;        // encode plans: one counter per task
  PinnedBuffer h_tasks, h_tile_begin, h_tile_task;
  hipStream_t last_stream = nullptr;
  bool reusable = false;

  Plan(Context* ctx, const mi_col_task* tasks, int32_t n_tasks);
  //! Reusable plan (scan / writer pipelines): tables are re-filled with Set() and uploaded asynchronously from
  //! pinned host mirrors, so a new record batch costs no device allocation and no synchronous copy.
  explicit Plan(Context* ctx);
  void Set(const mi_col_task* tasks, int32_t n_tasks, hipStream_t upload_stream);
  Plan(const Plan&) = delete;
  Plan& operator=(const Plan&) = delete;
  void Launch(hipStream_t stream);
  void LaunchSlice(const ClassSlice& cs, hipStream_t stream);
  //! Launch with hipEvents around each class; returns milliseconds per class after synchronising the stream
  void LaunchTimed(hipStream_t stream, float* ms_per_class);
  uint32_t Status();
  std::vector<int64_t> NullCounts(bool reset);
  //! Clears the status word and the NULL counters on `stream`, for callers that copy both back asynchronously themselves
  void ResetCounters(hipStream_t stream);
};

// status word -> the exception the reference would throw
void ThrowForStatus(uint32_t bits);

}  // namespace miarrow
