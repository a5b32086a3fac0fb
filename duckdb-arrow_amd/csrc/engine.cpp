// engine.cpp -- device context + transcode plans.  See engine.hpp.
#include "engine.hpp"

#include "io_pool.hpp"

#include <hip/hip_runtime.h>

#include <sched.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

namespace miarrow {

Context::Context(int device_id) : device(device_id) {
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    // The product path has no CPU fallback: without a HIP device it fails loudly.
    throw Exception(MI_ENODEV, std::string("No HIP device available (hipGetDeviceCount: ") +
                                   (e == hipSuccess ? "0 devices" : hipGetErrorString(e)) +
                                   "); the MI355X Arrow IPC path has no CPU fallback");
  }
  if (device_id < 0 || device_id >= count) {
    throw Exception(MI_ENODEV, "HIP device " + std::to_string(device_id) + " out of range (" + std::to_string(count) + " devices)");
  }
  MI_HIP_CHECK(hipSetDevice(device));
  hipDeviceProp_t prop;
  MI_HIP_CHECK(hipGetDeviceProperties(&prop, device));
  num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  stream = HipStream::Create();
  h2d_stream = HipStream::Create();
  d2h_stream = HipStream::Create();
  // the device's place in the host (best effort: any failure leaves numa_node = -1 and nothing is bound)
  const char* nb = std::getenv("MI_NUMA_BIND");
  char bus[64] = {0};
  if (!(nb && nb[0] == '0') && hipDeviceGetPCIBusId(bus, sizeof(bus) - 1, device) == hipSuccess) {
    for (char* q = bus; *q; q++) *q = static_cast<char>(std::tolower(static_cast<unsigned char>(*q)));
    const std::string dir = std::string("/sys/bus/pci/devices/") + bus + "/";
    std::ifstream fn(dir + "numa_node"), fc(dir + "local_cpulist");
    int node = -1;
    std::string list;
    if (fn >> node && node >= 0 && std::getline(fc, list) && !list.empty()) {
      // "0-63,128-191"
      std::vector<int> cpus;
      size_t at = 0;
      bool ok = true;
      while (at < list.size() && ok) {
        size_t end = list.find(',', at);
        if (end == std::string::npos) end = list.size();
        const std::string part = list.substr(at, end - at);
        int lo = 0, hi = 0;
        const int got = std::sscanf(part.c_str(), "%d-%d", &lo, &hi);
        if (got == 1) hi = lo;
        ok = got >= 1 && lo >= 0 && hi >= lo && hi < CPU_SETSIZE;
        for (int c = lo; ok && c <= hi; c++) cpus.push_back(c);
        at = end + 1;
      }
      if (ok && !cpus.empty()) {
        numa_node = node;
        local_cpus = std::move(cpus);
        local_cpulist = list;
      }
    }
  }
  (void)hipGetLastError();
}

void Context::BindThisThread() const { BindThisThreadToNode(numa_node, local_cpus); }

Context::PreferNode::PreferNode(const Context* c) {
  if (c && c->numa_node >= 0 && c->numa_node < static_cast<int>(sizeof(saved_mask) * 8)) {
    // the calling thread is the host program's: remember its policy (most have none: MPOL_DEFAULT)
    if (syscall(SYS_get_mempolicy, &saved_mode, saved_mask, sizeof(saved_mask) * 8, nullptr, 0) != 0) return;
    miarrow::PreferNode(c->numa_node);
    on = true;
  }
}
Context::PreferNode::~PreferNode() {
  if (on) (void)syscall(SYS_set_mempolicy, saved_mode, saved_mode == 0 ? nullptr : saved_mask, saved_mode == 0 ? 0 : sizeof(saved_mask) * 8);
}

void Context::Bind() const { MI_HIP_CHECK(hipSetDevice(device)); }

// hipMemset() is enqueued on the null stream and may return before it has run; the plans run on non-blocking streams, which
// the null stream does not order with.  Everything that must be zero before such a stream touches it is waited for.
static void SyncMemset(void* p, int value, size_t bytes) {
  MI_HIP_CHECK(hipMemset(p, value, bytes));
  MI_HIP_CHECK(hipStreamSynchronize(nullptr));
}

Plan::Plan(Context* ctx_p, const mi_col_task* in_tasks, int32_t n_tasks) : ctx(ctx_p) {
  Set(in_tasks, n_tasks, nullptr);
}

Plan::Plan(Context* ctx_p) : ctx(ctx_p), reusable(true) {
  ctx->Bind();
  d_status = DeviceBuffer(64);
  SyncMemset(d_status.get(), 0, 64);
}

// A device table of `n` elements: the element count at least doubles (64 at least), the outgrown table is freed at once.
template <typename T>
static void GrowTable(DeviceBuffer& table, size_t n) {
  Grow(table, n * sizeof(T), std::max<size_t>({n, table.size() / sizeof(T) * 2, 64}) * sizeof(T));
}

void Plan::Set(const mi_col_task* in_tasks, int32_t n_tasks, hipStream_t upload_stream) {
  ctx->Bind();
  LayOutPlan(in_tasks, n_tasks, this);
  // device tables
  GrowTable<mi_col_task>(d_tasks, tasks.size());
  GrowTable<uint32_t>(d_tile_begin, tile_begin.size());
  GrowTable<uint32_t>(d_tile_task, tile_task.size());
  if (!d_status) {
    d_status = DeviceBuffer(64);
    SyncMemset(d_status.get(), 0, 64);
  }
  if (class_tiles[device::kClassEncString]) GrowTable<int64_t>(d_tile_sums, 2 * static_cast<size_t>(class_tiles[device::kClassEncString]) + 1);
  if (class_tiles[device::kClassGather]) GrowTable<int64_t>(d_gather_bases, tile_task.size());
  if (n_null_counts) {
    const size_t before = d_null_counts.size();
    GrowTable<int64_t>(d_null_counts, static_cast<size_t>(n_null_counts));
    if (d_null_counts.size() != before) SyncMemset(d_null_counts.get(), 0, d_null_counts.size());
  }
  if (reusable && upload_stream) {
    // a pinned mirror as large as its device table (a new one whenever the table grew)
    auto mirror = [](PinnedBuffer& h, const DeviceBuffer& d) {
      if (h.size() != d.size()) h = PinnedBuffer(d.size());
    };
    mirror(h_tasks, d_tasks);
    mirror(h_tile_begin, d_tile_begin);
    if (!tasks.empty()) {
      std::memcpy(h_tasks.get(), tasks.data(), tasks.size() * sizeof(mi_col_task));
      MI_HIP_CHECK(hipMemcpyAsync(d_tasks.get(), h_tasks.get(), tasks.size() * sizeof(mi_col_task), hipMemcpyHostToDevice, upload_stream));
    }
    std::memcpy(h_tile_begin.get(), tile_begin.data(), tile_begin.size() * sizeof(uint32_t));
    MI_HIP_CHECK(hipMemcpyAsync(d_tile_begin.get(), h_tile_begin.get(), tile_begin.size() * sizeof(uint32_t), hipMemcpyHostToDevice, upload_stream));
    mirror(h_tile_task, d_tile_task);
    if (!tile_task.empty()) {
      std::memcpy(h_tile_task.get(), tile_task.data(), tile_task.size() * sizeof(uint32_t));
      MI_HIP_CHECK(hipMemcpyAsync(d_tile_task.get(), h_tile_task.get(), tile_task.size() * sizeof(uint32_t), hipMemcpyHostToDevice, upload_stream));
    }
  } else {
    if (!tasks.empty())
      MI_HIP_CHECK(hipMemcpy(d_tasks.get(), tasks.data(), tasks.size() * sizeof(mi_col_task), hipMemcpyHostToDevice));
    MI_HIP_CHECK(hipMemcpy(d_tile_begin.get(), tile_begin.data(), tile_begin.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (!tile_task.empty())
      MI_HIP_CHECK(hipMemcpy(d_tile_task.get(), tile_task.data(), tile_task.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
}

void Plan::LaunchSlice(const ClassSlice& cs, hipStream_t s) {
  if (cs.total_tiles == 0) return;
  const mi_col_task* t = d_tasks.get<mi_col_task>() + cs.first_task;
  const uint32_t* tb = d_tile_begin.get<uint32_t>() + cs.tile_begin_at;
  const uint32_t* tt = d_tile_task.get<uint32_t>() + cs.tile_task_at;
  uint32_t* status = d_status.get<uint32_t>();
  int64_t* null_counts = d_null_counts.get<int64_t>();
  switch (static_cast<int>(cs.slot)) {
    case device::kSlotRunEnd:
      MI_HIP_CHECK(device::LaunchRunEnd(t, tb, tt, cs.n_tasks, cs.total_tiles, status, s));
      break;
    case device::kSlotUnionTags:
    case device::kSlotUnionDense:
      MI_HIP_CHECK(device::LaunchUnion(cs.slot == device::kSlotUnionDense, t, tb, tt, cs.n_tasks, cs.total_tiles, status, s));
      break;
    case device::kSlotEncView:   // the look-back words are those of encode_string_1p's slice, which has run by now (same stream)
      MI_HIP_CHECK(device::LaunchEncodeStringView(t, tb, tt, cs.n_tasks, cs.total_tiles, d_tile_sums.get<int64_t>(), null_counts, status, s));
      break;
    case device::kClassEncFixed:
      MI_HIP_CHECK(device::LaunchEncodeFixed(t, tb, tt, cs.n_tasks, cs.total_tiles, null_counts, status, cs.kernel_mask, s));
      break;
    case device::kClassEncString:
      MI_HIP_CHECK(device::LaunchEncodeString(t, tb, tt, cs.n_tasks, cs.total_tiles, d_tile_sums.get<int64_t>(), null_counts, status, (cs.kernel_mask & 2u) != 0, s));
      break;
    case device::kClassGather:
      MI_HIP_CHECK(device::LaunchGather(t, tb, tt, cs.n_tasks, cs.total_tiles, d_gather_bases.get<int64_t>() + cs.tile_task_at, status, s));
      break;
    default:
      MI_HIP_CHECK(device::LaunchTranscode(cs.slot, t, tb, tt, cs.n_tasks, cs.total_tiles, status, cs.kernel_mask, s));
      break;
  }
}

void Plan::Launch(hipStream_t s) {
  ctx->Bind();
  if (!s) s = ctx->stream;
  last_stream = s;
  for (const auto& sl : slices) LaunchSlice(sl, s);
}

void Plan::LaunchTimed(hipStream_t s, float* ms_per_class) {
  ctx->Bind();
  if (!s) s = ctx->stream;
  last_stream = s;
  std::vector<hipEvent_t> ev(slices.size() + 1);
  for (auto& e : ev) MI_HIP_CHECK(hipEventCreate(&e));
  MI_HIP_CHECK(hipEventRecord(ev[0], s));
  for (size_t i = 0; i < slices.size(); i++) {
    LaunchSlice(slices[i], s);
    MI_HIP_CHECK(hipEventRecord(ev[i + 1], s));
  }
  MI_HIP_CHECK(hipStreamSynchronize(s));
  for (int c = 0; c < device::kNumClasses; c++) ms_per_class[c] = 0;
  for (size_t i = 0; i < slices.size(); i++) {
    float ms = 0;
    MI_HIP_CHECK(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
    ms_per_class[device::kSlots[slices[i].slot].cls] += ms;
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
}

uint32_t Plan::Status() {
  ctx->Bind();
  hipStream_t s = last_stream ? last_stream : ctx->stream;
  MI_HIP_CHECK(hipStreamSynchronize(s));
  uint32_t bits = 0;
  MI_HIP_CHECK(hipMemcpy(&bits, d_status.get(), sizeof(bits), hipMemcpyDeviceToHost));
  if (bits) {   // on the plan's own stream: a memset on the null stream is not ordered with the non-blocking streams the plans run on
    MI_HIP_CHECK(hipMemsetAsync(d_status.get(), 0, sizeof(bits), s));
    MI_HIP_CHECK(hipStreamSynchronize(s));
  }
  return bits;
}

std::vector<int64_t> Plan::NullCounts(bool reset) {
  ctx->Bind();
  std::vector<int64_t> per_slot(static_cast<size_t>(n_null_counts), 0);
  if (n_null_counts) {
    hipStream_t s = last_stream ? last_stream : ctx->stream;
    MI_HIP_CHECK(hipStreamSynchronize(s));
    MI_HIP_CHECK(hipMemcpy(per_slot.data(), d_null_counts.get(), per_slot.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (reset) {
      // on the plan's own stream and finished before this returns: hipMemset() goes to the null stream, which is not ordered
      // with the non-blocking streams the plans run on -- the next row group's kernels could add their NULLs to the counters
      // BEFORE the memset of this row group cleared them (seen as null_count 0 in a file written by several sink threads)
      MI_HIP_CHECK(hipMemsetAsync(d_null_counts.get(), 0, per_slot.size() * sizeof(int64_t), s));
      MI_HIP_CHECK(hipStreamSynchronize(s));
    }
  }
  return MapNullCounts(per_slot.data());
}

void Plan::ResetCounters(hipStream_t stream) {
  MI_HIP_CHECK(hipMemsetAsync(d_status.get(), 0, sizeof(uint32_t), stream));
  if (n_null_counts) MI_HIP_CHECK(hipMemsetAsync(d_null_counts.get(), 0, static_cast<size_t>(n_null_counts) * 8, stream));
}

void ThrowForStatus(uint32_t bits) {
  if (bits == 0) return;
  if (bits & MI_ST_BAD_OFFSETS)
    throw InternalException("Arrow IPC validation failed: offsets buffer is not monotonically non-decreasing or exceeds the data buffer");
  if (bits & MI_ST_STRING_TOO_LARGE) throw ConversionException("DuckDB does not support Strings over 4GB");
  if (bits & MI_ST_MUL_OVERFLOW) throw ConversionException("Could not convert Timestamp to Microsecond");
  if (bits & MI_ST_INDEX_RANGE) throw ConversionException("DuckDB only supports indices that fit on an uint32");
  if (bits & MI_ST_DICT_INDEX) throw InternalException("Arrow IPC validation failed: dictionary index out of range");
  if (bits & MI_ST_DECIMAL_RANGE) throw ConversionException("Decimal value does not fit the physical type of its declared precision");
  if (bits & MI_ST_BAD_RUN_ENDS)
    throw InternalException("Arrow IPC validation failed: run ends are not positive and strictly increasing or end before the array does");
  if (bits & MI_ST_BAD_UNION_TAG) throw InvalidInputException("Arrow union tag out of range");
  if (bits & MI_ST_BAD_UNION_OFFSET) throw InternalException("Arrow IPC validation failed: union offsets are negative or exceed the member array");
  if (bits & MI_ST_DECOMPRESS)
    throw IOException("LZ4_FRAME compressed buffer is malformed or does not decompress to its declared size (Expected decompressed size mismatch)");
  if (bits & MI_ST_INTERNAL) throw InternalException("a kernel gave up waiting for another workgroup (bounded spin exceeded)");
  if (bits & MI_ST_SEL_RANGE) throw InvalidInputException("aggregate: a selection index names no row of its 2048-row window (skipped: the results are not valid)");
  if (bits & MI_ST_GROUP_KEY_LONG) throw NotImplementedException("a VARCHAR / BLOB group key longer than 12 bytes stays above the scan");
  if (bits & MI_ST_GROUP_LIMIT)
    throw NotImplementedException("GROUP BY with more than " + std::to_string(MI_GROUP_WINDOW_LIMIT) + " groups among the selected rows of a 2048-row window or more than " +
                                  std::to_string(MI_MAX_GROUPS) + " groups in a scan stays above the scan");
  if (bits & MI_ST_OFFSET_OVERFLOW)
    throw InvalidInputException(
        "Arrow Appender: The maximum total string size for regular string buffers is 2147483647 but the offset exceeds this.\n"
        "* SET arrow_large_buffer_size=true to use large string buffers");
  throw InternalException("unknown device status " + std::to_string(bits));
}

}  // namespace miarrow
