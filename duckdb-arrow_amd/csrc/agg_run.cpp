// agg_run.cpp -- see agg_run.hpp.
#include "agg_run.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>

#include "engine.hpp"

namespace miarrow {

namespace {
std::atomic<int64_t> g_events_ns[3][2];   // per AggMode: the device time of its two kernels, nanoseconds
//! K11's buffer: the table (hashgroup::TableBytes), then -- on a multiple of 256 bytes -- what hash_group_collect writes
size_t HashTableBytesAligned(uint32_t max_groups, int n_aggs) { return (hashgroup::TableBytes(max_groups, n_aggs) + 255) / 256 * 256; }
}  // namespace

void AggTimingTotals(AggMode mode, double out_ms[2]) {
  for (int i = 0; i < 2; i++) out_ms[i] = static_cast<double>(g_events_ns[static_cast<int>(mode)][i].load()) * 1e-6;
}

AggRun::AggRun(AggMode mode, int n_keys, int32_t key_cls, const std::vector<int32_t>& ops, const std::vector<int32_t>& classes, uint32_t max_groups, bool count_time)
    : mode_(mode), n_keys_(n_keys), n_aggs_(static_cast<int>(ops.size())), max_groups_(max_groups), shape_() {
  shape_.n_keys = n_keys;
  shape_.keys[0].cls = key_cls;
  shape_.aggs.n_aggs = n_aggs_;
  for (int a = 0; a < n_aggs_; a++) {
    shape_.aggs.aggs[a].op = ops[static_cast<size_t>(a)];
    shape_.aggs.aggs[a].a.cls = classes[static_cast<size_t>(a)];
  }
  const char* timing = count_time ? std::getenv("MI_AGG_TIMING") : nullptr;
  timed_ = timing && timing[0] == '1';
}

void AggRun::Begin(hipStream_t stream) {
  if (mode_ == AggMode::kPlain) {
    d_state_ = DeviceBuffer(aggmerge::kMaxAggregates * sizeof(aggmerge::Partial));
    MI_HIP_CHECK(hipMemsetAsync(d_state_.get(), 0, d_state_.size(), stream));   // count 0: the identity of every merge
  } else if (mode_ == AggMode::kGrouped) {
    d_state_ = DeviceBuffer(device::GroupTableBytes(n_keys_, n_aggs_));
    MI_HIP_CHECK(device::GroupTableClear(d_state_.get(), n_keys_, n_aggs_, stream));
  } else {
    d_state_ = DeviceBuffer(HashTableBytesAligned(max_groups_, n_aggs_) + device::HashCollectBytes(max_groups_, n_aggs_));
    MI_HIP_CHECK(device::LaunchHashGroupClear(shape_, device::HashTableAt(d_state_.get(), max_groups_, n_aggs_), stream));   // on the caller's stream, never the null stream
  }
}

void AggRun::Stamp(hipStream_t stream) {
  if (!timed_) return;
  events_.push_back(HipEvent::CreateTimed());
  MI_HIP_CHECK(hipEventRecord(events_.back(), stream));
}

void AggRun::Batch(const device::GroupProgram& prog, const device::AggExprTable* exprs, const mi_sel_t* sel, const uint32_t* sel_count, int64_t nrows,
                   hipStream_t stream) {
  if (nrows <= 0) return;
  const int64_t n_windows = (nrows + MI_VECTOR_SIZE - 1) / MI_VECTOR_SIZE;
  auto scratch = [&](size_t bytes, size_t floor) {
    DeviceBuffer old = Grow(d_scratch_, bytes, GrownCapacity(bytes, d_scratch_.size(), floor));
    if (old) outgrown_.push_back(std::move(old));
  };
  if (mode_ == AggMode::kHash) {
    Stamp(stream);
    MI_HIP_CHECK(device::LaunchHashGroupRows(prog, sel, sel_count, nrows, device::HashTableAt(d_state_.get(), max_groups_, n_aggs_), stream, exprs));
    Stamp(stream);
  } else if (mode_ == AggMode::kGrouped) {
    scratch(device::GroupWindowsBytes(n_windows, n_keys_, n_aggs_), 1 << 16);
    const device::GroupWindowsOut win = device::GroupWindowsAt(d_scratch_.get(), n_windows, n_keys_, n_aggs_);
    Stamp(stream);
    MI_HIP_CHECK(device::LaunchGroupWindows(prog, sel, sel_count, nrows, win, stream, exprs));
    Stamp(stream);
    MI_HIP_CHECK(device::LaunchGroupCombine(prog, win, n_windows, device::GroupTableAt(d_state_.get(), n_keys_, n_aggs_), stream, exprs));
    Stamp(stream);
  } else {
    scratch(static_cast<size_t>(n_windows) * static_cast<size_t>(n_aggs_) * sizeof(aggmerge::Partial), 1 << 12);   // partials[window][aggregate]
    aggmerge::Partial* partials = d_scratch_.get<aggmerge::Partial>();
    Stamp(stream);
    MI_HIP_CHECK(device::LaunchAggWindows(prog.aggs, sel, sel_count, nrows, partials, stream, exprs));
    Stamp(stream);
    MI_HIP_CHECK(device::LaunchAggCombine(prog.aggs, partials, n_windows, d_state_.get<aggmerge::Partial>(), stream, exprs));
    Stamp(stream);
  }
}

void AggRun::Finish(hipStream_t stream, GroupResult* out) {
  const size_t n_aggs = static_cast<size_t>(n_aggs_), n_keys = static_cast<size_t>(n_keys_);
  const bool hash = mode_ == AggMode::kHash;
  std::vector<uint8_t> host;   // K9: the accumulators in use; K10: the table (one copy: keys, accumulators, group count, flags)
  uint32_t head[hashgroup::kHeadWords];
  device::HashCollectOut rec;
  if (hash) {
    const device::HashTableDev table = device::HashTableAt(d_state_.get(), max_groups_, n_aggs_);
    rec = device::HashCollectAt(d_state_.get() + HashTableBytesAligned(max_groups_, n_aggs_), max_groups_, n_aggs_);
    Stamp(stream);
    MI_HIP_CHECK(device::LaunchHashGroupCollect(shape_, table, rec, stream));
    Stamp(stream);
    MI_HIP_CHECK(hipMemcpyAsync(head, table.head, sizeof(head), hipMemcpyDeviceToHost, stream));
  } else {
    host.resize(mode_ == AggMode::kGrouped ? device::GroupTableBytes(n_keys_, n_aggs_) : n_aggs * sizeof(aggmerge::Partial));
    MI_HIP_CHECK(hipMemcpyAsync(host.data(), d_state_.get(), host.size(), hipMemcpyDeviceToHost, stream));
  }
  MI_HIP_CHECK(hipStreamSynchronize(stream));
  // the intervals between a batch's stamps are its launches, in order; K11's last pair is around the collect
  const size_t stride = hash ? 2 : 3;
  for (size_t e = 0; e + stride <= events_.size(); e += stride)
    for (size_t i = 0; i + 1 < stride; i++) {
      float ms = 0;
      MI_HIP_CHECK(hipEventElapsedTime(&ms, events_[e + i], events_[e + i + 1]));
      g_events_ns[static_cast<int>(mode_)][hash ? (e + stride == events_.size() ? 1 : 0) : i] += static_cast<int64_t>(static_cast<double>(ms) * 1e6);
    }
  events_.clear();
  if (mode_ == AggMode::kPlain) {
    const aggmerge::Partial* acc = reinterpret_cast<const aggmerge::Partial*>(host.data());
    uint32_t flags = 0;
    for (size_t a = 0; a < n_aggs; a++) flags |= static_cast<uint32_t>(acc[a].flags);
    ThrowForStatus(flags);
    out->values.insert(out->values.end(), acc, acc + n_aggs);
    return;
  }
  if (mode_ == AggMode::kGrouped) {
    const device::GroupTableDev t = device::GroupTableAt(host.data(), n_keys_, n_aggs_);
    ThrowForStatus(t.head[1]);
    const size_t n = std::min<size_t>(t.head[0], groupkey::kMaxGroups);
    for (size_t g = 0; g < n; g++) {
      groupkey::Key k;
      std::memset(&k, 0, sizeof(k));
      k.nulls = t.nulls[g];
      for (size_t i = 0; i < n_keys; i++) {
        k.lo[i] = t.keys[(g * n_keys + i) * 2];
        k.hi[i] = t.keys[(g * n_keys + i) * 2 + 1];
      }
      out->keys.push_back(k);
      out->values.insert(out->values.end(), t.acc + g * n_aggs, t.acc + (g + 1) * n_aggs);
    }
    return;
  }
  const uint32_t status = head[hashgroup::kHeadStatus];
  if (status & MI_ST_GROUP_LIMIT)
    throw NotImplementedException("hash GROUP BY found more than max_groups = " + std::to_string(max_groups_) + " distinct keys among the selected rows: call again with a larger "
                                  "max_groups (at most " + std::to_string(hashgroup::kMaxHashGroups) + ")");
  ThrowForStatus(status);
  const size_t n = std::min<size_t>(head[hashgroup::kHeadCollected], max_groups_);
  if (n == 0) return;
  std::vector<uint64_t> keys(n);
  std::vector<uint32_t> nulls(n);
  const size_t v0 = out->values.size();
  out->values.resize(v0 + n * n_aggs);
  MI_HIP_CHECK(hipMemcpyAsync(keys.data(), rec.keys, n * 8, hipMemcpyDeviceToHost, stream));
  MI_HIP_CHECK(hipMemcpyAsync(nulls.data(), rec.nulls, n * 4, hipMemcpyDeviceToHost, stream));
  MI_HIP_CHECK(hipMemcpyAsync(out->values.data() + v0, rec.partials, n * n_aggs * sizeof(aggmerge::Partial), hipMemcpyDeviceToHost, stream));
  MI_HIP_CHECK(hipStreamSynchronize(stream));
  out->keys.reserve(out->keys.size() + n);
  for (size_t g = 0; g < n; g++) out->keys.push_back(HashGroupKey(keys[g], nulls[g] != 0, shape_.keys[0].cls));
}

}  // namespace miarrow
