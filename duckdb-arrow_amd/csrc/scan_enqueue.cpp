// scan_enqueue.cpp -- the GPU work ArrowScan queues for one record batch (see scan_operator.hpp): stage A and, for a compacted
// batch, stage B, as named steps; the K8 staging of a compressed body (its arithmetic: scan_k8.hpp); what both stages share.
#include "scan_k8.hpp"
#include "scan_operator.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <tuple>

namespace miarrow {

namespace {
int64_t WindowsOf(int64_t rows) { return (rows + MI_VECTOR_SIZE - 1) / MI_VECTOR_SIZE; }
int32_t WidthOf(const ScanColumn& c) {
  int32_t kind, w;
  int64_t param;
  c.field.Plan(&kind, &param, &w);
  return w;
}
}  // namespace

// ------------------------------------------------------------------------------------------------ shared by both stages
void ArrowScan::EnsureHostOut(Slot& s, size_t bytes) {
  if (opts.device_resident || bytes <= s.h_out.size()) return;
  ctx->Bind();
  Context::PreferNode near_the_gpu(ctx);   // (the caller's thread allocates: only its policy, for the length of this call)
  Retire(Grow(s.h_out, bytes, GrownCapacity(bytes, s.h_out.size(), 1 << 16)));
}

// Tables the tasks read from HBM (list windows, string-view buffers) travel in a pinned aux buffer beside the body.
void ArrowScan::UploadAux(Slot& s, const std::vector<uint64_t>& aux) {
  const size_t aux_bytes = aux.size() * 8;
  if (!aux_bytes) return;
  Retire(Grow(s.h_aux, aux_bytes, AlignUp(aux_bytes * 2, 4096)));   // the two grow together: twice the need
  Retire(Grow(s.d_aux, aux_bytes, AlignUp(aux_bytes * 2, 4096)));
  std::memcpy(s.h_aux.get(), aux.data(), aux_bytes);
  MI_HIP_CHECK(hipMemcpyAsync(s.d_aux.get(), s.h_aux.get(), aux_bytes, hipMemcpyHostToDevice, ctx->h2d_stream));
}

// Where the planner finds the batch of a slot and where the consumer of its vectors will see the body.
BatchPlacement ArrowScan::MakePlacement(const Slot& s) {
  BatchPlacement where;
  where.batch = &s.batch;
  where.in_base = s.d_in.get();
  // a host consumer of a body that only exists decompressed in HBM: string_t rows point into a pinned mirror of the body
  where.consumer_base = opts.device_resident ? reinterpret_cast<uint64_t>(s.d_in.get())
                                             : reinterpret_cast<uint64_t>(s.batch.deferred ? s.h_mirror.get() : s.batch.body);
  where.dict_len = [this](int64_t id) -> int64_t {
    auto it = dicts.find(id);
    if (it == dicts.end()) throw IOException("RecordBatch uses dictionary id " + std::to_string(id) + " before its DictionaryBatch");
    return it->second->dict_len;
  };
  return where;
}

void ArrowScan::CopyRanges(std::vector<std::pair<int64_t, int64_t>> ranges, const uint8_t* from, uint8_t* to, int64_t align_within) {
  std::sort(ranges.begin(), ranges.end());
  int64_t lo = -1, hi = -1;
  auto flush = [&]() {
    if (lo < 0) return;
    if (align_within >= 0) hi = std::min<int64_t>((hi + 63) & ~int64_t(63), align_within);
    MI_HIP_CHECK(hipMemcpyAsync(to + lo, from + lo, static_cast<size_t>(hi - lo), hipMemcpyHostToDevice, ctx->h2d_stream));
    stats.h2d_bytes += hi - lo;
  };
  for (const auto& r : ranges) {
    if (lo >= 0 && r.first <= hi + (64 << 10)) {   // a gap this small is cheaper to copy than to split
      hi = std::max(hi, r.first + r.second);
      continue;
    }
    flush();
    lo = align_within >= 0 ? r.first & ~int64_t(63) : r.first;
    hi = r.first + r.second;
  }
  flush();
}

// A column absent from a file (union_by_name) is an all-NULL vector: reserved by the planner of the stage that lays the
// projected columns out, zeroed (data 0, validity 0) on the compute stream, handed out by BuildChunk.
void ArrowScan::PlanAbsentColumn(Slot& s, BatchPlanner& planner, size_t c, int64_t rows) {
  Slot::Absent& a = s.absent[c];
  int64_t param;
  out_columns[c].field.Plan(&a.kind, &param, &a.width);
  std::tie(a.data_off, a.valid_off) = planner.AddAbsentColumn(rows, a.width);
}

void ArrowScan::ZeroAbsentColumn(const Slot& s, size_t c, uint8_t* base, int64_t rows) {
  const Slot::Absent& a = s.absent[c];
  MI_HIP_CHECK(hipMemsetAsync(base + a.data_off, 0, static_cast<size_t>(rows) * static_cast<size_t>(std::max(a.width, 1)), ctx->stream));
  MI_HIP_CHECK(hipMemsetAsync(base + a.valid_off, 0, static_cast<size_t>((rows + 63) / 64) * 8, ctx->stream));
}

void ArrowScan::PlanOutputColumns(Slot& s, BatchPlanner& planner, const BatchPlacement& where, int64_t rows) {
  const Source& src = sources[static_cast<size_t>(s.source)];
  for (size_t c = 0; c < out_columns.size(); c++) {
    if (out_columns[c].is_constant()) continue;
    const int32_t fc = src.out_to_file_column[c];
    if (fc < 0) PlanAbsentColumn(s, planner, c, rows);
    else s.col_root[c] = planner.AddColumn(where, s.batch.column_node[static_cast<size_t>(fc)]);
  }
}

void ArrowScan::BindNodeDicts(Slot& s, const std::vector<PlannedNode>& nodes) {
  s.node_dict.assign(nodes.size(), nullptr);
  for (size_t i = 0; i < nodes.size(); i++)
    if (nodes[i].dict_id >= 0) s.node_dict[i] = dicts[nodes[i].dict_id];
}

void ArrowScan::SendStatusHome(Slot& s, bool with_gather) {
  uint32_t* st = s.h_status.get<uint32_t>();
  MI_HIP_CHECK(hipMemcpyAsync(st, s.plan->d_status.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->d2h_stream));
  if (with_gather) MI_HIP_CHECK(hipMemcpyAsync(st + 1, s.gather_plan->d_status.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->d2h_stream));
  else st[1] = 0;
  MI_HIP_CHECK(hipEventRecord(s.d2h_done, ctx->d2h_stream));
}

// ------------------------------------------------------------------------------------------------ stage A
// Stage A of a record batch: H2D of the body, the full-width decode tasks (every projected column; with compaction only
// the filter columns), the filter, the fused aggregate and -- unless the batch is compacted, which needs the selected row
// count on the host first (stage B) -- the copy back.
void ArrowScan::EnqueueBatch(Slot& s) {
  ctx->Bind();
  const int64_t n = s.batch.length;
  s.nrows = n;
  s.compact = compact && n > 0;
  s.needs_stage_b = false;
  // d_in must be final before tasks take addresses inside it
  const size_t in_bytes = static_cast<size_t>(s.batch.body_size) + 64;
  Retire(Grow(s.d_in, in_bytes, GrownCapacity(in_bytes, s.d_in.size(), 1 << 16)));
  const bool mirror = SetPlannerOptions(s, in_bytes);
  LayOutStageA(s);
  SizeSlotBuffers(s);
  stats.record_batches++;
  s.h_status.get<uint32_t>()[2] = 0;
  UploadBody(s, mirror);
  MI_HIP_CHECK(hipEventRecord(s.h2d_done, ctx->h2d_stream));
  MI_HIP_CHECK(hipStreamWaitEvent(ctx->stream, s.h2d_done, 0));
  LaunchStageA(s);
  MI_HIP_CHECK(hipEventRecord(s.compute_done, ctx->stream));
  MI_HIP_CHECK(hipStreamWaitEvent(ctx->d2h_stream, s.compute_done, 0));
  CopyBackStageA(s);
}

// 1. The planner's options for this batch; returns whether a host consumer needs the pinned mirror of the body (grown here).
bool ArrowScan::SetPlannerOptions(Slot& s, size_t in_bytes) {
  PlannerOptions po;
  po.array_align = kAlign;
  // DirectConversion: a plain fixed-width column without NULLs needs no kernel at all -- its vector IS the
  // Arrow buffer.  For a device-resident consumer that is the HBM copy of the body; for a HOST consumer it is the pinned host
  // body itself, so the column crosses PCIe in neither direction (lineitem: 7 of 16 columns, 46 of 175 B/row in, 46 of 158
  // B/row back).  On unless asked otherwise (-1) -- except while a consumer reads the vectors on the GPU (the fused COPY).
  const bool zero_copy = opts.zero_copy_direct >= 0 && (opts.device_resident || !keep_on_device);
  // a host consumer of a body that only exists decompressed in HBM: string_t rows point into a pinned mirror of the body
  const bool mirror = s.batch.deferred && !opts.device_resident;
  // (mi_scan_aggregate reads the vectors in HBM: a host consumer's alias would be the pinned host body)
  po.zero_copy_direct = zero_copy && !agg.on && !s.compact && !mirror && !(aggn.on && !opts.device_resident);
  if (mirror) Retire(Grow(s.h_mirror, in_bytes, GrownCapacity(in_bytes, s.h_mirror.size(), 1 << 16)));
  po.unset_all_valid = opts.unset_all_valid != 0;
  s.planner.opts = po;
  return mirror;
}

// 2. The arena of stage A.  Full decode: [projected columns | sel | counts] travel back, then the filter-only columns.
//    Compaction: only the filter columns + sel + counts; the projected columns are planned in stage B.
void ArrowScan::LayOutStageA(Slot& s) {
  const DecodedBatch& b = s.batch;
  const Source& src = sources[static_cast<size_t>(s.source)];
  const int64_t n = b.length;
  s.planner.Clear();
  s.col_root.assign(out_columns.size(), -1);
  s.absent.assign(out_columns.size(), {});
  s.filter_root.assign(filter.columns.size(), -1);
  s.node_dict.clear();

  BatchPlacement where = MakePlacement(s);
  // filter columns read their decoded vectors from HBM: never aliased into a body that may not even be uploaded
  std::vector<char> no_alias(b.nodes.size(), 0);
  if (has_filter) {
    for (const int32_t wc : filter.columns) {
      const int32_t fc = src.FileColumn(wc);
      if (fc >= 0) no_alias[static_cast<size_t>(b.column_node[static_cast<size_t>(fc)])] = 1;
    }
    where.no_alias = &no_alias;
  }
  if (!s.compact) PlanOutputColumns(s, s.planner, where, n);
  if (aggn.on) RefuseAbsentAggregateColumns(src);   // before anything of this record batch is queued on the GPU
  if (has_filter) {
    s.sel_off = s.planner.Reserve(static_cast<size_t>(n) * 4 + 16);
    s.sel_count_off = s.planner.Reserve(static_cast<size_t>(WindowsOf(n)) * 4 + 16);
  }
  s.d2h_bytes = (s.compact || aggn.on) ? 0 : s.planner.arena_bytes;   // (the aggregates' vectors never leave HBM)
  if (has_filter) {
    for (size_t k = 0; k < filter.columns.size(); k++) {
      const int32_t wc = filter.columns[k];
      if (wc >= 0 && !s.compact) {
        s.filter_root[k] = s.col_root[static_cast<size_t>(wc)];
        continue;
      }
      const int32_t fc = src.FileColumn(wc);
      if (fc >= 0) s.filter_root[k] = s.planner.AddColumn(where, b.column_node[static_cast<size_t>(fc)]);
    }
  }
  s.stage_a_bytes = s.planner.arena_bytes;
  BindNodeDicts(s, s.planner.nodes);
}

void ArrowScan::RefuseAbsentAggregateColumns(const Source& src) const {
  auto present = [&](int32_t c) {
    if (c >= 0 && src.out_to_file_column[static_cast<size_t>(c)] < 0)
      throw InvalidInputException("aggregate column '" + out_columns[static_cast<size_t>(c)].name + "' is absent from a file of the scan");
  };
  for (const auto& a : aggn.plan.aggs) {
    present(a.col_a);
    present(a.col_b);
    for (const auto& f : a.factors) present(f.col);
  }
  for (const auto& k : aggn.plan.keys)
    if (src.out_to_file_column[static_cast<size_t>(k.col)] < 0)
      throw InvalidInputException("GROUP BY column '" + out_columns[static_cast<size_t>(k.col)].name + "' is absent from a file of the scan");
}

// 3. The slot's buffers for that arena: d_out (with stage B's worst case behind stage A's arrays), h_out, h_counts, the aux
//    tables; then the tasks get their addresses.
void ArrowScan::SizeSlotBuffers(Slot& s) {
  const int64_t n = s.batch.length, n_windows = WindowsOf(n);
  // worst case for stage B: every row selected
  size_t stage_b_worst = 0;
  if (s.compact) {
    stage_b_worst = 4096;
    for (auto& c : out_columns)
      if (!c.is_constant())
        stage_b_worst += AlignUp(static_cast<size_t>(n) * static_cast<size_t>(std::max(WidthOf(c), 1)) + 16) + AlignUp(static_cast<size_t>((n + 63) / 64) * 8 + 8);
  }
  const size_t out_bytes = s.stage_a_bytes + stage_b_worst + 64;
  Retire(Grow(s.d_out, out_bytes, GrownCapacity(out_bytes, s.d_out.size(), 1 << 16)));
  EnsureHostOut(s, s.d2h_bytes + 64);
  Retire(Grow(s.h_counts, static_cast<size_t>(n_windows + 1) * 4, AlignUp(static_cast<size_t>(n_windows + 1) * 8, 4096)));
  UploadAux(s, s.planner.aux);
  s.planner.Rebase(0, s.d_out.get(), s.d_aux.get());
}

// 4. The body into s.d_in.  Compressed (deferred): through the K8 kernels, and for a host consumer the string payload back
//    into the mirror.  Otherwise H2D on the copy stream of only what the kernels read (projected columns; with zero_copy_direct
//    not even all of those): the buffer ranges merged, gaps below 64 KiB are cheaper to copy than to split.  A full scan is one copy.
void ArrowScan::UploadBody(Slot& s, bool mirror) {
  const DecodedBatch& b = s.batch;
  if (b.deferred) {
    EnqueueLz4(s);   // compressed body -> HBM -> K8 kernels -> d_in; ctx->stream waits for them
    if (mirror) MirrorStringPayload(s);
    return;
  }
  const Source& src = sources[static_cast<size_t>(s.source)];
  std::vector<std::pair<int64_t, int64_t>> upload = s.planner.upload;
  if (opts.device_resident)  // aliased vectors of a GPU consumer point into the HBM copy of the body
    for (auto& nd : s.planner.nodes)
      if (nd.alias_body_off >= 0) upload.emplace_back(nd.alias_body_off, nd.nrows * nd.width);
  if (s.compact) {  // stage B reads every projected column
    for (size_t c = 0; c < out_columns.size(); c++) {
      const int32_t fc = out_columns[c].is_constant() ? -1 : src.out_to_file_column[c];
      if (fc < 0) continue;
      for (const auto& sp : b.nodes[static_cast<size_t>(b.column_node[static_cast<size_t>(fc)])].spans)
        if (sp.length > 0) upload.emplace_back(sp.offset, sp.length);
    }
  }
  if (b.body_size > 0) CopyRanges(std::move(upload), b.body, s.d_in.get(), /*align_within*/ b.body_size);
}

// A host consumer of a body expanded in HBM: the payload of every string-like buffer goes back to the host, into the pinned
// mirror the string_t rows point into, as soon as it is decompressed.
void ArrowScan::MirrorStringPayload(Slot& s) {
  for (const DecodedNode& nd : s.batch.nodes) {
    if (!nd.field) continue;
    size_t first = 0, last = 0;   // spans [first, last) hold bytes that string_t rows point at
    switch (nd.field->type) {
      case MI_AT_UTF8: case MI_AT_BINARY: case MI_AT_LARGE_UTF8: case MI_AT_LARGE_BINARY: first = 2; last = 3; break;
      case MI_AT_FIXED_BINARY: first = 1; last = 2; break;
      case MI_AT_UTF8_VIEW: case MI_AT_BINARY_VIEW: first = 2; last = nd.spans.size(); break;
      default: break;
    }
    for (size_t k = first; k < last && k < nd.spans.size(); k++) {
      if (nd.spans[k].length <= 0) continue;
      MI_HIP_CHECK(hipMemcpyAsync(s.h_mirror.get() + nd.spans[k].offset, s.d_in.get() + nd.spans[k].offset, static_cast<size_t>(nd.spans[k].length),
                                  hipMemcpyDeviceToHost, ctx->d2h_stream));
      stats.d2h_bytes += nd.spans[k].length;
    }
  }
}

// 5. On the compute stream, behind the body: all-NULL vectors of absent columns, the decode, the filter, the fused aggregates.
void ArrowScan::LaunchStageA(Slot& s) {
  const DecodedBatch& b = s.batch;
  const Source& src = sources[static_cast<size_t>(s.source)];
  const int64_t n = b.length;
  if (!s.compact && n > 0)
    for (size_t c = 0; c < out_columns.size(); c++)
      if (!out_columns[c].is_constant() && src.out_to_file_column[c] < 0) ZeroAbsentColumn(s, c, s.d_out.get(), n);
  s.plan->Set(s.planner.tasks.data(), static_cast<int32_t>(s.planner.tasks.size()), ctx->stream);
  MI_HIP_CHECK(hipMemsetAsync(s.plan->d_status.get(), 0, sizeof(uint32_t), ctx->stream));
  s.plan->Launch(ctx->stream);
  if (has_filter && n > 0) {
    const device::FilterProgram prog =
        filter.Program(out_columns, {b, s.planner.nodes, s.filter_root, s.node_dict, s.d_in.get(), s.d_out.get(), s.d_out.get() + s.sel_off}, ctx->stream);
    MI_HIP_CHECK(device::LaunchFilterProgram(prog, n, reinterpret_cast<mi_sel_t*>(s.d_out.get() + s.sel_off),
                                             reinterpret_cast<uint32_t*>(s.d_out.get() + s.sel_count_off), ctx->stream));
  }
  if (agg.on && n > 0) EnqueueSumProduct(s);
  if (aggn.on && n > 0) EnqueueAggregates(s);
}

// mi_scan_sum_product's fused consumer: the decoded vectors are read once more by the aggregate kernel and never leave HBM
void ArrowScan::EnqueueSumProduct(Slot& s) {
  device::AggSumProductArgs a;
  std::memset(&a, 0, sizeof(a));
  auto column = [&](int32_t c, const void** data, const uint64_t** valid, int32_t* width) {
    if (s.col_root[static_cast<size_t>(c)] < 0) throw InvalidInputException("aggregate column '" + out_columns[static_cast<size_t>(c)].name + "' is absent from a file of the scan");
    const PlannedNode& o = s.planner.nodes[static_cast<size_t>(s.col_root[static_cast<size_t>(c)])];
    *data = s.d_out.get() + o.data_off;
    *valid = o.valid_off >= 0 ? reinterpret_cast<const uint64_t*>(s.d_out.get() + o.valid_off) : nullptr;
    *width = o.width;
  };
  a.n_filters = static_cast<int32_t>(agg.filter_cols.size());
  for (int32_t k = 0; k < a.n_filters; k++) {
    column(agg.filter_cols[static_cast<size_t>(k)], &a.fcol[k], &a.fvalid[k], &a.fwidth[k]);
    a.lo[k] = agg.lo[static_cast<size_t>(k)];
    a.hi[k] = agg.hi[static_cast<size_t>(k)];
  }
  column(agg.col_a, &a.a, &a.avalid, &a.awidth);
  column(agg.col_b, &a.b, &a.bvalid, &a.bwidth);
  a.nrows = s.batch.length;
  MI_HIP_CHECK(device::LaunchAggSumProduct(a, agg.d_acc.get<unsigned long long>(), ctx->num_cus, ctx->stream));
  agg.rows_scanned += s.batch.length;
}

// 6. On the copy-back stream, behind the kernels: the filter's counts, and -- unless stage B has to come first -- the decoded
//    vectors and the status word.
void ArrowScan::CopyBackStageA(Slot& s) {
  const int64_t n = s.batch.length;
  if (has_filter && n > 0)  // the per-window counts always come back (tiny): chunk sizes, Count(), the stage-B layout
    MI_HIP_CHECK(hipMemcpyAsync(s.h_counts.get<uint32_t>(), s.d_out.get() + s.sel_count_off, static_cast<size_t>(WindowsOf(n)) * 4, hipMemcpyDeviceToHost, ctx->d2h_stream));
  if (s.compact) {
    MI_HIP_CHECK(hipEventRecord(s.filter_done, ctx->d2h_stream));
    s.needs_stage_b = true;
    return;
  }
  s.host_vectors = !opts.device_resident && !agg.on && !aggn.on && s.d2h_bytes > 0 && !keep_on_device;
  if (s.host_vectors) {
    MI_HIP_CHECK(hipMemcpyAsync(s.h_out.get(), s.d_out.get(), s.d2h_bytes, hipMemcpyDeviceToHost, ctx->d2h_stream));
    stats.d2h_bytes += static_cast<int64_t>(s.d2h_bytes);
  }
  for (const auto& nd : s.planner.nodes)
    if (nd.alias_body_off >= 0) stats.aliased_bytes += nd.nrows * nd.width;
  SendStatusHome(s, /*with_gather*/ false);
}

// ------------------------------------------------------------------------------------------------ K8
// The slots share kLz4Streams streams (slot i uses stream i mod 3): the K8 kernels of neighbouring record batches overlap
// -- the token walk is latency-bound and leaves the chip idle -- without every slot holding a hardware queue of its own
// (one stream: 0.65 s for SF10, two 0.42, three 0.39, one per slot (8) 0.46)
// ZSTD: the entropy stage is one serial chain per block (milliseconds, a few lanes busy): more batches side by side
// With hardware queues to spare -- GPU_MAX_HW_QUEUES, which the HIP runtime reads at start-up (default 4), raised by
// the deployment to at least slots + 3 -- every slot gets a stream of its own: 0.24 s instead of 0.29 s at 8 slots
// and 20 queues (profiles/r02/lz4/streams_ab.txt); on the default 4 queues the same choice was the 0.46 s above.
void ArrowScan::ChooseLz4Stream(Slot& s, int32_t codec) {
  int kLz4Streams = codec == 1 ? 16 : 3;
  const int n_slots = static_cast<int>(slots.size());
  if (HardwareQueues() >= n_slots + 3) kLz4Streams = n_slots;
  const int idx = static_cast<int>(&s - slots.data());
  if (idx >= kLz4Streams) {
    Slot& owner = slots[static_cast<size_t>(idx % kLz4Streams)];
    if (!owner.lz4_stream) owner.lz4_stream = owner.own_lz4_stream = HipStream::Create();
    s.lz4_stream = owner.lz4_stream;
  } else {
    s.lz4_stream = s.own_lz4_stream = HipStream::Create();
  }
  s.lz4_done = HipEvent::Create();
}

// K8: the record batch arrived with its LZ4_FRAME buffers still compressed (DecodedBatch::deferred).  The compressed bytes
// cross PCIe, the frames' blocks (tables built by the host reader from the block headers) are expanded into s.d_in at the
// decompressed layout every span of the batch already refers to.
void ArrowScan::EnqueueLz4(Slot& s) {
  const int64_t t_k8 = trace ? TraceNow() : 0;
  const DecodedBatch& b = s.batch;
  const DeferredBody& d = *b.deferred;
  if (!s.lz4_stream) ChooseLz4Stream(s, d.codec);
  const K8Layout l = LayOutK8Scratch(d, static_cast<size_t>(b.body_size));
  Retire(Grow(s.d_lz4, l.arena_bytes, GrownCapacity(l.arena_bytes, s.d_lz4.size(), 1 << 20)));
  Retire(Grow(s.d_comp, l.comp_need, GrownCapacity(l.comp_need, s.d_comp.size(), 1 << 16)));
  Retire(Grow(s.h_lz4, l.tables_bytes, AlignUp(std::max(l.tables_bytes, s.h_lz4.size() * 2), 1 << 16)));   // doubles
  FillK8Tables(d, l, s.h_lz4.get());
  // H2D on the copy stream: the compressed bytes of the needed buffers (neighbours closer than 64 KiB travel as one copy)
  std::vector<std::pair<int64_t, int64_t>> ranges;
  for (auto& f : d.buffers) ranges.emplace_back(f.comp_off, f.comp_len);
  if (d.codec == 1) stats.zstd_batches_on_device++;
  else stats.lz4_batches_on_device++;
  stats.decompressed_bytes += b.body_size;
  CopyRanges(std::move(ranges), d.comp, s.d_comp.get(), /*align_within*/ -1);
  MI_HIP_CHECK(hipMemcpyAsync(s.d_lz4.get(), s.h_lz4.get(), l.tables_bytes, hipMemcpyHostToDevice, ctx->h2d_stream));
  MI_HIP_CHECK(hipEventRecord(s.h2d_done, ctx->h2d_stream));
  hipStream_t q = s.lz4_stream;
  MI_HIP_CHECK(hipStreamWaitEvent(q, s.h2d_done, 0));
  // ONE memset per record batch: counters, status, marks.  The link words need none (every word a stage reads was written
  // by the stage before it), nor does the body: the bytes between its buffers are padding nobody reads.
  MI_HIP_CHECK(hipMemsetAsync(s.d_lz4.get() + l.tables_bytes, 0, l.counters_end - l.tables_bytes, q));
  for (auto& f : d.buffers)   // a raw buffer has no blocks: its bytes are copied
    if (f.raw && f.out_len > 0)
      MI_HIP_CHECK(hipMemcpyAsync(s.d_in.get() + f.out_off, s.d_comp.get() + f.comp_off, static_cast<size_t>(f.out_len), hipMemcpyDeviceToDevice, q));
  device::Lz4Args a;
  FillK8Args(d, l, s.d_lz4.get(), s.d_comp.get(), s.d_in.get(), &a);
  const int64_t t_launch = trace ? TraceNow() : 0;
  MI_HIP_CHECK(device::LaunchLz4Decompress(a, ctx->num_cus, q));
  if (trace) {
    tr_k8_prep_ns += t_launch - t_k8;
    tr_k8_launch_ns += TraceNow() - t_launch;
  }
  MI_HIP_CHECK(hipMemcpyAsync(s.h_status.get<uint32_t>() + 2, a.status, sizeof(uint32_t), hipMemcpyDeviceToHost, q));
  MI_HIP_CHECK(hipMemcpyAsync(s.h_status.get<uint32_t>() + 4, a.round_left + 37, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, q));
  s.lz4_counted = false;
  MI_HIP_CHECK(hipEventRecord(s.lz4_done, q));
  MI_HIP_CHECK(hipStreamWaitEvent(ctx->stream, s.lz4_done, 0));
  MI_HIP_CHECK(hipStreamWaitEvent(ctx->d2h_stream, s.lz4_done, 0));
}

// ------------------------------------------------------------------------------------------------ stage B
// Stage B of a compacted batch: the filter's counts are on the host, so the projected columns get a dense layout sized
// for the rows that survived; the gather kernel decodes exactly those and only they travel back.
void ArrowScan::EnqueueStageB(Slot& s) {
  ctx->Bind();
  MI_HIP_CHECK(hipEventSynchronize(s.filter_done));
  const int64_t n_windows = WindowsOf(s.batch.length);
  int64_t total = 0;
  for (int64_t w = 0; w < n_windows; w++) total += s.h_counts.get<uint32_t>()[w];
  s.needs_stage_b = false;
  // a fresh planner pass for the projected columns: arena offsets relative to the compact region behind stage A's arrays
  BatchPlanner cp(s.planner.opts);
  cp.opts.zero_copy_direct = false;
  BatchPlacement where = MakePlacement(s);
  where.alloc_rows = total;
  s.col_root.assign(out_columns.size(), -1);
  PlanOutputColumns(s, cp, where, total);
  s.d2h_bytes = cp.arena_bytes;
  const size_t region_off = AlignUp(s.stage_a_bytes, 4096);
  if (region_off + cp.arena_bytes + 64 > s.d_out.size()) throw InternalException("compact region exceeds the slot");
  uint8_t* region = s.d_out.get() + region_off;
  EnsureHostOut(s, s.d2h_bytes + 64);
  cp.Rebase(0, region, nullptr);
  for (auto& t : cp.tasks) {
    t.sel = s.d_out.get() + s.sel_off;
    t.sel_count = s.d_out.get() + s.sel_count_off;
  }
  hipStream_t st = ctx->stream;
  // validity words start as all ones (the gather kernel clears the NULLs); absent columns are all NULL
  for (size_t c = 0; c < out_columns.size(); c++) {
    if (out_columns[c].is_constant() || total == 0) continue;
    if (s.col_root[c] < 0) {
      ZeroAbsentColumn(s, c, region, total);
      continue;
    }
    const PlannedNode& pn = cp.nodes[static_cast<size_t>(s.col_root[c])];
    if (pn.valid_off >= 0) MI_HIP_CHECK(hipMemsetAsync(region + pn.valid_off, 0xFF, static_cast<size_t>((total + 63) / 64) * 8 + 8, st));
  }
  s.gather_plan->Set(cp.tasks.data(), static_cast<int32_t>(total > 0 ? cp.tasks.size() : 0), st);
  MI_HIP_CHECK(hipMemsetAsync(s.gather_plan->d_status.get(), 0, sizeof(uint32_t), st));
  if (total > 0) s.gather_plan->Launch(st);
  MI_HIP_CHECK(hipEventRecord(s.compute_done, st));
  MI_HIP_CHECK(hipStreamWaitEvent(ctx->d2h_stream, s.compute_done, 0));
  if (!opts.device_resident && s.d2h_bytes > 0 && total > 0) {
    MI_HIP_CHECK(hipMemcpyAsync(s.h_out.get(), region, s.d2h_bytes, hipMemcpyDeviceToHost, ctx->d2h_stream));
    stats.d2h_bytes += static_cast<int64_t>(s.d2h_bytes);
  }
  SendStatusHome(s, /*with_gather*/ true);
  // the chunk builder reads the compact layout from here on
  BindNodeDicts(s, cp.nodes);
  s.compact_region = region;
  s.planner.nodes = std::move(cp.nodes);
}

}  // namespace miarrow
