// scan_operator.cpp -- see scan_operator.hpp.
#include "scan_operator.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>

namespace miarrow {

int WrapC(const std::function<void()>& f);  // c_api.cpp

namespace {
// a buffer that lives as long as any of the shared pointers to its memory (dictionary versions keep them)
template <typename Buffer>
std::shared_ptr<void> Shared(size_t bytes) {
  auto b = std::make_shared<Buffer>(bytes);
  return std::shared_ptr<void>(b, b->get());
}

std::map<std::string, std::string> ParseHive(const std::string& path) {
  // key=value path components (DuckDB's HivePartitioning::Parse behaviour for simple keys)
  std::map<std::string, std::string> out;
  size_t start = 0;
  while (start < path.size()) {
    size_t end = path.find_first_of("/\\", start);
    if (end == std::string::npos) break;  // the last component is the file name
    std::string part = path.substr(start, end - start);
    size_t eq = part.find('=');
    if (eq != std::string::npos && eq > 0 && eq + 1 < part.size()) out[part.substr(0, eq)] = part.substr(eq + 1);
    start = end + 1;
  }
  return out;
}

mi_string_t MakeHostString(const std::string& s) {
  mi_string_t r;
  std::memset(&r, 0, sizeof(r));
  r.value.inlined.length = static_cast<uint32_t>(s.size());
  if (s.size() <= 12) {
    std::memcpy(r.value.inlined.inlined, s.data(), s.size());
  } else {
    std::memcpy(r.value.pointer.prefix, s.data(), 4);
    r.value.pointer.ptr = reinterpret_cast<uint64_t>(s.data());
  }
  return r;
}

std::vector<std::string> AtLeastOne(std::vector<std::string> paths) {
  if (paths.empty()) throw InvalidInputException("read_arrow needs at least one file");
  return paths;
}
int PipelineDepth(const mi_scan_options& o) { return std::max(2, std::min(kMaxDepth, o.pipeline_depth > 0 ? o.pipeline_depth : 3)); }
}  // namespace

ArrowScan::ArrowScan(Context* ctx_p, std::vector<std::string> paths, const mi_scan_options& o) : ArrowScan(ctx_p, AtLeastOne(std::move(paths)), {}, o) {}
ArrowScan::ArrowScan(Context* ctx_p, std::vector<ArrowIPCBuffer> buffers, const mi_scan_options& o) : ArrowScan(ctx_p, {}, std::move(buffers), o) {}

ArrowScan::ArrowScan(Context* ctx_p, std::vector<std::string> paths, std::vector<ArrowIPCBuffer> buffers, const mi_scan_options& o)
    : ctx(ctx_p), opts(o), sources(std::max<size_t>(paths.size(), 1)), is_buffers(paths.empty()),
      readahead(paths, std::move(buffers), o, kMaxDepth,
                ReadAhead::Hooks{[this](size_t bytes, uint8_t** ptr) {
                                   ctx->Bind();
                                   std::shared_ptr<void> mem = Shared<PinnedBuffer>(bytes);
                                   *ptr = static_cast<uint8_t*>(mem.get());
                                   return mem;
                                 },
                                 [this] {
                                   ctx->Bind();
                                   ctx->BindThisThread();
                                 },
                                 [this](size_t si, const ArrowSchemaModel& schema) { return MapColumns(si, schema); }}) {
  if (opts.hive_partitioning)
    for (size_t i = 0; i < paths.size(); i++) sources[i].hive = ParseHive(paths[i]);
  slots.resize(static_cast<size_t>(PipelineDepth(opts)));
}

ArrowScan::~ArrowScan() {
  readahead.Stop();
  if (trace)
    std::fprintf(stderr, "mi scan trace: %lld batches, %.2f in flight after a submit, %.2f ms from a submit to its batch being handed out; pipeline thread: enqueue %.3f s (K8: tables and copies %.3f s, launches %.3f s), waiting for input %.3f s, waiting for the GPU %.3f s, polling %.3f s; "
                         "producers (%d, summed): reading %.3f s, queue full %.3f s, no staging buffer %.3f s\n",
                 static_cast<long long>(stats.record_batches), stats.record_batches ? double(tr_inflight_sum) / stats.record_batches : 0.0,
                 stats.record_batches ? tr_latency_ns * 1e-6 / stats.record_batches : 0.0, tr_enqueue_ns * 1e-9, tr_k8_prep_ns * 1e-9, tr_k8_launch_ns * 1e-9, tr_fetch_wait_ns * 1e-9, tr_event_wait_ns * 1e-9, tr_poll_ns * 1e-9, readahead.Producers(),
                 readahead.ReadSeconds(), readahead.PushWaitSeconds(), readahead.LeaseWaitSeconds());
  try {
    ctx->Bind();
  } catch (...) {
  }
  // The device is done with every buffer before any of them goes (the members, after this body).  The batches in the
  // slots and in the read-ahead queues hold staging leases, whose release marks the staging buffer free: they go first
  // (the slots' here, the queues' when the read-ahead, the last member, is the first to go).
  (void)hipStreamSynchronize(ctx->h2d_stream);
  (void)hipStreamSynchronize(ctx->stream);
  (void)hipStreamSynchronize(ctx->d2h_stream);
  for (auto& s : slots)
    if (s.lz4_stream) (void)hipStreamSynchronize(s.lz4_stream);   // a borrowed stream: its owner is still alive
  for (auto& s : slots) s.batch = DecodedBatch();
}

const std::vector<ScanColumn>& ArrowScan::Bind() {
  if (bound) return all_columns;
  // schema of the first file (ArrowFileScan ctor, arrow_file_scan.cpp:9-23); union_by_name visits every file
  auto add_file_columns = [&](size_t si, bool first) {
    const ArrowSchemaModel& schema = readahead.Schema(si);   // opens the file
    std::vector<std::string> names;
    for (auto& f : schema.fields) names.push_back(f.name);
    DeduplicateColumns(names);
    for (size_t c = 0; c < schema.fields.size(); c++) {
      auto it = std::find_if(all_columns.begin(), all_columns.end(), [&](const ScanColumn& sc) { return sc.name == names[c]; });
      if (it == all_columns.end()) {
        if (!first && !opts.union_by_name) continue;
        ScanColumn sc;
        sc.name = names[c];
        sc.field = schema.fields[c];
        all_columns.push_back(std::move(sc));
      }
    }
  };
  add_file_columns(0, true);
  if (opts.union_by_name) {
    for (size_t i = 1; i < sources.size(); i++) add_file_columns(i, false);
  }
  if (all_columns.empty()) {
    throw InvalidInputException("Provided table/dataframe must have at least one column");
  }
  if (opts.filename && !is_buffers) {
    ScanColumn sc;
    sc.name = "filename";
    sc.is_filename = true;
    sc.field.type = MI_AT_UTF8;
    sc.field.name = "filename";
    all_columns.push_back(sc);
  }
  if (opts.hive_partitioning && !is_buffers) {
    for (auto& kv : sources[0].hive) {
      ScanColumn sc;
      sc.name = kv.first;
      sc.is_hive = true;
      sc.hive_key = kv.first;
      sc.field.type = MI_AT_UTF8;
      sc.field.name = kv.first;
      all_columns.push_back(sc);
    }
  }
  bound = true;
  return all_columns;
}

void ArrowScan::SetFilter(FilterCnf cnf) {
  if (initialized) throw InvalidInputException("set the filter before mi_scan_init");
  filter.cnf.insert(filter.cnf.end(), cnf.begin(), cnf.end());   // a second filter is ANDed with the first
  size_t leaves = 0;
  for (auto& c : filter.cnf) leaves += c.size();
  if (leaves > static_cast<size_t>(device::kMaxFilterLeaves))
    throw NotImplementedException("filter needs more than " + std::to_string(device::kMaxFilterLeaves) + " leaves");
  has_filter = true;
}

void ArrowScan::Init(const std::vector<std::string>& projected) {
  Bind();
  out_columns.clear();
  if (projected.empty()) {
    out_columns = all_columns;
  } else {
    for (auto& name : projected) {
      auto it = std::find_if(all_columns.begin(), all_columns.end(), [&](const ScanColumn& sc) { return sc.name == name; });
      if (it == all_columns.end()) throw InternalException(std::string("Field '") + name + "' does not exist in IPC file schema");
      out_columns.push_back(*it);
    }
  }
  for (auto& c : out_columns) {
    if (c.is_constant()) continue;
    std::string why;
    if (!c.field.Supported(&why)) {
      throw NotImplementedException("Column '" + c.name + "': " + why + " is not decoded by the MI355X scan path yet");
    }
    if (c.field.has_dictionary && !opts.accept_dictionaries) {
      // the reference cannot read dictionary-encoded IPC at all (base_stream_reader.cpp:86-96)
      throw NotImplementedException("Column '" + c.name + "' is dictionary-encoded; enable accept_dictionaries");
    }
  }
  all_valid.assign(MI_VECTOR_SIZE / 64, ~0ull);
  ctx->Bind();
  compact = false;
  if (has_filter) {
    filter.Resolve(all_columns, out_columns);
    filter.UploadConstants();
    if (opts.filter_compact && !aggn.on) {   // mi_scan_aggregate materialises nothing for a consumer
      for (auto& c : out_columns) {
        if (c.is_constant()) continue;
        int32_t kind, w;
        int64_t param;
        c.field.Plan(&kind, &param, &w);
        if (!device::KindCanGather(kind) || !c.field.children.empty())
          throw NotImplementedException("filter_compact needs flat projected columns: '" + c.name + "' (" + c.field.DuckType() +
                                        ") is decoded window by window, use the selection vector instead");
      }
      compact = true;
    }
  }
  for (auto& s : slots) InitSlot(s);
  initialized = true;
}

void ArrowScan::InitSlot(Slot& s) {
  if (s.h2d_done) return;
  ctx->Bind();
  s.h2d_done = HipEvent::Create();
  s.compute_done = HipEvent::Create();
  s.d2h_done = HipEvent::Create();
  s.filter_done = HipEvent::Create();
  s.plan = std::make_unique<Plan>(ctx);
  s.gather_plan = std::make_unique<Plan>(ctx);
  s.h_status = PinnedBuffer(64);
  uint32_t* st = s.h_status.get<uint32_t>();
  st[0] = st[1] = st[2] = 0;
}

// More record batches in flight / held by the caller at once (the COPY pump hands whole batches to several sink threads).
// Takes effect only before the first batch has been requested: the read-ahead thread sizes its staging ring from the slot
// count (a pump that asks later works with the slots there are: it waits for a release when all of them are held).
void ArrowScan::EnsurePipelineDepth(int depth) {
  depth = std::min(depth, kMaxDepth);
  if (static_cast<int>(slots.size()) >= depth) return;
  if (readahead.Started() || !inflight.empty()) return;   // a scan that has started keeps the depth it has
  GrowSlots(static_cast<size_t>(depth));
}

// (only the pipeline thread touches the slots; the rest of the scan names them by index)
void ArrowScan::GrowSlots(size_t n) {
  std::vector<Slot> bigger(n);
  for (size_t i = 0; i < slots.size(); i++) bigger[i] = std::move(slots[i]);
  slots = std::move(bigger);
  if (initialized)
    for (auto& s : slots) InitSlot(s);   // (those that came along keep what they have)
}

ArrowScan::Slot* ArrowScan::FreeSlot() {
  for (auto& s : slots)
    if (!s.busy) return &s;
  return nullptr;
}

void ArrowScan::DecodeDictionary(const DecodedBatch& b) {
  ctx->Bind();
  if (b.column_node.empty() || b.nodes.empty()) throw InternalException("DictionaryBatch without a value node");
  const ArrowField& f = *b.nodes[static_cast<size_t>(b.column_node[0])].field;  // the field that carries the id (any depth)
  int32_t kind, w;
  int64_t param;
  if (!f.Plan(&kind, &param, &w, /*value_only*/ true))
    throw NotImplementedException("Dictionary value type " + f.Format() + " is not decoded by the MI355X scan path");
  if (!DictionaryKindIsFlat(kind))
    throw NotImplementedException("Dictionary of value type " + f.Format() + " (field '" + f.name +
                                  "') is not decoded by the MI355X scan path: only flat value types are");
  // isDelta: the new values are appended to the existing dictionary (indices keep their meaning); otherwise the
  // dictionary is replaced.  Either way a NEW version is built; batches already in flight keep theirs.
  std::shared_ptr<DictState> old = dicts.count(b.dict_id) ? dicts[b.dict_id] : nullptr;
  const bool delta = b.is_delta && old;
  if (delta && old->kind != kind) throw IOException("Delta dictionary changes the value type");
  auto d = std::make_shared<DictState>();
  const int64_t n_new = b.column_length[0];
  const int64_t n_old = delta ? old->dict_len : 0;
  const int64_t n = n_old + n_new;
  d->dict_len = n;
  d->kind = kind;
  d->out_width = w;
  if (delta) {
    d->d_heaps = old->d_heaps;
    d->host_bodies = old->host_bodies;
  }
  if (b.owner) d->host_bodies.push_back(b.owner);
  const size_t data_bytes = AlignUp(static_cast<size_t>(n + 1) * static_cast<size_t>(w));
  const size_t valid_bytes = AlignUp(static_cast<size_t>((n + 1 + 63) / 64) * 8);
  // Nothing below waits for the device: the body goes up on the copy stream, the values are decoded on the compute stream
  // behind it (the record batches that use the dictionary follow on the same stream), the decode's status word comes back
  // with the first such batch (DictState::h_status, checked in AcquireBatch).  The validity words are built on the host.
  d->d_data = DeviceBuffer(data_bytes);
  d->d_validity = DeviceBuffer(valid_bytes);
  d->h_words = PinnedBuffer(valid_bytes);
  d->h_status = PinnedBuffer(64);
  d->h_status.get<uint32_t>()[0] = 0;
  MI_HIP_CHECK(hipMemsetAsync(d->d_data.get(), 0, data_bytes, ctx->stream));
  uint8_t* heap = nullptr;
  if (b.body_size > 0) {
    d->d_heaps.push_back(Shared<DeviceBuffer>(AlignUp(static_cast<size_t>(b.body_size) + 16)));
    heap = static_cast<uint8_t*>(d->d_heaps.back().get());
    // the body is pinned (the read-ahead's allocator for DICTIONARY_BATCH messages) and lives in host_bodies
    MI_HIP_CHECK(hipMemcpyAsync(heap, b.body, static_cast<size_t>(b.body_size), hipMemcpyHostToDevice, ctx->h2d_stream));
    if (!d->uploaded) d->uploaded = HipEvent::Create();
    MI_HIP_CHECK(hipEventRecord(d->uploaded, ctx->h2d_stream));
    MI_HIP_CHECK(hipStreamWaitEvent(ctx->stream, d->uploaded, 0));
  }
  if (n_old > 0)
    MI_HIP_CHECK(hipMemcpyAsync(d->d_data.get(), old->d_data.get(), static_cast<size_t>(n_old) * static_cast<size_t>(w), hipMemcpyDeviceToDevice, ctx->stream));
  if (n_new > 0) {
    // decode the new values into a tile-aligned scratch vector, then append (the scratch lives as long as the version:
    // freeing it here would wait for the device)
    d->d_heaps.push_back(Shared<DeviceBuffer>(AlignUp(static_cast<size_t>(n_new) * static_cast<size_t>(w) + 16)));
    void* scratch_data = d->d_heaps.back().get();
    mi_col_task t;
    std::memset(&t, 0, sizeof(t));
    const mi_buffer_span* sp = &b.buffers[0];
    t.validity = sp[0].length ? heap + sp[0].offset : nullptr;
    t.buf1 = heap + sp[1].offset;
    const bool payload = f.Layout(/*value_only*/ true).n > 2;   // strings: offsets in buffer 1, their bytes in buffer 2
    t.buf2 = payload ? heap + sp[2].offset : nullptr;
    t.buf2_len = payload ? sp[2].length : 0;
    t.out_data = scratch_data;
    t.out_validity = nullptr;   // built on the host, below
    const int64_t data_off = payload ? sp[2].offset : sp[1].offset;
    t.ptr_base = opts.device_resident ? reinterpret_cast<uint64_t>(heap + data_off) : reinterpret_cast<uint64_t>(b.body + data_off);
    t.nrows = n_new;
    t.null_count = b.null_count[0];
    t.kind = kind;
    t.param = param;
    d->decode_plan = std::make_unique<Plan>(ctx, &t, 1);
    d->decode_plan->Launch(ctx->stream);
    MI_HIP_CHECK(hipMemcpyAsync(d->d_data.get() + static_cast<size_t>(n_old) * static_cast<size_t>(w), scratch_data,
                                static_cast<size_t>(n_new) * static_cast<size_t>(w), hipMemcpyDeviceToDevice, ctx->stream));
    MI_HIP_CHECK(hipMemcpyAsync(d->h_status.get(), d->decode_plan->d_status.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  }
  // The host side (scan_dictionary.cpp): the validity words, and for string-valued and FLOAT / DOUBLE / 128-bit dictionaries
  // the values themselves -- pushed-down predicates are matched against the dictionary once and against the rows by index
  uint64_t* words = d->h_words.get<uint64_t>();
  BuildDictionaryHost(b, kind, w, param, FilterClassOf(f) != FilterValueClass::kOther, delta ? old.get() : nullptr, words, valid_bytes / 8, d.get());
  words[static_cast<size_t>(n >> 6)] &= ~(1ull << (n & 63));  // the extra NULL entry at index dict_len (ColumnArrowToDuckDBDictionary)
  MI_HIP_CHECK(hipMemcpyAsync(d->d_validity.get(), words, valid_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (!opts.device_resident) {
    // host consumers read the values from pinned memory: the copy rides the compute stream too, and every batch that uses
    // the dictionary is handed out only after its own results have come back behind it
    d->h_data = PinnedBuffer(data_bytes);
    MI_HIP_CHECK(hipMemcpyAsync(d->h_data.get(), d->d_data.get(), data_bytes, hipMemcpyDeviceToHost, ctx->stream));
    d->h_validity = words;   // the same pinned words
  }
  dicts[b.dict_id] = d;
}

// The vector of node `node` for chunk window `window`, children included.  Full layout: rows win[window] .. win[window + 1]
// of the node; compacted batches: rows [2048 window, 2048 window + compact_rows) of the dense arrays.
void ArrowScan::BuildVector(const Slot& s, int32_t node, size_t window, int64_t compact_rows, uint8_t* base, ChunkStorage* st, mi_vector* v) {
  const PlannedNode& o = s.planner.nodes[static_cast<size_t>(node)];
  std::memset(v, 0, sizeof(*v));
  const int64_t r0 = compact_rows >= 0 ? static_cast<int64_t>(window) * MI_VECTOR_SIZE : o.win[window];
  const int64_t r1 = compact_rows >= 0 ? r0 + compact_rows : o.win[window + 1];
  if (o.alias_body_off >= 0) {
    const uint8_t* body = opts.device_resident ? s.d_in.get() : s.batch.body;
    v->data = const_cast<uint8_t*>(body) + o.alias_body_off + static_cast<size_t>(r0) * static_cast<size_t>(o.width);
    v->validity = nullptr;  // all valid
  } else {
    v->data = base + o.data_off + static_cast<size_t>(r0) * static_cast<size_t>(o.width);
    if (o.valid_off >= 0) {
      v->validity = reinterpret_cast<mi_validity_t*>(base + o.valid_off) + r0 / 64;
      v->validity_shift = static_cast<int32_t>(r0 % 64);
    }
  }
  v->kind = o.kind;
  v->out_width = o.width;
  v->count = r1 - r0;
  const int32_t vk = o.kind == MI_K_RUN_END || o.kind == MI_K_UNION_DENSE ? o.value_kind : o.kind;  // run-end encoded, dense union member: the values' string heap
  if (IsStringKind(vk)) {
    v->heap = reinterpret_cast<const void*>(o.ptr_base);
    v->heap_size = o.heap_size;
  }
  if (o.kind == MI_K_DICT && s.node_dict[static_cast<size_t>(node)]) {
    const DictState& d = *s.node_dict[static_cast<size_t>(node)];
    v->dictionary = opts.device_resident ? d.d_data.get() : d.h_data.get();
    v->dictionary_validity = static_cast<const mi_validity_t*>(opts.device_resident ? d.d_validity.get() : d.h_validity);
    v->dict_len = d.dict_len;
  }
  if (!o.children.empty()) {
    if (st->child_pool_used + o.children.size() > st->child_pool.size()) throw InternalException("nested vector pool exhausted");
    mi_vector* kids = st->child_pool.data() + st->child_pool_used;
    st->child_pool_used += o.children.size();
    for (size_t k = 0; k < o.children.size(); k++) BuildVector(s, o.children[k], window, -1, base, st, &kids[k]);
    v->children = kids;
    v->n_children = static_cast<int32_t>(o.children.size());
  }
}

// Per-file column mapping by name (DuckDB's multi-file column mapping): where every output and filter-only column lies in
// the batches of file `si`, and with that the columns its readers project.
std::vector<std::string> ArrowScan::MapColumns(size_t si, const ArrowSchemaModel& schema) {
  Source& src = sources[si];
  const std::string& path = readahead.Path(si);
  std::vector<std::string> names;
  for (auto& f : schema.fields) names.push_back(f.name);
  DeduplicateColumns(names);
  std::vector<std::string> wanted;
  auto map_column = [&](const ScanColumn& col) -> int32_t {
    auto it = std::find(names.begin(), names.end(), col.name);
    if (it == names.end()) {
      if (!opts.union_by_name) {
        throw InvalidInputException("Failed to read file \"" + path + "\": schema mismatch: column \"" + col.name +
                                    "\" is missing. If you are trying to read files with different schemas, try setting union_by_name=True");
      }
      return -1;
    }
    const ArrowField& ff = schema.fields[static_cast<size_t>(it - names.begin())];
    if (ff.Format() != col.field.Format()) {
      throw NotImplementedException("Column \"" + col.name + "\" has type " + ff.DuckType() + " in file \"" + path +
                                    "\" but " + col.field.DuckType() +
                                    " in the first file; cross-file casts are done by DuckDB's MultiFileReader above this path");
    }
    auto dup = std::find(wanted.begin(), wanted.end(), *it);
    if (dup != wanted.end()) return static_cast<int32_t>(dup - wanted.begin());
    wanted.push_back(*it);
    return static_cast<int32_t>(wanted.size() - 1);
  };
  src.out_to_file_column.assign(out_columns.size(), -1);
  for (size_t c = 0; c < out_columns.size(); c++)
    if (!out_columns[c].is_constant()) src.out_to_file_column[c] = map_column(out_columns[c]);
  src.filter_to_file_column.assign(filter.only.size(), -1);
  for (size_t c = 0; c < filter.only.size(); c++) src.filter_to_file_column[c] = map_column(filter.only[c]);
  return wanted;
}

bool ArrowScan::SubmitNextBatch(bool may_block) {
  if (!readahead.Started()) {
    trace = std::getenv("MI_SCAN_TRACE") != nullptr;
    readahead.Start(trace);
  }
  while (!exhausted) {
    Slot* slot = FreeSlot();
    if (!slot) return false;
    Fetched f;
    const int64_t t0 = trace && may_block ? TraceNow() : 0;
    if (!readahead.Take(&f, may_block)) return false;
    if (trace && may_block) tr_fetch_wait_ns += TraceNow() - t0;
    if (f.error) {
      exhausted = true;
      std::rethrow_exception(f.error);
    }
    if (f.end) {
      exhausted = true;
      return false;
    }
    if (f.batch.is_dictionary) {
      DecodeDictionary(f.batch);
      continue;
    }
    if (f.batch.deferred && opts.pipeline_depth == 0) {
      // compressed bodies that are expanded in HBM spend 0.5 (LZ4) to 5 ms (ZSTD) in latency-bound kernels that leave the chip
      // nearly idle: a caller who left the depth to the scan gets as many record batches side by side as that takes
      const size_t wanted = f.batch.deferred->codec == 1 ? 16 : 8;
      if (slots.size() < wanted) {
        GrowSlots(wanted);
        slot = FreeSlot();
      }
    }
    Slot& s = *slot;
    s.batch = std::move(f.batch);
    s.source = f.source;
    s.batch_index = f.ordinal;
    s.busy = true;
    try {
      const int64_t t0 = trace ? TraceNow() : 0;
      EnqueueBatch(s);
      if (trace) {
        s.tr_enqueued_ns = TraceNow();
        tr_enqueue_ns += s.tr_enqueued_ns - t0;
        tr_inflight_sum += static_cast<int64_t>(inflight.size()) + 1;
      }
    } catch (...) {
      s.busy = false;
      s.batch = DecodedBatch();
      throw;
    }
    inflight.push_back(static_cast<int>(&s - slots.data()));
    return true;
  }
  return false;
}

bool ArrowScan::AcquireBatch(BatchRef* out) {
  if (!initialized) Init({});
  ctx->Bind();
  for (;;) {
    // keep the pipeline full (blocks for input only when nothing is in flight: the batch the caller needs next)
    while (FreeSlot() != nullptr && SubmitNextBatch(/*may_block*/ inflight.empty())) {
    }
    // compacted batches whose selected-row counts have arrived get their second stage, in batch order
    for (size_t k = 0; k < inflight.size(); k++) {
      Slot& s = slots[static_cast<size_t>(inflight[k])];
      if (!s.needs_stage_b) continue;
      if (k == 0 || hipEventQuery(s.filter_done) == hipSuccess) EnqueueStageB(s);
      else break;
    }
    if (inflight.empty()) return false;  // exhausted
    Slot& front = slots[static_cast<size_t>(inflight.front())];
    // Wait for the batch the caller needs.  While slots are free and the input is not exhausted, keep an eye on the producers
    // instead of sleeping in the event: a scan whose record batches spend milliseconds on the GPU (compressed bodies in HBM,
    // 16 slots) otherwise submits only what the producers had ready at the moment of this call -- their queues hold a few
    // batches -- and then waits a whole batch time with most slots idle.
    if (exhausted || FreeSlot() == nullptr) {
      const int64_t t0 = trace ? TraceNow() : 0;
      MI_HIP_CHECK(hipEventSynchronize(front.d2h_done));
      if (trace) tr_event_wait_ns += TraceNow() - t0;
      break;
    }
    const hipError_t q = hipEventQuery(front.d2h_done);
    if (q == hipSuccess) break;
    if (q != hipErrorNotReady) MI_HIP_CHECK(q);
    const int64_t t0 = trace ? TraceNow() : 0;
    readahead.WaitReady(std::chrono::microseconds(100));
    if (trace) tr_poll_ns += TraceNow() - t0;
  }
  const int si = inflight.front();
  Slot& s = slots[static_cast<size_t>(si)];
  inflight.pop_front();
  if (trace) tr_latency_ns += TraceNow() - s.tr_enqueued_ns;
  try {
    const uint32_t* st = s.h_status.get<uint32_t>();
    if (s.batch.deferred && !s.lz4_counted) {
      s.lz4_counted = true;
      stats.lz4_blocks += st[4];
      stats.lz4_parse_rounds += st[6];
      stats.lz4_parse_rounds_max = std::max<int64_t>(stats.lz4_parse_rounds_max, st[5]);
    }
    uint32_t dict_status = 0;   // the decode of the dictionary versions this batch uses ran in front of it on the same stream
    for (auto& nd : s.node_dict)
      if (nd && nd->h_status) dict_status |= nd->h_status.get<uint32_t>()[0];
    ThrowForStatus(st[0] | st[1] | st[2] | dict_status);
  } catch (...) {
    s.busy = false;
    s.batch.owner.reset();
    throw;
  }
  out->slot = si;
  out->batch_index = s.batch_index;
  out->nrows = s.nrows;
  out->source = s.source;
  out->selected = s.nrows;
  if (has_filter) {
    out->selected = 0;
    const int64_t n_windows = (s.nrows + MI_VECTOR_SIZE - 1) / MI_VECTOR_SIZE;
    for (int64_t w = 0; w < n_windows; w++) out->selected += s.h_counts.get<uint32_t>()[w];
  }
  out->chunk_rows = s.compact ? out->selected : s.nrows;
  out->n_windows = static_cast<int32_t>((out->chunk_rows + MI_VECTOR_SIZE - 1) / MI_VECTOR_SIZE);
  return true;
}

void ArrowScan::ReleaseBatch(const BatchRef& ref) {
  Slot& s = slots[static_cast<size_t>(ref.slot)];
  s.busy = false;
  s.batch.owner.reset();
}

void ArrowScan::EnsureHostVectors(const BatchRef& ref) {
  Slot& s = slots[static_cast<size_t>(ref.slot)];
  if (s.host_vectors || opts.device_resident || s.compact || s.d2h_bytes == 0) return;
  ctx->Bind();
  MI_HIP_CHECK(hipMemcpy(s.h_out.get(), s.d_out.get(), s.d2h_bytes, hipMemcpyDeviceToHost));
  stats.d2h_bytes += static_cast<int64_t>(s.d2h_bytes);
  s.host_vectors = true;
}

void ArrowScan::DeviceColumn(const BatchRef& ref, size_t c, DeviceColumnView* out) const {
  *out = DeviceColumnView();
  const Slot& s = slots[static_cast<size_t>(ref.slot)];
  if (s.compact || s.batch.deferred || c >= out_columns.size() || out_columns[c].is_constant() || s.col_root[c] < 0) return;
  const PlannedNode& pn = s.planner.nodes[static_cast<size_t>(s.col_root[c])];
  if (!pn.children.empty() || pn.dict_id >= 0 || pn.source_node < 0) return;
  if (pn.alias_body_off >= 0 && !opts.device_resident) return;   // aliased into the HOST body: not in HBM at all
  const DecodedNode& dn = s.batch.nodes[static_cast<size_t>(pn.source_node)];
  out->kind = pn.kind;
  out->width = pn.width;
  out->null_count = pn.null_count;
  out->d_data = pn.alias_body_off >= 0 ? s.d_in.get() + pn.alias_body_off : s.d_out.get() + pn.data_off;
  out->d_validity = (pn.valid_off >= 0 && pn.null_count != 0) ? s.d_out.get() + pn.valid_off : nullptr;
  if (pn.null_count != 0 && pn.valid_off < 0) return;
  if (pn.kind == MI_K_STR32 || pn.kind == MI_K_STR64) {
    if (dn.spans.size() < 3) return;
    out->offset_width = pn.kind == MI_K_STR64 ? 8 : 4;
    out->d_heap = s.d_in.get() + dn.spans[2].offset;
    out->ptr_base = pn.ptr_base;
    out->h_offsets = s.batch.body + dn.spans[1].offset;
    out->h_validity = dn.spans[0].length > 0 ? s.batch.body + dn.spans[0].offset : nullptr;
  }
  if (pn.kind == MI_K_UUID) out->h_validity = dn.spans[0].length > 0 ? s.batch.body + dn.spans[0].offset : nullptr;   // (sizes its text)
  out->flat = true;
}

void ArrowScan::BuildChunk(const BatchRef& ref, int32_t window, ChunkStorage* st, mi_data_chunk* out) {
  const Slot& s = slots[static_cast<size_t>(ref.slot)];
  std::memset(out, 0, sizeof(*out));
  const int64_t chunk_rows = s.compact ? ref.selected : s.nrows;
  const int64_t row0 = static_cast<int64_t>(window) * MI_VECTOR_SIZE;
  const int64_t n = std::min<int64_t>(MI_VECTOR_SIZE, chunk_rows - row0);
  if (window < 0 || n <= 0) throw InvalidInputException("chunk window outside the record batch");
  uint8_t* base = opts.device_resident ? (s.compact ? s.compact_region : s.d_out.get()) : s.h_out.get();
  st->vectors.assign(out_columns.size(), mi_vector{});
  if (st->child_pool.size() < s.planner.nodes.size() + 1) st->child_pool.resize(s.planner.nodes.size() + 1);
  st->child_pool_used = 0;
  const Source& src = sources[static_cast<size_t>(s.source)];
  for (size_t c = 0; c < out_columns.size(); c++) {
    mi_vector& v = st->vectors[c];
    if (out_columns[c].is_constant()) {
      // strings are kept alive in the source (path / hive map), one vector of 2048 copies per (file, column)
      const std::string& stable = out_columns[c].is_filename ? readahead.Path(static_cast<size_t>(s.source)) : src.hive.at(out_columns[c].hive_key);
      const mi_string_t* cv;
      {
        std::lock_guard<std::mutex> lk(const_mu);
        auto& vec = const_vectors[{s.source, c}];
        if (vec.empty()) vec.assign(MI_VECTOR_SIZE, MakeHostString(stable));
        cv = vec.data();
      }
      v.data = const_cast<mi_string_t*>(cv);
      v.validity = all_valid.data();
      v.kind = MI_K_STR32;
      v.out_width = 16;
      v.count = n;
      continue;
    }
    if (s.col_root[c] >= 0) {
      BuildVector(s, s.col_root[c], static_cast<size_t>(window), s.compact ? n : -1, base, st, &v);
    } else {  // absent in this file: all NULL
      const Slot::Absent& a = s.absent[c];
      v.data = base + a.data_off + static_cast<size_t>(row0) * static_cast<size_t>(std::max(a.width, 1));
      v.validity = reinterpret_cast<mi_validity_t*>(base + a.valid_off) + row0 / 64;
      v.kind = a.kind;
      v.out_width = a.width;
      v.count = n;
    }
  }
  out->size = n;
  out->n_columns = static_cast<int32_t>(out_columns.size());
  out->file_index = s.source;
  out->batch_index = s.batch_index;
  out->chunk_offset = row0;
  out->columns = st->vectors.data();
  out->sel_count = n;
  out->source_rows = s.compact ? (window == 0 ? s.nrows : 0) : n;
  if (has_filter && !s.compact) {
    out->sel = reinterpret_cast<const mi_sel_t*>(base + s.sel_off) + row0;
    out->sel_count = s.h_counts.get<uint32_t>()[window];
  }
}

void ArrowScan::Next(mi_data_chunk* out) {
  if (!initialized) Init({});
  std::memset(out, 0, sizeof(*out));
  while (true) {
    if (have_cur && cur_window >= cur_ref.n_windows) {  // the previous chunk was the batch's last: recycle its slot
      ReleaseBatch(cur_ref);
      have_cur = false;
    }
    if (have_cur) break;
    if (!AcquireBatch(&cur_ref)) {
      out->size = 0;
      out->n_columns = static_cast<int32_t>(out_columns.size());
      return;  // exhausted
    }
    have_cur = true;
    cur_window = 0;  // an empty (or, when compacting, fully filtered) batch has no windows: the loop moves on
  }
  BuildChunk(cur_ref, cur_window, &next_storage, out);
  cur_window++;
}

void ArrowScan::Count(int64_t* rows, int64_t* selected, int64_t* chunks) {
  if (!initialized) Init({});
  int64_t r = 0, sel = 0, n = 0;
  if (have_cur) {  // mid-batch after mi_scan_next: the rest of the current batch counts chunk by chunk
    mi_data_chunk ch;
    while (cur_window < cur_ref.n_windows) {
      BuildChunk(cur_ref, cur_window++, &next_storage, &ch);
      r += ch.source_rows;
      sel += ch.sel ? ch.sel_count : ch.size;
      n++;
    }
    ReleaseBatch(cur_ref);
    have_cur = false;
  }
  BatchRef ref;
  while (AcquireBatch(&ref)) {   // whole batches: no chunk is materialised for a count
    r += ref.nrows;
    sel += ref.selected;
    n += ref.n_windows;
    ReleaseBatch(ref);
  }
  if (rows) *rows = r;
  if (selected) *selected = sel;
  if (chunks) *chunks = n;
}

void ArrowScan::SumProduct(const std::string& a, const std::string& b, const std::vector<std::string>& filter_columns_p,
                           const std::vector<int64_t>& lo, const std::vector<int64_t>& hi, mi_sum_product_result* out) {
  if (initialized) throw InvalidInputException("mi_scan_sum_product replaces mi_scan_init / mi_scan_next: call it right after bind");
  if (filter_columns_p.size() > 4) throw InvalidInputException("at most 4 range filters");
  if (has_filter) throw InvalidInputException("give the filters to mi_scan_sum_product instead of mi_scan_set_filter");
  ctx->Bind();
  // project exactly the columns the aggregate reads
  std::vector<std::string> proj;
  auto slot_of = [&](const std::string& name) {
    for (size_t i = 0; i < proj.size(); i++)
      if (proj[i] == name) return static_cast<int32_t>(i);
    proj.push_back(name);
    return static_cast<int32_t>(proj.size() - 1);
  };
  agg.col_a = slot_of(a);
  agg.col_b = slot_of(b);
  agg.filter_cols.clear();
  for (auto& f : filter_columns_p) agg.filter_cols.push_back(slot_of(f));
  agg.lo = lo;
  agg.hi = hi;
  Init(proj);
  for (auto& name : proj) {
    const ScanColumn& c = out_columns[static_cast<size_t>(slot_of(name))];
    int32_t kind, w;
    int64_t param;
    if (!(!c.is_constant() && c.field.Plan(&kind, &param, &w) && IsIntegerLike(kind, w, c.field, /*allow_bool*/ false))) throw InvalidInputException("Column '" + name + "' (" + c.field.DuckType() + ") is not a fixed-width integer-like column: the fused aggregate takes integers, DATE, TIME/TIMESTAMP and DECIMAL(<=18)");
    // the kernel loads every value sign-extended: a uint16 60000 would be summed and range-tested as -5536
    if (c.field.type == MI_AT_INT && !c.field.is_signed)
      throw NotImplementedException("Column '" + name + "' (" + c.field.DuckType() + ") is unsigned: mi_scan_sum_product reads signed columns only; "
                                    "mi_scan_aggregate (MI_AGG_SUM_PRODUCT over mi_scan_set_filter) handles unsigned columns at the same speed");
  }
  agg.d_acc = DeviceBuffer(4 * sizeof(unsigned long long));
  MI_HIP_CHECK(hipMemsetAsync(agg.d_acc.get(), 0, agg.d_acc.size(), ctx->stream));
  agg.on = true;
  agg.rows_scanned = 0;
  try {
    BatchRef ref;
    while (AcquireBatch(&ref)) ReleaseBatch(ref);   // the pull loop only recycles slots: nothing is copied back
    unsigned long long acc[4] = {0, 0, 0, 0};
    MI_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MI_HIP_CHECK(hipMemcpy(acc, agg.d_acc.get(), sizeof(acc), hipMemcpyDeviceToHost));
    out->sum_lo = acc[0];
    out->sum_hi = static_cast<int64_t>(acc[1]);
    out->rows_selected = static_cast<int64_t>(acc[2]);
    out->rows_scanned = agg.rows_scanned;
  } catch (...) {
    agg.on = false;
    throw;
  }
  agg.on = false;
}

double ArrowScan::Progress() { return readahead.Progress(); }

void ArrowScan::Stats(mi_scan_stats* out) {
  out->record_batches += stats.record_batches;
  out->lz4_batches_on_device += stats.lz4_batches_on_device;
  out->h2d_bytes += stats.h2d_bytes;
  out->decompressed_bytes += stats.decompressed_bytes;
  out->lz4_blocks += stats.lz4_blocks;
  out->lz4_parse_rounds += stats.lz4_parse_rounds;
  out->lz4_parse_rounds_max = std::max(out->lz4_parse_rounds_max, stats.lz4_parse_rounds_max);
  out->zstd_batches_on_device += stats.zstd_batches_on_device;
  out->d2h_bytes += stats.d2h_bytes;
  out->aliased_bytes += stats.aliased_bytes;
}

}  // namespace miarrow

// ------------------------------------------------------------------------------------------------ C ABI
using namespace miarrow;

namespace miarrow {
Context* ContextOf(mi_ctx* c);
}

struct mi_scan {
  std::unique_ptr<ScanBase> scan;
  ArrowScan* single = nullptr;  // the scan when it is not a multi-device one (the COPY pump pulls whole batches from it)
};

namespace miarrow {
ArrowScan* SingleScanOf(mi_scan* s) { return s ? s->single : nullptr; }
ScanBase* ScanOf(mi_scan* s) { return s ? s->scan.get() : nullptr; }   // (the aggregate calls of scan_aggregate.cpp)
}  // namespace miarrow

namespace {
// the mi_scan_open_* calls: the options (all zero when the caller gives none), the scan `make` builds from them, the handle
template <typename Make>
void OpenScan(const mi_scan_options* opts, mi_scan** out, Make make) {
  mi_scan_options o;
  std::memset(&o, 0, sizeof(o));
  if (opts) o = *opts;
  auto s = std::make_unique<mi_scan>();
  auto scan = make(o);
  s->single = dynamic_cast<ArrowScan*>(scan.get());
  s->scan = std::move(scan);
  *out = s.release();
}
}  // namespace

extern "C" {

int mi_scan_open_files(mi_ctx* ctx, const char* const* paths, int32_t n_paths, const mi_scan_options* opts, mi_scan** out) {
  return WrapC([&] {
    if (!ctx || !paths || n_paths <= 0 || !out) throw InvalidInputException("mi_scan_open_files: bad argument");
    OpenScan(opts, out, [&](const mi_scan_options& o) {
      return std::make_unique<ArrowScan>(ContextOf(ctx), std::vector<std::string>(paths, paths + n_paths), o);
    });
  });
}

int mi_scan_open_files_multi(mi_ctx* const* ctxs, int32_t n_ctxs, const char* const* paths, int32_t n_paths,
                             const mi_scan_options* opts, mi_scan** out) {
  return WrapC([&] {
    if (!ctxs || n_ctxs <= 0 || !paths || n_paths <= 0 || !out) throw InvalidInputException("mi_scan_open_files_multi: bad argument");
    OpenScan(opts, out, [&](const mi_scan_options& o) {
      std::vector<Context*> cs;
      for (int32_t i = 0; i < n_ctxs; i++) cs.push_back(ContextOf(ctxs[i]));
      return std::make_unique<MultiDeviceScan>(cs, std::vector<std::string>(paths, paths + n_paths), o);
    });
  });
}

int mi_scan_open_buffers(mi_ctx* ctx, const mi_ipc_buffer* buffers, int32_t n_buffers, const mi_scan_options* opts, mi_scan** out) {
  return WrapC([&] {
    if (!ctx || (!buffers && n_buffers) || n_buffers < 0 || !out) throw InvalidInputException("mi_scan_open_buffers: bad argument");
    OpenScan(opts, out, [&](const mi_scan_options& o) {
      std::vector<ArrowIPCBuffer> v;
      for (int32_t i = 0; i < n_buffers; i++) v.emplace_back(buffers[i].ptr, buffers[i].size);
      return std::make_unique<ArrowScan>(ContextOf(ctx), std::move(v), o);
    });
  });
}

void mi_scan_close(mi_scan* s) { delete s; }

int mi_scan_bind(mi_scan* s, mi_field* fields, int32_t cap, int32_t* n_fields) {
  return WrapC([&] {
    if (!s || !n_fields) throw InvalidInputException("mi_scan_bind: NULL argument");
    const auto& cols = s->scan->Bind();
    *n_fields = static_cast<int32_t>(cols.size());
    for (size_t i = 0; i < cols.size() && fields && static_cast<int32_t>(i) < cap; i++) {
      FillCField(cols[i].field, static_cast<int32_t>(i), &fields[i]);
      std::snprintf(fields[i].name, sizeof(fields[i].name), "%s", cols[i].name.c_str());
    }
  });
}

int mi_scan_init(mi_scan* s, const char* const* projected_names, int32_t n_projected) {
  return WrapC([&] {
    if (!s) throw InvalidInputException("mi_scan_init: NULL scan");
    std::vector<std::string> v;
    for (int32_t i = 0; i < n_projected; i++) v.emplace_back(projected_names[i]);
    s->scan->Init(v);
  });
}

int mi_scan_set_filter(mi_scan* s, const mi_filter_node* nodes, int32_t n_nodes, int32_t root) {
  return WrapC([&] {
    if (!s || !nodes) throw InvalidInputException("mi_scan_set_filter: NULL argument");
    // the bind result tells what each leaf's constants are compared as (FLOAT / DOUBLE keys, 128-bit integers)
    const std::vector<ScanColumn>& columns = s->scan->Bind();
    s->scan->SetFilter(NormaliseFilter(nodes, n_nodes, root, &columns));
  });
}

int mi_scan_set_filter_range(mi_scan* s, const char* column, int64_t lo, int64_t hi) {
  return WrapC([&] {
    if (!s || !column) throw InvalidInputException("mi_scan_set_filter_range: NULL argument");
    mi_filter_node nodes[3];
    std::memset(nodes, 0, sizeof(nodes));
    nodes[0].op = MI_F_AND;
    nodes[0].first_child = 1;
    nodes[0].n_children = 2;
    nodes[1].op = MI_F_GE;
    nodes[1].column = column;
    nodes[1].value = lo;
    nodes[2].op = MI_F_LT;
    nodes[2].column = column;
    nodes[2].value = hi;
    s->scan->SetFilter(NormaliseFilter(nodes, 3, 0));
  });
}

int mi_scan_next(mi_scan* s, mi_data_chunk* out) {
  return WrapC([&] {
    if (!s || !out) throw InvalidInputException("mi_scan_next: NULL argument");
    s->scan->Next(out);
  });
}

int mi_scan_count(mi_scan* s, int64_t* rows, int64_t* selected, int64_t* chunks) {
  return WrapC([&] {
    if (!s) throw InvalidInputException("mi_scan_count: NULL argument");
    s->scan->Count(rows, selected, chunks);
  });
}

int mi_scan_sum_product(mi_scan* s, const char* column_a, const char* column_b, const mi_range_filter* filters,
                        int32_t n_filters, mi_sum_product_result* out) {
  return WrapC([&] {
    if (!s || !column_a || !column_b || !out || (n_filters > 0 && !filters)) throw InvalidInputException("mi_scan_sum_product: NULL argument");
    std::vector<std::string> cols;
    std::vector<int64_t> lo, hi;
    for (int32_t i = 0; i < n_filters; i++) {
      if (!filters[i].column) throw InvalidInputException("mi_scan_sum_product: filter without a column");
      cols.emplace_back(filters[i].column);
      lo.push_back(filters[i].lo);
      hi.push_back(filters[i].hi);
    }
    std::memset(out, 0, sizeof(*out));
    s->scan->SumProduct(column_a, column_b, cols, lo, hi, out);
  });
}

double mi_scan_progress(mi_scan* s) { return s ? s->scan->Progress() : 0; }

int mi_scan_get_stats(mi_scan* s, mi_scan_stats* out) {
  return WrapC([&] {
    if (!s || !out) throw InvalidInputException("mi_scan_get_stats: NULL argument");
    std::memset(out, 0, sizeof(*out));
    s->scan->Stats(out);
  });
}

}  // extern "C"
