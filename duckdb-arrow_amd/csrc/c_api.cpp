// c_api.cpp -- the extern "C" boundary (include/mi_arrow_ipc.h).  Nothing throws across it: exceptions are mapped
// to errno-style codes + a thread-local message, the way IpcArrayStream::Wrap does at the reference's C stream
// boundary (src/include/ipc/array_stream.hpp:29-48).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/mi_arrow_ipc.h"
#include "engine.hpp"
#include "filter_key.hpp"
#include "ipc_format.hpp"
#include "ipc_stream_reader.hpp"
#include "like_match.hpp"
#include "scan_aggregate.hpp"
#include "scan_operator.hpp"
#include "writer.hpp"

using namespace miarrow;

namespace {
thread_local std::string g_last_error;

template <typename F>
int Wrap(F&& f) {
  try {
    f();
    return MI_OK;
  } catch (const Exception& e) {
    g_last_error = e.what();
    return e.code;
  } catch (const std::bad_alloc&) {
    g_last_error = "out of memory";
    return MI_ENOMEM;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return MI_EINVAL;
  }
}
}  // namespace

struct mi_reader {
  std::unique_ptr<IPCStreamReader> reader;
  DecodedBatch batch;
  std::vector<mi_batch_node> nodes;
  std::vector<mi_buffer_span> node_spans;
  std::vector<mi_batch_index_entry> index;
};
struct mi_ctx {
  std::unique_ptr<Context> ctx;
};
namespace miarrow {
// the reader moves into an exported Arrow C stream (c_stream.cpp); the handle stays valid for mi_reader_close only
std::unique_ptr<IPCStreamReader> TakeReader(mi_reader* r) { return std::move(r->reader); }
}  // namespace miarrow
static IPCStreamReader& Live(mi_reader* r) {
  if (!r || !r->reader) throw InvalidInputException("the reader was exported as an Arrow C stream (or is NULL): only mi_reader_close is valid");
  return *r->reader;
}
struct mi_plan {
  std::unique_ptr<Plan> plan;
};

extern "C" {

const char* mi_last_error(void) { return g_last_error.c_str(); }
const char* mi_version(void) { return "mi_arrow_ipc 2 gfx950 0.7.0-SNAPSHOT"; }
// nanoarrow_version() (src/nanoarrow_extension.cpp:20-31) returns the linked nanoarrow's version; the metadata
// dialect implemented here is the one of apache/arrow-nanoarrow@4bf5a932 = "0.7.0-SNAPSHOT" (test/sql/nanoarrow.test:18).
const char* mi_nanoarrow_version(void) { return "0.7.0-SNAPSHOT"; }

// ------------------------------------------------------------------------------------------------ readers
int mi_reader_open_file(const char* path, mi_reader** out) {
  return Wrap([&] {
    if (!path || !out) throw InvalidInputException("mi_reader_open_file: NULL argument");
    auto r = std::make_unique<mi_reader>();
    r->reader = std::make_unique<IPCFileStreamReader>(path);
    *out = r.release();
  });
}

int mi_reader_open_buffers(const mi_ipc_buffer* buffers, int32_t n_buffers, mi_reader** out) {
  return Wrap([&] {
    if ((!buffers && n_buffers) || !out || n_buffers < 0) throw InvalidInputException("mi_reader_open_buffers: bad argument");
    std::vector<ArrowIPCBuffer> v;
    for (int32_t i = 0; i < n_buffers; i++) v.emplace_back(buffers[i].ptr, buffers[i].size);
    auto r = std::make_unique<mi_reader>();
    r->reader = std::make_unique<IPCBufferStreamReader>(std::move(v));
    *out = r.release();
  });
}

void mi_reader_close(mi_reader* r) { delete r; }

int mi_reader_schema(mi_reader* r, mi_field* fields, int32_t cap, int32_t* n_fields) {
  return Wrap([&] {
    if (!r || !n_fields) throw InvalidInputException("mi_reader_schema: NULL argument");
    const ArrowSchemaModel& s = Live(r).GetBaseSchema();
    *n_fields = static_cast<int32_t>(s.fields.size());
    int64_t flat = 0;
    for (size_t i = 0; i < s.fields.size(); i++) {
      if (fields && static_cast<int32_t>(i) < cap) FillCField(s.fields[i], static_cast<int32_t>(flat), &fields[i]);
      flat += s.fields[i].CountFields();
    }
  });
}

int mi_reader_schema_metadata(mi_reader* r, int32_t idx, const char** key, int32_t* key_len, const char** value,
                              int32_t* value_len, int32_t* count) {
  return Wrap([&] {
    if (!r) throw InvalidInputException("mi_reader_schema_metadata: NULL reader");
    const ArrowSchemaModel& s = Live(r).GetBaseSchema();
    if (count) *count = static_cast<int32_t>(s.metadata.size());
    if (idx < 0 || static_cast<size_t>(idx) >= s.metadata.size()) {
      if (key || value) throw InvalidInputException("schema metadata index out of range");
      return;
    }
    if (key) *key = s.metadata[static_cast<size_t>(idx)].first.data();
    if (key_len) *key_len = static_cast<int32_t>(s.metadata[static_cast<size_t>(idx)].first.size());
    if (value) *value = s.metadata[static_cast<size_t>(idx)].second.data();
    if (value_len) *value_len = static_cast<int32_t>(s.metadata[static_cast<size_t>(idx)].second.size());
  });
}

int mi_reader_set_projection(mi_reader* r, const char* const* names, int32_t n) {
  return Wrap([&] {
    if (!r) throw InvalidInputException("mi_reader_set_projection: NULL reader");
    std::vector<std::string> v;
    for (int32_t i = 0; i < n; i++) v.emplace_back(names[i]);
    Live(r).SetColumnProjection(v);
  });
}

int mi_reader_next_batch(mi_reader* r, int32_t accept_dictionaries, mi_batch* out) {
  bool got = false;
  int rc = Wrap([&] {
    if (!r || !out) throw InvalidInputException("mi_reader_next_batch: NULL argument");
    got = Live(r).GetNextBatch(&r->batch, accept_dictionaries != 0);
    if (!got) return;
    const DecodedBatch& b = r->batch;
    out->length = b.length;
    out->body = b.body;
    out->body_size = b.body_size;
    out->body_file_offset = b.body_file_offset;
    out->n_columns = static_cast<int32_t>(b.column_field.size());
    out->is_dictionary = b.is_dictionary;
    out->dict_id = b.dict_id;
    out->is_delta = b.is_delta;
    out->compression = b.compression;
    out->column_field = b.column_field.data();
    out->null_count = b.null_count.data();
    out->buffers = b.buffers.data();
    r->nodes.clear();
    r->node_spans.clear();
    for (auto& nd : b.nodes) {
      mi_batch_node c;
      std::memset(&c, 0, sizeof(c));
      std::snprintf(c.name, sizeof(c.name), "%s", nd.field->name.c_str());
      c.arrow_type = nd.field->type;
      int32_t kind = 0, w = 0;
      int64_t param = 0;
      if (nd.field->Plan(&kind, &param, &w, nd.value_only)) {
        c.kind = kind;
        c.out_width = w;
        c.param = param;
      }
      c.parent = nd.parent;
      c.depth = nd.depth;
      c.n_children = static_cast<int32_t>(nd.children.size());
      c.first_span = static_cast<int32_t>(r->node_spans.size());
      c.n_spans = static_cast<int32_t>(nd.spans.size());
      c.length = nd.length;
      c.null_count = nd.null_count;
      r->node_spans.insert(r->node_spans.end(), nd.spans.begin(), nd.spans.end());
      r->nodes.push_back(c);
    }
    out->n_nodes = static_cast<int32_t>(r->nodes.size());
    out->nodes = r->nodes.data();
    out->node_spans = r->node_spans.data();
    out->column_node = b.column_node.data();
  });
  if (rc != MI_OK) return rc;
  return got ? MI_OK : MI_ENODATA;
}

double mi_reader_progress(mi_reader* r) { return (r && r->reader) ? r->reader->GetProgress() : 0; }

int mi_reader_index(mi_reader* r, const mi_batch_index_entry** entries, int32_t* n) {
  return Wrap([&] {
    if (!r || !entries || !n) throw InvalidInputException("mi_reader_index: NULL argument");
    const auto& idx = Live(r).BuildIndex();
    r->index.clear();
    for (auto& e : idx) r->index.push_back(mi_batch_index_entry{e.prefix_offset, e.meta_len, e.type, e.body_offset, e.body_len, e.n_rows});
    *entries = r->index.data();
    *n = static_cast<int32_t>(r->index.size());
  });
}

// ------------------------------------------------------------------------------------------------ device
// The HIP runtime multiplexes every stream of a process onto GPU_MAX_HW_QUEUES hardware queues (4 unless the variable says
// otherwise) and reads the variable ONCE, when it initialises at the process's first HIP call.  The compressed-body scans (K8)
// are sets of latency-bound kernels that want the record batches of many pipeline slots side by side, each slot on a stream of
// its own: on 4 queues their kernels queue up behind one another (ZSTD, SF10: 0.63 s against 0.34 s).  So when the
// library is loaded and nobody has chosen a value, it asks for 24 -- 16 slots + the context's three streams, and a few for
// whatever else in the process makes streams (with torch beside it the scan lost a fifth on 20) -- effective when the library
// is loaded before the process touches HIP (a DuckDB process loading the extension; bench.py and the tools import the
// package first), a no-op otherwise; an explicit GPU_MAX_HW_QUEUES in the environment always wins.
namespace {
__attribute__((constructor)) void MiRuntimeDefaults() { (void)setenv("GPU_MAX_HW_QUEUES", "24", /*overwrite*/ 0); }
}  // namespace

int mi_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int mi_ctx_create(int32_t device_id, mi_ctx** out) {
  return Wrap([&] {
    if (!out) throw InvalidInputException("mi_ctx_create: NULL out");
    auto c = std::make_unique<mi_ctx>();
    c->ctx = std::make_unique<Context>(device_id);
    *out = c.release();
  });
}

void mi_ctx_destroy(mi_ctx* ctx) { delete ctx; }

int mi_ctx_numa(mi_ctx* ctx, int32_t* node, char* cpulist, int32_t cap) {
  return Wrap([&] {
    if (!ctx || !node) throw InvalidInputException("mi_ctx_numa: NULL argument");
    *node = ctx->ctx->numa_node;
    if (cpulist && cap > 0) {
      const std::string& l = ctx->ctx->local_cpulist;
      const size_t n = std::min(l.size(), static_cast<size_t>(cap - 1));
      std::memcpy(cpulist, l.data(), n);
      cpulist[n] = 0;
    }
  });
}

int mi_plan_create(mi_ctx* ctx, const mi_col_task* tasks, int32_t n_tasks, mi_plan** out) {
  return Wrap([&] {
    if (!ctx || !out || n_tasks < 0 || (!tasks && n_tasks)) throw InvalidInputException("mi_plan_create: bad argument");
    auto p = std::make_unique<mi_plan>();
    p->plan = std::make_unique<Plan>(ctx->ctx.get(), tasks, n_tasks);
    *out = p.release();
  });
}

void mi_plan_destroy(mi_plan* plan) { delete plan; }

int mi_plan_launch(mi_plan* plan, void* stream) {
  return Wrap([&] {
    if (!plan) throw InvalidInputException("mi_plan_launch: NULL plan");
    plan->plan->Launch(static_cast<hipStream_t>(stream));
  });
}

int mi_plan_status(mi_plan* plan, uint32_t* status_bits) {
  return Wrap([&] {
    if (!plan || !status_bits) throw InvalidInputException("mi_plan_status: NULL argument");
    *status_bits = plan->plan->Status();
  });
}

int mi_plan_stats(const mi_plan* plan, int64_t* bytes_read, int64_t* bytes_written, int64_t* rows, int64_t* tiles) {
  return Wrap([&] {
    if (!plan) throw InvalidInputException("mi_plan_stats: NULL plan");
    if (bytes_read) *bytes_read = plan->plan->bytes_read;
    if (bytes_written) *bytes_written = plan->plan->bytes_written;
    if (rows) *rows = plan->plan->rows;
    if (tiles) *tiles = plan->plan->total_tiles;
  });
}

int mi_plan_class_stats(const mi_plan* plan, int32_t cls, int64_t* bytes_read, int64_t* bytes_written, int64_t* rows,
                        int64_t* tiles, const char** kernel_name) {
  return Wrap([&] {
    if (!plan || cls < 0 || cls >= device::kNumClasses) throw InvalidInputException("mi_plan_class_stats: bad argument");
    if (bytes_read) *bytes_read = plan->plan->class_bytes_read[cls];
    if (bytes_written) *bytes_written = plan->plan->class_bytes_written[cls];
    if (rows) *rows = plan->plan->class_rows[cls];
    if (tiles) *tiles = plan->plan->class_tiles[cls];
    if (kernel_name) *kernel_name = device::KernelNameOfClass(cls);
  });
}

int mi_plan_launch_timed(mi_plan* plan, void* stream, float* ms_per_class) {
  return Wrap([&] {
    if (!plan || !ms_per_class) throw InvalidInputException("mi_plan_launch_timed: NULL argument");
    plan->plan->LaunchTimed(static_cast<hipStream_t>(stream), ms_per_class);
  });
}

int mi_plan_null_counts(mi_plan* plan, int64_t* out, int32_t n_tasks) {
  return Wrap([&] {
    if (!plan || !out) throw InvalidInputException("mi_plan_null_counts: NULL argument");
    auto v = plan->plan->NullCounts(/*reset*/ true);
    if (static_cast<size_t>(n_tasks) != v.size()) throw InvalidInputException("mi_plan_null_counts: task count mismatch");
    std::memcpy(out, v.data(), v.size() * sizeof(int64_t));
  });
}

int mi_status_to_error(uint32_t status_bits) {
  return Wrap([&] { ThrowForStatus(status_bits); });
}

int mi_filter_range(mi_ctx* ctx, const void* values, int32_t width, const void* validity, int64_t nrows, int64_t lo,
                    int64_t hi, mi_sel_t* sel_out, uint32_t* count_out, void* stream) {
  return Wrap([&] {
    if (!ctx || !values || !sel_out || !count_out) throw InvalidInputException("mi_filter_range: NULL argument");
    if (width != 1 && width != 2 && width != 4 && width != 8) throw InvalidInputException("mi_filter_range: width must be 1, 2, 4 or 8");
    ctx->ctx->Bind();
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->ctx->stream;
    MI_HIP_CHECK(device::LaunchFilterRange(values, width, validity, nrows, lo, hi, sel_out, count_out, s));
  });
}

int mi_filter_between(mi_ctx* ctx, const void* values, int32_t width, const void* validity, int64_t nrows, int32_t value_kind,
                      const int64_t* bounds, mi_sel_t* sel_out, uint32_t* count_out, void* stream) {
  return Wrap([&] {
    if (!ctx || !values || !bounds || !sel_out || !count_out) throw InvalidInputException("mi_filter_between: NULL argument");
    const bool is_float = value_kind == MI_FV_DOUBLE && (width == 4 || width == 8), is_wide = value_kind == MI_FV_INT128 && width == 16;
    if (!is_float && !is_wide) throw InvalidInputException("mi_filter_between: MI_FV_DOUBLE takes width 4 or 8, MI_FV_INT128 width 16");
    ctx->ctx->Bind();
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->ctx->stream;
    device::FilterProgram prog;
    std::memset(&prog, 0, sizeof(prog));
    prog.n_leaves = 1;
    device::FilterLeafDev& L = prog.leaves[0];
    L.data = values;
    L.validity = static_cast<const uint64_t*>(validity);
    L.width = width;
    L.flags = device::kLeafEndsClause;
    if (is_float) {
      double lo, hi;
      std::memcpy(&lo, &bounds[0], 8);
      std::memcpy(&hi, &bounds[1], 8);
      L.op = device::kLeafRange;
      L.flags |= device::kLeafFloat;
      L.lo = filterkey::FloatKeyOfDouble(lo, width);
      L.hi = filterkey::FloatKeyOfDouble(hi, width);
      MI_HIP_CHECK(device::LaunchFilterProgram(prog, nrows, sel_out, count_out, s));
      return;
    }
    DeviceBuffer d_bounds(32);
    MI_HIP_CHECK(hipMemcpy(d_bounds.get(), bounds, 32, hipMemcpyHostToDevice));
    L.op = device::kLeafWideRange;
    L.in_values = d_bounds.get<int64_t>();
    MI_HIP_CHECK(device::LaunchFilterProgram(prog, nrows, sel_out, count_out, s));
    MI_HIP_CHECK(hipStreamSynchronize(s));   // the bounds die with this call
  });
}

int mi_filter_string(mi_ctx* ctx, const void* rows, const void* validity, int64_t nrows, const void* heap, uint64_t ptr_base, int32_t op,
                     const char* str_value, int32_t str_len, mi_sel_t* sel_out, uint32_t* count_out, int32_t launches, float* ms) {
  return Wrap([&] {
    if (!ctx || !rows || !sel_out || !count_out || launches < 1) throw InvalidInputException("mi_filter_string: NULL argument or no launch");
    if (op == MI_F_IN || op == MI_F_AND || op == MI_F_OR || op == MI_F_IS_NULL || op == MI_F_IS_NOT_NULL || !str_value)
      throw InvalidInputException("mi_filter_string: one comparison of a string_t vector with one byte string");
    ctx->ctx->Bind();
    mi_filter_node node;
    std::memset(&node, 0, sizeof(node));
    node.op = op;
    node.column = "rows";
    node.str_value = str_value;
    node.str_len = str_len;
    BoundFilter filter;
    filter.cnf = NormaliseFilter(&node, 1, 0);
    filter.UploadConstants();
    device::FilterProgram prog;
    std::memset(&prog, 0, sizeof(prog));
    prog.n_leaves = 1;
    device::FilterLeafDev& L = prog.leaves[0];
    LeafConstants(filter.cnf[0][0], filter.d_in_lists[0], true, L);
    L.data = rows;
    L.validity = static_cast<const uint64_t*>(validity);
    L.width = 16;
    L.lo = static_cast<int64_t>(reinterpret_cast<uintptr_t>(heap));
    L.hi = static_cast<int64_t>(ptr_base);
    hipStream_t s = ctx->ctx->stream;
    const HipEvent begin = HipEvent::CreateTimed(), end = HipEvent::CreateTimed();
    MI_HIP_CHECK(hipEventRecord(begin, s));
    for (int32_t i = 0; i < launches; i++) MI_HIP_CHECK(device::LaunchFilterProgram(prog, nrows, sel_out, count_out, s));
    MI_HIP_CHECK(hipEventRecord(end, s));
    MI_HIP_CHECK(hipStreamSynchronize(s));   // the constants die with this call
    float total = 0;
    MI_HIP_CHECK(hipEventElapsedTime(&total, begin, end));
    if (ms) *ms = total / static_cast<float>(launches);
  });
}

namespace {
//! the expression of vector spec `a` into exprs->exprs[a] and desc->a (the first column factor's column: its class is the
//! expression's), for the call `api` names in its messages; what is left to check is device::AggProgramIsValid's
void VectorExprOf(const char* api, const mi_agg_vector_spec& spec, device::AggDescDev* desc, device::AggExprDev* out) {
  const mi_agg_vector_expr* e = spec.expr;
  if (!e) throw InvalidInputException(std::string(api) + ": SUM_EXPR without an expression");
  if (e->n_factors < 1 || e->n_factors > MI_MAX_EXPR_FACTORS)
    throw InvalidInputException(std::string(api) + ": SUM_EXPR takes 1 to " + std::to_string(MI_MAX_EXPR_FACTORS) + " factors, not " + std::to_string(e->n_factors));
  auto is_constant = [](const mi_agg_vector_factor& f) { return f.column.data == nullptr && f.column.value_class == MI_AGG_CLASS_ANY; };
  const mi_agg_vector_factor* first = nullptr;
  for (int32_t f = 0; f < e->n_factors && !first; f++)
    if (!is_constant(e->factors[f])) first = &e->factors[f];
  if (!first) throw InvalidInputException(std::string(api) + ": SUM_EXPR needs at least one factor with a column");
  const bool is_float = first->column.value_class == MI_AGG_CLASS_FLOAT;
  std::memset(out, 0, sizeof(*out));
  out->n_factors = e->n_factors;
  for (int32_t f = 0; f < e->n_factors; f++) {
    const mi_agg_vector_factor& in = e->factors[f];
    device::AggFactorDev& fd = out->factors[f];
    ExprFactorConstants(std::string(api) + ": SUM_EXPR factor " + std::to_string(f), is_float, in.constants, in.mul, in.add, in.fmul, in.fadd, &fd.mul, &fd.add);
    if (is_constant(in)) continue;
    fd.col.data = in.column.data;
    fd.col.validity = static_cast<const uint64_t*>(in.column.validity);
    fd.col.width = in.column.width;
    fd.col.cls = in.column.value_class;
    if (&in == first) desc->a = fd.col;
    else if ((in.column.value_class == MI_AGG_CLASS_FLOAT) != is_float)
      throw NotImplementedException(std::string(api) + ": SUM_EXPR factors " + std::to_string(static_cast<int>(first - e->factors)) + " and " + std::to_string(f) +
                                    ": both factors must be integer-like or both floating point");
  }
}

//! What a vector call makes of its arguments: the program as the launchers take it (exprs: NULL without a SUM_EXPR), each
//! aggregate's operation, and the result with its kinds and classes
struct VectorCall {
  device::GroupProgram prog = {};
  device::AggExprTable table;
  const device::AggExprTable* exprs = nullptr;
  std::vector<int32_t> ops;
  GroupResult r;

  void Key(const mi_group_key_column& c, int32_t kind) {
    device::GroupKeyColumnDev& k = prog.keys[prog.n_keys++];
    k.data = c.data;
    k.validity = static_cast<const uint64_t*>(c.validity);
    k.width = c.width;
    k.cls = c.key_class;
    r.kinds.push_back(kind);
  }
  //! the vector specs of the call `api` names in its messages; what is left to check is the *ProgramIsValid of its kernels
  void Aggregates(const char* api, const mi_agg_vector_spec* aggs, int32_t n_aggs) {
    auto column = [](const mi_agg_column& c) {
      device::AggColumnDev d;
      d.data = c.data;
      d.validity = static_cast<const uint64_t*>(c.validity);
      d.width = c.width;
      d.cls = c.value_class;
      return d;
    };
    prog.aggs.n_aggs = n_aggs;
    for (int32_t i = 0; i < n_aggs; i++) {
      device::AggDescDev& d = prog.aggs.aggs[i];
      d.op = aggs[i].op;
      if (aggs[i].op == MI_AGG_SUM_EXPR) {
        if (!exprs) {
          std::memset(&table, 0, sizeof(table));
          exprs = &table;
        }
        VectorExprOf(api, aggs[i], &d, &table.exprs[i]);
      } else {
        d.a = column(aggs[i].a);
        d.b = column(aggs[i].b);
      }
      ops.push_back(d.op);
      r.classes.push_back(d.a.cls);
    }
  }
  //! the call's one batch through a run of `mode` (what the scan gives every record batch): the groups come out sorted
  void Run(mi_ctx* ctx, AggMode mode, uint32_t max_groups, bool count_time, const mi_sel_t* sel, const uint32_t* sel_count, int64_t nrows, void* stream) {
    ctx->ctx->Bind();
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->ctx->stream;
    AggRun run(mode, prog.n_keys, r.key_cls, ops, r.classes, max_groups, count_time);
    run.Begin(s);
    run.Batch(prog, exprs, sel, sel_count, nrows, s);
    run.Finish(s, &r);
    if (prog.n_keys) SortGroups(&r);
  }
};
}  // namespace

int mi_aggregate_vectors(mi_ctx* ctx, const mi_agg_vector_spec* aggs, int32_t n_aggs, const mi_sel_t* sel, const uint32_t* sel_count,
                         int64_t nrows, mi_agg_value* out, void* stream) {
  return Wrap([&] {
    if (!ctx || !aggs || !out) throw InvalidInputException("mi_aggregate_vectors: NULL argument");
    if (n_aggs < 1 || n_aggs > MI_MAX_AGGREGATES)
      throw InvalidInputException("mi_aggregate_vectors takes 1 to " + std::to_string(MI_MAX_AGGREGATES) + " aggregates, not " + std::to_string(n_aggs));
    if ((sel == nullptr) != (sel_count == nullptr)) throw InvalidInputException("mi_aggregate_vectors: sel and sel_count go together");
    if (nrows < 0) throw InvalidInputException("mi_aggregate_vectors: negative row count");
    VectorCall v;
    v.Aggregates("mi_aggregate_vectors", aggs, n_aggs);
    if (!device::AggProgramIsValid(v.prog.aggs, v.exprs))
      throw InvalidInputException("mi_aggregate_vectors: an operation, value class or width that does not fit (SUM takes integers of width 1 / 2 / 4 / 8 "
                                  "or floats of width 4 / 8, MIN / MAX also width 16, a product two integers or two floats)");
    v.Run(ctx, AggMode::kPlain, 0, /*count_time*/ false, sel, sel_count, nrows, stream);
    for (size_t i = 0; i < v.ops.size(); i++) FillAggValue(v.ops[i], v.r.classes[i], v.r.values[i], &out[i]);
  });
}

int mi_group_aggregate_vectors(mi_ctx* ctx, const mi_group_key_column* keys, int32_t n_keys, const mi_agg_vector_spec* aggs, int32_t n_aggs,
                               const mi_sel_t* sel, const uint32_t* sel_count, int64_t nrows, mi_group_key_value* out_keys,
                               mi_agg_value* out_values, int32_t capacity, int32_t* n_groups, void* stream) {
  return Wrap([&] {
    if (n_groups) *n_groups = 0;
    if (!ctx || !keys || !aggs || !out_keys || !out_values || !n_groups) throw InvalidInputException("mi_group_aggregate_vectors: NULL argument");
    if (n_keys < 1 || n_keys > MI_MAX_GROUP_KEYS)
      throw InvalidInputException("mi_group_aggregate_vectors takes 1 to " + std::to_string(MI_MAX_GROUP_KEYS) + " key columns, not " + std::to_string(n_keys));
    if (n_aggs < 1 || n_aggs > MI_MAX_AGGREGATES)
      throw InvalidInputException("mi_group_aggregate_vectors takes 1 to " + std::to_string(MI_MAX_AGGREGATES) + " aggregates, not " + std::to_string(n_aggs));
    if ((sel == nullptr) != (sel_count == nullptr)) throw InvalidInputException("mi_group_aggregate_vectors: sel and sel_count go together");
    if (nrows < 0 || capacity < 0) throw InvalidInputException("mi_group_aggregate_vectors: negative row count or capacity");
    VectorCall v;
    for (int32_t k = 0; k < n_keys; k++) v.Key(keys[k], groupkey::KindOfClass(keys[k].key_class));
    v.Aggregates("mi_group_aggregate_vectors", aggs, n_aggs);
    if (!device::GroupProgramIsValid(v.prog, v.exprs))
      throw InvalidInputException("mi_group_aggregate_vectors: a key class, operation, value class or width that does not fit (keys: signed / unsigned of width "
                                  "1 / 2 / 4 / 8, wide or string of width 16; aggregates as mi_aggregate_vectors takes them)");
    v.Run(ctx, AggMode::kGrouped, 0, /*count_time*/ false, sel, sel_count, nrows, stream);
    FillGroupOutputs(v.r, v.ops, out_keys, out_values, capacity, n_groups);
  });
}

int mi_hash_aggregate_vectors(mi_ctx* ctx, const mi_group_key_column* key, const mi_agg_vector_spec* aggs, int32_t n_aggs, const mi_sel_t* sel,
                              const uint32_t* sel_count, int64_t nrows, int32_t max_groups, mi_group_key_value* out_keys,
                              mi_agg_value* out_values, int32_t capacity, int32_t* n_groups, void* stream) {
  return Wrap([&] {
    if (n_groups) *n_groups = 0;
    if (!ctx || !key || !aggs || !out_keys || !out_values || !n_groups) throw InvalidInputException("mi_hash_aggregate_vectors: NULL argument");
    if (n_aggs < 1 || n_aggs > MI_MAX_AGGREGATES)
      throw InvalidInputException("mi_hash_aggregate_vectors takes 1 to " + std::to_string(MI_MAX_AGGREGATES) + " aggregates, not " + std::to_string(n_aggs));
    if ((sel == nullptr) != (sel_count == nullptr)) throw InvalidInputException("mi_hash_aggregate_vectors: sel and sel_count go together");
    if (nrows < 0 || capacity < 0) throw InvalidInputException("mi_hash_aggregate_vectors: negative row count or capacity");
    CheckHashMaxGroups("mi_hash_aggregate_vectors", max_groups);
    if (key->key_class == MI_GROUP_KEY_CLASS_WIDE || key->key_class == MI_GROUP_KEY_CLASS_STRING) RefuseHashKeyClass("the key column", key->key_class);
    VectorCall v;
    v.Key(*key, groupkey::kKindInt128);
    v.r.key_cls = key->key_class;
    v.Aggregates("mi_hash_aggregate_vectors", aggs, n_aggs);
    for (int32_t i = 0; i < n_aggs; i++) RefuseHashAggregate("aggregate " + std::to_string(i), aggs[i].op, v.r.classes[static_cast<size_t>(i)]);
    if (!device::HashGroupProgramIsValid(v.prog, v.exprs))
      throw InvalidInputException("mi_hash_aggregate_vectors: a key class, operation, value class or width that does not fit (key: signed / unsigned of width "
                                  "1 / 2 / 4 / 8; aggregates as mi_aggregate_vectors takes them, without floating-point sums and 16-byte MIN / MAX)");
    v.Run(ctx, AggMode::kHash, static_cast<uint32_t>(max_groups), /*count_time*/ true, sel, sel_count, nrows, stream);
    FillGroupOutputs(v.r, v.ops, out_keys, out_values, capacity, n_groups);
  });
}

int mi_filter_float_key(double v, int32_t width, int64_t* key) {
  return Wrap([&] {
    if (!key || (width != 4 && width != 8)) throw InvalidInputException("mi_filter_float_key: width must be 4 or 8");
    *key = filterkey::FloatKeyOfDouble(v, width);
  });
}

int mi_filter_launch_counts(int64_t* base, int64_t* extended) {
  return Wrap([&] {
    if (!base || !extended) throw InvalidInputException("mi_filter_launch_counts: NULL argument");
    int64_t n[2];
    device::FilterLaunchCounts(n);
    *base = n[0];
    *extended = n[1];
  });
}

int mi_filter_like_match(int32_t op, const char* pattern, int32_t pattern_len, const char* row, int32_t row_len, int32_t* result) {
  return Wrap([&] {
    if (!result || pattern_len < 0 || row_len < 0 || (!pattern && pattern_len > 0) || (!row && row_len > 0))
      throw InvalidInputException("mi_filter_like_match: NULL argument or negative length");
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(pattern);
    likematch::Pattern pat;
    CheckPattern(likematch::Compile(op, bytes, static_cast<uint32_t>(pattern_len), &pat), op, std::string());
    *result = likematch::Passes(pat, bytes, reinterpret_cast<const uint8_t*>(row), static_cast<uint32_t>(row_len)) ? 1 : 0;
  });
}

int mi_filter_pattern_launches(int64_t* n) {
  return Wrap([&] {
    if (!n) throw InvalidInputException("mi_filter_pattern_launches: NULL argument");
    *n = device::FilterPatternLaunches();
  });
}

// the header restates the kernel's leaf forms and flag bits, and the leaf itself
static_assert(MI_FL_RANGE == device::kLeafRange && MI_FL_IS_NULL == device::kLeafIsNull && MI_FL_IS_NOT_NULL == device::kLeafIsNotNull &&
              MI_FL_IN == device::kLeafIn && MI_FL_STR_IN == device::kLeafStrIn && MI_FL_DICT_MAP == device::kLeafDictMap &&
              MI_FL_STR_RANGE == device::kLeafStrRange && MI_FL_WIDE_RANGE == device::kLeafWideRange && MI_FL_WIDE_IN == device::kLeafWideIn &&
              MI_FL_STR_MATCH == device::kLeafStrMatch, "mi_filter_leaf_op restates kLeaf*");
static_assert(MI_FLF_UNSIGNED == device::kLeafUnsigned && MI_FLF_NEGATE == device::kLeafNegate && MI_FLF_ENDS_CLAUSE == device::kLeafEndsClause &&
              MI_FLF_BIAS == device::kLeafBias && MI_FLF_FLOAT == device::kLeafFloat, "mi_filter_leaf_flag restates the flag bits");
static_assert(MI_MAX_FILTER_LEAVES == device::kMaxFilterLeaves, "MI_MAX_FILTER_LEAVES restates kMaxFilterLeaves");
static_assert(sizeof(mi_filter_vector_leaf) == sizeof(device::FilterLeafDev) &&
              offsetof(mi_filter_vector_leaf, data) == offsetof(device::FilterLeafDev, data) &&
              offsetof(mi_filter_vector_leaf, validity) == offsetof(device::FilterLeafDev, validity) &&
              offsetof(mi_filter_vector_leaf, in_values) == offsetof(device::FilterLeafDev, in_values) &&
              offsetof(mi_filter_vector_leaf, lo) == offsetof(device::FilterLeafDev, lo) &&
              offsetof(mi_filter_vector_leaf, hi) == offsetof(device::FilterLeafDev, hi) &&
              offsetof(mi_filter_vector_leaf, op) == offsetof(device::FilterLeafDev, op) &&
              offsetof(mi_filter_vector_leaf, width) == offsetof(device::FilterLeafDev, width) &&
              offsetof(mi_filter_vector_leaf, flags) == offsetof(device::FilterLeafDev, flags) &&
              offsetof(mi_filter_vector_leaf, n_in) == offsetof(device::FilterLeafDev, n_in), "mi_filter_vector_leaf is FilterLeafDev, field for field");

int mi_filter_program_vectors(mi_ctx* ctx, const mi_filter_vector_leaf* leaves, int32_t n_leaves, int64_t nrows, mi_sel_t* sel_out,
                              uint32_t* count_out, void* stream) {
  return Wrap([&] {
    if (!ctx || !sel_out || !count_out) throw InvalidInputException("mi_filter_program_vectors: NULL argument");
    if (n_leaves < 0 || n_leaves > MI_MAX_FILTER_LEAVES)
      throw InvalidInputException("mi_filter_program_vectors takes 0 to " + std::to_string(MI_MAX_FILTER_LEAVES) + " leaves, not " + std::to_string(n_leaves));
    if (n_leaves > 0 && !leaves) throw InvalidInputException("mi_filter_program_vectors: NULL leaves");
    if (nrows < 0) throw InvalidInputException("mi_filter_program_vectors: negative row count");
    device::FilterProgram prog;
    std::memset(&prog, 0, sizeof(prog));
    prog.n_leaves = n_leaves;
    for (int32_t l = 0; l < n_leaves; l++) {
      const mi_filter_vector_leaf& in = leaves[l];
      auto refuse = [&](const std::string& what) { throw InvalidInputException("mi_filter_program_vectors: leaf " + std::to_string(l) + ": " + what); };
      const bool is_null_op = in.op == MI_FL_IS_NULL || in.op == MI_FL_IS_NOT_NULL;
      const bool is_int_op = in.op == MI_FL_RANGE || in.op == MI_FL_IN;
      const bool is_str_op = in.op == MI_FL_STR_IN || in.op == MI_FL_STR_RANGE || in.op == MI_FL_STR_MATCH;
      const bool is_wide_op = in.op == MI_FL_WIDE_RANGE || in.op == MI_FL_WIDE_IN;
      if (!is_null_op && !is_int_op && !is_str_op && !is_wide_op && in.op != MI_FL_DICT_MAP) refuse("unknown op " + std::to_string(in.op));
      if (!is_null_op) {
        if (!in.data) refuse("NULL data");
        bool fits;
        if (is_int_op) fits = (in.flags & MI_FLF_FLOAT) ? (in.width == 4 || in.width == 8) : (in.width == 1 || in.width == 2 || in.width == 4 || in.width == 8);
        else fits = in.width == (in.op == MI_FL_DICT_MAP ? 4 : 16);
        if (!fits) refuse("width " + std::to_string(in.width) + " does not fit the op (integers 1 / 2 / 4 / 8, floats 4 / 8, wide and string rows 16, dictionary indices 4)");
      }
      if (in.n_in < 0) refuse("negative n_in");
      if ((in.op == MI_FL_IN || in.op == MI_FL_WIDE_IN || in.op == MI_FL_STR_IN) && in.n_in > 256) refuse("more than 256 constants");
      // the bounds of a string or wide range, the segments and a wide list are read whatever n_in says; the other tables entry by entry
      const bool reads_table = in.op == MI_FL_STR_RANGE || in.op == MI_FL_STR_MATCH || is_wide_op ||
                               ((in.op == MI_FL_IN || in.op == MI_FL_STR_IN || in.op == MI_FL_DICT_MAP) && in.n_in > 0);
      if (reads_table && !in.in_values) refuse("NULL in_values");
      if (in.op == MI_FL_STR_RANGE && (in.n_in & ~0xF)) refuse("a string range's n_in holds four bits");
      if (in.op == MI_FL_STR_MATCH && ((in.n_in & 0xFF) < 1 || (in.n_in & 0xFF) > likematch::kMaxSegments || (in.n_in & ~0x3FF)))
        refuse("a pattern leaf takes 1 to 8 segments and two anchor bits");
      if (in.op == MI_FL_DICT_MAP && (in.lo < 0 || in.lo > 3)) refuse("dictionary map mode " + std::to_string(in.lo) + " outside 0 .. 3");
      if ((in.flags & MI_FLF_NEGATE) && (is_null_op || in.op == MI_FL_DICT_MAP)) refuse("MI_FLF_NEGATE on IS [NOT] NULL or a dictionary map");
      if (reinterpret_cast<uintptr_t>(in.data) & 7u) refuse("data is not 8-byte aligned");
      if (reinterpret_cast<uintptr_t>(in.validity) & 7u) refuse("validity is not 8-byte aligned");
      if (l == n_leaves - 1 && !(in.flags & MI_FLF_ENDS_CLAUSE)) refuse("the last leaf does not end its clause");
      device::FilterLeafDev& L = prog.leaves[l];
      L.data = in.data;
      L.validity = static_cast<const uint64_t*>(in.validity);
      L.in_values = in.in_values;
      L.lo = in.lo;
      L.hi = in.hi;
      L.op = in.op;
      L.width = in.width;
      L.flags = in.flags;
      L.n_in = in.n_in;
    }
    if (nrows == 0) return;
    ctx->ctx->Bind();
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->ctx->stream;
    const hipError_t e = device::LaunchFilterProgram(prog, nrows, sel_out, count_out, s);
    if (e == hipErrorInvalidValue) throw InvalidInputException("mi_filter_program_vectors: the launcher refuses the program (a pattern leaf takes 1 to 8 segments and no other bit in n_in)");
    MI_HIP_CHECK(e);
  });
}

}  // extern "C"

// scan operator, aggregate + writer entry points live in scan_operator.cpp / scan_aggregate.cpp / writer_api.cpp (same extern "C" rules)
namespace miarrow {
int WrapC(const std::function<void()>& f) { return Wrap(f); }
Context* ContextOf(mi_ctx* c) { return c ? c->ctx.get() : nullptr; }
}  // namespace miarrow
