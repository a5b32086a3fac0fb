// scan_aggregate.cpp -- see scan_aggregate.hpp: the fused aggregates of a scan.  The ArrowScan methods here bind a call
// (agg_bind), project exactly the columns it reads, give every record batch the run's launches behind the filter on the compute
// stream (agg_run) and read the result back once at the end; the MultiDeviceScan methods merge the devices' results
// (agg_result); the C ABI of the three calls closes the file.
#include "scan_operator.hpp"

#include <hip/hip_runtime.h>

#include <cstring>
#include <functional>

namespace miarrow {

int WrapC(const std::function<void()>& f);  // c_api.cpp
ScanBase* ScanOf(mi_scan* s);               // scan_operator.cpp

namespace {
std::vector<int32_t> OpsOf(const std::vector<AggSpec>& specs) {
  std::vector<int32_t> ops;
  for (const AggSpec& sp : specs) ops.push_back(sp.op);
  return ops;
}
}  // namespace

// ------------------------------------------------------------------------------------------------ one scan
// SELECT agg_1 .. agg_n over the rows the pushed-down filter keeps (K9), per group of 1 .. 4 key columns for few groups (K10), or
// per group of ONE integer key for many (K11).  Nothing but the filter's counts comes back per batch, the result once at the end.
void ArrowScan::Aggregate(const std::vector<AggSpec>& specs, AggResult* out) {
  if (initialized) throw InvalidInputException("mi_scan_aggregate replaces mi_scan_init / mi_scan_next: call it right after bind");
  GroupResult r;
  RunAggregates(BindAggregates(Bind(), specs), &r);
  *out = r;   // (the part without keys)
}

void ArrowScan::GroupAggregate(const std::vector<std::string>& keys, const std::vector<AggSpec>& specs, GroupResult* out) {
  if (initialized) throw InvalidInputException("mi_scan_group_aggregate replaces mi_scan_init / mi_scan_next: call it right after bind");
  RunAggregates(BindGroupAggregates(Bind(), keys, specs), out);
}

void ArrowScan::HashAggregate(const std::string& key, const std::vector<AggSpec>& specs, uint32_t max_groups, GroupResult* out) {
  if (initialized) throw InvalidInputException("mi_scan_hash_aggregate replaces mi_scan_init / mi_scan_next: call it right after bind");
  RunAggregates(BindHashAggregates(Bind(), key, specs, max_groups), out);
}

void ArrowScan::RunAggregates(BoundAggregates plan, GroupResult* out) {
  *out = GroupResult();
  const bool hash = plan.mode == AggMode::kHash;
  for (const BoundKey& k : plan.keys) out->kinds.push_back(hash ? groupkey::kKindInt128 : groupkey::KindOfClass(k.cls));
  if (hash) out->key_cls = plan.keys[0].cls;
  std::vector<int32_t> ops;
  for (const BoundAgg& b : plan.aggs) {
    ops.push_back(b.op);
    out->classes.push_back(b.cls);
  }
  aggn.run = std::make_unique<AggRun>(plan.mode, static_cast<int>(plan.keys.size()), out->key_cls, ops, out->classes, plan.max_groups, /*count_time*/ true);
  aggn.plan = std::move(plan);
  try {
    out->rows_selected = DrainAggregates();
    aggn.run->Finish(ctx->stream, out);
    if (!aggn.plan.keys.empty()) SortGroups(out);
    out->rows_scanned = aggn.rows_scanned;
  } catch (...) {
    aggn.on = false;
    aggn.run.reset();
    throw;
  }
  aggn.on = false;
  aggn.run.reset();
}

int64_t ArrowScan::DrainAggregates() {
  ctx->Bind();
  aggn.on = true;
  aggn.rows_scanned = 0;
  Init(aggn.plan.projection);
  aggn.run->Begin(ctx->stream);
  int64_t selected = 0;
  BatchRef ref;
  while (AcquireBatch(&ref)) {   // the pull loop only recycles slots and adds up the filter's counts
    selected += ref.selected;
    ReleaseBatch(ref);
  }
  return selected;
}

// ---- per record batch: the programs over the slot's decoded vectors, then the run's launches
bool ArrowScan::FillAggregatePrograms(const Slot& s, device::GroupProgram* gprog, device::AggExprTable* exprs) const {
  auto column = [&](int32_t c, const void** data, const uint64_t** validity, int32_t* width) {
    // (a column that this file lacks was refused by EnqueueBatch before anything was queued: col_root is a node here)
    const PlannedNode& o = s.planner.nodes[static_cast<size_t>(s.col_root[static_cast<size_t>(c)])];
    *data = o.alias_body_off >= 0 ? static_cast<const void*>(s.d_in.get() + o.alias_body_off) : static_cast<const void*>(s.d_out.get() + o.data_off);
    *validity = o.valid_off >= 0 ? reinterpret_cast<const uint64_t*>(s.d_out.get() + o.valid_off) : nullptr;
    *width = o.width;
  };
  const std::vector<BoundAgg>& aggs = aggn.plan.aggs;
  const std::vector<BoundKey>& keys = aggn.plan.keys;
  std::memset(gprog, 0, sizeof(*gprog));
  bool has_expr = false;   // (the table is filled, and handed to the launches, only when an aggregate is an expression)
  device::AggProgram& prog = gprog->aggs;
  prog.n_aggs = static_cast<int32_t>(aggs.size());
  for (size_t a = 0; a < aggs.size(); a++) {
    const BoundAgg& b = aggs[a];
    device::AggDescDev& d = prog.aggs[a];
    d.op = b.op;
    d.a.cls = b.cls;
    d.b.cls = b.cls_b;
    if (b.col_a >= 0) column(b.col_a, &d.a.data, &d.a.validity, &d.a.width);
    if (b.col_b >= 0) column(b.col_b, &d.b.data, &d.b.validity, &d.b.width);
    if (b.op != aggmerge::kOpSumExpr) continue;
    if (!has_expr) std::memset(exprs, 0, sizeof(*exprs));
    has_expr = true;
    device::AggExprDev& e = exprs->exprs[a];
    e.n_factors = static_cast<int32_t>(b.factors.size());
    for (size_t f = 0; f < b.factors.size(); f++) {
      device::AggFactorDev& fd = e.factors[f];
      fd.mul = b.factors[f].mul;
      fd.add = b.factors[f].add;
      fd.col.cls = b.factors[f].cls;
      if (b.factors[f].col >= 0) column(b.factors[f].col, &fd.col.data, &fd.col.validity, &fd.col.width);
    }
  }
  gprog->n_keys = static_cast<int32_t>(keys.size());
  for (size_t k = 0; k < keys.size(); k++) {
    device::GroupKeyColumnDev& kc = gprog->keys[k];
    kc.cls = keys[k].cls;
    column(keys[k].col, &kc.data, &kc.validity, &kc.width);
  }
  return has_expr;
}

void ArrowScan::EnqueueAggregates(Slot& s) {
  device::GroupProgram gprog;
  device::AggExprTable exprs_table;
  const device::AggExprTable* exprs = FillAggregatePrograms(s, &gprog, &exprs_table) ? &exprs_table : nullptr;
  const mi_sel_t* sel = has_filter ? reinterpret_cast<const mi_sel_t*>(s.d_out.get() + s.sel_off) : nullptr;
  const uint32_t* sel_count = has_filter ? reinterpret_cast<const uint32_t*>(s.d_out.get() + s.sel_count_off) : nullptr;
  aggn.run->Batch(gprog, exprs, sel, sel_count, s.nrows, ctx->stream);
  aggn.rows_scanned += s.nrows;
}

// ------------------------------------------------------------------------------------------------ multi-device
void MultiDeviceScan::Aggregate(const std::vector<AggSpec>& specs, AggResult* out) {
  std::vector<AggResult> parts(subs.size());
  ForEachParallel([&](size_t i) { subs[i]->Aggregate(specs, &parts[i]); });
  MergeAggResults(parts, OpsOf(specs), out);
}

void MultiDeviceScan::GroupAggregate(const std::vector<std::string>& keys, const std::vector<AggSpec>& specs, GroupResult* out) {
  std::vector<GroupResult> parts(subs.size());
  ForEachParallel([&](size_t i) { subs[i]->GroupAggregate(keys, specs, &parts[i]); });
  if (!MergeGroupResults(parts, OpsOf(specs), out)) ThrowForStatus(MI_ST_GROUP_LIMIT);
}

void MultiDeviceScan::HashAggregate(const std::string& key, const std::vector<AggSpec>& specs, uint32_t max_groups, GroupResult* out) {
  CheckHashMaxGroups("mi_scan_hash_aggregate", max_groups);
  std::vector<GroupResult> parts(subs.size());
  ForEachParallel([&](size_t i) { subs[i]->HashAggregate(key, specs, max_groups, &parts[i]); });
  if (!MergeHashResults(parts, OpsOf(specs), max_groups, out))
    throw NotImplementedException("hash GROUP BY found more than max_groups = " + std::to_string(max_groups) + " distinct keys among the selected rows of the "
                                  "devices together: call again with a larger max_groups");
}

}  // namespace miarrow

// ------------------------------------------------------------------------------------------------ C ABI
using namespace miarrow;

namespace {
//! the aggregates of the C ABI by column name, for the call `api` names in its messages
std::vector<AggSpec> SpecsOf(const char* api, const mi_agg_spec* aggs, int32_t n_aggs) {
  if (n_aggs < 1 || n_aggs > MI_MAX_AGGREGATES)   // (BindAggregateSpecs checks the specs; this one guards the read of aggs[])
    throw InvalidInputException(std::string(api) + " takes 1 to " + std::to_string(MI_MAX_AGGREGATES) + " aggregates, not " + std::to_string(n_aggs));
  std::vector<AggSpec> specs;
  for (int32_t i = 0; i < n_aggs; i++) {
    AggSpec sp;
    sp.op = aggs[i].op;
    if (sp.op < MI_AGG_COUNT_STAR || sp.op > MI_AGG_SUM_EXPR) throw InvalidInputException(std::string(api) + ": unknown operation " + std::to_string(sp.op));
    if (sp.op == MI_AGG_SUM_EXPR) {
      const mi_agg_expr* e = aggs[i].expr;
      if (!e) throw InvalidInputException(std::string(api) + ": SUM_EXPR without an expression");
      if (e->n_factors < 1 || e->n_factors > MI_MAX_EXPR_FACTORS)
        throw InvalidInputException(std::string(api) + ": SUM_EXPR takes 1 to " + std::to_string(MI_MAX_EXPR_FACTORS) + " factors, not " + std::to_string(e->n_factors));
      for (int32_t f = 0; f < e->n_factors; f++) {
        const mi_agg_factor& in = e->factors[f];
        AggFactorSpec fs;
        fs.has_column = in.column != nullptr;
        if (in.column) fs.column = in.column;
        fs.mul = in.mul;
        fs.add = in.add;
        fs.fmul = in.fmul;
        fs.fadd = in.fadd;
        fs.constants = in.constants;
        sp.factors.push_back(std::move(fs));
      }
      specs.push_back(std::move(sp));
      continue;
    }
    if (sp.op != MI_AGG_COUNT_STAR && !aggs[i].column_a) throw InvalidInputException(std::string(api) + ": " + AggOpName(sp.op) + " without a column");
    if (sp.op == MI_AGG_SUM_PRODUCT && !aggs[i].column_b) throw InvalidInputException(std::string(api) + ": SUM_PRODUCT without a second column");
    if (sp.op != MI_AGG_COUNT_STAR) sp.a = aggs[i].column_a;
    if (sp.op == MI_AGG_SUM_PRODUCT) sp.b = aggs[i].column_b;
    specs.push_back(std::move(sp));
  }
  return specs;
}

//! launches by this process and, with MI_AGG_TIMING=1, their summed device time: of one mode's two kernels
int Counters(void (*launches)(int64_t[2]), AggMode mode, int64_t* window_launches, int64_t* combine_launches, double* windows_ms,
             double* combine_ms) {
  return WrapC([&] {
    int64_t n[2];
    double ms[2];
    launches(n);
    AggTimingTotals(mode, ms);
    if (window_launches) *window_launches = n[0];
    if (combine_launches) *combine_launches = n[1];
    if (windows_ms) *windows_ms = ms[0];
    if (combine_ms) *combine_ms = ms[1];
  });
}
}  // namespace

extern "C" {

int mi_scan_aggregate(mi_scan* s, const mi_agg_spec* aggs, int32_t n_aggs, mi_agg_value* out, int64_t* rows_scanned, int64_t* rows_selected) {
  return WrapC([&] {
    if (!s || !aggs || !out) throw InvalidInputException("mi_scan_aggregate: NULL argument");
    const std::vector<AggSpec> specs = SpecsOf("mi_scan_aggregate", aggs, n_aggs);
    AggResult r;
    ScanOf(s)->Aggregate(specs, &r);
    for (int32_t i = 0; i < n_aggs; i++) FillAggValue(specs[static_cast<size_t>(i)].op, r.classes[static_cast<size_t>(i)], r.values[static_cast<size_t>(i)], &out[i]);
    if (rows_scanned) *rows_scanned = r.rows_scanned;
    if (rows_selected) *rows_selected = r.rows_selected;
  });
}

int mi_aggregate_counters(int64_t* window_launches, int64_t* combine_launches, double* windows_ms, double* combine_ms) {
  return Counters(device::AggLaunchCounts, AggMode::kPlain, window_launches, combine_launches, windows_ms, combine_ms);
}

int mi_scan_group_aggregate(mi_scan* s, const char* const* key_columns, int32_t n_keys, const mi_agg_spec* aggs, int32_t n_aggs,
                            mi_group_key_value* out_keys, mi_agg_value* out_values, int32_t capacity, int32_t* n_groups, int64_t* rows_scanned,
                            int64_t* rows_selected) {
  return WrapC([&] {
    if (n_groups) *n_groups = 0;
    if (!s || !key_columns || !aggs || !out_keys || !out_values || !n_groups) throw InvalidInputException("mi_scan_group_aggregate: NULL argument");
    if (n_keys < 1 || n_keys > MI_MAX_GROUP_KEYS)
      throw InvalidInputException("mi_scan_group_aggregate takes 1 to " + std::to_string(MI_MAX_GROUP_KEYS) + " key columns, not " + std::to_string(n_keys));
    if (capacity < 0) throw InvalidInputException("mi_scan_group_aggregate: negative capacity");
    std::vector<std::string> keys;
    for (int32_t k = 0; k < n_keys; k++) {
      if (!key_columns[k]) throw InvalidInputException("mi_scan_group_aggregate: NULL key column");
      keys.emplace_back(key_columns[k]);
    }
    const std::vector<AggSpec> specs = SpecsOf("mi_scan_group_aggregate", aggs, n_aggs);
    GroupResult r;
    ScanOf(s)->GroupAggregate(keys, specs, &r);
    FillGroupOutputs(r, OpsOf(specs), out_keys, out_values, capacity, n_groups);
    if (rows_scanned) *rows_scanned = r.rows_scanned;
    if (rows_selected) *rows_selected = r.rows_selected;
  });
}

int mi_group_aggregate_counters(int64_t* window_launches, int64_t* combine_launches, double* windows_ms, double* combine_ms) {
  return Counters(device::GroupLaunchCounts, AggMode::kGrouped, window_launches, combine_launches, windows_ms, combine_ms);
}

int mi_scan_hash_aggregate(mi_scan* s, const char* key_column, const mi_agg_spec* aggs, int32_t n_aggs, int32_t max_groups,
                           mi_group_key_value* out_keys, mi_agg_value* out_values, int32_t capacity, int32_t* n_groups, int64_t* rows_scanned,
                           int64_t* rows_selected) {
  return WrapC([&] {
    if (n_groups) *n_groups = 0;
    if (!s || !key_column || !aggs || !out_keys || !out_values || !n_groups) throw InvalidInputException("mi_scan_hash_aggregate: NULL argument");
    if (capacity < 0) throw InvalidInputException("mi_scan_hash_aggregate: negative capacity");
    CheckHashMaxGroups("mi_scan_hash_aggregate", max_groups);
    const std::vector<AggSpec> specs = SpecsOf("mi_scan_hash_aggregate", aggs, n_aggs);
    GroupResult r;
    ScanOf(s)->HashAggregate(key_column, specs, static_cast<uint32_t>(max_groups), &r);
    FillGroupOutputs(r, OpsOf(specs), out_keys, out_values, capacity, n_groups);
    if (rows_scanned) *rows_scanned = r.rows_scanned;
    if (rows_selected) *rows_selected = r.rows_selected;
  });
}

int mi_hash_aggregate_counters(int64_t* rows_launches, int64_t* collect_launches, double* rows_ms, double* collect_ms) {
  return Counters(device::HashGroupLaunchCounts, AggMode::kHash, rows_launches, collect_launches, rows_ms, collect_ms);
}

}  // extern "C"
