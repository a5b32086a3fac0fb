// scan_aggregate.cpp -- see scan_aggregate.hpp: the fused aggregates of a scan.  The ArrowScan methods here validate the
// aggregates at bind time (messages name the column and the operation), project exactly the columns they read, give every
// record batch its launches behind the filter on the compute stream and read the result back once at the end; the
// MultiDeviceScan methods merge the devices' results; the C ABI of the three calls closes the file.
#include "scan_operator.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <functional>

namespace miarrow {

int WrapC(const std::function<void()>& f);  // c_api.cpp
ScanBase* ScanOf(mi_scan* s);               // scan_operator.cpp

// ------------------------------------------------------------------------------------------------ fused aggregates
// mi_scan_aggregate: SELECT agg_1 .. agg_n over the rows the pushed-down filter keeps.  The columns are validated at bind
// time (messages name the column and the operation), the call projects exactly the aggregate columns, and every record
// batch gets agg_windows + agg_combine behind its filter on the compute stream (EnqueueAggregates): nothing but the
// filter's counts comes back per batch, the accumulator block once at the end.
namespace {
std::atomic<int64_t> g_agg_events_ns[2];   // MI_AGG_TIMING=1: device time of agg_windows / agg_combine, nanoseconds
std::atomic<int64_t> g_group_events_ns[2]; // ... and of group_windows / group_combine

//! aggmerge::kClass* of the values SUM / MIN / MAX read from `c`, kClassAny when they read none of its kind
int32_t AggClassOf(const ScanColumn& c) {
  if (c.is_constant() || c.field.has_dictionary) return aggmerge::kClassAny;
  const ArrowField& vf = ValueField(c.field);
  int32_t kind, w;
  int64_t param;
  if (vf.has_dictionary || !c.field.Plan(&kind, &param, &w)) return aggmerge::kClassAny;
  switch (FilterClassOf(c.field)) {
    case FilterValueClass::kFloat32: case FilterValueClass::kFloat64: return aggmerge::kClassFloat;
    case FilterValueClass::kWide: return aggmerge::kClassWide;
    default: break;
  }
  if (vf.Plan(&kind, &param, &w) && IsIntegerLike(kind, w, vf, /*allow_bool*/ false))
    return vf.type == MI_AT_INT && !vf.is_signed ? aggmerge::kClassUnsigned : aggmerge::kClassSigned;
  return aggmerge::kClassAny;
}

int32_t SlotOf(std::vector<std::string>* proj, const std::string& name) {
  for (size_t i = 0; i < proj->size(); i++)
    if ((*proj)[i] == name) return static_cast<int32_t>(i);
  proj->push_back(name);
  return static_cast<int32_t>(proj->size() - 1);
}

//! the factors of a product are all integer-like or all floating point
void SameFamily(int32_t op, const ScanColumn& a, int32_t cls_a, const ScanColumn& b, int32_t cls_b) {
  if ((cls_a == aggmerge::kClassFloat) != (cls_b == aggmerge::kClassFloat))
    throw NotImplementedException(std::string(AggOpName(op)) + " of '" + a.name + "' (" + a.field.DuckType() + ") and '" + b.name + "' (" + b.field.DuckType() +
                                  "): both factors must be integer-like or both floating point");
}
}  // namespace

const char* AggOpName(int32_t op) {
  switch (op) {
    case aggmerge::kOpCountStar: return "COUNT(*)";
    case aggmerge::kOpCount: return "COUNT";
    case aggmerge::kOpSum: return "SUM";
    case aggmerge::kOpSumProduct: return "SUM_PRODUCT";
    case aggmerge::kOpMin: return "MIN";
    case aggmerge::kOpMax: return "MAX";
    case aggmerge::kOpSumExpr: return "SUM_EXPR";
    default: return "?";
  }
}

void ExprFactorConstants(const std::string& what, bool is_float, int32_t constants, int64_t mul, int64_t add, double fmul, double fadd,
                         uint64_t* mul_bits, uint64_t* add_bits) {
  if (constants != MI_AGG_CONST_INT && constants != MI_AGG_CONST_DOUBLE)
    throw InvalidInputException(what + ": constants must be MI_AGG_CONST_INT or MI_AGG_CONST_DOUBLE, not " + std::to_string(constants));
  if (!is_float) {
    if (constants == MI_AGG_CONST_DOUBLE)
      throw NotImplementedException(what + ": double constants on an expression over integer-like columns are not computed in the scan (give int64 constants)");
    *mul_bits = static_cast<uint64_t>(mul);
    *add_bits = static_cast<uint64_t>(add);
    return;
  }
  if (constants == MI_AGG_CONST_INT) {
    // exact when the double, which then lies inside int64's range, converts back to the same integer
    auto exact = [&](int64_t v) {
      const double d = static_cast<double>(v);
      if (!(d >= -9223372036854775808.0 && d < 9223372036854775808.0) || static_cast<int64_t>(d) != v)
        throw InvalidInputException(what + ": the integer constant " + std::to_string(v) + " is not exactly representable in a double");
      return d;
    };
    fmul = exact(mul);
    fadd = exact(add);
  }
  *mul_bits = aggmerge::BitsOf(fmul);
  *add_bits = aggmerge::BitsOf(fadd);
}

void AggTimingTotals(double out_ms[2]) {
  out_ms[0] = static_cast<double>(g_agg_events_ns[0].load()) * 1e-6;
  out_ms[1] = static_cast<double>(g_agg_events_ns[1].load()) * 1e-6;
}

const ScanColumn& ArrowScan::AggregateColumn(const std::string& name, const std::string& what) const {
  auto it = std::find_if(all_columns.begin(), all_columns.end(), [&](const ScanColumn& sc) { return sc.name == name; });
  if (it == all_columns.end()) throw InvalidInputException(what + ": Field '" + name + "' does not exist in IPC file schema");
  const std::string typed = "'" + name + "' (" + it->field.DuckType() + ")";   // every refusal names the column and its DuckDB type
  if (it->is_constant()) throw NotImplementedException(what + " on the constant column " + typed + " is not computed in the scan");
  std::string why;
  if (!it->field.Supported(&why)) throw NotImplementedException(what + " on column " + typed + ": " + why + " is not decoded by the MI355X scan path yet");
  if (it->field.has_dictionary || ValueField(it->field).has_dictionary)
    throw NotImplementedException(what + " on the dictionary-encoded column " + typed + " is not computed in the scan");
  // a union's vector is a tag vector over member vectors: no aggregate (COUNT included) and no GROUP BY key reads that tree
  if (it->field.type == MI_AT_UNION)
    throw NotImplementedException(what + " on the union column '" + name + "' (" + it->field.DuckType() + ") is not computed in the scan");
  return *it;
}

const ScanColumn& ArrowScan::FactorColumn(const std::string& name, int32_t op, int32_t* cls) const {
  const ScanColumn& c = AggregateColumn(name, AggOpName(op));
  *cls = AggClassOf(c);
  if (*cls == aggmerge::kClassAny || *cls == aggmerge::kClassWide)
    throw NotImplementedException(std::string(AggOpName(op)) + " on column '" + name + "' (" + c.field.DuckType() + "): a factor is an integer, DATE, TIME / "
                                  "TIMESTAMP, DECIMAL(<=18), FLOAT or DOUBLE column");
  return c;
}

// ---- bind-time validation, and the projection: exactly the columns the aggregates read
void ArrowScan::BindAggregateSpecs(const std::vector<AggSpec>& specs, const char* api, std::vector<std::string>* proj) {
  if (specs.empty() || specs.size() > static_cast<size_t>(aggmerge::kMaxAggregates))
    throw InvalidInputException(std::string(api) + " takes 1 to " + std::to_string(aggmerge::kMaxAggregates) + " aggregates, not " + std::to_string(specs.size()));
  aggn.aggs.clear();
  for (const AggSpec& sp : specs) {
    AggregateState::Bound b;
    b.op = sp.op;
    if (sp.op == aggmerge::kOpCountStar) {
      aggn.aggs.push_back(b);
      continue;
    }
    if (sp.op < aggmerge::kOpCountStar || sp.op > aggmerge::kOpSumExpr) throw InvalidInputException(std::string(api) + ": unknown operation " + std::to_string(sp.op));
    if (sp.op == aggmerge::kOpSumExpr) {
      // every named column is validated and classified, then the constants are converted and the columns projected; the
      // class of the first column is the expression's
      if (sp.factors.empty() || sp.factors.size() > static_cast<size_t>(aggmerge::kMaxExprFactors))
        throw InvalidInputException(std::string(api) + ": SUM_EXPR takes 1 to " + std::to_string(aggmerge::kMaxExprFactors) + " factors, not " + std::to_string(sp.factors.size()));
      b.factors.resize(sp.factors.size());
      const ScanColumn* first = nullptr;
      for (size_t f = 0; f < sp.factors.size(); f++) {
        if (!sp.factors[f].has_column) continue;
        const ScanColumn& c = FactorColumn(sp.factors[f].column, sp.op, &b.factors[f].cls);
        if (!first) {
          first = &c;
          b.cls = b.factors[f].cls;
        } else {
          SameFamily(sp.op, *first, b.cls, c, b.factors[f].cls);
        }
      }
      if (!first) throw InvalidInputException(std::string(api) + ": SUM_EXPR needs at least one factor with a column");
      for (size_t f = 0; f < sp.factors.size(); f++) {
        const AggFactorSpec& fs = sp.factors[f];
        AggregateState::Bound::Factor& fb = b.factors[f];
        ExprFactorConstants(std::string(AggOpName(sp.op)) + (fs.has_column ? " on column '" + fs.column + "'" : std::string(" constant factor")), b.cls == aggmerge::kClassFloat,
                            fs.constants, fs.mul, fs.add, fs.fmul, fs.fadd, &fb.mul, &fb.add);
        if (!fs.has_column) continue;
        fb.col = SlotOf(proj, fs.column);
        if (b.col_a < 0) b.col_a = fb.col;
      }
      aggn.aggs.push_back(b);
      continue;
    }
    const ScanColumn& ca = AggregateColumn(sp.a, AggOpName(sp.op));
    if (sp.op != aggmerge::kOpCount) {
      b.cls = AggClassOf(ca);
      const bool sums = sp.op == aggmerge::kOpSum || sp.op == aggmerge::kOpSumProduct;
      if (b.cls == aggmerge::kClassAny || (sums && b.cls == aggmerge::kClassWide))
        throw NotImplementedException(std::string(AggOpName(sp.op)) + " on column '" + sp.a + "' (" + ca.field.DuckType() + "): SUM takes integers, DATE, TIME / "
                                      "TIMESTAMP, DECIMAL(<=18), FLOAT and DOUBLE columns, MIN / MAX those and HUGEINT / DECIMAL(19..38) / UUID");
      if (sp.op == aggmerge::kOpSumProduct) {
        const ScanColumn& cb = FactorColumn(sp.b, sp.op, &b.cls_b);
        SameFamily(sp.op, ca, b.cls, cb, b.cls_b);
      }
    }
    b.col_a = SlotOf(proj, sp.a);
    if (sp.op == aggmerge::kOpSumProduct) b.col_b = SlotOf(proj, sp.b);
    aggn.aggs.push_back(b);
  }
}

int64_t ArrowScan::DrainAggregates(const std::vector<std::string>& proj, const std::function<void()>& begin, std::atomic<int64_t>* timing_ns) {
  ctx->Bind();
  aggn.on = true;
  aggn.rows_scanned = 0;
  const char* timing = std::getenv("MI_AGG_TIMING");
  aggn.timed = timing && timing[0] == '1';
  aggn.events.clear();
  int64_t selected = 0;
  try {
    Init(proj);
    begin();
    BatchRef ref;
    while (AcquireBatch(&ref)) {   // the pull loop only recycles slots and adds up the filter's counts
      selected += ref.selected;
      ReleaseBatch(ref);
    }
    MI_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (size_t e = 0; e + 2 < aggn.events.size(); e += 3) {
      float w_ms = 0, c_ms = 0;
      MI_HIP_CHECK(hipEventElapsedTime(&w_ms, aggn.events[e], aggn.events[e + 1]));
      MI_HIP_CHECK(hipEventElapsedTime(&c_ms, aggn.events[e + 1], aggn.events[e + 2]));
      timing_ns[0] += static_cast<int64_t>(static_cast<double>(w_ms) * 1e6);
      timing_ns[1] += static_cast<int64_t>(static_cast<double>(c_ms) * 1e6);
    }
    aggn.events.clear();
  } catch (...) {
    aggn.on = false;
    throw;
  }
  aggn.on = false;
  return selected;
}

void ArrowScan::Aggregate(const std::vector<AggSpec>& specs, AggResult* out) {
  if (initialized) throw InvalidInputException("mi_scan_aggregate replaces mi_scan_init / mi_scan_next: call it right after bind");
  Bind();
  std::vector<std::string> proj;
  aggn.keys.clear();
  BindAggregateSpecs(specs, "mi_scan_aggregate", &proj);
  if (proj.empty()) {
    // COUNT(*) alone reads no column, but a scan decodes at least one: the narrowest fixed-width column, else the first it can decode
    const ScanColumn* pick = nullptr;
    int32_t pick_w = 0;
    for (const ScanColumn& c : all_columns) {
      std::string why;
      if (c.is_constant() || c.field.has_dictionary || !c.field.Supported(&why)) continue;
      int32_t kind, w = 0;
      int64_t param;
      const bool fixed = AggClassOf(c) != aggmerge::kClassAny && c.field.Plan(&kind, &param, &w);
      if (!pick || (fixed && (pick_w == 0 || w < pick_w))) {
        pick = &c;
        pick_w = fixed ? w : 0;
      }
    }
    if (!pick) throw NotImplementedException("COUNT(*): the scan has no column it decodes without a dictionary");
    proj.push_back(pick->name);
  }
  const size_t n_aggs = aggn.aggs.size();
  const int64_t selected = DrainAggregates(proj, [&] {
    aggn.d_acc = DeviceBuffer(aggmerge::kMaxAggregates * sizeof(aggmerge::Partial));
    MI_HIP_CHECK(hipMemsetAsync(aggn.d_acc.get(), 0, aggn.d_acc.size(), ctx->stream));   // count 0: the identity of every merge
  }, g_agg_events_ns);
  std::vector<aggmerge::Partial> acc(static_cast<size_t>(aggmerge::kMaxAggregates));
  MI_HIP_CHECK(hipMemcpy(acc.data(), aggn.d_acc.get(), acc.size() * sizeof(aggmerge::Partial), hipMemcpyDeviceToHost));
  uint32_t flags = 0;
  for (size_t a = 0; a < n_aggs; a++) flags |= static_cast<uint32_t>(acc[a].flags);
  ThrowForStatus(flags);
  out->values.assign(acc.begin(), acc.begin() + static_cast<std::ptrdiff_t>(n_aggs));
  out->classes.clear();
  for (auto& b : aggn.aggs) out->classes.push_back(b.cls);
  out->rows_scanned = aggn.rows_scanned;
  out->rows_selected = selected;
}

// ------------------------------------------------------------------------------------------------ grouped aggregates
// mi_scan_group_aggregate: the aggregates above per group of 1 .. 4 key columns, for few groups (K10, kernels_group.hip).
// Every record batch gets group_windows + group_combine behind its filter; the scan-wide table -- keys, accumulators,
// group count, flags -- lives in HBM for the whole call and is copied back once at the end, where the host sorts it.
namespace {
//! groupkey::kKey* of a key column, 0 when its type stays above the scan
int32_t GroupKeyClassOf(const ScanColumn& c) {
  const ArrowField& vf = ValueField(c.field);
  int32_t kind, w;
  int64_t param;
  if (!c.field.Plan(&kind, &param, &w) || !vf.Plan(&kind, &param, &w)) return 0;
  switch (FilterClassOf(c.field)) {
    case FilterValueClass::kFloat32: case FilterValueClass::kFloat64: return 0;
    case FilterValueClass::kWide: return groupkey::kKeyWide;
    default: break;
  }
  if (IsStringKind(kind) || kind == MI_K_STRVIEW) return groupkey::kKeyString;   // (a decoded string view is a string_t row as the others are)
  if (kind == MI_K_BOOL || kind == MI_K_BOOL8) return groupkey::kKeyUnsigned;
  if (IsIntegerLike(kind, w, vf, /*allow_bool*/ false)) return vf.type == MI_AT_INT && !vf.is_signed ? groupkey::kKeyUnsigned : groupkey::kKeySigned;
  return 0;
}
}  // namespace

void GroupTimingTotals(double out_ms[2]) {
  out_ms[0] = static_cast<double>(g_group_events_ns[0].load()) * 1e-6;
  out_ms[1] = static_cast<double>(g_group_events_ns[1].load()) * 1e-6;
}

void ReadGroupTable(const void* d_table, int n_keys, int n_aggs, hipStream_t stream, GroupResult* out) {
  std::vector<uint8_t> host(device::GroupTableBytes(n_keys, n_aggs));
  MI_HIP_CHECK(hipMemcpyAsync(host.data(), d_table, host.size(), hipMemcpyDeviceToHost, stream));
  MI_HIP_CHECK(hipStreamSynchronize(stream));
  const device::GroupTableDev t = device::GroupTableAt(host.data(), n_keys, n_aggs);
  ThrowForStatus(t.head[1]);
  const size_t n = std::min<size_t>(t.head[0], groupkey::kMaxGroups);
  for (size_t g = 0; g < n; g++) {
    groupkey::Key k;
    std::memset(&k, 0, sizeof(k));
    k.nulls = t.nulls[g];
    for (int i = 0; i < n_keys; i++) {
      k.lo[i] = t.keys[(g * static_cast<size_t>(n_keys) + static_cast<size_t>(i)) * 2];
      k.hi[i] = t.keys[(g * static_cast<size_t>(n_keys) + static_cast<size_t>(i)) * 2 + 1];
    }
    out->keys.push_back(k);
    out->values.insert(out->values.end(), t.acc + g * static_cast<size_t>(n_aggs), t.acc + (g + 1) * static_cast<size_t>(n_aggs));
  }
}

void SortGroups(GroupResult* r) {
  const size_t n_aggs = r->classes.size();
  const int n_keys = static_cast<int>(r->kinds.size());
  std::vector<uint32_t> order(r->keys.size());
  for (size_t i = 0; i < order.size(); i++) order[i] = static_cast<uint32_t>(i);
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return groupkey::KeyLess(r->kinds.data(), r->keys[a], r->keys[b], n_keys); });
  std::vector<groupkey::Key> keys;
  std::vector<aggmerge::Partial> values;
  for (const uint32_t g : order) {
    keys.push_back(r->keys[g]);
    values.insert(values.end(), r->values.begin() + static_cast<std::ptrdiff_t>(g * n_aggs), r->values.begin() + static_cast<std::ptrdiff_t>((g + 1) * n_aggs));
  }
  r->keys.swap(keys);
  r->values.swap(values);
}

void FillGroupOutputs(const GroupResult& r, const std::vector<int32_t>& ops, mi_group_key_value* out_keys, mi_agg_value* out_values,
                      int32_t capacity, int32_t* n_groups) {
  const size_t n = r.keys.size(), n_keys = r.kinds.size(), n_aggs = ops.size();
  if (n_groups) *n_groups = static_cast<int32_t>(n);
  if (n > static_cast<size_t>(capacity < 0 ? 0 : capacity))
    throw InvalidInputException("GROUP BY found " + std::to_string(n) + " groups, the caller's arrays hold " + std::to_string(capacity));
  for (size_t g = 0; g < n; g++) {
    for (size_t k = 0; k < n_keys; k++) {
      mi_group_key_value& v = out_keys[g * n_keys + k];
      std::memset(&v, 0, sizeof(v));
      v.kind = r.kinds[k];
      v.is_null = (r.keys[g].nulls >> k) & 1u;
      if (v.is_null) continue;
      std::memcpy(v.bytes, &r.keys[g].lo[k], 8);   // (little-endian hosts only, as the whole library)
      std::memcpy(v.bytes + 8, &r.keys[g].hi[k], 8);
    }
    for (size_t a = 0; a < n_aggs; a++) FillAggValue(ops[a], r.classes[a], r.values[g * n_aggs + a], &out_values[g * n_aggs + a]);
  }
}

void ArrowScan::GroupAggregate(const std::vector<std::string>& keys, const std::vector<AggSpec>& specs, GroupResult* out) {
  if (initialized) throw InvalidInputException("mi_scan_group_aggregate replaces mi_scan_init / mi_scan_next: call it right after bind");
  if (keys.empty() || keys.size() > static_cast<size_t>(groupkey::kMaxKeys))
    throw InvalidInputException("mi_scan_group_aggregate takes 1 to " + std::to_string(groupkey::kMaxKeys) + " key columns, not " + std::to_string(keys.size()));
  Bind();
  std::vector<std::string> proj;
  aggn.keys.clear();
  *out = GroupResult();
  for (const std::string& name : keys) {
    if (std::count(keys.begin(), keys.end(), name) > 1) throw InvalidInputException("GROUP BY: the key column '" + name + "' is named twice");
    const ScanColumn& c = AggregateColumn(name, "GROUP BY");
    AggregateState::KeyBound kb;
    kb.cls = GroupKeyClassOf(c);
    if (kb.cls == 0)
      throw NotImplementedException("GROUP BY on column '" + name + "' (" + c.field.DuckType() + ") stays above the scan: a key is an integer, BOOLEAN, DATE, TIME / "
                                    "TIMESTAMP, DECIMAL, HUGEINT, UUID, VARCHAR or BLOB column");
    kb.col = SlotOf(&proj, name);
    aggn.keys.push_back(kb);
    out->kinds.push_back(groupkey::KindOfClass(kb.cls));
  }
  try {
    BindAggregateSpecs(specs, "mi_scan_group_aggregate", &proj);
    const int n_keys = static_cast<int>(aggn.keys.size()), n_aggs = static_cast<int>(aggn.aggs.size());
    const int64_t selected = DrainAggregates(proj, [&] {
      aggn.d_table = DeviceBuffer(device::GroupTableBytes(n_keys, n_aggs));
      MI_HIP_CHECK(device::GroupTableClear(aggn.d_table.get(), n_keys, n_aggs, ctx->stream));
    }, g_group_events_ns);
    for (auto& b : aggn.aggs) out->classes.push_back(b.cls);
    ReadGroupTable(aggn.d_table.get(), n_keys, n_aggs, ctx->stream, out);
    SortGroups(out);
    out->rows_scanned = aggn.rows_scanned;
    out->rows_selected = selected;
  } catch (...) {
    aggn.keys.clear();
    throw;
  }
  aggn.keys.clear();
}

// ------------------------------------------------------------------------------------------------ hash GROUP BY
// mi_scan_hash_aggregate: the aggregates whose merge is exact in any order per group of ONE integer key, for many groups
// (K11, kernels_hash_group.hip; the rules are hash_group.hpp).  The table is cleared on the scan's stream in the setup hook,
// every record batch gets one hash_group_rows behind its filter, and hash_group_collect runs once at the end: the head and
// exactly the records in use come back, and the host sorts them.
namespace {
std::atomic<int64_t> g_hash_events_ns[2];   // MI_AGG_TIMING=1: device time of hash_group_rows / hash_group_collect, nanoseconds
size_t HashTableBytesAligned(uint32_t max_groups, int n_aggs) { return AlignUp(hashgroup::TableBytes(max_groups, n_aggs)); }
bool AggTimingOn() {
  const char* timing = std::getenv("MI_AGG_TIMING");
  return timing && timing[0] == '1';
}
}  // namespace

void HashTimingTotals(double out_ms[2]) {
  out_ms[0] = static_cast<double>(g_hash_events_ns[0].load()) * 1e-6;
  out_ms[1] = static_cast<double>(g_hash_events_ns[1].load()) * 1e-6;
}

void AddHashTiming(int which, double ms) { g_hash_events_ns[which] += static_cast<int64_t>(ms * 1e6); }

void RefuseHashKeyClass(const std::string& who, int32_t key_cls) {
  if (key_cls == groupkey::kKeySigned || key_cls == groupkey::kKeyUnsigned) return;
  if (key_cls != groupkey::kKeyWide && key_cls != groupkey::kKeyString)   // FLOAT / DOUBLE, INTERVAL, nested ...: no grouped call takes these
    throw NotImplementedException("hash GROUP BY on " + who + " stays above the scan: the key is one integer, BOOLEAN, DATE, TIME / TIMESTAMP or DECIMAL(<=18) column");
  const char* what = key_cls == groupkey::kKeyWide ? "a 16-byte key" : "a VARCHAR / BLOB key";
  throw NotImplementedException("hash GROUP BY on " + who + ": " + what + " is not one 64-bit word -- the key is one integer, BOOLEAN, DATE, TIME / TIMESTAMP or "
                                "DECIMAL(<=18) column; mi_scan_group_aggregate takes " + what + " for few groups");
}

void RefuseHashAggregate(const std::string& who, int32_t op, int32_t cls) {
  const bool sums = op == aggmerge::kOpSum || op == aggmerge::kOpSumProduct || op == aggmerge::kOpSumExpr;
  if (sums && cls == aggmerge::kClassFloat)
    throw NotImplementedException(std::string(AggOpName(op)) + " on " + who + ": the hash GROUP BY adds in arrival order, so a floating-point sum would differ from run "
                                  "to run; mi_scan_group_aggregate keeps it bit-reproducible for few groups");
  if ((op == aggmerge::kOpMin || op == aggmerge::kOpMax) && cls == aggmerge::kClassWide)
    throw NotImplementedException(std::string(AggOpName(op)) + " on " + who + ": there is no 128-bit atomic, so MIN / MAX of a 16-byte column is not taken by the hash "
                                  "GROUP BY; mi_scan_group_aggregate takes it for few groups");
}

void CheckHashMaxGroups(const char* api, int64_t max_groups) {
  if (max_groups < 1 || max_groups > static_cast<int64_t>(hashgroup::kMaxHashGroups))
    throw InvalidInputException(std::string(api) + ": max_groups must be 1 to " + std::to_string(hashgroup::kMaxHashGroups) + " (MI_MAX_HASH_GROUPS), not " + std::to_string(max_groups));
}

size_t HashBufferBytes(uint32_t max_groups, int n_aggs) { return HashTableBytesAligned(max_groups, n_aggs) + device::HashCollectBytes(max_groups, n_aggs); }

void ClearHashBuffer(const device::GroupProgram& prog, void* d_buf, uint32_t max_groups, hipStream_t stream) {
  MI_HIP_CHECK(device::LaunchHashGroupClear(prog, device::HashTableAt(d_buf, max_groups, prog.aggs.n_aggs), stream));
}

void CollectHashGroups(const device::GroupProgram& prog, void* d_buf, uint32_t max_groups, hipStream_t stream, GroupResult* out) {
  const int n_aggs = prog.aggs.n_aggs;
  const device::HashTableDev table = device::HashTableAt(d_buf, max_groups, n_aggs);
  const device::HashCollectOut rec = device::HashCollectAt(static_cast<uint8_t*>(d_buf) + HashTableBytesAligned(max_groups, n_aggs), max_groups, n_aggs);
  const bool timed = AggTimingOn();
  HipEvent begin, end;
  if (timed) {
    begin = HipEvent::CreateTimed();
    end = HipEvent::CreateTimed();
    MI_HIP_CHECK(hipEventRecord(begin, stream));
  }
  MI_HIP_CHECK(device::LaunchHashGroupCollect(prog, table, rec, stream));
  if (timed) MI_HIP_CHECK(hipEventRecord(end, stream));
  uint32_t head[hashgroup::kHeadWords];
  MI_HIP_CHECK(hipMemcpyAsync(head, table.head, sizeof(head), hipMemcpyDeviceToHost, stream));
  MI_HIP_CHECK(hipStreamSynchronize(stream));
  if (timed) {
    float ms = 0;
    MI_HIP_CHECK(hipEventElapsedTime(&ms, begin, end));
    AddHashTiming(1, ms);
  }
  const uint32_t status = head[hashgroup::kHeadStatus];
  if (status & MI_ST_GROUP_LIMIT)
    throw NotImplementedException("hash GROUP BY found more than max_groups = " + std::to_string(max_groups) + " distinct keys among the selected rows: call again with a larger "
                                  "max_groups (at most " + std::to_string(hashgroup::kMaxHashGroups) + ")");
  ThrowForStatus(status);
  const size_t n = std::min<size_t>(head[hashgroup::kHeadCollected], max_groups);
  if (n == 0) return;
  std::vector<uint64_t> keys(n);
  std::vector<uint32_t> nulls(n);
  const size_t v0 = out->values.size();
  out->values.resize(v0 + n * static_cast<size_t>(n_aggs));
  MI_HIP_CHECK(hipMemcpyAsync(keys.data(), rec.keys, n * 8, hipMemcpyDeviceToHost, stream));
  MI_HIP_CHECK(hipMemcpyAsync(nulls.data(), rec.nulls, n * 4, hipMemcpyDeviceToHost, stream));
  MI_HIP_CHECK(hipMemcpyAsync(out->values.data() + v0, rec.partials, n * static_cast<size_t>(n_aggs) * sizeof(aggmerge::Partial), hipMemcpyDeviceToHost, stream));
  MI_HIP_CHECK(hipStreamSynchronize(stream));
  const int key_cls = prog.keys[0].cls;
  out->keys.reserve(out->keys.size() + n);
  for (size_t g = 0; g < n; g++) {
    groupkey::Key k;
    std::memset(&k, 0, sizeof(k));
    k.nulls = nulls[g] ? 1u : 0u;
    if (!k.nulls) {
      k.lo[0] = keys[g];
      k.hi[0] = hashgroup::KeyHigh(key_cls, keys[g]);
    }
    out->keys.push_back(k);
  }
}

void ArrowScan::HashAggregate(const std::string& key, const std::vector<AggSpec>& specs, uint32_t max_groups, GroupResult* out) {
  if (initialized) throw InvalidInputException("mi_scan_hash_aggregate replaces mi_scan_init / mi_scan_next: call it right after bind");
  CheckHashMaxGroups("mi_scan_hash_aggregate", max_groups);
  Bind();
  std::vector<std::string> proj;
  aggn.keys.clear();
  *out = GroupResult();
  const ScanColumn& c = AggregateColumn(key, "GROUP BY");
  AggregateState::KeyBound kb;
  kb.cls = GroupKeyClassOf(c);
  RefuseHashKeyClass("column '" + key + "' (" + c.field.DuckType() + ")", kb.cls);
  kb.col = SlotOf(&proj, key);
  out->kinds.push_back(groupkey::kKindInt128);
  out->key_cls = kb.cls;
  try {
    BindAggregateSpecs(specs, "mi_scan_hash_aggregate", &proj);
    for (size_t a = 0; a < aggn.aggs.size(); a++) {
      const AggregateState::Bound& b = aggn.aggs[a];
      if (b.col_a < 0) continue;   // COUNT(*)
      const std::string& name = proj[static_cast<size_t>(b.col_a)];
      const ScanColumn& ac = AggregateColumn(name, AggOpName(b.op));
      RefuseHashAggregate("column '" + name + "' (" + ac.field.DuckType() + ")", b.op, b.cls);
    }
    aggn.keys.push_back(kb);
    aggn.hash_max_groups = max_groups;
    const int n_aggs = static_cast<int>(aggn.aggs.size());
    device::GroupProgram shape;   // what the clear and the collect read of a program: the operations and classes
    std::memset(&shape, 0, sizeof(shape));
    shape.n_keys = 1;
    shape.keys[0].cls = kb.cls;
    shape.aggs.n_aggs = n_aggs;
    for (int a = 0; a < n_aggs; a++) {
      shape.aggs.aggs[a].op = aggn.aggs[static_cast<size_t>(a)].op;
      shape.aggs.aggs[a].a.cls = aggn.aggs[static_cast<size_t>(a)].cls;
    }
    std::atomic<int64_t> batch_ns[2];   // [0] hash_group_rows; [1] the empty interval behind it, which is nobody's time
    batch_ns[0] = 0;
    batch_ns[1] = 0;
    const int64_t selected = DrainAggregates(proj, [&] {
      aggn.d_hash = DeviceBuffer(HashBufferBytes(max_groups, n_aggs));
      ClearHashBuffer(shape, aggn.d_hash.get(), max_groups, ctx->stream);   // on the scan's own stream, never the null stream
    }, batch_ns);
    g_hash_events_ns[0] += batch_ns[0].load();
    for (auto& b : aggn.aggs) out->classes.push_back(b.cls);
    CollectHashGroups(shape, aggn.d_hash.get(), max_groups, ctx->stream, out);
    SortGroups(out);
    out->rows_scanned = aggn.rows_scanned;
    out->rows_selected = selected;
  } catch (...) {
    aggn.keys.clear();
    aggn.hash_max_groups = 0;
    aggn.d_hash = DeviceBuffer();
    throw;
  }
  aggn.keys.clear();
  aggn.hash_max_groups = 0;
  aggn.d_hash = DeviceBuffer();
}

// ---- per record batch: the programs over the slot's decoded vectors, then the two launches
bool ArrowScan::FillAggregatePrograms(const Slot& s, device::GroupProgram* gprog, device::AggExprTable* exprs) const {
  auto column = [&](int32_t c, const void** data, const uint64_t** validity, int32_t* width) {
    // (a column that this file lacks was refused by EnqueueBatch before anything was queued: col_root is a node here)
    const PlannedNode& o = s.planner.nodes[static_cast<size_t>(s.col_root[static_cast<size_t>(c)])];
    *data = o.alias_body_off >= 0 ? static_cast<const void*>(s.d_in.get() + o.alias_body_off) : static_cast<const void*>(s.d_out.get() + o.data_off);
    *validity = o.valid_off >= 0 ? reinterpret_cast<const uint64_t*>(s.d_out.get() + o.valid_off) : nullptr;
    *width = o.width;
  };
  std::memset(gprog, 0, sizeof(*gprog));
  bool has_expr = false;   // (the table is filled, and handed to the launches, only when an aggregate is an expression)
  device::AggProgram& prog = gprog->aggs;
  prog.n_aggs = static_cast<int32_t>(aggn.aggs.size());
  for (size_t a = 0; a < aggn.aggs.size(); a++) {
    const AggregateState::Bound& b = aggn.aggs[a];
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
  gprog->n_keys = static_cast<int32_t>(aggn.keys.size());
  for (size_t k = 0; k < aggn.keys.size(); k++) {
    device::GroupKeyColumnDev& kc = gprog->keys[k];
    kc.cls = aggn.keys[k].cls;
    column(aggn.keys[k].col, &kc.data, &kc.validity, &kc.width);
  }
  return has_expr;
}

void ArrowScan::EnqueueAggregates(Slot& s) {
  const int64_t n = s.nrows;
  const int64_t n_windows = (n + MI_VECTOR_SIZE - 1) / MI_VECTOR_SIZE;
  device::GroupProgram gprog;
  device::AggExprTable exprs_table;
  const device::AggExprTable* exprs = FillAggregatePrograms(s, &gprog, &exprs_table) ? &exprs_table : nullptr;
  const device::AggProgram& prog = gprog.aggs;
  const mi_sel_t* sel = has_filter ? reinterpret_cast<const mi_sel_t*>(s.d_out.get() + s.sel_off) : nullptr;
  const uint32_t* sel_count = has_filter ? reinterpret_cast<const uint32_t*>(s.d_out.get() + s.sel_count_off) : nullptr;
  auto stamp = [&] {
    if (!aggn.timed) return;
    aggn.events.push_back(HipEvent::CreateTimed());
    MI_HIP_CHECK(hipEventRecord(aggn.events.back(), ctx->stream));
  };
  if (aggn.hash_max_groups != 0) {   // K11: one launch; the stamps keep DrainAggregates' three-per-batch shape
    stamp();
    MI_HIP_CHECK(device::LaunchHashGroupRows(gprog, sel, sel_count, n, device::HashTableAt(aggn.d_hash.get(), aggn.hash_max_groups, prog.n_aggs), ctx->stream, exprs));
    stamp();
    stamp();
    aggn.rows_scanned += n;
    return;
  }
  if (!aggn.keys.empty()) {
    const size_t bytes = device::GroupWindowsBytes(n_windows, gprog.n_keys, prog.n_aggs);
    Retire(Grow(aggn.d_windows, bytes, GrownCapacity(bytes, aggn.d_windows.size(), 1 << 16)));
    const device::GroupWindowsOut win = device::GroupWindowsAt(aggn.d_windows.get(), n_windows, gprog.n_keys, prog.n_aggs);
    stamp();
    MI_HIP_CHECK(device::LaunchGroupWindows(gprog, sel, sel_count, n, win, ctx->stream, exprs));
    stamp();
    MI_HIP_CHECK(device::LaunchGroupCombine(gprog, win, n_windows, device::GroupTableAt(aggn.d_table.get(), gprog.n_keys, prog.n_aggs), ctx->stream, exprs));
    stamp();
    aggn.rows_scanned += n;
    return;
  }
  const size_t bytes = static_cast<size_t>(n_windows) * aggn.aggs.size() * sizeof(aggmerge::Partial);
  Retire(Grow(aggn.d_partials, bytes, GrownCapacity(bytes, aggn.d_partials.size(), 1 << 12)));
  aggmerge::Partial* partials = aggn.d_partials.get<aggmerge::Partial>();
  stamp();
  MI_HIP_CHECK(device::LaunchAggWindows(prog, sel, sel_count, n, partials, ctx->stream, exprs));
  stamp();
  MI_HIP_CHECK(device::LaunchAggCombine(prog, partials, n_windows, aggn.d_acc.get<aggmerge::Partial>(), ctx->stream, exprs));
  stamp();
  aggn.rows_scanned += n;
}

// ------------------------------------------------------------------------------------------------ multi-device
void MultiDeviceScan::Aggregate(const std::vector<AggSpec>& specs, AggResult* out) {
  std::vector<AggResult> parts(subs.size());
  ForEachParallel([&](size_t i) { subs[i]->Aggregate(specs, &parts[i]); });
  // sub-scan order, by the rules the kernels merge by: the double sums come out the same for the same device count
  *out = AggResult();
  out->values.assign(specs.size(), aggmerge::Partial{0, 0, 0, 0});
  out->classes = parts[0].classes;
  for (auto& p : parts) {
    for (size_t a = 0; a < specs.size(); a++) aggmerge::Merge(specs[a].op, out->classes[a], &out->values[a], p.values[a]);
    out->rows_scanned += p.rows_scanned;
    out->rows_selected += p.rows_selected;
  }
}

void MultiDeviceScan::GroupAggregate(const std::vector<std::string>& keys, const std::vector<AggSpec>& specs, GroupResult* out) {
  std::vector<GroupResult> parts(subs.size());
  ForEachParallel([&](size_t i) { subs[i]->GroupAggregate(keys, specs, &parts[i]); });
  // sub-scan order, group by group, by the rules the kernels merge by (groupkey::GroupTable)
  *out = GroupResult();
  out->kinds = parts[0].kinds;
  out->classes = parts[0].classes;
  std::vector<int> ops, classes(out->classes.begin(), out->classes.end());
  for (const AggSpec& sp : specs) ops.push_back(sp.op);
  groupkey::GroupTable table(static_cast<int>(keys.size()), ops, classes);
  const size_t n_aggs = specs.size();
  for (auto& p : parts) {
    for (size_t g = 0; g < p.keys.size(); g++)
      if (!table.Merge(p.keys[g], &p.values[g * n_aggs])) ThrowForStatus(MI_ST_GROUP_LIMIT);
    out->rows_scanned += p.rows_scanned;
    out->rows_selected += p.rows_selected;
  }
  for (size_t g = 0; g < table.size(); g++) {
    out->keys.push_back(table.key(g));
    out->values.insert(out->values.end(), table.partials(g), table.partials(g) + n_aggs);
  }
  SortGroups(out);
}

void MultiDeviceScan::HashAggregate(const std::string& key, const std::vector<AggSpec>& specs, uint32_t max_groups, GroupResult* out) {
  CheckHashMaxGroups("mi_scan_hash_aggregate", max_groups);
  std::vector<GroupResult> parts(subs.size());
  ForEachParallel([&](size_t i) { subs[i]->HashAggregate(key, specs, max_groups, &parts[i]); });
  // sub-scan order, group by group, through the serial model of the device's table (hashgroup::SerialTable)
  *out = GroupResult();
  out->kinds = parts[0].kinds;
  out->classes = parts[0].classes;
  std::vector<int> ops, classes(out->classes.begin(), out->classes.end());
  for (const AggSpec& sp : specs) ops.push_back(sp.op);
  hashgroup::SerialTable table(max_groups, ops, classes);
  const size_t n_aggs = specs.size();
  for (auto& p : parts) {
    for (size_t g = 0; g < p.keys.size(); g++)
      if (!table.Merge(p.keys[g].lo[0], (p.keys[g].nulls & 1u) != 0, &p.values[g * n_aggs]))
        throw NotImplementedException("hash GROUP BY found more than max_groups = " + std::to_string(max_groups) + " distinct keys among the selected rows of the "
                                      "devices together: call again with a larger max_groups");
    out->rows_scanned += p.rows_scanned;
    out->rows_selected += p.rows_selected;
  }
  const int key_cls = parts[0].key_cls;   // (one column, one class: every sub-scan bound the same)
  out->key_cls = key_cls;
  for (size_t g = 0; g < table.size(); g++) {
    groupkey::Key k;
    std::memset(&k, 0, sizeof(k));
    k.nulls = table.is_null(g) ? 1u : 0u;
    if (!k.nulls) {
      k.lo[0] = table.key(g);
      k.hi[0] = hashgroup::KeyHigh(key_cls, k.lo[0]);
    }
    out->keys.push_back(k);
    out->values.insert(out->values.end(), table.partials(g), table.partials(g) + n_aggs);
  }
  SortGroups(out);
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

//! launches by this process and, with MI_AGG_TIMING=1, their summed device time: of K9 or of K10
int Counters(void (*launches)(int64_t[2]), void (*timing)(double[2]), int64_t* window_launches, int64_t* combine_launches, double* windows_ms,
             double* combine_ms) {
  return WrapC([&] {
    int64_t n[2];
    double ms[2];
    launches(n);
    timing(ms);
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
  return Counters(device::AggLaunchCounts, AggTimingTotals, window_launches, combine_launches, windows_ms, combine_ms);
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
    std::vector<int32_t> ops;
    for (const AggSpec& sp : specs) ops.push_back(sp.op);
    FillGroupOutputs(r, ops, out_keys, out_values, capacity, n_groups);
    if (rows_scanned) *rows_scanned = r.rows_scanned;
    if (rows_selected) *rows_selected = r.rows_selected;
  });
}

int mi_group_aggregate_counters(int64_t* window_launches, int64_t* combine_launches, double* windows_ms, double* combine_ms) {
  return Counters(device::GroupLaunchCounts, GroupTimingTotals, window_launches, combine_launches, windows_ms, combine_ms);
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
    std::vector<int32_t> ops;
    for (const AggSpec& sp : specs) ops.push_back(sp.op);
    FillGroupOutputs(r, ops, out_keys, out_values, capacity, n_groups);
    if (rows_scanned) *rows_scanned = r.rows_scanned;
    if (rows_selected) *rows_selected = r.rows_selected;
  });
}

int mi_hash_aggregate_counters(int64_t* rows_launches, int64_t* collect_launches, double* rows_ms, double* collect_ms) {
  return Counters(device::HashGroupLaunchCounts, HashTimingTotals, rows_launches, collect_launches, rows_ms, collect_ms);
}

}  // extern "C"
