// agg_bind.cpp -- see agg_bind.hpp.
#include "agg_bind.hpp"

#include <algorithm>

namespace miarrow {

namespace {
//! a column an aggregate (or GROUP BY, `what`) may read
const ScanColumn& AggregateColumn(const std::vector<ScanColumn>& columns, const std::string& name, const std::string& what) {
  auto it = std::find_if(columns.begin(), columns.end(), [&](const ScanColumn& sc) { return sc.name == name; });
  if (it == columns.end()) throw InvalidInputException(what + ": Field '" + name + "' does not exist in IPC file schema");
  const std::string typed = "'" + name + "' (" + it->field.DuckType() + ")";   // every refusal names the column and its DuckDB type
  if (it->is_constant()) throw NotImplementedException(what + " on the constant column " + typed + " is not computed in the scan");
  std::string why;
  if (!it->field.Supported(&why)) throw NotImplementedException(what + " on column " + typed + ": " + why + " is not decoded by the MI355X scan path yet");
  if (it->field.has_dictionary || ValueField(it->field).has_dictionary)
    throw NotImplementedException(what + " on the dictionary-encoded column " + typed + " is not computed in the scan");
  // a union's vector is a tag vector over member vectors: no aggregate (COUNT included) and no GROUP BY key reads that tree
  if (it->field.type == MI_AT_UNION) throw NotImplementedException(what + " on the union column " + typed + " is not computed in the scan");
  return *it;
}

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

//! a factor of SUM_PRODUCT / SUM_EXPR (`op`): a column an aggregate may read, of a class a product takes, which goes to *cls
const ScanColumn& FactorColumn(const std::vector<ScanColumn>& columns, const std::string& name, int32_t op, int32_t* cls) {
  const ScanColumn& c = AggregateColumn(columns, name, AggOpName(op));
  *cls = AggClassOf(c);
  if (*cls == aggmerge::kClassAny || *cls == aggmerge::kClassWide)
    throw NotImplementedException(std::string(AggOpName(op)) + " on column '" + name + "' (" + c.field.DuckType() + "): a factor is an integer, DATE, TIME / "
                                  "TIMESTAMP, DECIMAL(<=18), FLOAT or DOUBLE column");
  return c;
}

//! validates `specs` into plan->aggs and adds the columns they read to the projection; `api` begins the messages
void BindAggregateSpecs(const std::vector<ScanColumn>& columns, const std::vector<AggSpec>& specs, const char* api, BoundAggregates* plan) {
  if (specs.empty() || specs.size() > static_cast<size_t>(aggmerge::kMaxAggregates))
    throw InvalidInputException(std::string(api) + " takes 1 to " + std::to_string(aggmerge::kMaxAggregates) + " aggregates, not " + std::to_string(specs.size()));
  for (const AggSpec& sp : specs) {
    BoundAgg b;
    b.op = sp.op;
    if (sp.op == aggmerge::kOpCountStar) {
      plan->aggs.push_back(b);
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
        const ScanColumn& c = FactorColumn(columns, sp.factors[f].column, sp.op, &b.factors[f].cls);
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
        BoundAgg::Factor& fb = b.factors[f];
        ExprFactorConstants(std::string(AggOpName(sp.op)) + (fs.has_column ? " on column '" + fs.column + "'" : std::string(" constant factor")), b.cls == aggmerge::kClassFloat,
                            fs.constants, fs.mul, fs.add, fs.fmul, fs.fadd, &fb.mul, &fb.add);
        if (!fs.has_column) continue;
        fb.col = SlotOf(&plan->projection, fs.column);
        if (b.col_a < 0) b.col_a = fb.col;
      }
      plan->aggs.push_back(b);
      continue;
    }
    const ScanColumn& ca = AggregateColumn(columns, sp.a, AggOpName(sp.op));
    if (sp.op != aggmerge::kOpCount) {
      b.cls = AggClassOf(ca);
      const bool sums = sp.op == aggmerge::kOpSum || sp.op == aggmerge::kOpSumProduct;
      if (b.cls == aggmerge::kClassAny || (sums && b.cls == aggmerge::kClassWide))
        throw NotImplementedException(std::string(AggOpName(sp.op)) + " on column '" + sp.a + "' (" + ca.field.DuckType() + "): SUM takes integers, DATE, TIME / "
                                      "TIMESTAMP, DECIMAL(<=18), FLOAT and DOUBLE columns, MIN / MAX those and HUGEINT / DECIMAL(19..38) / UUID");
      if (sp.op == aggmerge::kOpSumProduct) {
        const ScanColumn& cb = FactorColumn(columns, sp.b, sp.op, &b.cls_b);
        SameFamily(sp.op, ca, b.cls, cb, b.cls_b);
      }
    }
    b.col_a = SlotOf(&plan->projection, sp.a);
    if (sp.op == aggmerge::kOpSumProduct) b.col_b = SlotOf(&plan->projection, sp.b);
    plan->aggs.push_back(b);
  }
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

BoundAggregates BindAggregates(const std::vector<ScanColumn>& columns, const std::vector<AggSpec>& specs) {
  BoundAggregates plan;
  BindAggregateSpecs(columns, specs, "mi_scan_aggregate", &plan);
  if (!plan.projection.empty()) return plan;
  // COUNT(*) alone reads no column, but a scan decodes at least one: the narrowest fixed-width column, else the first it can decode
  const ScanColumn* pick = nullptr;
  int32_t pick_w = 0;
  for (const ScanColumn& c : columns) {
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
  plan.projection.push_back(pick->name);
  return plan;
}

BoundAggregates BindGroupAggregates(const std::vector<ScanColumn>& columns, const std::vector<std::string>& keys, const std::vector<AggSpec>& specs) {
  if (keys.empty() || keys.size() > static_cast<size_t>(groupkey::kMaxKeys))
    throw InvalidInputException("mi_scan_group_aggregate takes 1 to " + std::to_string(groupkey::kMaxKeys) + " key columns, not " + std::to_string(keys.size()));
  BoundAggregates plan;
  plan.mode = AggMode::kGrouped;
  for (const std::string& name : keys) {
    if (std::count(keys.begin(), keys.end(), name) > 1) throw InvalidInputException("GROUP BY: the key column '" + name + "' is named twice");
    const ScanColumn& c = AggregateColumn(columns, name, "GROUP BY");
    BoundKey kb;
    kb.cls = GroupKeyClassOf(c);
    if (kb.cls == 0)
      throw NotImplementedException("GROUP BY on column '" + name + "' (" + c.field.DuckType() + ") stays above the scan: a key is an integer, BOOLEAN, DATE, TIME / "
                                    "TIMESTAMP, DECIMAL, HUGEINT, UUID, VARCHAR or BLOB column");
    kb.col = SlotOf(&plan.projection, name);
    plan.keys.push_back(kb);
  }
  BindAggregateSpecs(columns, specs, "mi_scan_group_aggregate", &plan);
  return plan;
}

BoundAggregates BindHashAggregates(const std::vector<ScanColumn>& columns, const std::string& key, const std::vector<AggSpec>& specs, int64_t max_groups) {
  CheckHashMaxGroups("mi_scan_hash_aggregate", max_groups);
  BoundAggregates plan;
  plan.mode = AggMode::kHash;
  plan.max_groups = static_cast<uint32_t>(max_groups);
  const ScanColumn& c = AggregateColumn(columns, key, "GROUP BY");
  BoundKey kb;
  kb.cls = GroupKeyClassOf(c);
  RefuseHashKeyClass("column '" + key + "' (" + c.field.DuckType() + ")", kb.cls);
  kb.col = SlotOf(&plan.projection, key);
  plan.keys.push_back(kb);
  BindAggregateSpecs(columns, specs, "mi_scan_hash_aggregate", &plan);
  for (const BoundAgg& b : plan.aggs) {
    if (b.col_a < 0) continue;   // COUNT(*)
    const std::string& name = plan.projection[static_cast<size_t>(b.col_a)];
    const ScanColumn& ac = AggregateColumn(columns, name, AggOpName(b.op));
    RefuseHashAggregate("column '" + name + "' (" + ac.field.DuckType() + ")", b.op, b.cls);
  }
  return plan;
}

}  // namespace miarrow
