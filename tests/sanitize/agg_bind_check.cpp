// agg_bind_check.cpp -- bind time and result side of the fused aggregates (duckdb-arrow_amd/csrc/agg_bind.cpp, agg_result.cpp)
// without a GPU, under AddressSanitizer + UBSan (test infrastructure, never shipped).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include
//       tests/sanitize/agg_bind_check.cpp duckdb-arrow_amd/csrc/agg_bind.cpp duckdb-arrow_amd/csrc/agg_result.cpp
//       duckdb-arrow_amd/csrc/ipc_format.cpp
//
// Every expected value below is a literal: classes and slots from the rules of a bind (agg_bind.hpp), message texts as the calls
// gave them before bind time was a unit of its own, merged values by hand from agg_merge.hpp's rules.  Every refusal stands beside
// a twin that differs in the one thing refused and binds.  Prints "<n> checks, <failed> failed"; exit 1 on a failure.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../duckdb-arrow_amd/csrc/agg_bind.hpp"
#include "../../duckdb-arrow_amd/csrc/agg_result.hpp"
#include "../../duckdb-arrow_amd/csrc/extension_format.hpp"

using namespace miarrow;
using aggmerge::Partial;

namespace {
int g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                    \
  do {                                      \
    g_checks++;                             \
    if (!(cond)) {                          \
      std::fprintf(stderr, "FAILED: ");     \
      std::fprintf(stderr, __VA_ARGS__);    \
      std::fprintf(stderr, "\n");           \
      g_failed++;                           \
    }                                       \
  } while (0)

enum { kCountStar = 1, kCount, kSum, kSumProduct, kMin, kMax, kSumExpr };   // MI_AGG_*
enum { kAny = 0, kSigned, kUnsigned, kFloat, kWide };                       // MI_AGG_CLASS_*
enum { kKeySigned = 1, kKeyUnsigned, kKeyWide, kKeyString };                // MI_GROUP_KEY_CLASS_*

// ------------------------------------------------------------------------------------------------ columns
template <typename Fill>
ScanColumn Col(const std::string& name, int32_t type, Fill&& fill) {
  ScanColumn c;
  c.name = name;
  c.field.name = name;
  c.field.type = type;
  fill(c.field);
  return c;
}
ScanColumn Int(const std::string& name, int bits, bool is_signed) {
  return Col(name, MI_AT_INT, [&](ArrowField& f) { f.bit_width = bits; f.is_signed = is_signed; });
}
ScanColumn Decimal(const std::string& name, int bits, int precision) {
  return Col(name, MI_AT_DECIMAL, [&](ArrowField& f) { f.bit_width = bits; f.precision = precision; f.scale = 2; });
}
ScanColumn Plain(const std::string& name, int32_t type, int unit = 0) {
  return Col(name, type, [&](ArrowField& f) { f.unit = unit; });
}
ScanColumn RunEnd(const std::string& name, const ScanColumn& values) {
  return Col(name, MI_AT_RUN_END, [&](ArrowField& f) { f.children = {Int("run_ends", 32, true).field, values.field}; });
}

// every column type the scan binds, and the ones a bind refuses
std::vector<ScanColumn> Columns() {
  std::vector<ScanColumn> v;
  for (int bits : {8, 16, 32, 64}) {
    v.push_back(Int("i" + std::to_string(bits), bits, true));
    v.push_back(Int("u" + std::to_string(bits), bits, false));
  }
  v.push_back(Plain("date32", MI_AT_DATE, 0));
  v.push_back(Plain("date64", MI_AT_DATE, 1));
  v.push_back(Plain("time_s", MI_AT_TIME, 0));
  v.push_back(Plain("time_ns", MI_AT_TIME, 3));
  v.push_back(Plain("ts", MI_AT_TIMESTAMP, 2));
  v.push_back(Col("tstz", MI_AT_TIMESTAMP, [](ArrowField& f) { f.unit = 1; f.timezone = "UTC"; }));
  v.push_back(Decimal("dec4", 128, 4));
  v.push_back(Decimal("dec9", 32, 9));
  v.push_back(Decimal("dec18", 64, 18));
  v.push_back(Decimal("dec19", 128, 19));
  v.push_back(Decimal("dec38", 128, 38));
  v.push_back(Col("uuid", MI_AT_FIXED_BINARY, [](ArrowField& f) { f.byte_width = 16; f.extension = extfmt::kUuid; }));
  v.push_back(Col("f32", MI_AT_FLOAT, [](ArrowField& f) { f.precision = 1; }));
  v.push_back(Col("f64", MI_AT_FLOAT, [](ArrowField& f) { f.precision = 2; }));
  v.push_back(Plain("flag", MI_AT_BOOL));
  v.push_back(Col("flag8", MI_AT_INT, [](ArrowField& f) { f.bit_width = 8; f.is_signed = true; f.extension = extfmt::kBool8; }));
  v.push_back(Plain("s", MI_AT_UTF8));
  v.push_back(Plain("blob", MI_AT_LARGE_BINARY));
  v.push_back(Plain("view", MI_AT_UTF8_VIEW));
  v.push_back(Col("fixed", MI_AT_FIXED_BINARY, [](ArrowField& f) { f.byte_width = 7; }));
  v.push_back(RunEnd("ree_u16", Int("values", 16, false)));
  v.push_back(RunEnd("ree_f64", Col("values", MI_AT_FLOAT, [](ArrowField& f) { f.precision = 2; })));
  v.push_back(RunEnd("ree_dec38", Decimal("values", 128, 38)));
  v.push_back(RunEnd("ree_s", Plain("values", MI_AT_UTF8)));
  // what a bind refuses
  v.push_back(Plain("dur", MI_AT_DURATION, 2));
  v.push_back(Plain("day_time", MI_AT_INTERVAL, 1));
  v.push_back(Col("dict", MI_AT_UTF8, [](ArrowField& f) { f.has_dictionary = true; }));
  v.push_back(Col("dict_i64", MI_AT_INT, [](ArrowField& f) { f.bit_width = 64; f.is_signed = true; f.has_dictionary = true; }));
  v.push_back(RunEnd("ree_dict", Col("values", MI_AT_UTF8, [](ArrowField& f) { f.has_dictionary = true; })));
  v.push_back(Col("un", MI_AT_UNION, [](ArrowField& f) { f.children = {Int("a", 32, true).field, Plain("b", MI_AT_UTF8).field}; }));
  v.push_back(Col("filename", MI_AT_UTF8, [](ArrowField&) {}));
  v.back().is_filename = true;
  v.push_back(Col("year", MI_AT_UTF8, [](ArrowField&) {}));
  v.back().is_hive = true;
  return v;
}

// ------------------------------------------------------------------------------------------------ specs and what a bind said
AggSpec Agg(int32_t op, const std::string& a = "", const std::string& b = "") {
  AggSpec sp;
  sp.op = op;
  sp.a = a;
  sp.b = b;
  return sp;
}
AggFactorSpec Factor(const std::string& column, int64_t mul = 1, int64_t add = 0) {
  AggFactorSpec f;
  f.has_column = true;
  f.column = column;
  f.mul = mul;
  f.add = add;
  return f;
}
AggFactorSpec Constant(int64_t add) {
  AggFactorSpec f;
  f.add = add;
  return f;
}
AggFactorSpec DoubleFactor(const std::string& column, double fmul, double fadd) {
  AggFactorSpec f = Factor(column);
  f.constants = MI_AGG_CONST_DOUBLE;
  f.fmul = fmul;
  f.fadd = fadd;
  return f;
}
AggSpec Expr(std::vector<AggFactorSpec> factors) {
  AggSpec sp = Agg(kSumExpr);
  sp.factors = std::move(factors);
  return sp;
}

// "" when `f` returns, else "<code>: <message>"
template <typename F>
std::string Said(F&& f) {
  try {
    f();
  } catch (const Exception& e) {
    return std::to_string(e.code) + ": " + e.what();
  }
  return "";
}
std::string Invalid(const std::string& m) { return std::to_string(MI_EINVAL) + ": " + m; }
std::string NotSup(const std::string& m) { return std::to_string(MI_ENOTSUP) + ": " + m; }

const std::vector<ScanColumn> kCols = Columns();

std::string SaidPlain(const std::vector<AggSpec>& specs) { return Said([&] { BindAggregates(kCols, specs); }); }
std::string SaidGroup(const std::vector<std::string>& keys, const std::vector<AggSpec>& specs) { return Said([&] { BindGroupAggregates(kCols, keys, specs); }); }
std::string SaidHash(const std::string& key, const std::vector<AggSpec>& specs, int64_t max_groups = 1000) {
  return Said([&] { BindHashAggregates(kCols, key, specs, max_groups); });
}
void Expect(const char* what, const std::string& said, const std::string& want) {
  CHECK(said == want, "%s: '%s', not '%s'", what, said.c_str(), want.c_str());
}
// the refusal of `bad` through all three calls (the texts differ in nothing but the call's name, where it has one), beside `good`
void RefusedEverywhere(const char* what, const AggSpec& good, const AggSpec& bad, const std::string& want) {
  Expect(what, SaidPlain({good}), "");
  Expect(what, SaidGroup({"i32"}, {good}), "");
  Expect(what, SaidHash("i32", {good}), "");
  Expect(what, SaidPlain({bad}), want);
  Expect(what, SaidGroup({"i32"}, {bad}), want);
  Expect(what, SaidHash("i32", {bad}), want);
}

// ------------------------------------------------------------------------------------------------ bind: refusals
void CheckColumnRefusals() {
  // what AggregateColumn says of a column, for an aggregate (the operation begins the message) and for a key (GROUP BY does)
  struct Row {
    const char* column;
    std::string tail;   // behind "<what>"
    int code;
  };
  const Row rows[] = {
      {"nope", ": Field 'nope' does not exist in IPC file schema", MI_EINVAL},
      {"filename", " on the constant column 'filename' (VARCHAR) is not computed in the scan", MI_ENOTSUP},
      {"year", " on the constant column 'year' (VARCHAR) is not computed in the scan", MI_ENOTSUP},
      {"day_time", " on column 'day_time' (INTERVAL): Arrow type tiD of field 'day_time' is not decoded by the MI355X scan path yet", MI_ENOTSUP},
      {"dict", " on the dictionary-encoded column 'dict' (VARCHAR) is not computed in the scan", MI_ENOTSUP},
      {"dict_i64", " on the dictionary-encoded column 'dict_i64' (BIGINT) is not computed in the scan", MI_ENOTSUP},
      // (run-end encoded over dictionary values has no transcode plan at all: the scan's own refusal speaks first)
      {"ree_dict", " on column 'ree_dict' (VARCHAR): Arrow type +r of field 'ree_dict' is not decoded by the MI355X scan path yet", MI_ENOTSUP},
      {"un", " on the union column 'un' (UNION(a INTEGER, b VARCHAR)) is not computed in the scan", MI_ENOTSUP},
  };
  for (const Row& r : rows) {
    const std::string code = std::to_string(r.code) + ": ";
    RefusedEverywhere(r.column, Agg(kCount, "s"), Agg(kCount, r.column), code + "COUNT" + r.tail);
    RefusedEverywhere(r.column, Agg(kMin, "i64"), Agg(kMin, r.column), code + "MIN" + r.tail);
    RefusedEverywhere(r.column, Agg(kSumProduct, "i64", "i8"), Agg(kSumProduct, "i64", r.column), code + "SUM_PRODUCT" + r.tail);
    RefusedEverywhere(r.column, Expr({Factor("i64")}), Expr({Factor("i64"), Factor(r.column)}), code + "SUM_EXPR" + r.tail);
    Expect(r.column, SaidGroup({"i64", r.column}, {Agg(kCountStar)}), code + "GROUP BY" + r.tail);
    Expect(r.column, SaidHash(r.column, {Agg(kCountStar)}), code + "GROUP BY" + r.tail);
  }
  Expect("valid keys", SaidGroup({"i64", "s"}, {Agg(kCountStar)}), "");
  Expect("valid key", SaidHash("i64", {Agg(kCountStar)}), "");
}

void CheckClassRefusals() {
  const std::string sum_tail = "): SUM takes integers, DATE, TIME / TIMESTAMP, DECIMAL(<=18), FLOAT and DOUBLE columns, MIN / MAX those and HUGEINT / DECIMAL(19..38) / UUID";
  const std::string factor_tail = "): a factor is an integer, DATE, TIME / TIMESTAMP, DECIMAL(<=18), FLOAT or DOUBLE column";
  // wide columns: MIN / MAX take them, no sum does
  const char* wide[][2] = {{"dec19", "DECIMAL(19,2)"}, {"dec38", "DECIMAL(38,2)"}, {"uuid", "UUID"}, {"ree_dec38", "DECIMAL(38,2)"}};
  for (auto& w : wide) {
    const std::string typed = std::string("'") + w[0] + "' (" + w[1];
    Expect(w[0], SaidPlain({Agg(kMin, w[0]), Agg(kMax, w[0]), Agg(kCount, w[0])}), "");
    Expect(w[0], SaidPlain({Agg(kSum, w[0])}), NotSup("SUM on column " + typed + sum_tail));
    Expect(w[0], SaidGroup({"i8"}, {Agg(kSumProduct, w[0], "i64")}), NotSup("SUM_PRODUCT on column " + typed + sum_tail));
    Expect(w[0], SaidPlain({Agg(kSumProduct, "i64", w[0])}), NotSup("SUM_PRODUCT on column " + typed + factor_tail));
    Expect(w[0], SaidHash("i8", {Expr({Factor(w[0])})}), NotSup("SUM_EXPR on column " + typed + factor_tail));
  }
  // columns of no orderable class: COUNT alone
  const char* other[][2] = {{"flag", "BOOLEAN"}, {"flag8", "BOOLEAN"}, {"s", "VARCHAR"}, {"blob", "BLOB"}, {"view", "VARCHAR"}, {"fixed", "BLOB"},
                            {"ree_s", "VARCHAR"}, {"dur", "INTERVAL"}};
  for (auto& o : other) {
    const std::string typed = std::string("'") + o[0] + "' (" + o[1];
    Expect(o[0], SaidPlain({Agg(kCount, o[0])}), "");
    for (int op : {kSum, kMin, kMax})
      Expect(o[0], SaidPlain({Agg(op, o[0])}), NotSup(std::string(AggOpName(op)) + " on column " + typed + sum_tail));
    Expect(o[0], SaidPlain({Agg(kSumProduct, "i8", o[0])}), NotSup("SUM_PRODUCT on column " + typed + factor_tail));
    Expect(o[0], SaidGroup({"i8"}, {Expr({Constant(2), Factor(o[0])})}), NotSup("SUM_EXPR on column " + typed + factor_tail));
  }
  // integer and floating-point factors do not mix
  Expect("families", SaidPlain({Agg(kSumProduct, "i32", "dec18"), Agg(kSumProduct, "f32", "ree_f64")}), "");
  Expect("families", SaidPlain({Agg(kSumProduct, "i32", "f64")}),
         NotSup("SUM_PRODUCT of 'i32' (INTEGER) and 'f64' (DOUBLE): both factors must be integer-like or both floating point"));
  Expect("families", SaidPlain({Agg(kSumProduct, "f32", "u8")}),
         NotSup("SUM_PRODUCT of 'f32' (FLOAT) and 'u8' (UTINYINT): both factors must be integer-like or both floating point"));
  Expect("families", SaidGroup({"s"}, {Expr({Factor("date32"), Constant(3), Factor("u64")}), Expr({Factor("f64"), Factor("f32")})}), "");
  Expect("families", SaidGroup({"s"}, {Expr({Factor("date32"), Constant(3), Factor("ree_f64")})}),
         NotSup("SUM_EXPR of 'date32' (DATE) and 'ree_f64' (DOUBLE): both factors must be integer-like or both floating point"));
}

void CheckShapeRefusals() {
  const char* apis[3] = {"mi_scan_aggregate", "mi_scan_group_aggregate", "mi_scan_hash_aggregate"};
  auto said = [&](int call, const std::vector<AggSpec>& specs) {
    return call == 0 ? SaidPlain(specs) : call == 1 ? SaidGroup({"i16"}, specs) : SaidHash("i16", specs);
  };
  for (int call = 0; call < 3; call++) {
    const std::string api = apis[call];
    // 1 .. 8 aggregates
    Expect("8 aggregates", said(call, std::vector<AggSpec>(8, Agg(kCountStar))), "");
    Expect("1 aggregate", said(call, {Agg(kCountStar)}), "");
    Expect("0 aggregates", said(call, {}), Invalid(api + " takes 1 to 8 aggregates, not 0"));
    Expect("9 aggregates", said(call, std::vector<AggSpec>(9, Agg(kCountStar))), Invalid(api + " takes 1 to 8 aggregates, not 9"));
    // the operations are 1 .. 7
    Expect("operation 0", said(call, {Agg(0, "i64")}), Invalid(api + ": unknown operation 0"));
    Expect("operation 8", said(call, {Agg(8, "i64")}), Invalid(api + ": unknown operation 8"));
    Expect("operation -1", said(call, {Agg(-1, "i64")}), Invalid(api + ": unknown operation -1"));
    // 1 .. 4 factors, one of them a column
    Expect("4 factors", said(call, {Expr({Factor("i64"), Constant(1), Constant(2), Factor("i8")})}), "");
    Expect("0 factors", said(call, {Expr({})}), Invalid(api + ": SUM_EXPR takes 1 to 4 factors, not 0"));
    Expect("5 factors", said(call, {Expr(std::vector<AggFactorSpec>(5, Factor("i64")))}), Invalid(api + ": SUM_EXPR takes 1 to 4 factors, not 5"));
    Expect("constants alone", said(call, {Expr({Constant(1), Constant(2)})}), Invalid(api + ": SUM_EXPR needs at least one factor with a column"));
  }
  // constants: int64 on an integer expression; on a floating-point one doubles, or integers a double holds exactly
  Expect("int constants", SaidPlain({Expr({Factor("i64", -3, 1ll << 62)})}), "");
  Expect("double constants", SaidPlain({Expr({DoubleFactor("f64", 0.5, -1.25), DoubleFactor("f32", 1.0, 0.0)})}), "");
  Expect("double constants on integers", SaidPlain({Expr({DoubleFactor("i64", 0.5, 0.0)})}),
         NotSup("SUM_EXPR on column 'i64': double constants on an expression over integer-like columns are not computed in the scan (give int64 constants)"));
  AggFactorSpec constant_double = Constant(0);
  constant_double.constants = MI_AGG_CONST_DOUBLE;
  Expect("double constant factor on integers", SaidPlain({Expr({Factor("i64"), constant_double})}),
         NotSup("SUM_EXPR constant factor: double constants on an expression over integer-like columns are not computed in the scan (give int64 constants)"));
  Expect("double constant factor on doubles", SaidPlain({Expr({Factor("f64"), constant_double})}), "");
  AggFactorSpec odd = Factor("i64");
  odd.constants = 7;
  Expect("constants 7", SaidPlain({Expr({odd})}), Invalid("SUM_EXPR on column 'i64': constants must be MI_AGG_CONST_INT or MI_AGG_CONST_DOUBLE, not 7"));
  Expect("2^53", SaidPlain({Expr({Factor("f64", 9007199254740992ll, -9007199254740992ll)})}), "");
  Expect("2^53 + 1", SaidPlain({Expr({Factor("f64", 9007199254740993ll, 0)})}),
         Invalid("SUM_EXPR on column 'f64': the integer constant 9007199254740993 is not exactly representable in a double"));
  Expect("-(2^53 + 1) added", SaidPlain({Expr({Factor("f32", 1, -9007199254740993ll)})}),
         Invalid("SUM_EXPR on column 'f32': the integer constant -9007199254740993 is not exactly representable in a double"));
  Expect("INT64_MAX", SaidPlain({Expr({Factor("f64"), Constant(INT64_MAX)})}),
         Invalid("SUM_EXPR constant factor: the integer constant 9223372036854775807 is not exactly representable in a double"));
  Expect("INT64_MIN", SaidPlain({Expr({Factor("f64"), Constant(INT64_MIN)})}), "");   // -2^63 is a double
  Expect("INT64_MAX on integers", SaidPlain({Expr({Factor("i64"), Constant(INT64_MAX)})}), "");
}

void CheckKeyRefusals() {
  // 1 .. 4 keys, each named once
  Expect("4 keys", SaidGroup({"i8", "s", "uuid", "flag"}, {Agg(kCountStar)}), "");
  Expect("0 keys", SaidGroup({}, {Agg(kCountStar)}), Invalid("mi_scan_group_aggregate takes 1 to 4 key columns, not 0"));
  Expect("5 keys", SaidGroup({"i8", "s", "uuid", "flag", "i16"}, {Agg(kCountStar)}), Invalid("mi_scan_group_aggregate takes 1 to 4 key columns, not 5"));
  Expect("a key twice", SaidGroup({"i8", "s", "i8"}, {Agg(kCountStar)}), Invalid("GROUP BY: the key column 'i8' is named twice"));
  Expect("a key that is an aggregate's column too", SaidGroup({"i8"}, {Agg(kSum, "i8")}), "");
  const std::string tail = ") stays above the scan: a key is an integer, BOOLEAN, DATE, TIME / TIMESTAMP, DECIMAL, HUGEINT, UUID, VARCHAR or BLOB column";
  const char* no_key[][2] = {{"f32", "FLOAT"}, {"f64", "DOUBLE"}, {"ree_f64", "DOUBLE"}, {"dur", "INTERVAL"}};
  for (auto& k : no_key) {
    const std::string typed = std::string("'") + k[0] + "' (" + k[1];
    Expect(k[0], SaidGroup({"i8", k[0]}, {Agg(kCountStar)}), NotSup("GROUP BY on column " + typed + tail));
    Expect(k[0], SaidHash(k[0], {Agg(kCountStar)}),
           NotSup("hash GROUP BY on column " + typed + ") stays above the scan: the key is one integer, BOOLEAN, DATE, TIME / TIMESTAMP or DECIMAL(<=18) column"));
  }
  // the hash call: one 64-bit word
  const char* wide[][2] = {{"dec19", "DECIMAL(19,2)"}, {"uuid", "UUID"}, {"ree_dec38", "DECIMAL(38,2)"}};
  for (auto& k : wide) {
    Expect(k[0], SaidGroup({k[0]}, {Agg(kCountStar)}), "");
    Expect(k[0], SaidHash(k[0], {Agg(kCountStar)}),
           NotSup(std::string("hash GROUP BY on column '") + k[0] + "' (" + k[1] + "): a 16-byte key is not one 64-bit word -- the key is one integer, BOOLEAN, DATE, TIME / TIMESTAMP or "
                  "DECIMAL(<=18) column; mi_scan_group_aggregate takes a 16-byte key for few groups"));
  }
  const char* strings[][2] = {{"s", "VARCHAR"}, {"blob", "BLOB"}, {"view", "VARCHAR"}, {"fixed", "BLOB"}, {"ree_s", "VARCHAR"}};
  for (auto& k : strings) {
    Expect(k[0], SaidGroup({k[0]}, {Agg(kCountStar)}), "");
    Expect(k[0], SaidHash(k[0], {Agg(kCountStar)}),
           NotSup(std::string("hash GROUP BY on column '") + k[0] + "' (" + k[1] + "): a VARCHAR / BLOB key is not one 64-bit word -- the key is one integer, BOOLEAN, DATE, TIME / TIMESTAMP or "
                  "DECIMAL(<=18) column; mi_scan_group_aggregate takes a VARCHAR / BLOB key for few groups"));
  }
  // the hash call: merges that are exact in any order
  const std::string float_tail = "): the hash GROUP BY adds in arrival order, so a floating-point sum would differ from run to run; mi_scan_group_aggregate keeps it "
                                 "bit-reproducible for few groups";
  Expect("float MIN / MAX / COUNT", SaidHash("i64", {Agg(kMin, "f64"), Agg(kMax, "f32"), Agg(kCount, "f64"), Agg(kSum, "i64")}), "");
  Expect("float SUM", SaidGroup({"i64"}, {Agg(kSum, "f64"), Agg(kSumProduct, "f32", "f64"), Expr({Factor("ree_f64")})}), "");
  Expect("float SUM", SaidHash("i64", {Agg(kSum, "f64")}), NotSup("SUM on column 'f64' (DOUBLE" + float_tail));
  Expect("float SUM_PRODUCT", SaidHash("i64", {Agg(kCountStar), Agg(kSumProduct, "f32", "f64")}), NotSup("SUM_PRODUCT on column 'f32' (FLOAT" + float_tail));
  Expect("float SUM_EXPR", SaidHash("i64", {Expr({Constant(2), Factor("ree_f64")})}), NotSup("SUM_EXPR on column 'ree_f64' (DOUBLE" + float_tail));
  const std::string wide_tail = "): there is no 128-bit atomic, so MIN / MAX of a 16-byte column is not taken by the hash GROUP BY; mi_scan_group_aggregate takes it for few groups";
  Expect("wide MIN", SaidGroup({"i64"}, {Agg(kMin, "dec38"), Agg(kMax, "uuid")}), "");
  Expect("wide COUNT", SaidHash("i64", {Agg(kCount, "dec38")}), "");
  Expect("wide MIN", SaidHash("i64", {Agg(kMin, "dec38")}), NotSup("MIN on column 'dec38' (DECIMAL(38,2)" + wide_tail));
  Expect("wide MAX", SaidHash("i64", {Agg(kMax, "uuid")}), NotSup("MAX on column 'uuid' (UUID" + wide_tail));
  // max_groups: 1 .. 2^24
  Expect("max_groups 1", SaidHash("i64", {Agg(kCountStar)}, 1), "");
  Expect("max_groups 2^24", SaidHash("i64", {Agg(kCountStar)}, 1 << 24), "");
  Expect("max_groups 0", SaidHash("i64", {Agg(kCountStar)}, 0), Invalid("mi_scan_hash_aggregate: max_groups must be 1 to 16777216 (MI_MAX_HASH_GROUPS), not 0"));
  Expect("max_groups 2^24 + 1", SaidHash("i64", {Agg(kCountStar)}, (1 << 24) + 1),
         Invalid("mi_scan_hash_aggregate: max_groups must be 1 to 16777216 (MI_MAX_HASH_GROUPS), not 16777217"));
  Expect("max_groups -1", Said([] { CheckHashMaxGroups("mi_hash_aggregate_vectors", -1); }),
         Invalid("mi_hash_aggregate_vectors: max_groups must be 1 to 16777216 (MI_MAX_HASH_GROUPS), not -1"));
  BoundAggregates plan = BindHashAggregates(kCols, "u16", {Agg(kCountStar)}, 12345);
  CHECK(plan.mode == AggMode::kHash && plan.max_groups == 12345 && plan.keys.size() == 1, "the hash plan");
  CHECK(BindGroupAggregates(kCols, {"u16"}, {Agg(kCountStar)}).mode == AggMode::kGrouped && BindAggregates(kCols, {Agg(kCountStar)}).mode == AggMode::kPlain, "the modes");
}

// ------------------------------------------------------------------------------------------------ bind: the valid plans
void CheckClasses() {
  struct Row {
    const char* column;
    int agg_cls, key_cls;   // agg_cls kAny: COUNT alone; key_cls 0: no key
  };
  const Row rows[] = {{"i8", kSigned, kKeySigned},      {"u8", kUnsigned, kKeyUnsigned},   {"i16", kSigned, kKeySigned},    {"u16", kUnsigned, kKeyUnsigned},
                      {"i32", kSigned, kKeySigned},     {"u32", kUnsigned, kKeyUnsigned},  {"i64", kSigned, kKeySigned},    {"u64", kUnsigned, kKeyUnsigned},
                      {"date32", kSigned, kKeySigned},  {"date64", kSigned, kKeySigned},   {"time_s", kSigned, kKeySigned}, {"time_ns", kSigned, kKeySigned},
                      {"ts", kSigned, kKeySigned},      {"tstz", kSigned, kKeySigned},     {"dec4", kSigned, kKeySigned},   {"dec9", kSigned, kKeySigned},
                      {"dec18", kSigned, kKeySigned},   {"dec19", kWide, kKeyWide},        {"dec38", kWide, kKeyWide},      {"uuid", kWide, kKeyWide},
                      {"f32", kFloat, 0},               {"f64", kFloat, 0},                {"flag", kAny, kKeyUnsigned},    {"flag8", kAny, kKeyUnsigned},
                      {"s", kAny, kKeyString},          {"blob", kAny, kKeyString},        {"view", kAny, kKeyString},      {"fixed", kAny, kKeyString},
                      {"ree_u16", kUnsigned, kKeyUnsigned}, {"ree_f64", kFloat, 0},        {"ree_dec38", kWide, kKeyWide},  {"ree_s", kAny, kKeyString}};
  for (const Row& r : rows) {
    if (r.agg_cls != kAny) {
      const BoundAggregates p = BindAggregates(kCols, {Agg(kMin, r.column), Agg(kCount, r.column)});
      CHECK(p.aggs.size() == 2 && p.aggs[0].cls == r.agg_cls && p.aggs[0].op == kMin && p.aggs[0].col_a == 0 && p.aggs[0].col_b == -1, "MIN(%s) has class %d", r.column,
            p.aggs[0].cls);
      CHECK(p.aggs[1].cls == kAny && p.aggs[1].op == kCount && p.aggs[1].col_a == 0, "COUNT(%s) has class %d", r.column, p.aggs[1].cls);
      CHECK(p.projection == std::vector<std::string>{r.column} && p.keys.empty(), "MIN(%s) projects %zu columns", r.column, p.projection.size());
      if (r.agg_cls != kWide) {
        const BoundAggregates q = BindAggregates(kCols, {Agg(kSum, r.column), Expr({Factor(r.column, 2, 3)})});
        CHECK(q.aggs[0].cls == r.agg_cls && q.aggs[1].cls == r.agg_cls && q.aggs[1].factors.size() == 1 && q.aggs[1].factors[0].cls == r.agg_cls, "SUM(%s)", r.column);
      }
    }
    if (r.key_cls != 0) {
      const BoundAggregates p = BindGroupAggregates(kCols, {r.column}, {Agg(kCountStar)});
      CHECK(p.keys.size() == 1 && p.keys[0].cls == r.key_cls && p.keys[0].col == 0 && p.projection == std::vector<std::string>{r.column}, "key %s has class %d", r.column,
            p.keys.empty() ? -1 : p.keys[0].cls);
      if (r.key_cls == kKeySigned || r.key_cls == kKeyUnsigned) {
        const BoundAggregates h = BindHashAggregates(kCols, r.column, {Agg(kCountStar)}, 10);
        CHECK(h.keys.size() == 1 && h.keys[0].cls == r.key_cls && h.keys[0].col == 0, "hash key %s has class %d", r.column, h.keys[0].cls);
      }
    }
  }
  const char* names[] = {"?", "COUNT(*)", "COUNT", "SUM", "SUM_PRODUCT", "MIN", "MAX", "SUM_EXPR", "?"};
  for (int op = 0; op <= 8; op++) CHECK(std::string(AggOpName(op)) == names[op], "operation %d is %s", op, AggOpName(op));
}

void CheckProjection() {
  // the first use of a column fixes its slot; keys come before aggregates
  const std::vector<AggSpec> specs = {Agg(kSum, "i32"),     Agg(kSumProduct, "i64", "i32"), Agg(kCountStar), Agg(kCount, "s"),
                                      Expr({Factor("u8", 3, -1), Constant(7), Factor("i64")}), Agg(kMax, "u8"), Agg(kSumProduct, "f32", "f64")};
  const BoundAggregates p = BindAggregates(kCols, specs);
  CHECK(p.projection == (std::vector<std::string>{"i32", "i64", "s", "u8", "f32", "f64"}), "the projection has %zu columns", p.projection.size());
  const int want[7][5] = {// op, cls, col_a, col_b, cls_b
                          {kSum, kSigned, 0, -1, 0}, {kSumProduct, kSigned, 1, 0, kSigned}, {kCountStar, 0, -1, -1, 0}, {kCount, 0, 2, -1, 0},
                          {kSumExpr, kUnsigned, 3, -1, 0}, {kMax, kUnsigned, 3, -1, 0}, {kSumProduct, kFloat, 4, 5, kFloat}};
  CHECK(p.aggs.size() == 7, "%zu aggregates", p.aggs.size());
  for (size_t a = 0; a < 7 && a < p.aggs.size(); a++) {
    const BoundAgg& b = p.aggs[a];
    CHECK(b.op == want[a][0] && b.cls == want[a][1] && b.col_a == want[a][2] && b.col_b == want[a][3] && b.cls_b == want[a][4], "aggregate %zu is {%d, %d, %d, %d, %d}", a, b.op,
          b.cls, b.col_a, b.col_b, b.cls_b);
    CHECK(b.factors.size() == (a == 4 ? 3u : 0u), "aggregate %zu has %zu factors", a, b.factors.size());
  }
  const BoundAgg& e = p.aggs[4];   // (3 u8 - 1) * 7 * i64: the class of the first column is the expression's
  CHECK(e.factors[0].col == 3 && e.factors[0].cls == kUnsigned && e.factors[0].mul == 3 && e.factors[0].add == ~0ull, "factor 0");
  CHECK(e.factors[1].col == -1 && e.factors[1].cls == kAny && e.factors[1].mul == 1 && e.factors[1].add == 7, "factor 1");
  CHECK(e.factors[2].col == 1 && e.factors[2].cls == kSigned && e.factors[2].mul == 1 && e.factors[2].add == 0, "factor 2");
  // double constants travel as bits, integer ones on a floating-point expression as the double they are
  const BoundAggregates d = BindAggregates(kCols, {Expr({DoubleFactor("f64", 0.5, -2.0), Factor("f32", -3, 1ll << 53)})});
  CHECK(d.aggs[0].cls == kFloat && d.aggs[0].factors[0].mul == 0x3FE0000000000000ull && d.aggs[0].factors[0].add == 0xC000000000000000ull, "0.5 and -2.0");
  CHECK(d.aggs[0].factors[1].mul == 0xC008000000000000ull && d.aggs[0].factors[1].add == 0x4340000000000000ull, "-3 and 2^53 as doubles");

  const BoundAggregates g = BindGroupAggregates(kCols, {"s", "i64", "flag"}, {Agg(kSum, "i32"), Agg(kMin, "i64"), Agg(kCount, "s"), Agg(kMax, "dec38")});
  CHECK(g.projection == (std::vector<std::string>{"s", "i64", "flag", "i32", "dec38"}), "the grouped projection has %zu columns", g.projection.size());
  CHECK(g.keys.size() == 3 && g.keys[0].col == 0 && g.keys[1].col == 1 && g.keys[2].col == 2, "the keys' slots");
  CHECK(g.keys[0].cls == kKeyString && g.keys[1].cls == kKeySigned && g.keys[2].cls == kKeyUnsigned, "the keys' classes");
  CHECK(g.aggs[0].col_a == 3 && g.aggs[1].col_a == 1 && g.aggs[2].col_a == 0 && g.aggs[3].col_a == 4 && g.aggs[3].cls == kWide, "the aggregates' slots");
  const BoundAggregates h = BindHashAggregates(kCols, "date32", {Agg(kSum, "i32"), Agg(kMin, "date32"), Agg(kCountStar)}, 5);
  CHECK(h.projection == (std::vector<std::string>{"date32", "i32"}) && h.keys[0].col == 0 && h.aggs[0].col_a == 1 && h.aggs[1].col_a == 0 && h.aggs[2].col_a == -1,
        "the hash projection has %zu columns", h.projection.size());
}

void CheckCountStar() {
  auto picked = [](const std::vector<const char*>& names) {
    std::vector<ScanColumn> cols;
    for (const char* n : names)
      for (const ScanColumn& c : kCols)
        if (c.name == n) cols.push_back(c);
    std::string out;
    const std::string said = Said([&] {
      const BoundAggregates p = BindAggregates(cols, {Agg(kCountStar), Agg(kCountStar)});
      out = p.projection.size() == 1 ? p.projection[0] : "?";
    });
    return said.empty() ? out : said;
  };
  // the narrowest fixed-width column the aggregates could read, the first of them among equals
  Expect("narrowest", picked({"s", "i64", "u16", "i32", "i16", "dec38"}), "u16");
  Expect("narrowest", picked({"f64", "dec38", "f32", "date32"}), "f32");
  Expect("narrowest", picked({"filename", "dict", "dict_i64", "day_time", "ree_dict", "uuid", "s"}), "uuid");
  Expect("narrowest", picked({"i64", "ree_u16", "i8"}), "i8");
  // else the first column the scan decodes without a dictionary
  Expect("first decodable", picked({"filename", "dict", "s", "blob", "flag"}), "s");
  Expect("first decodable", picked({"dict_i64", "flag", "s"}), "flag");
  Expect("nothing to decode", picked({"filename", "dict", "day_time", "year"}), NotSup("COUNT(*): the scan has no column it decodes without a dictionary"));
  // with another aggregate, or a key, nothing is added
  CHECK(BindAggregates(kCols, {Agg(kCountStar), Agg(kCount, "s")}).projection == std::vector<std::string>{"s"}, "COUNT(*) beside COUNT(s)");
  CHECK(BindGroupAggregates(kCols, {"s"}, {Agg(kCountStar)}).projection == std::vector<std::string>{"s"}, "COUNT(*) per s");
  CHECK(BindAggregates(kCols, {Agg(kCountStar)}).projection == std::vector<std::string>{"i8"}, "COUNT(*) over every column");
}

// ------------------------------------------------------------------------------------------------ results
Partial P(uint64_t lo, uint64_t hi, uint64_t count, uint64_t flags = 0) { return Partial{lo, hi, count, flags}; }
bool Same(const Partial& a, const Partial& b) { return a.lo == b.lo && a.hi == b.hi && a.count == b.count && a.flags == b.flags; }
groupkey::Key Key1(uint64_t lo, uint64_t hi, bool null = false) {
  groupkey::Key k;
  std::memset(&k, 0, sizeof(k));
  k.lo[0] = null ? 0 : lo;
  k.hi[0] = null ? 0 : hi;
  k.nulls = null ? 1u : 0u;
  return k;
}
// the inline string_t image of a string of at most 12 bytes
groupkey::Key StringKey(const char* s) {
  uint8_t image[16] = {0};
  const uint32_t len = static_cast<uint32_t>(std::strlen(s));
  std::memcpy(image, &len, 4);
  std::memcpy(image + 4, s, len);
  groupkey::Key k;
  std::memset(&k, 0, sizeof(k));
  std::memcpy(&k.lo[0], image, 8);
  std::memcpy(&k.hi[0], image + 8, 8);
  return k;
}

void CheckSortGroups() {
  {  // 128-bit integers by value, NULLS LAST; the aggregates of a group travel with its key
    GroupResult r;
    r.kinds = {groupkey::kKindInt128};
    r.classes = {kSigned, kSigned};
    const int64_t keys[] = {5, -1, 0, INT64_MIN, INT64_MAX};
    for (int64_t k : keys) r.keys.push_back(Key1(static_cast<uint64_t>(k), k < 0 ? ~0ull : 0ull));
    r.keys.insert(r.keys.begin() + 2, Key1(0, 0, true));
    r.keys.push_back(Key1(1, 1));           // 2^64 + 1
    r.keys.push_back(Key1(~0ull, 0));       // 2^64 - 1: not -1
    for (uint64_t g = 0; g < 8; g++) {
      r.values.push_back(P(100 + g, 0, 1));
      r.values.push_back(P(200 + g, 0, 2));
    }
    SortGroups(&r);
    const uint64_t order[8] = {4, 1, 3, 0, 5, 7, 6, 2};   // INT64_MIN, -1, 0, 5, INT64_MAX, 2^64 - 1, 2^64 + 1, NULL
    CHECK(r.keys.size() == 8 && r.values.size() == 16, "sizes after the sort");
    for (size_t g = 0; g < 8 && r.values.size() == 16; g++)
      CHECK(r.values[2 * g].lo == 100 + order[g] && r.values[2 * g + 1].lo == 200 + order[g], "integer group %zu is the one that came as %llu", g,
            (unsigned long long)(r.values[2 * g].lo - 100));
    CHECK(r.keys[7].nulls == 1 && r.keys[0].lo[0] == 0x8000000000000000ull && r.keys[5].lo[0] == ~0ull && r.keys[5].hi[0] == 0, "the keys moved with them");
  }
  {  // strings bytewise and then shorter first; two parts: the first decides, then the second, NULLS LAST in each
    GroupResult r;
    r.kinds = {groupkey::kKindString, groupkey::kKindInt128};
    r.classes = {kSigned};
    struct Row {
      const char* s;   // NULL: a NULL part
      int64_t i;
      bool i_null;
    };
    const Row rows[] = {{"b", 1, false}, {"ab", 2, false}, {"a", 3, false}, {nullptr, 0, false}, {"", 9, false}, {"a", 0, true}, {"a", -3, false},
                        {"abcdefghijkl", 0, false}, {"\xff", 0, false}, {nullptr, 0, true}, {"B", 0, false}};
    for (size_t g = 0; g < sizeof(rows) / sizeof(rows[0]); g++) {
      groupkey::Key k = rows[g].s ? StringKey(rows[g].s) : Key1(0, 0);
      if (!rows[g].s) k.nulls |= 1u;
      if (rows[g].i_null) k.nulls |= 2u;
      else {
        k.lo[1] = static_cast<uint64_t>(rows[g].i);
        k.hi[1] = rows[g].i < 0 ? ~0ull : 0ull;
      }
      r.keys.push_back(k);
      r.values.push_back(P(g, 0, 1));
    }
    SortGroups(&r);
    const uint64_t order[11] = {4, 10, 6, 2, 5, 1, 7, 0, 8, 3, 9};   // "", "B", ("a", -3), ("a", 3), ("a", NULL), "ab", "abcdefghijkl", "b", "\xff", (NULL, 0), (NULL, NULL)
    for (size_t g = 0; g < 11 && r.values.size() == 11; g++) CHECK(r.values[g].lo == order[g], "string group %zu is the one that came as %llu", g, (unsigned long long)r.values[g].lo);
  }
  GroupResult none;
  none.kinds = {groupkey::kKindInt128};
  none.classes = {kSigned};
  SortGroups(&none);
  CHECK(none.keys.empty() && none.values.empty(), "no group");
}

void CheckFill() {
  // every operation x class: COUNTs are their count, the others {lo, hi} of the class's kind, NULL without a contributor
  for (int op = kCountStar; op <= kSumExpr; op++)
    for (int cls = kAny; cls <= kWide; cls++) {
      mi_agg_value v;
      std::memset(&v, 0xAB, sizeof(v));
      FillAggValue(op, cls, P(0x1111, 0xFFFFFFFFFFFFFFFFull, 7, 0), &v);
      const bool count = op == kCountStar || op == kCount;
      CHECK(v.count == 7 && v.is_null == 0 && v.reserved[0] == 0 && v.reserved[1] == 0, "op %d class %d: count %lld, is_null %d", op, cls, (long long)v.count, v.is_null);
      CHECK(v.kind == (!count && cls == kFloat ? MI_AGG_VALUE_DOUBLE : MI_AGG_VALUE_INT128), "op %d class %d: kind %d", op, cls, v.kind);
      CHECK(count ? (v.lo == 7 && v.hi == 0) : (v.lo == 0x1111 && v.hi == -1), "op %d class %d: {%llu, %lld}", op, cls, (unsigned long long)v.lo, (long long)v.hi);
      std::memset(&v, 0xAB, sizeof(v));
      FillAggValue(op, cls, P(0x1111, 5, 0, 0), &v);   // no contributor: what lo / hi hold is not looked at
      CHECK(v.count == 0 && v.lo == 0 && v.hi == 0 && v.is_null == (count ? 0 : 1), "op %d class %d without a row: is_null %d, {%llu, %lld}", op, cls, v.is_null,
            (unsigned long long)v.lo, (long long)v.hi);
    }
  // a sorted result into the caller's arrays
  GroupResult r;
  r.kinds = {groupkey::kKindInt128, groupkey::kKindString};
  r.classes = {kSigned, kFloat};
  const std::vector<int32_t> ops = {kSum, kMax};
  for (int g = 0; g < 3; g++) {
    groupkey::Key k = Key1(static_cast<uint64_t>(-g), g ? ~0ull : 0ull);
    const groupkey::Key s = StringKey(g == 0 ? "x" : "yz");
    k.lo[1] = s.lo[0];
    k.hi[1] = s.hi[0];
    if (g == 2) {
      k.nulls = 2u;
      k.lo[1] = k.hi[1] = 0;
    }
    r.keys.push_back(k);
    r.values.push_back(P(10 + g, 0, 1));
    r.values.push_back(P(0x4000000000000000ull + g, 0, g));   // g == 0: NULL
  }
  mi_group_key_value keys[6];
  mi_agg_value values[6];
  int32_t n = -1;
  std::memset(keys, 0xCD, sizeof(keys));
  Expect("capacity n - 1", Said([&] { FillGroupOutputs(r, ops, keys, values, 2, &n); }), Invalid("GROUP BY found 3 groups, the caller's arrays hold 2"));
  CHECK(n == 3 && keys[0].kind == static_cast<int32_t>(0xCDCDCDCD), "n_groups is set before the throw (%d) and nothing is written", n);
  n = -1;
  Expect("capacity -1", Said([&] { FillGroupOutputs(r, ops, keys, values, -1, &n); }), Invalid("GROUP BY found 3 groups, the caller's arrays hold -1"));
  n = -1;
  Expect("capacity n", Said([&] { FillGroupOutputs(r, ops, keys, values, 3, &n); }), "");
  CHECK(n == 3, "%d groups", n);
  const uint8_t minus_one[16] = {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255};
  const uint8_t yz[16] = {2, 0, 0, 0, 'y', 'z', 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, zero[16] = {0};
  CHECK(keys[2].kind == MI_GROUP_KEY_INT128 && keys[2].is_null == 0 && std::memcmp(keys[2].bytes, minus_one, 16) == 0, "group 1, part 0 is -1");
  CHECK(keys[3].kind == MI_GROUP_KEY_STRING && keys[3].is_null == 0 && std::memcmp(keys[3].bytes, yz, 16) == 0, "group 1, part 1 is 'yz'");
  CHECK(keys[5].kind == MI_GROUP_KEY_STRING && keys[5].is_null == 1 && std::memcmp(keys[5].bytes, zero, 16) == 0, "group 2, part 1 is NULL");
  CHECK(keys[0].is_null == 0 && std::memcmp(keys[0].bytes, zero, 16) == 0 && keys[4].bytes[0] == 254 && keys[4].bytes[15] == 255, "groups 0 and 2, part 0");
  CHECK(values[0].lo == 10 && values[0].kind == MI_AGG_VALUE_INT128 && values[1].is_null == 1 && values[1].kind == MI_AGG_VALUE_DOUBLE && values[1].lo == 0, "group 0's values");
  CHECK(values[4].lo == 12 && values[5].lo == 0x4000000000000002ull && values[5].is_null == 0 && values[5].count == 2, "group 2's values");
  Expect("no n_groups", Said([&] { FillGroupOutputs(r, ops, keys, values, 3, nullptr); }), "");
}

void CheckHashGroupKey() {
  const groupkey::Key neg = HashGroupKey(0xFFFFFFFFFFFFFFFEull, false, kKeySigned);     // -2
  CHECK(neg.lo[0] == 0xFFFFFFFFFFFFFFFEull && neg.hi[0] == ~0ull && neg.nulls == 0, "a negative signed key is sign-extended");
  const groupkey::Key pos = HashGroupKey(0x7FFFFFFFFFFFFFFFull, false, kKeySigned);
  CHECK(pos.lo[0] == 0x7FFFFFFFFFFFFFFFull && pos.hi[0] == 0, "INT64_MAX");
  const groupkey::Key big = HashGroupKey(0x8000000000000000ull, false, kKeyUnsigned);   // 2^63
  CHECK(big.lo[0] == 0x8000000000000000ull && big.hi[0] == 0 && big.nulls == 0, "an unsigned key of 2^63 is zero-extended");
  const groupkey::Key top = HashGroupKey(~0ull, false, kKeyUnsigned);
  CHECK(top.lo[0] == ~0ull && top.hi[0] == 0, "UINT64_MAX");
  for (int cls : {kKeySigned, kKeyUnsigned}) {
    const groupkey::Key null = HashGroupKey(0xDEADBEEFull, true, cls);   // the word under a NULL is not looked at
    CHECK(null.nulls == 1 && null.lo[0] == 0 && null.hi[0] == 0, "NULL");
    for (int k = 1; k < groupkey::kMaxKeys; k++) CHECK(null.lo[k] == 0 && null.hi[k] == 0 && neg.lo[k] == 0 && neg.hi[k] == 0, "part %d is zero", k);
  }
}

// ------------------------------------------------------------------------------------------------ merges
const uint64_t kOne = 0x3FF0000000000000ull, kTwo = 0x4000000000000000ull, kThree = 0x4008000000000000ull, kSix = 0x4018000000000000ull;   // doubles

void CheckMergeAgg() {
  const std::vector<int32_t> ops = {kCountStar, kSum, kMin, kMax, kSum, kMin};
  const std::vector<int32_t> classes = {kAny, kSigned, kSigned, kUnsigned, kFloat, kFloat};
  auto part = [&](std::vector<Partial> values, int64_t scanned, int64_t selected) {
    AggResult r;
    r.values = std::move(values);
    r.classes = classes;
    r.rows_scanned = scanned;
    r.rows_selected = selected;
    return r;
  };
  const AggResult a = part({P(0, 0, 4), P(~0ull, ~0ull, 4), P(5, 0, 4), P(5, 0, 4), P(kOne, 0, 4), P(kTwo, 0, 4)}, 10, 4);             // SUM -1
  const AggResult none = part(std::vector<Partial>(6, P(0, 0, 0)), 7, 0);                                                               // no row selected
  const AggResult b = part({P(0, 0, 2), P(~0ull, 0, 2, 1024), P(~2ull, ~0ull, 2), P(~0ull, 0, 2), P(kTwo, 0, 2), P(kOne, 0, 2)}, 5, 2);   // SUM 2^64 - 1, MIN -3
  AggResult out;
  MergeAggResults({a}, ops, &out);
  CHECK(out.values.size() == 6 && out.classes == classes && out.rows_scanned == 10 && out.rows_selected == 4, "one part: rows %lld / %lld", (long long)out.rows_scanned,
        (long long)out.rows_selected);
  for (size_t i = 0; i < 6 && out.values.size() == 6; i++) CHECK(Same(out.values[i], a.values[i]), "one part: aggregate %zu", i);
  MergeAggResults({none}, ops, &out);
  for (size_t i = 0; i < 6 && out.values.size() == 6; i++) CHECK(Same(out.values[i], P(0, 0, 0)), "an empty part alone: aggregate %zu", i);
  for (const std::vector<AggResult>& parts : {std::vector<AggResult>{a, b}, std::vector<AggResult>{a, none, b}, std::vector<AggResult>{none, a, b}}) {
    MergeAggResults(parts, ops, &out);
    const Partial want[6] = {P(0, 0, 6), P(~1ull, 0, 6, 1024), P(~2ull, ~0ull, 6), P(~0ull, 0, 6), P(kThree, 0, 6), P(kOne, 0, 6)};   // -1 + 2^64 - 1 = 2^64 - 2
    CHECK(out.rows_scanned == (parts.size() == 3 ? 22 : 15) && out.rows_selected == 6 && out.values.size() == 6, "%zu parts: rows", parts.size());
    for (size_t i = 0; i < 6 && out.values.size() == 6; i++)
      CHECK(Same(out.values[i], want[i]), "%zu parts: aggregate %zu is {%llx, %llx, %llu, %llu}", parts.size(), i, (unsigned long long)out.values[i].lo,
            (unsigned long long)out.values[i].hi, (unsigned long long)out.values[i].count, (unsigned long long)out.values[i].flags);
  }
  // the double sum is folded in part order: (1e16 + 1) + 1 is not 1e16 + (1 + 1)
  const std::vector<int32_t> sum = {kSum};
  auto one = [&](uint64_t bits) {
    AggResult r;
    r.values = {P(bits, 0, 1)};
    r.classes = {kFloat};
    return r;
  };
  const uint64_t e16 = 0x4341C37937E08000ull;   // 1e16: the doubles around it are 2 apart
  MergeAggResults({one(e16), one(kOne), one(kOne)}, sum, &out);
  CHECK(out.values[0].lo == e16 && out.values[0].count == 3, "1e16 + 1 + 1 in part order is %llx", (unsigned long long)out.values[0].lo);
  MergeAggResults({one(kOne), one(kOne), one(e16)}, sum, &out);
  CHECK(out.values[0].lo == e16 + 1, "1 + 1 + 1e16 in part order is %llx", (unsigned long long)out.values[0].lo);
}

GroupResult GroupPart(const std::vector<int32_t>& kinds, const std::vector<int32_t>& classes, int32_t key_cls, int64_t scanned, int64_t selected) {
  GroupResult r;
  r.kinds = kinds;
  r.classes = classes;
  r.key_cls = key_cls;
  r.rows_scanned = scanned;
  r.rows_selected = selected;
  return r;
}
void AddGroup(GroupResult* r, const groupkey::Key& k, std::vector<Partial> values) {
  r->keys.push_back(k);
  r->values.insert(r->values.end(), values.begin(), values.end());
}

// K10 (`hash` false) and K11 over the same parts: one signed key; SUM, MIN, MAX(double) per group
void CheckMergeGroups(bool hash) {
  const char* what = hash ? "hash merge" : "group merge";
  const std::vector<int32_t> ops = {kSum, kMin, kMax}, classes = {kSigned, kSigned, kFloat}, kinds = {groupkey::kKindInt128};
  auto merge = [&](const std::vector<GroupResult>& parts, uint32_t max_groups, GroupResult* out) {
    return hash ? MergeHashResults(parts, ops, max_groups, out) : MergeGroupResults(parts, ops, out);
  };
  const groupkey::Key k7 = Key1(7, 0), kneg = Key1(~4ull, ~0ull), knull = Key1(0, 0, true);   // 7, -5, NULL
  GroupResult a = GroupPart(kinds, classes, kKeySigned, 100, 10), b = GroupPart(kinds, classes, kKeySigned, 50, 5), empty = GroupPart(kinds, classes, kKeySigned, 30, 0);
  AddGroup(&a, k7, {P(10, 0, 2), P(4, 0, 2), P(kTwo, 0, 2)});
  AddGroup(&a, knull, {P(1, 0, 1), P(1, 0, 1), P(kOne, 0, 1)});
  AddGroup(&a, kneg, {P(0, 0, 0), P(0, 0, 0), P(0, 0, 0, 1024)});              // every row of the group NULL in this part; a flag
  AddGroup(&b, kneg, {P(~0ull, ~0ull, 3), P(~8ull, ~0ull, 3), P(kSix, 0, 3)});   // SUM -1, MIN -9
  AddGroup(&b, k7, {P(~10ull, ~0ull, 1), P(9, 0, 1), P(kOne, 0, 1)});          // SUM -11
  AddGroup(&b, knull, {P(5, 0, 2), P(0, 0, 2), P(kThree, 0, 2)});
  GroupResult out;
  CHECK(merge({a}, 3, &out), "%s: one part", what);
  CHECK(out.keys.size() == 3 && out.values.size() == 9 && out.rows_scanned == 100 && out.rows_selected == 10 && out.kinds == kinds && out.classes == classes && out.key_cls == kKeySigned,
        "%s: one part: %zu groups", what, out.keys.size());
  if (out.keys.size() == 3)   // sorted: -5, 7, NULL
    CHECK(groupkey::Equal(out.keys[0], kneg, 1) && groupkey::Equal(out.keys[1], k7, 1) && groupkey::Equal(out.keys[2], knull, 1) && Same(out.values[3], P(10, 0, 2)) &&
              Same(out.values[2], P(0, 0, 0, 1024)),
          "%s: one part comes out sorted", what);
  CHECK(merge({empty}, 3, &out) && out.keys.empty() && out.values.empty() && out.rows_scanned == 30, "%s: an empty part alone", what);
  for (const std::vector<GroupResult>& parts : {std::vector<GroupResult>{a, b}, std::vector<GroupResult>{empty, a, b}, std::vector<GroupResult>{a, empty, b}}) {
    CHECK(merge(parts, 3, &out), "%s: %zu parts", what, parts.size());
    CHECK(out.keys.size() == 3 && out.values.size() == 9 && out.rows_scanned == (parts.size() == 3 ? 180 : 150) && out.rows_selected == 15, "%s: %zu parts: %zu groups", what,
          parts.size(), out.keys.size());
    if (out.keys.size() != 3 || out.values.size() != 9) continue;
    const Partial want[9] = {P(~0ull, ~0ull, 3), P(~8ull, ~0ull, 3), P(kSix, 0, 3, 1024),   // -5: the part without a row changes nothing but the flags
                             P(~0ull, ~0ull, 3), P(4, 0, 3),         P(kTwo, 0, 3),         //  7: 10 - 11, min(4, 9), max(2.0, 1.0)
                             P(6, 0, 3),         P(0, 0, 3),         P(kThree, 0, 3)};      // NULL
    CHECK(groupkey::Equal(out.keys[0], kneg, 1) && groupkey::Equal(out.keys[1], k7, 1) && groupkey::Equal(out.keys[2], knull, 1), "%s: %zu parts: the keys", what, parts.size());
    for (size_t i = 0; i < 9; i++)
      CHECK(Same(out.values[i], want[i]), "%s: %zu parts: value %zu is {%llx, %llx, %llu, %llu}", what, parts.size(), i, (unsigned long long)out.values[i].lo,
            (unsigned long long)out.values[i].hi, (unsigned long long)out.values[i].count, (unsigned long long)out.values[i].flags);
  }
}

void CheckGroupLimits() {
  const std::vector<int32_t> ops = {kCountStar}, classes = {kAny}, kinds = {groupkey::kKindInt128};
  // K11 with max_groups = 2: each part holds two groups, together three
  GroupResult a = GroupPart(kinds, classes, kKeyUnsigned, 0, 0), b = a, c = a;
  AddGroup(&a, Key1(1, 0), {P(0, 0, 1)});
  AddGroup(&a, Key1(~0ull, 0), {P(0, 0, 1)});   // the word of a free slot: an extra record
  AddGroup(&b, Key1(~0ull, 0), {P(0, 0, 1)});
  AddGroup(&b, Key1(0, 0, true), {P(0, 0, 1)});
  AddGroup(&c, Key1(1, 0), {P(0, 0, 5)});
  GroupResult out;
  CHECK(MergeHashResults({a}, ops, 2, &out) && out.keys.size() == 2 && MergeHashResults({b}, ops, 2, &out) && out.keys.size() == 2, "two groups fit max_groups = 2");
  CHECK(MergeHashResults({a, c}, ops, 2, &out) && out.keys.size() == 2 && out.values[0].count == 6 && out.keys[1].lo[0] == ~0ull && out.keys[1].hi[0] == 0, "the same two groups twice");
  CHECK(!MergeHashResults({a, b}, ops, 2, &out), "three groups by two parts together cross max_groups = 2");
  CHECK(!MergeHashResults({c, b, a}, ops, 2, &out) && !MergeHashResults({a, c, b}, ops, 2, &out), "... and by three parts");
  CHECK(MergeHashResults({a, b, c}, ops, 3, &out) && out.keys.size() == 3 && out.keys[2].nulls == 1 && out.values[0].count == 6 && out.values[1].count == 2, "three groups fit max_groups = 3");
  // K10: 4096 groups in a scan; two parts of 2049 distinct keys each cross it together, two that share all but one do not
  GroupResult lo = GroupPart(kinds, classes, 0, 0, 0), hi = lo, same = lo;
  for (uint64_t g = 0; g < 2049; g++) {
    AddGroup(&lo, Key1(g, 0), {P(0, 0, 1)});
    AddGroup(&hi, Key1(5000 + g, 0), {P(0, 0, 1)});
    AddGroup(&same, Key1(g + 1, 0), {P(0, 0, 2)});
  }
  CHECK(MergeGroupResults({lo}, ops, &out) && out.keys.size() == 2049, "2049 groups");
  CHECK(MergeGroupResults({lo, same}, ops, &out) && out.keys.size() == 2050 && out.values[0].count == 1 && out.values[1].count == 3 && out.values[2049].count == 2, "2050 groups by two parts");
  hi.keys.pop_back();
  hi.values.pop_back();
  hi.keys.pop_back();
  hi.values.pop_back();
  CHECK(MergeGroupResults({lo, hi}, ops, &out) && out.keys.size() == 4096 && out.keys[4095].lo[0] == 7046, "4096 groups by two parts");
  CHECK(!MergeGroupResults({lo, hi, same}, ops, &out), "4097 groups by three parts together cross the limit of a scan");
  CHECK(MergeGroupResults({hi, same}, ops, &out) && out.keys.size() == 4096 && out.keys[0].lo[0] == 1, "4096 groups by two other parts");
  AddGroup(&hi, Key1(9999, 0), {P(0, 0, 1)});
  CHECK(!MergeGroupResults({lo, hi}, ops, &out), "4097 groups by two parts together cross the limit of a scan");
}

}  // namespace

int main() {
  CheckColumnRefusals();
  CheckClassRefusals();
  CheckShapeRefusals();
  CheckKeyRefusals();
  CheckClasses();
  CheckProjection();
  CheckCountStar();
  CheckSortGroups();
  CheckFill();
  CheckHashGroupKey();
  CheckMergeAgg();
  CheckMergeGroups(false);
  CheckMergeGroups(true);
  CheckGroupLimits();
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed == 0 ? 0 : 1;
}
