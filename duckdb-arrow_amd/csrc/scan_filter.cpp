// scan_filter.cpp -- the host side of pushed-down predicates: trees -> conjunctive normal form over normalised leaves
// (NormaliseFilter), the leaves bound to the scan's columns and their constants in HBM (BoundFilter::Resolve /
// UploadConstants), the leaves as the kernel takes them for one record batch (BoundFilter::Program).
//
// The reference pushes no filters (filter_pushdown = false, src/scanner/read_arrow.cpp:47-48); what is accepted here is
// what DuckDB's TableFilterSet can hand a scan: constant comparisons, IS [NOT] NULL, IN-lists,
// AND / OR trees.  On integers every comparison is an inclusive range (v < c is [MIN, c-1], v <> c is NOT [c, c]), so
// the kernel knows four leaf forms only and adjacent range conjuncts on one column intersect into one leaf.  FLOAT /
// DOUBLE columns go the same way on the order-preserving keys of filter_key.hpp (DuckDB's total order: NaN = NaN, NaN
// greatest, -0.0 = +0.0; a strict bound is an inclusive one on key +- 1), so everything here works on keys unchanged;
// HUGEINT / DECIMAL(19..38) columns are a leaf form of their own, as strings are, with 128-bit inclusive ranges.
// contains / ends_with / LIKE with `%` (like_match.hpp) fold into the string leaves above where they can -- no `%` is =,
// 'abc%' the prefix range, '%' IS NOT NULL -- and are kLeafStrMatch otherwise, opaque to range merging.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <limits>

#include "extension_format.hpp"
#include "filter_key.hpp"
#include "like_match.hpp"
#include "scan_operator.hpp"

namespace miarrow {

namespace {
using wide_t = __int128;
constexpr wide_t kWideMax = static_cast<wide_t>(~static_cast<unsigned __int128>(0) >> 1), kWideMin = -kWideMax - 1;
wide_t WideOf(int64_t lower, int64_t upper) {
  return static_cast<wide_t>((static_cast<unsigned __int128>(static_cast<uint64_t>(upper)) << 64) | static_cast<uint64_t>(lower));
}
uint64_t LowerOf(wide_t v) { return static_cast<uint64_t>(static_cast<unsigned __int128>(v)); }
int64_t UpperOf(wide_t v) { return static_cast<int64_t>(static_cast<uint64_t>(static_cast<unsigned __int128>(v) >> 64)); }

constexpr int64_t kMin = std::numeric_limits<int64_t>::min(), kMax = std::numeric_limits<int64_t>::max();
constexpr size_t kMaxLeaves = static_cast<size_t>(device::kMaxFilterLeaves);
size_t RoundUp(size_t v, size_t a) { return (v + a - 1) / a * a; }

// 128-bit columns: every comparison is an inclusive range on the stored integer, as on narrow integers
FilterLeaf WideLeafOf(const mi_filter_node& n, FilterLeaf l) {
  const bool is128 = n.value_kind == MI_FV_INT128;
  auto constant = [&](int64_t lower, int64_t upper) { return is128 ? WideOf(lower, upper) : static_cast<wide_t>(lower); };   // an int64 is sign-extended
  const wide_t c = constant(n.value, n.value_hi);
  l.is_wide = true;
  l.op = device::kLeafWideRange;
  l.wide_lo = kWideMin;
  l.wide_hi = kWideMax;
  auto closed = [&](wide_t lo, wide_t hi) { l.wide_lo = lo; l.wide_hi = hi; };
  switch (n.op) {
    case MI_F_EQ: closed(c, c); break;
    case MI_F_NE: closed(c, c); l.negate = true; break;
    case MI_F_LT: if (c == kWideMin) closed(1, 0); else l.wide_hi = c - 1; break;
    case MI_F_LE: l.wide_hi = c; break;
    case MI_F_GT: if (c == kWideMax) closed(1, 0); else l.wide_lo = c + 1; break;
    case MI_F_GE: l.wide_lo = c; break;
    case MI_F_IN:
      if (n.n_values < 0 || (n.n_values > 0 && (!n.values || (is128 && !n.values_hi)))) throw InvalidInputException("IN filter without values");
      if (n.n_values > 256) throw NotImplementedException("IN-list with more than 256 values is not pushed down");
      for (int32_t k = 0; k < n.n_values; k++) l.wide_in.push_back(constant(n.values[k], is128 ? n.values_hi[k] : 0));
      std::sort(l.wide_in.begin(), l.wide_in.end());
      l.wide_in.erase(std::unique(l.wide_in.begin(), l.wide_in.end()), l.wide_in.end());
      if (l.wide_in.empty()) closed(1, 0);
      else if (l.wide_in.size() == 1) { closed(l.wide_in[0], l.wide_in[0]); l.wide_in.clear(); }
      else l.op = device::kLeafWideIn;
      break;
    default: throw InvalidInputException("unknown filter op " + std::to_string(n.op));
  }
  return l;
}

}  // namespace

void CheckPattern(int compiled, int32_t op, const std::string& column) {
  const std::string on = column.empty() ? std::string() : " (column '" + column + "')";
  switch (compiled) {
    case likematch::kCompiled: return;
    case likematch::kHasUnderscore:
      throw NotImplementedException("LIKE pattern with '_'" + on + ": '_' steps over UTF-8 characters, the scan compares bytes; the filter stays above the scan");
    case likematch::kTooManySegments:
      throw NotImplementedException("LIKE pattern with more than " + std::to_string(likematch::kMaxSegments) + " literal segments" + on + " is not pushed into the scan");
    default: throw InvalidInputException("unknown filter op " + std::to_string(op));
  }
}

namespace {
FilterLeaf LeafOf(const mi_filter_node& n, const std::vector<ScanColumn>* columns) {
  if (!n.column || !*n.column) throw InvalidInputException("filter leaf without a column name");
  FilterLeaf l;
  l.column = n.column;
  l.op = device::kLeafRange;
  l.lo = kMin;
  l.hi = kMax;
  // What the constants are compared as: by the column where it is known (an unknown one is refused when the filter is
  // bound), else by their kind
  const bool has_constant = n.op != MI_F_IS_NULL && n.op != MI_F_IS_NOT_NULL && !n.str_value && !n.str_values;
  FilterValueClass cls = FilterValueClass::kOther;
  if (has_constant) {
    if (n.value_kind != MI_FV_INT64 && n.value_kind != MI_FV_DOUBLE && n.value_kind != MI_FV_INT128)
      throw InvalidInputException("filter on column '" + l.column + "': unknown value_kind " + std::to_string(n.value_kind));
    const ScanColumn* sc = nullptr;
    if (columns)
      for (auto& c : *columns)
        if (c.name == l.column) sc = &c;
    if (sc && !sc->is_constant()) {
      cls = FilterClassOf(sc->field);
      const bool is_float = cls == FilterValueClass::kFloat32 || cls == FilterValueClass::kFloat64;
      const std::string what = "filter on column '" + l.column + "' (" + sc->field.DuckType() + "): ";
      if (n.value_kind == MI_FV_DOUBLE && !is_float) throw InvalidInputException(what + "a double constant (MI_FV_DOUBLE) needs a FLOAT / DOUBLE column");
      if (n.value_kind != MI_FV_DOUBLE && is_float) throw InvalidInputException(what + "a FLOAT / DOUBLE column needs double constants (MI_FV_DOUBLE)");
      if (n.value_kind == MI_FV_INT128 && cls != FilterValueClass::kWide)
        throw InvalidInputException(what + "a 128-bit constant (MI_FV_INT128) needs a HUGEINT / DECIMAL(19..38) / UUID column");
      // an int64 is no UUID: sign-extended, as on HUGEINT, it would name a value no text maps to
      if (n.value_kind == MI_FV_INT64 && ValueField(sc->field).extension == extfmt::kUuid)
        throw InvalidInputException(what + "a UUID column needs 128-bit constants (MI_FV_INT128): the hugeint_t image of the UUID");
    } else {
      cls = n.value_kind == MI_FV_DOUBLE ? FilterValueClass::kFloat64 : n.value_kind == MI_FV_INT128 ? FilterValueClass::kWide : FilterValueClass::kOther;
    }
  }
  if (cls == FilterValueClass::kWide) return WideLeafOf(n, l);
  // FLOAT / DOUBLE: the constants become their order-preserving keys, everything below works on keys unchanged
  if (cls != FilterValueClass::kOther) l.float_width = cls == FilterValueClass::kFloat32 ? 4 : 8;
  auto constant = [&](int64_t v) {
    if (!l.float_width) return v;
    double d;
    std::memcpy(&d, &v, 8);
    return filterkey::FloatKeyOfDouble(d, l.float_width);
  };
  const int64_t c = constant(n.value);
  auto closed = [&](int64_t lo, int64_t hi) { l.lo = lo; l.hi = hi; l.lo_open = l.hi_open = false; };
  if (n.str_value || n.str_values) {   // byte-string constants: a VARCHAR / BLOB column
    l.is_string = true;
    l.op = device::kLeafStrIn;
    auto add = [&](const char* p, int32_t len) {
      if (!p || len < 0) throw InvalidInputException("string filter constant without bytes");
      l.str_values.emplace_back(p, static_cast<size_t>(len));
    };
    switch (n.op) {
      case MI_F_EQ: add(n.str_value, n.str_len); break;
      case MI_F_NE: add(n.str_value, n.str_len); l.negate = true; break;
      case MI_F_IN:
        if (n.n_values < 0 || (n.n_values > 0 && (!n.str_values || !n.str_lens))) throw InvalidInputException("IN filter without values");
        if (n.n_values > 256) throw NotImplementedException("IN-list with more than 256 values is not pushed down");
        for (int32_t k = 0; k < n.n_values; k++) add(n.str_values[k], n.str_lens[k]);
        break;
      case MI_F_CONTAINS: case MI_F_ENDS_WITH: case MI_F_LIKE: case MI_F_NOT_LIKE: {
        if (!n.str_value || n.str_len < 0) throw InvalidInputException("string filter constant without bytes");
        const uint8_t* bytes = reinterpret_cast<const uint8_t*>(n.str_value);
        likematch::Pattern pat;
        CheckPattern(likematch::Compile(n.op, bytes, static_cast<uint32_t>(n.str_len), &pat), n.op, l.column);
        // What the existing leaves already say.  No segment: '%' alone or an empty needle is IS NOT NULL (NOT LIKE '%' keeps
        // nothing: an empty IN-list).  No '%': =.  'abc%': the prefix range.  Negated, the last two still drop NULL rows.
        if (pat.n_seg == 0 && !(pat.head && pat.tail)) {
          if (!pat.negate) l.op = device::kLeafIsNotNull;
          return l;
        }
        if (pat.n_seg <= 1 && pat.head) {   // anchored at both ends: no '%' at all; at the head alone: 'abc%'
          mi_filter_node folded = n;
          folded.op = pat.tail ? MI_F_EQ : MI_F_STARTS_WITH;
          folded.str_value = n.str_value + (pat.n_seg ? pat.off[0] : 0);
          folded.str_len = static_cast<int32_t>(pat.n_seg ? pat.len[0] : 0);
          FilterLeaf f = LeafOf(folded, columns);
          f.negate = pat.negate;
          return f;
        }
        l.op = device::kLeafStrMatch;
        l.negate = pat.negate;
        l.match_head = pat.head;
        l.match_tail = pat.tail;
        for (int s = 0; s < pat.n_seg; s++) l.str_values.emplace_back(n.str_value + pat.off[s], pat.len[s]);
        return l;
      }
      case MI_F_LT: case MI_F_LE: case MI_F_GT: case MI_F_GE: case MI_F_STARTS_WITH: {
        // ordering and prefix tests: one range leaf [lower, upper] with open / closed ends (byte-wise order)
        if (!n.str_value || n.str_len < 0) throw InvalidInputException("string filter constant without bytes");
        const std::string c(n.str_value, static_cast<size_t>(n.str_len));
        l.op = device::kLeafStrRange;
        l.str_values.assign(2, std::string());
        l.lo_open = l.hi_open = true;
        if (n.op == MI_F_LT || n.op == MI_F_LE) {
          l.str_values[1] = c;
          l.hi_open = false;
          l.hi_incl = n.op == MI_F_LE;
        } else if (n.op == MI_F_GT || n.op == MI_F_GE) {
          l.str_values[0] = c;
          l.lo_open = false;
          l.lo_incl = n.op == MI_F_GE;
        } else {
          // begins with c  <=>  c <= row < successor(c), the successor being c with its last byte that is not 0xFF
          // incremented and everything behind it dropped (all 0xFF or empty: no upper bound)
          l.str_values[0] = c;
          l.lo_open = false;
          l.lo_incl = true;
          std::string up = c;
          while (!up.empty() && static_cast<unsigned char>(up.back()) == 0xFF) up.pop_back();
          if (!up.empty()) {
            up.back() = static_cast<char>(static_cast<unsigned char>(up.back()) + 1);
            l.str_values[1] = up;
            l.hi_open = false;
            l.hi_incl = false;
          }
        }
        return l;
      }
      default:
        throw NotImplementedException("this comparison is not pushed down on VARCHAR / BLOB columns (column '" + l.column + "')");
    }
    std::sort(l.str_values.begin(), l.str_values.end());
    l.str_values.erase(std::unique(l.str_values.begin(), l.str_values.end()), l.str_values.end());
    return l;
  }
  if (n.op == MI_F_STARTS_WITH || n.op == MI_F_CONTAINS || n.op == MI_F_ENDS_WITH || n.op == MI_F_LIKE || n.op == MI_F_NOT_LIKE)
    throw InvalidInputException("filter on column '" + l.column + "': this operator takes a byte string (str_value)");
  switch (n.op) {
    case MI_F_EQ: closed(c, c); break;
    case MI_F_NE: closed(c, c); l.negate = true; break;
    case MI_F_LT: if (c == kMin) closed(1, 0); else { l.hi = c - 1; l.hi_open = false; } break;   // nothing is < MIN: an empty range
    case MI_F_LE: l.hi = c; l.hi_open = false; break;
    // nothing signed is > MAX, but a uint64 column reaches past it: Program decides (keys of FLOAT / DOUBLE end at NaN's)
    case MI_F_GT: if (c == kMax) { closed(1, 0); l.above_int64_max = !l.float_width; } else { l.lo = c + 1; l.lo_open = false; } break;
    case MI_F_GE: l.lo = c; l.lo_open = false; break;
    case MI_F_IS_NULL: l.op = device::kLeafIsNull; break;
    case MI_F_IS_NOT_NULL: l.op = device::kLeafIsNotNull; break;
    case MI_F_IN:
      if (n.n_values < 0 || (n.n_values > 0 && !n.values)) throw InvalidInputException("IN filter without values");
      if (n.n_values > 256) throw NotImplementedException("IN-list with more than 256 values is not pushed down");
      for (int32_t k = 0; k < n.n_values; k++) l.in_values.push_back(constant(n.values[k]));
      std::sort(l.in_values.begin(), l.in_values.end());
      l.in_values.erase(std::unique(l.in_values.begin(), l.in_values.end()), l.in_values.end());
      if (l.in_values.empty()) closed(1, 0);                                  // IN () keeps nothing
      else if (l.in_values.size() == 1) { closed(l.in_values[0], l.in_values[0]); l.in_values.clear(); }
      else l.op = device::kLeafIn;
      break;
    default: throw InvalidInputException("unknown filter op " + std::to_string(n.op));
  }
  return l;
}

size_t LeafCount(const FilterCnf& cnf) {
  size_t n = 0;
  for (auto& c : cnf) n += c.size();
  return n;
}

FilterCnf ToCnf(const mi_filter_node* nodes, int32_t n_nodes, int32_t at, int depth, const std::vector<ScanColumn>* columns) {
  if (at < 0 || at >= n_nodes) throw InvalidInputException("filter node index out of range");
  if (depth > 32) throw InvalidInputException("filter tree too deep");
  const mi_filter_node& n = nodes[at];
  if (n.op != MI_F_AND && n.op != MI_F_OR) return FilterCnf{{LeafOf(n, columns)}};
  if (n.n_children <= 0 || n.first_child < 0 || n.first_child > n_nodes - n.n_children) throw InvalidInputException("AND / OR filter node without children");
  FilterCnf out;
  if (n.op == MI_F_AND) {
    for (int32_t k = 0; k < n.n_children; k++) {
      FilterCnf c = ToCnf(nodes, n_nodes, n.first_child + k, depth + 1, columns);
      out.insert(out.end(), c.begin(), c.end());
    }
  } else {
    // (A1 & A2) | (B1 & B2) = (A1|B1) & (A1|B2) & (A2|B1) & (A2|B2): distribute child by child
    out = FilterCnf{{}};
    for (int32_t k = 0; k < n.n_children; k++) {
      FilterCnf c = ToCnf(nodes, n_nodes, n.first_child + k, depth + 1, columns);
      FilterCnf next;
      for (auto& left : out)
        for (auto& right : c) {
          next.push_back(left);
          next.back().insert(next.back().end(), right.begin(), right.end());
          if (LeafCount(next) > 4 * kMaxLeaves) throw NotImplementedException("filter is too complex to push into the scan");
        }
      out.swap(next);
    }
  }
  return out;
}
}  // namespace

FilterCnf NormaliseFilter(const mi_filter_node* nodes, int32_t n_nodes, int32_t root, const std::vector<ScanColumn>* columns) {
  if (!nodes || n_nodes <= 0) throw InvalidInputException("empty filter");
  FilterCnf cnf = ToCnf(nodes, n_nodes, root, 0, columns);
  // single-leaf range clauses on one column intersect (lo <= v AND v < hi -> one leaf)
  FilterCnf merged;
  for (auto& clause : cnf) {
    bool folded = false;
    if (clause.size() == 1 && clause[0].op == device::kLeafRange && !clause[0].negate && !clause[0].above_int64_max) {
      for (auto& m : merged) {
        if (m.size() == 1 && m[0].op == device::kLeafRange && !m[0].negate && !m[0].above_int64_max && m[0].column == clause[0].column) {
          if (!clause[0].lo_open) { m[0].lo = m[0].lo_open ? clause[0].lo : std::max(m[0].lo, clause[0].lo); m[0].lo_open = false; }
          if (!clause[0].hi_open) { m[0].hi = m[0].hi_open ? clause[0].hi : std::min(m[0].hi, clause[0].hi); m[0].hi_open = false; }
          folded = true;
          break;
        }
      }
    }
    if (!folded) merged.push_back(std::move(clause));
  }
  if (LeafCount(merged) > kMaxLeaves)
    throw NotImplementedException("filter needs " + std::to_string(LeafCount(merged)) + " leaves in conjunctive normal form, at most " +
                                  std::to_string(kMaxLeaves) + " are pushed into the scan");
  return merged;
}

void BoundFilter::Resolve(const std::vector<ScanColumn>& all_columns, const std::vector<ScanColumn>& out_columns) {
  // a filter column is either projected (its decoded vector is reused) or decoded for the filter alone
  columns.clear();
  only.clear();
  std::vector<std::string> filter_names;
  for (auto& clause : cnf) {
    for (auto& leaf : clause) {
      auto known = std::find(filter_names.begin(), filter_names.end(), leaf.column);
      if (known == filter_names.end()) {
        int32_t where = -1;
        for (size_t i = 0; i < out_columns.size(); i++)
          if (out_columns[i].name == leaf.column) where = static_cast<int32_t>(i);
        if (where < 0) {
          auto it = std::find_if(all_columns.begin(), all_columns.end(), [&](const ScanColumn& sc) { return sc.name == leaf.column; });
          if (it == all_columns.end()) throw InvalidInputException("filter column '" + leaf.column + "' does not exist in IPC file schema");
          only.push_back(*it);
          where = ~static_cast<int32_t>(only.size() - 1);
        }
        filter_names.push_back(leaf.column);
        columns.push_back(where);
        known = filter_names.end() - 1;
      }
      leaf.out_col = static_cast<int32_t>(known - filter_names.begin());
      const ScanColumn& sc = Column(static_cast<size_t>(leaf.out_col), out_columns);
      if (sc.is_constant()) throw NotImplementedException("filter on the constant column '" + sc.name + "' is not pushed into the scan");
      if ((leaf.op == device::kLeafIsNull || leaf.op == device::kLeafIsNotNull) && !leaf.is_string) {
        std::string why;
        if (!sc.field.Supported(&why)) throw NotImplementedException("Column '" + sc.name + "': " + why + " is not decoded by the MI355X scan path yet");
        continue;
      }
      int32_t kind, w;
      int64_t param;
      const ArrowField& vf = ValueField(sc.field);
      if (&vf != &sc.field && !sc.field.Plan(&kind, &param, &w))
        throw NotImplementedException("Column '" + sc.name + "': Arrow type +r with these children is not decoded by the MI355X scan path");
      // IN () -- an empty range -- keeps nothing (its negation every valid row) whatever the column holds
      if (!leaf.is_string && leaf.op == device::kLeafRange && !leaf.lo_open && !leaf.hi_open && leaf.lo > leaf.hi) continue;
      if (leaf.is_string) {
        // byte-string constants: the column must decode to string_t rows that point into ONE data buffer
        if (!(vf.Plan(&kind, &param, &w, /*value_only*/ true) && IsStringKind(kind)))
          throw NotImplementedException("string filter pushdown on column '" + sc.name + "' (" + sc.field.DuckType() +
                                        ") needs a utf8 / large_utf8 / binary / fixed_size_binary column (dictionary-encoded or not)");
        continue;
      }
      if (leaf.is_wide || leaf.float_width) {
        // FLOAT / DOUBLE / 128-bit constants: the column must be what they were made for (dictionary-encoded or not)
        const FilterValueClass cls = FilterClassOf(sc.field);
        const FilterValueClass want = leaf.is_wide ? FilterValueClass::kWide : leaf.float_width == 4 ? FilterValueClass::kFloat32 : FilterValueClass::kFloat64;
        if (cls != want)
          throw NotImplementedException("filter pushdown on column '" + sc.name + "' (" + sc.field.DuckType() + "): its constants are " +
                                        (leaf.is_wide ? "128-bit integers" : leaf.float_width == 4 ? "FLOAT keys" : "DOUBLE keys"));
        continue;
      }
      if (!(vf.Plan(&kind, &param, &w) && !vf.has_dictionary && IsIntegerLike(kind, w, vf, /*allow_bool*/ true)))
        throw NotImplementedException("filter pushdown on column '" + sc.name + "' (" + sc.field.DuckType() +
                                      ") with integer constants needs an integer / boolean / date / time / timestamp / decimal(<=18) column; FLOAT / "
                                      "DOUBLE and HUGEINT / DECIMAL(19..38) columns take constants of their own kind, VARCHAR / BLOB byte strings; "
                                      "intervals, nested types and string views are not compared in the scan");
    }
  }
}

void BoundFilter::UploadConstants() {
  d_in_lists.clear();
  for (auto& clause : cnf)
    for (auto& leaf : clause) {
      DeviceBuffer list;
      if (leaf.op == device::kLeafIn) {
        list = DeviceBuffer(leaf.in_values.size() * 8);
        MI_HIP_CHECK(hipMemcpy(list.get(), leaf.in_values.data(), leaf.in_values.size() * 8, hipMemcpyHostToDevice));
      } else if (leaf.is_wide) {
        // kLeafWideRange: {lo.lower, lo.upper, hi.lower, hi.upper}; kLeafWideIn: {lower, upper} per constant
        std::vector<int64_t> words;
        auto add = [&](wide_t v) { words.push_back(static_cast<int64_t>(LowerOf(v))); words.push_back(UpperOf(v)); };
        if (leaf.op == device::kLeafWideRange) { add(leaf.wide_lo); add(leaf.wide_hi); }
        else for (wide_t v : leaf.wide_in) add(v);
        list = DeviceBuffer(words.size() * 8);
        MI_HIP_CHECK(hipMemcpy(list.get(), words.data(), words.size() * 8, hipMemcpyHostToDevice));
      } else if ((leaf.op == device::kLeafStrIn || leaf.op == device::kLeafStrRange || leaf.op == device::kLeafStrMatch) && !leaf.str_values.empty()) {
        // 3 words per constant (its string_t image + the device address of its bytes), the bytes behind the table
        const size_t nc = leaf.str_values.size();
        size_t bytes = 0;
        for (auto& v : leaf.str_values) bytes += RoundUp(v.size() + 1, 8);
        std::vector<uint8_t> img(nc * 24 + bytes, 0);
        list = DeviceBuffer(img.size());
        size_t at = nc * 24;
        for (size_t k = 0; k < nc; k++) {
          const std::string& v = leaf.str_values[k];
          if (v.size() > 0xFFFFFFFFull) throw InvalidInputException("string filter constant too long");
          uint32_t dw[3] = {0, 0, 0};
          std::memcpy(dw, v.data(), std::min<size_t>(v.size(), v.size() <= 12 ? 12 : 4));
          const uint64_t w0 = static_cast<uint64_t>(v.size()) | (static_cast<uint64_t>(dw[0]) << 32);
          const uint64_t w1 = v.size() <= 12 ? (static_cast<uint64_t>(dw[1]) | (static_cast<uint64_t>(dw[2]) << 32)) : 0;
          const uint64_t w2 = reinterpret_cast<uint64_t>(list.get() + at);
          std::memcpy(&img[k * 24], &w0, 8);
          std::memcpy(&img[k * 24 + 8], &w1, 8);
          std::memcpy(&img[k * 24 + 16], &w2, 8);
          std::memcpy(&img[at], v.data(), v.size());
          at += RoundUp(v.size() + 1, 8);
        }
        MI_HIP_CHECK(hipMemcpy(list.get(), img.data(), img.size(), hipMemcpyHostToDevice));
      }
      d_in_lists.push_back(std::move(list));
    }
}

namespace {
// Does dictionary value `p` (decoded, `width` bytes) pass the FLOAT / DOUBLE / 128-bit leaf?  The kernel's comparison, once
// per entry; a negated leaf is negated by the look-up (kLeafDictMap mode 1), so that a NULL entry fails both.
bool ValuePasses(const FilterLeaf& leaf, const uint8_t* p, int32_t width) {
  if (leaf.is_wide) {
    uint64_t lower;
    int64_t upper;
    std::memcpy(&lower, p, 8);
    std::memcpy(&upper, p + 8, 8);
    if (leaf.op == device::kLeafWideIn) return std::binary_search(leaf.wide_in.begin(), leaf.wide_in.end(), WideOf(static_cast<int64_t>(lower), upper));
    return filterkey::WideInRange(upper, lower, UpperOf(leaf.wide_lo), LowerOf(leaf.wide_lo), UpperOf(leaf.wide_hi), LowerOf(leaf.wide_hi));
  }
  int64_t key;
  if (width == 4) {
    int32_t b;
    std::memcpy(&b, p, 4);
    key = filterkey::FloatKey(b);
  } else {
    int64_t b;
    std::memcpy(&b, p, 8);
    key = filterkey::FloatKey(b);
  }
  if (leaf.op == device::kLeafIn) return std::binary_search(leaf.in_values.begin(), leaf.in_values.end(), key);
  return key >= leaf.lo && key <= leaf.hi;   // open ends are kMin / kMax
}

// Which entries of a dictionary version pass `leaf` (one byte per entry: 0 no, 1 yes, 2 NULL), in HBM.
// Made once per (version, leaf); the upload rides `stream` in front of the filter kernel that reads it.
const void* DictMatchMap(DictState* dict, size_t li, const FilterLeaf& leaf, hipStream_t stream) {
  auto it = dict->match_maps.find(li);
  if (it != dict->match_maps.end()) return it->second.get();
  std::vector<uint8_t> codes(static_cast<size_t>(dict->dict_len) + 1, 0);
  struct LeafSegments {   // the segments of a kLeafStrMatch leaf as likematch::Matches takes them
    const std::vector<std::string>& v;
    uint32_t len(int s) const { return static_cast<uint32_t>(v[static_cast<size_t>(s)].size()); }
    uint8_t byte(int s, uint32_t i) const { return static_cast<uint8_t>(v[static_cast<size_t>(s)][i]); }
  };
  auto passes = [&](const std::string& v) {   // std::string compares byte-wise (unsigned), a proper prefix first
    if (leaf.op == device::kLeafStrMatch)
      return likematch::Matches(LeafSegments{leaf.str_values}, static_cast<int>(leaf.str_values.size()), leaf.match_head, leaf.match_tail,
                                reinterpret_cast<const uint8_t*>(v.data()), static_cast<uint32_t>(v.size()));
    if (leaf.op != device::kLeafStrRange) return std::binary_search(leaf.str_values.begin(), leaf.str_values.end(), v);
    auto cmp = [](const std::string& a, const std::string& b) {
      const int c = std::memcmp(a.data(), b.data(), std::min(a.size(), b.size()));
      return c != 0 ? c : (a.size() < b.size() ? -1 : a.size() > b.size() ? 1 : 0);
    };
    if (!leaf.lo_open) {
      const int c = cmp(v, leaf.str_values[0]);
      if (c < 0 || (c == 0 && !leaf.lo_incl)) return false;
    }
    if (!leaf.hi_open) {
      const int c = cmp(v, leaf.str_values[1]);
      if (c > 0 || (c == 0 && !leaf.hi_incl)) return false;
    }
    return true;
  };
  const bool by_value = leaf.is_wide || leaf.float_width != 0;
  const bool null_test = leaf.op == device::kLeafIsNull || leaf.op == device::kLeafIsNotNull;
  const size_t vw = static_cast<size_t>(dict->out_width);
  for (int64_t e = 0; e < dict->dict_len; e++)
    codes[static_cast<size_t>(e)] = !dict->host_valid[static_cast<size_t>(e)] ? 2
                                    : (by_value && !null_test) ? (ValuePasses(leaf, dict->host_values.data() + static_cast<size_t>(e) * vw, dict->out_width) ? 1 : 0)
                                    : (leaf.is_string && passes(dict->host_strings[static_cast<size_t>(e)])) ? 1 : 0;
  codes[static_cast<size_t>(dict->dict_len)] = 2;   // the NULL entry rows without a value point at
  // device copy + its pinned source
  const size_t map_bytes = RoundUp(codes.size() + 16, 256);
  auto map = std::make_shared<std::pair<DeviceBuffer, PinnedBuffer>>(DeviceBuffer(map_bytes), PinnedBuffer(map_bytes));
  std::memcpy(map->second.get(), codes.data(), codes.size());
  MI_HIP_CHECK(hipMemcpyAsync(map->first.get(), map->second.get(), codes.size(), hipMemcpyHostToDevice, stream));
  return dict->match_maps.emplace(li, std::shared_ptr<void>(map, map->first.get())).first->second.get();
}
}  // namespace

void LeafConstants(const FilterLeaf& leaf, const DeviceBuffer& constants, bool ends_clause, device::FilterLeafDev& L) {
  L.op = leaf.op;
  L.flags = (ends_clause ? device::kLeafEndsClause : 0) | (leaf.negate ? device::kLeafNegate : 0);
  L.lo = leaf.lo;
  L.hi = leaf.hi;
  L.in_values = constants.get<int64_t>();
  L.n_in = static_cast<int32_t>(leaf.is_string ? leaf.str_values.size() : leaf.is_wide ? leaf.wide_in.size() : leaf.in_values.size());
  if (leaf.op == device::kLeafStrRange)
    L.n_in = (leaf.lo_open ? 0 : 1) | (leaf.lo_incl ? 2 : 0) | (leaf.hi_open ? 0 : 4) | (leaf.hi_incl ? 8 : 0);
  if (leaf.op == device::kLeafStrMatch) L.n_in |= (leaf.match_head ? 0x100 : 0) | (leaf.match_tail ? 0x200 : 0);
  L.width = 1;
}

device::FilterProgram BoundFilter::Program(const std::vector<ScanColumn>& out_columns, const Batch& b, hipStream_t stream) const {
  device::FilterProgram prog;
  std::memset(&prog, 0, sizeof(prog));
  size_t li = 0;
  for (auto& clause : cnf) {
    for (size_t j = 0; j < clause.size(); j++, li++) {
      const FilterLeaf& leaf = clause[j];
      device::FilterLeafDev& L = prog.leaves[prog.n_leaves++];
      const int32_t root = b.roots[static_cast<size_t>(leaf.out_col)];
      LeafConstants(leaf, d_in_lists[li], j + 1 == clause.size(), L);
      if (root < 0) {
        // the column is absent from this file (union_by_name): every row is NULL -- IS NULL keeps every row, everything
        // else keeps none (an empty, non-negated range over any readable bytes: the selection buffer itself)
        L.validity = nullptr;
        L.flags &= ~device::kLeafNegate;
        if (leaf.op == device::kLeafIsNull) {
          L.op = device::kLeafIsNotNull;
        } else {
          L.op = device::kLeafRange;
          L.lo = 1;
          L.hi = 0;
          L.data = b.d_empty;
        }
        continue;
      }
      const PlannedNode& pn = b.nodes[static_cast<size_t>(root)];
      L.data = pn.alias_body_off >= 0 ? static_cast<const void*>(b.d_in + pn.alias_body_off) : static_cast<const void*>(b.d_out + pn.data_off);
      L.validity = pn.valid_off >= 0 ? reinterpret_cast<const uint64_t*>(b.d_out + pn.valid_off) : nullptr;
      L.width = std::max(pn.width, 1);
      const bool null_test = leaf.op == device::kLeafIsNull || leaf.op == device::kLeafIsNotNull;
      const bool by_value = !null_test && (leaf.is_wide || leaf.float_width != 0);
      if (pn.kind == MI_K_DICT && (leaf.is_string || null_test || by_value)) {
        // dictionary-encoded: match the dictionary version this batch uses once (host), the rows by index.  IS [NOT] NULL
        // goes the same way: a row is NULL when its index or its dictionary entry is
        const std::shared_ptr<DictState>& dict = b.node_dict[static_cast<size_t>(root)];
        if (!dict || (leaf.is_string && static_cast<int64_t>(dict->host_strings.size()) != dict->dict_len))
          throw NotImplementedException("string filter on the dictionary-encoded column '" + leaf.column + "': its dictionary values are not strings");
        if (by_value && (dict->out_width != (leaf.is_wide ? 16 : leaf.float_width) ||
                         dict->host_values.size() != static_cast<size_t>(dict->dict_len) * static_cast<size_t>(dict->out_width)))
          throw NotImplementedException("filter on the dictionary-encoded column '" + leaf.column + "': its dictionary values are not " +
                                        (leaf.is_wide ? "128-bit integers" : leaf.float_width == 4 ? "FLOAT" : "DOUBLE"));
        L.op = device::kLeafDictMap;
        L.in_values = static_cast<const int64_t*>(DictMatchMap(dict.get(), li, leaf, stream));
        L.n_in = static_cast<int32_t>(std::min<int64_t>(dict->dict_len + 1, 0x7FFFFFFF));
        L.lo = leaf.op == device::kLeafIsNull ? 2 : leaf.op == device::kLeafIsNotNull ? 3 : leaf.negate ? 1 : 0;
        L.flags &= ~device::kLeafNegate;   // applied inside the kernel: a NULL entry fails = and <> alike
        L.width = 4;
        continue;
      }
      if (leaf.is_string) {
        // the rows' long-string pointers are consumer addresses (pn.ptr_base = byte 0 of the Arrow data buffer as the
        // consumer sees it); the kernel reads the bytes from the HBM copy of that buffer
        const DecodedNode& src = b.batch.nodes[static_cast<size_t>(pn.source_node)];
        // run-end encoded: the rows point into the values child's data buffer
        const DecodedNode& dn = pn.kind == MI_K_RUN_END ? b.batch.nodes[static_cast<size_t>(src.children[1])] : src;
        const int32_t vkind = pn.kind == MI_K_RUN_END ? pn.value_kind : pn.kind;
        const size_t data_span = vkind == MI_K_FIXED_BINARY ? 1 : 2;
        L.lo = static_cast<int64_t>(reinterpret_cast<uintptr_t>(b.d_in + (dn.spans.size() > data_span ? dn.spans[data_span].offset : 0)));
        L.hi = static_cast<int64_t>(pn.ptr_base);
        continue;
      }
      if (leaf.is_wide) {
        if (pn.width != 16) throw InternalException("128-bit filter leaf on column '" + leaf.column + "' of width " + std::to_string(pn.width));
        continue;   // op and constants are set above
      }
      if (leaf.float_width && !null_test) {
        if (pn.width != leaf.float_width) throw InternalException("floating-point filter leaf on column '" + leaf.column + "' of width " + std::to_string(pn.width));
        L.flags |= device::kLeafFloat;
        continue;
      }
      const ArrowField& vf = ValueField(Column(static_cast<size_t>(leaf.out_col), out_columns).field);
      if (vf.type == MI_AT_INT && !vf.is_signed) {
        L.flags |= device::kLeafUnsigned;
        if (pn.width == 8 && !null_test) {
          // uint64: compared through the order-preserving map x ^ 2^63 on both sides.  Constants arrive as int64, a
          // negative one is below every value of the column.
          L.flags |= device::kLeafBias;
          const int64_t bias = static_cast<int64_t>(0x8000000000000000ull);
          if (leaf.op == device::kLeafRange && leaf.above_int64_max) {
            L.lo = 0;                                                  // v > INT64_MAX: the images of 2^63 ..
            L.hi = static_cast<int64_t>(0x7FFFFFFFFFFFFFFFull);        // .. UINT64_MAX
          } else if (leaf.op == device::kLeafRange) {
            if (!leaf.hi_open && leaf.hi < 0) { L.lo = 1; L.hi = 0; }   // empty (its negation keeps every valid row, as it must)
            else {
              L.lo = (leaf.lo_open || leaf.lo < 0) ? bias : (leaf.lo ^ bias);            // bias = the image of 0
              L.hi = leaf.hi_open ? static_cast<int64_t>(0x7FFFFFFFFFFFFFFFull) : (leaf.hi ^ bias);   // image of UINT64_MAX
            }
          }
          // IN-lists of uint64 columns are uploaded unbiased: compare them unbiased too.  That compares bit patterns, and
          // a negative constant is no value of the column: the list is sorted, so those are its head and are stepped over
          if (leaf.op == device::kLeafIn) {
            L.flags &= ~device::kLeafBias;
            const int32_t negative = static_cast<int32_t>(std::lower_bound(leaf.in_values.begin(), leaf.in_values.end(), int64_t(0)) - leaf.in_values.begin());
            L.in_values += negative;
            L.n_in -= negative;
            if (L.n_in == 0) { L.op = device::kLeafRange; L.lo = 1; L.hi = 0; }   // none is left: the leaf keeps nothing
          }
        }
      }
    }
  }
  return prog;
}

}  // namespace miarrow
