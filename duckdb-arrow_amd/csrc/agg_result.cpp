// agg_result.cpp -- see agg_result.hpp.
#include "agg_result.hpp"

#include <algorithm>
#include <cstring>
#include <string>

#include "ipc_format.hpp"

namespace miarrow {

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

void FillAggValue(int32_t op, int32_t cls, const aggmerge::Partial& p, mi_agg_value* v) {
  std::memset(v, 0, sizeof(*v));
  v->count = static_cast<int64_t>(p.count);
  if (op == aggmerge::kOpCountStar || op == aggmerge::kOpCount) {
    v->kind = MI_AGG_VALUE_INT128;
    v->lo = p.count;
    return;
  }
  v->kind = cls == aggmerge::kClassFloat ? MI_AGG_VALUE_DOUBLE : MI_AGG_VALUE_INT128;
  v->is_null = aggmerge::IsNull(op, p) ? 1 : 0;
  if (v->is_null) return;
  v->lo = p.lo;
  v->hi = static_cast<int64_t>(p.hi);
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

groupkey::Key HashGroupKey(uint64_t word, bool is_null, int32_t key_cls) {
  groupkey::Key k;
  std::memset(&k, 0, sizeof(k));
  k.nulls = is_null ? 1u : 0u;
  if (!is_null) {
    k.lo[0] = word;
    k.hi[0] = hashgroup::KeyHigh(key_cls, word);
  }
  return k;
}

namespace {
//! *out: what every part agrees on (kinds, classes, key class: every sub-scan bound the same), no value yet, the rows added up
template <typename Result>
void StartMerge(const std::vector<Result>& parts, Result* out) {
  *out = parts[0];
  out->values.clear();
  out->rows_scanned = out->rows_selected = 0;
  for (const Result& p : parts) {
    out->rows_scanned += p.rows_scanned;
    out->rows_selected += p.rows_selected;
  }
}

//! group by group through `table`: merge(key, partials) folds one group in, key_at(g) is the key of the table's group g
template <typename Table, typename MergeGroup, typename KeyAt>
bool MergeThrough(const std::vector<GroupResult>& parts, const Table& table, MergeGroup&& merge, KeyAt&& key_at, GroupResult* out) {
  StartMerge(parts, out);
  out->keys.clear();
  const size_t n_aggs = out->classes.size();
  for (const GroupResult& p : parts)
    for (size_t g = 0; g < p.keys.size(); g++)
      if (!merge(p.keys[g], &p.values[g * n_aggs])) return false;
  for (size_t g = 0; g < table.size(); g++) {
    out->keys.push_back(key_at(g));
    out->values.insert(out->values.end(), table.partials(g), table.partials(g) + n_aggs);
  }
  SortGroups(out);
  return true;
}
}  // namespace

void MergeAggResults(const std::vector<AggResult>& parts, const std::vector<int32_t>& ops, AggResult* out) {
  StartMerge(parts, out);
  out->values.assign(ops.size(), aggmerge::Partial{0, 0, 0, 0});
  for (const AggResult& p : parts)
    for (size_t a = 0; a < ops.size(); a++) aggmerge::Merge(ops[a], out->classes[a], &out->values[a], p.values[a]);
}

bool MergeGroupResults(const std::vector<GroupResult>& parts, const std::vector<int32_t>& ops, GroupResult* out) {
  groupkey::GroupTable table(static_cast<int>(parts[0].kinds.size()), ops, parts[0].classes);   // (groupkey::GroupTable: the kernels' rules)
  return MergeThrough(parts, table, [&](const groupkey::Key& k, const aggmerge::Partial* p) { return table.Merge(k, p); },
                      [&](size_t g) { return table.key(g); }, out);
}

bool MergeHashResults(const std::vector<GroupResult>& parts, const std::vector<int32_t>& ops, uint32_t max_groups, GroupResult* out) {
  hashgroup::SerialTable table(max_groups, ops, parts[0].classes);   // the serial model of the device's table
  return MergeThrough(parts, table, [&](const groupkey::Key& k, const aggmerge::Partial* p) { return table.Merge(k.lo[0], (k.nulls & 1u) != 0, p); },
                      [&](size_t g) { return HashGroupKey(table.key(g), table.is_null(g), parts[0].key_cls); }, out);
}

}  // namespace miarrow
