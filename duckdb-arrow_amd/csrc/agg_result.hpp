// agg_result.hpp -- the result side of the fused aggregates: what a draining call returns, the result order, the values as the
// C ABI returns them, and the merge of several devices' results by the rules the kernels merge by.  Host code, no HIP call.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/mi_arrow_ipc.h"
#include "agg_merge.hpp"
#include "group_key.hpp"
#include "hash_group.hpp"

namespace miarrow {

//! What mi_scan_aggregate returns: one partial per aggregate, the value class each is merged by (aggmerge::kClass*), the rows seen
struct AggResult {
  std::vector<aggmerge::Partial> values;
  std::vector<int32_t> classes;
  int64_t rows_scanned = 0, rows_selected = 0;
};
//! What the grouped calls return: the groups' normalised keys (group_key.hpp) and one partial per group and aggregate,
//! values[g * classes.size() + a]; kinds: groupkey::kKind* per key part.  In the result order once SortGroups ran.
struct GroupResult : AggResult {
  std::vector<int32_t> kinds;
  int32_t key_cls = 0;       // mi_scan_hash_aggregate alone: groupkey::kKey* of its one key column (one INT128 key part)
  std::vector<groupkey::Key> keys;
};

//! the result order: ascending by key, NULLS LAST (groupkey::KeyLess); the aggregates of a group travel with its key
void SortGroups(GroupResult* r);
//! a finished accumulator as the C ABI returns it
void FillAggValue(int32_t op, int32_t cls, const aggmerge::Partial& p, mi_agg_value* v);
//! a sorted result as the C ABI returns it; more groups than `capacity` is MI_EINVAL with *n_groups set
void FillGroupOutputs(const GroupResult& r, const std::vector<int32_t>& ops, mi_group_key_value* out_keys, mi_agg_value* out_values,
                      int32_t capacity, int32_t* n_groups);
//! the normalised key of K11's (key word, NULL flag) for a key column of class `key_cls`
groupkey::Key HashGroupKey(uint64_t word, bool is_null, int32_t key_cls);

// ---- several devices: the parts folded in sub-scan order (the double sums come out the same for the same device count),
// ops[a] the operation of aggregate a; the grouped ones sort.  false: the parts together cross the group limit -- of a scan
// (K10), `max_groups` (K11) -- and *out is not a result
void MergeAggResults(const std::vector<AggResult>& parts, const std::vector<int32_t>& ops, AggResult* out);
bool MergeGroupResults(const std::vector<GroupResult>& parts, const std::vector<int32_t>& ops, GroupResult* out);
bool MergeHashResults(const std::vector<GroupResult>& parts, const std::vector<int32_t>& ops, uint32_t max_groups, GroupResult* out);

}  // namespace miarrow
