// scan_aggregate.hpp -- the host side of the fused aggregates (mi_scan_aggregate, mi_scan_group_aggregate,
// mi_scan_hash_aggregate; K9, K10 and K11):
// what a call is given by column name, what it returns, and the helpers the vector calls of c_api.cpp share with it.
// scan_aggregate.cpp holds the ArrowScan / MultiDeviceScan methods that bind, enqueue and drain them, and their C ABI.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi_arrow_ipc.h"
#include "agg_merge.hpp"
#include "group_key.hpp"
#include "hash_group.hpp"

namespace miarrow {

namespace device {
struct GroupProgram;   // kernels.hpp
}

//! One aggregate of mi_scan_aggregate by column name, and what a draining call returns: the accumulators, the value class
//! each is merged by (aggmerge::kClass*: what the host's merge of several devices needs), the rows seen
struct AggFactorSpec {
  bool has_column = false;   // false: the constant `add`
  std::string column;
  int64_t mul = 1, add = 0;  // MI_AGG_CONST_INT
  double fmul = 1.0, fadd = 0.0;   // MI_AGG_CONST_DOUBLE
  int32_t constants = MI_AGG_CONST_INT;
};
struct AggSpec {
  int32_t op = 0;            // aggmerge::kOp*
  std::string a, b;
  std::vector<AggFactorSpec> factors;   // kOpSumExpr
};
//! the constants of one factor as the kernels take them: int64 two's complement for an integer expression, the bits of a
//! double for a floating-point one.  Double constants on an integer expression are MI_ENOTSUP; integer constants a double
//! does not hold exactly are MI_EINVAL.  `what` begins the message.
void ExprFactorConstants(const std::string& what, bool is_float, int32_t constants, int64_t mul, int64_t add, double fmul, double fadd,
                         uint64_t* mul_bits, uint64_t* add_bits);
struct AggResult {
  std::vector<aggmerge::Partial> values;
  std::vector<int32_t> classes;
  int64_t rows_scanned = 0, rows_selected = 0;
};

//! What mi_scan_group_aggregate returns: the groups' normalised keys (group_key.hpp) and one partial per group and
//! aggregate, values[g * classes.size() + a]; kinds: groupkey::kKind* per key part.  In the result order once SortGroups ran.
struct GroupResult {
  std::vector<int32_t> kinds;
  std::vector<int32_t> classes;
  int32_t key_cls = 0;       // mi_scan_hash_aggregate alone: groupkey::kKey* of its one key column
  std::vector<groupkey::Key> keys;
  std::vector<aggmerge::Partial> values;
  int64_t rows_scanned = 0, rows_selected = 0;
};
//! copies the scan-wide table of K10 back (one copy: keys, accumulators, group count, flags), throws for the MI_ST_* bits it
//! carries and appends its groups to out->keys / out->values
void ReadGroupTable(const void* d_table, int n_keys, int n_aggs, hipStream_t stream, GroupResult* out);
//! the result order: ascending by key, NULLS LAST (groupkey::KeyLess)
void SortGroups(GroupResult* r);
//! a sorted result as the C ABI returns it; more groups than `capacity` is MI_EINVAL with *n_groups set
void FillGroupOutputs(const GroupResult& r, const std::vector<int32_t>& ops, mi_group_key_value* out_keys, mi_agg_value* out_values,
                      int32_t capacity, int32_t* n_groups);

// ---- K11, the hash GROUP BY for many groups (mi_scan_hash_aggregate, mi_hash_aggregate_vectors; hash_group.hpp).  Its result
// is a GroupResult with one INT128 key part.
//! MI_ENOTSUP for a key class the hash table does not take (16-byte and string keys: K10 takes them for few groups), and
//! for an aggregate whose merge is not exact in any order (a floating-point sum) or has no atomic (a 16-byte MIN / MAX);
//! `who` names the column
void RefuseHashKeyClass(const std::string& who, int32_t key_cls);
void RefuseHashAggregate(const std::string& who, int32_t op, int32_t cls);
//! MI_EINVAL unless 1 <= max_groups <= MI_MAX_HASH_GROUPS
void CheckHashMaxGroups(const char* api, int64_t max_groups);
//! the bytes of one call's device buffer: the table (hashgroup::TableBytes), then what hash_group_collect writes
size_t HashBufferBytes(uint32_t max_groups, int n_aggs);
//! hash_group_clear over such a buffer (asynchronous)
void ClearHashBuffer(const device::GroupProgram& prog, void* d_buf, uint32_t max_groups, hipStream_t stream);
//! hash_group_collect, then the head and exactly the records in use copied back: throws for the MI_ST_* bits the head carries
//! (MI_ST_GROUP_LIMIT with a message that names max_groups) and appends the groups to out->keys / out->values, unsorted
void CollectHashGroups(const device::GroupProgram& prog, void* d_buf, uint32_t max_groups, hipStream_t stream, GroupResult* out);

//! a finished accumulator as the C ABI returns it (mi_scan_aggregate, mi_aggregate_vectors)
inline void FillAggValue(int32_t op, int32_t cls, const aggmerge::Partial& p, mi_agg_value* v) {
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
//! "SUM", "MIN", ... for messages
const char* AggOpName(int32_t op);
//! MI_AGG_TIMING=1: device milliseconds of agg_windows / agg_combine summed over this process's calls of mi_scan_aggregate,
//! and of group_windows / group_combine over its calls of mi_scan_group_aggregate
void AggTimingTotals(double out_ms[2]);
void GroupTimingTotals(double out_ms[2]);
//! ... and of hash_group_rows / hash_group_collect over its calls of mi_scan_hash_aggregate and mi_hash_aggregate_vectors
void HashTimingTotals(double out_ms[2]);
//! adds one timed launch to those totals: which = 0 hash_group_rows, 1 hash_group_collect
void AddHashTiming(int which, double ms);

}  // namespace miarrow
