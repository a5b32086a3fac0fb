// agg_bind.hpp -- bind time of the fused aggregates (mi_scan_aggregate, mi_scan_group_aggregate, mi_scan_hash_aggregate; K9,
// K10 and K11): what a call is given by column name, and the plan it becomes over the scan's bound columns -- or the refusal,
// whose message names the column as 'name' (DUCKTYPE) and the operation.  Host code over ipc_format.cpp alone, no HIP call.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "agg_merge.hpp"
#include "group_key.hpp"
#include "hash_group.hpp"
#include "scan_column.hpp"

namespace miarrow {

struct AggFactorSpec {
  bool has_column = false;   // false: the constant `add`
  std::string column;
  int64_t mul = 1, add = 0;  // MI_AGG_CONST_INT
  double fmul = 1.0, fadd = 0.0;   // MI_AGG_CONST_DOUBLE
  int32_t constants = MI_AGG_CONST_INT;
};
//! One aggregate of a call, by column name
struct AggSpec {
  int32_t op = 0;            // aggmerge::kOp*
  std::string a, b;
  std::vector<AggFactorSpec> factors;   // kOpSumExpr
};

struct BoundAgg {
  int32_t op = 0, cls = 0;               // cls: aggmerge::kClass* the partial is merged by
  int32_t col_a = -1, col_b = -1;        // slots of the projection
  int32_t cls_b = 0;
  struct Factor {
    int32_t col = -1, cls = 0;           // slot (-1: a constant), its class
    uint64_t mul = 0, add = 0;           // as device::AggFactorDev takes them
  };
  std::vector<Factor> factors;           // kOpSumExpr; col_a is then the first column factor's column
};
struct BoundKey {
  int32_t col = -1, cls = 0;             // slot of the projection, groupkey::kKey*
};
enum class AggMode { kPlain, kGrouped, kHash };   // K9, K10, K11
//! A call after bind: the columns it reads, in the order the scan projects them -- the first use of a column fixes its slot,
//! keys come before aggregates -- and the aggregates and keys over those slots
struct BoundAggregates {
  AggMode mode = AggMode::kPlain;
  uint32_t max_groups = 0;               // kHash
  std::vector<BoundAgg> aggs;
  std::vector<BoundKey> keys;            // kGrouped: 1 .. groupkey::kMaxKeys; kHash: one
  std::vector<std::string> projection;
};

//! mi_scan_aggregate, mi_scan_group_aggregate and mi_scan_hash_aggregate over the scan's bound `columns`.  COUNT(*) alone
//! projects the narrowest fixed-width column, else the first decodable one
BoundAggregates BindAggregates(const std::vector<ScanColumn>& columns, const std::vector<AggSpec>& specs);
BoundAggregates BindGroupAggregates(const std::vector<ScanColumn>& columns, const std::vector<std::string>& keys, const std::vector<AggSpec>& specs);
BoundAggregates BindHashAggregates(const std::vector<ScanColumn>& columns, const std::string& key, const std::vector<AggSpec>& specs, int64_t max_groups);

//! the constants of one factor as the kernels take them: int64 two's complement for an integer expression, the bits of a
//! double for a floating-point one.  Double constants on an integer expression are MI_ENOTSUP; integer constants a double
//! does not hold exactly are MI_EINVAL.  `what` begins the message.
void ExprFactorConstants(const std::string& what, bool is_float, int32_t constants, int64_t mul, int64_t add, double fmul, double fadd,
                         uint64_t* mul_bits, uint64_t* add_bits);
//! MI_ENOTSUP for a key class the hash table does not take (16-byte and string keys: K10 takes them for few groups), and
//! for an aggregate whose merge is not exact in any order (a floating-point sum) or has no atomic (a 16-byte MIN / MAX);
//! `who` names the column
void RefuseHashKeyClass(const std::string& who, int32_t key_cls);
void RefuseHashAggregate(const std::string& who, int32_t op, int32_t cls);
//! MI_EINVAL unless 1 <= max_groups <= MI_MAX_HASH_GROUPS
void CheckHashMaxGroups(const char* api, int64_t max_groups);
//! "SUM", "MIN", ... for messages
const char* AggOpName(int32_t op);

}  // namespace miarrow
