// kernels_hash_group.hip -- K11: hash GROUP BY over decoded vectors for MANY groups (mi_scan_hash_aggregate,
// mi_hash_aggregate_vectors): ONE integer key column, up to hashgroup::kMaxHashGroups distinct keys in a call, up to 8
// aggregates of K9's kinds whose merge is exact in any order, under the selection vectors of the pushed-down filter (K6) or
// over every row.  The table, its layout, the hash, the carry rule and the ordered words of MIN / MAX are hash_group.hpp,
// shared with the host; how a row is read is kernels_agg_fold.inl, shared with K9 and K10.
//
// hash_group_clear:   one lane per slot: the key word free, the slot's records the identity of their operation; the head zero.
// hash_group_rows:    one 256-thread workgroup per 2048-row window, a lane per selected row, 256 rows at a time.  The lane
//   normalises its key (the bytes under a NULL are not read), hashes it and probes linearly with a 64-bit compare-and-swap
//   of (free -> key), relaxed, agent scope: the answer `free` (the lane claimed the slot: a new group, the group counter is
//   bumped) or `key` ends the probe, anything else steps on, masked to the table.  A key word is complete the moment it is
//   claimed, so there is no busy state and no lane ever waits for another lane or workgroup.  The NULL key and the key whose
//   word is the free mark own the two records behind the probed range and are never probed for.  Then, per aggregate, the
//   row is folded into an empty partial by K9's fold -- validity, loads, product and expression walk are that text -- and
//   what it holds goes to the slot's record by atomics: count by an add; a sum by a returning add on lo and one add on hi of
//   the value's high word plus the carry the returned value shows; MIN / MAX by an unsigned 64-bit atomic min / max of the
//   ordered word.  Every one of these commutes, so the table is a function of the selected rows alone.
//   A probe that runs through the whole table, or a group counter past max_groups, raises MI_ST_GROUP_LIMIT and the row
//   contributes nothing.  Status bits are ORed over the wave and go to the head by one atomic OR per wave that has any: a
//   clean run issues none.
// hash_group_collect: one lane per slot and extra record.  A record in use takes an output index from one atomic add per
//   wave, and writes its key word, its NULL bit and its aggregates as aggmerge::Partial (MIN / MAX words mapped back,
//   count == 0 left as the NULL rule) into dense arrays.  The host sorts them, so the output is a function of the data alone.
// Every loop is bounded by the table size, the aggregate count or the window's rows.  No loaded value is an address except
// a selection index -- the count of a window is clamped to its rows, an index at or past them is skipped and raises
// MI_ST_SEL_RANGE, as in agg_windows -- and a slot, which is masked to the table.  All writes to the table are vector
// atomics or plain vector stores.
#include "device_common.hpp"
#include "agg_merge.hpp"
#include "group_key.hpp"
#include "hash_group.hpp"

#include <atomic>

namespace miarrow {
namespace device {

namespace {

using aggmerge::Partial;

#include "kernels_agg_fold.inl"

#define MI_RELAXED_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// ops: 4 bits per aggregate, as PackOpsClasses packs them
__global__ __launch_bounds__(kBlockThreads) void hash_group_clear(const HashTableDev table, int32_t n_aggs, uint32_t ops) {
  const size_t t = static_cast<size_t>(blockIdx.x) * kBlockThreads + threadIdx.x;
  const size_t slots = table.slots;
  if (t < hashgroup::kHeadWords) GM<uint32_t>(table.head)[t] = 0;
  if (t >= slots + hashgroup::kExtraRecords) return;
  if (t < slots) GM<uint64_t>(table.keys)[t] = hashgroup::kEmptyKey;
  gptr<uint64_t> rec = GM<uint64_t>(table.records) + t * static_cast<size_t>(n_aggs) * hashgroup::kRecordWords;
  for (int a = 0; a < n_aggs; a++) {
    rec[a * hashgroup::kRecordWords] = hashgroup::RecordInit(static_cast<int>((ops >> (4 * a)) & 15u));
    rec[a * hashgroup::kRecordWords + 1] = 0;
    rec[a * hashgroup::kRecordWords + 2] = 0;
  }
}

// an extra record comes into use: the first lane to set its word bumps the group counter; false: past max_groups
__device__ __forceinline__ bool claim_extra(const HashTableDev& table, uint32_t which) {
  gptr<uint32_t> head = GM<uint32_t>(table.head);
  gptr<uint32_t> word = head + hashgroup::kHeadExtra + which;
  if (__hip_atomic_load(word, MI_RELAXED_AGENT) != 0) return true;
  if (__hip_atomic_fetch_or(word, 1u, MI_RELAXED_AGENT) != 0) return true;
  return __hip_atomic_fetch_add(head + hashgroup::kHeadGroups, 1u, MI_RELAXED_AGENT) < table.max_groups;
}

// The kernel's text, once.  EXPR: the program may hold kOpSumExpr aggregates and `exprs` is their table.
template <bool HAS_SEL, bool EXPR>
__device__ __forceinline__ void hash_group_rows_body(const GroupProgram& prog, const AggExprTable* exprs, const mi_sel_t* __restrict__ sel_p,
                                                     const uint32_t* __restrict__ sel_count_p, int64_t nrows, const HashTableDev& table) {
  const int64_t window = blockIdx.x;
  const int64_t row0 = window * kTileRows;
  const int64_t left = nrows - row0;
  const uint32_t n = left < kTileRows ? static_cast<uint32_t>(left < 0 ? 0 : left) : static_cast<uint32_t>(kTileRows);
  uint32_t cnt = n;
  if (HAS_SEL) {
    const uint32_t c = GC<uint32_t>(sel_count_p)[window];
    cnt = c < n ? c : n;   // a count past the window's rows is clamped: sel[] is read inside the window's slots only
  }
  gptr<const mi_sel_t> sel = GC<mi_sel_t>(sel_p) + row0;
  const GroupKeyColumnDev& kc = prog.keys[0];
  const int n_aggs = prog.aggs.n_aggs;
  const uint32_t mask = table.slots - 1;
  gptr<uint64_t> tkeys = GM<uint64_t>(table.keys);
  gptr<uint64_t> trecs = GM<uint64_t>(table.records);
  gptr<uint32_t> head = GM<uint32_t>(table.head);

  uint32_t flags = 0;
  for (uint32_t i = threadIdx.x; i < cnt; i += kBlockThreads) {
    uint32_t r = i;
    if (HAS_SEL) {
      r = sel[i];
      if (r >= n) {   // not a row of this window: never dereferenced
        flags |= MI_ST_SEL_RANGE;
        continue;
      }
    }
    const int64_t row = row0 + r;

    // ---- the row's record: the slot its key holds, or one of the two extra records
    size_t at;
    bool ok;
    if (!row_is_valid(kc.validity, row)) {   // the bytes under a NULL are not read
      at = static_cast<size_t>(table.slots) + hashgroup::kExtraNull;
      ok = claim_extra(table, hashgroup::kExtraNull);
    } else {
      uint64_t raw;
      switch (kc.width) {
        case 1: raw = GC<uint8_t>(kc.data)[row]; break;
        case 2: raw = GC<uint16_t>(kc.data)[row]; break;
        case 4: raw = GC<uint32_t>(kc.data)[row]; break;
        default: raw = GC<uint64_t>(kc.data)[row]; break;
      }
      uint64_t key, key_hi;
      groupkey::NormInteger(kc.cls, kc.width, raw, &key, &key_hi);
      if (key == hashgroup::kEmptyKey) {
        at = static_cast<size_t>(table.slots) + hashgroup::kExtraEmptyKey;
        ok = claim_extra(table, hashgroup::kExtraEmptyKey);
      } else {
        uint32_t h = static_cast<uint32_t>(hashgroup::Hash(key)) & mask;
        ok = false;
        for (uint32_t probe = 0; probe <= mask; probe++) {   // bounded by the table
          uint64_t seen = hashgroup::kEmptyKey;
          __hip_atomic_compare_exchange_strong(tkeys + h, &seen, key, __ATOMIC_RELAXED, MI_RELAXED_AGENT);
          if (seen == hashgroup::kEmptyKey) {   // claimed: a new group
            ok = __hip_atomic_fetch_add(head + hashgroup::kHeadGroups, 1u, MI_RELAXED_AGENT) < table.max_groups;
            break;
          }
          if (seen == key) {
            ok = true;
            break;
          }
          h = (h + 1) & mask;
        }
        at = h;
      }
    }
    if (!ok) {   // the table is full, or holds more than max_groups keys: the row joins no group, the call fails
      flags |= MI_ST_GROUP_LIMIT;
      continue;
    }

    // ---- the aggregates: the row folded into an empty partial, the partial applied to the record
    gptr<uint64_t> rec = trecs + at * static_cast<size_t>(n_aggs) * hashgroup::kRecordWords;
#pragma clang loop unroll(disable)
    for (int a = 0; a < n_aggs; a++, rec += hashgroup::kRecordWords) {
      const AggDescDev& d = prog.aggs.aggs[a];
      const int op = d.op, cls = d.a.cls;
      Partial p = {0ull, 0ull, 0ull, 0ull};
      if (EXPR && op == aggmerge::kOpSumExpr) fold_expr_row(exprs->exprs[a], cls, row, &p);
      else fold_row(d, op, cls, row, &p);
      if (p.count == 0) continue;   // a NULL input: nothing contributes
      if (op == aggmerge::kOpMin) {
        __hip_atomic_fetch_min(rec, hashgroup::OrderedWord(cls, p.lo), MI_RELAXED_AGENT);
      } else if (op == aggmerge::kOpMax) {
        __hip_atomic_fetch_max(rec, hashgroup::OrderedWord(cls, p.lo), MI_RELAXED_AGENT);
      } else if (op != aggmerge::kOpCountStar && op != aggmerge::kOpCount) {
        const uint64_t old = __hip_atomic_fetch_add(rec, p.lo, MI_RELAXED_AGENT);
        const uint64_t high = p.hi + hashgroup::CarryOf(old, p.lo);
        if (high != 0) __hip_atomic_fetch_add(rec + 1, high, MI_RELAXED_AGENT);
      }
      __hip_atomic_fetch_add(rec + 2, 1ull, MI_RELAXED_AGENT);
    }
  }

  // ---- status: ORed over the wave, one atomic per wave that has any
#pragma unroll
  for (int dist = 32; dist >= 1; dist >>= 1) flags |= __shfl_xor(flags, dist, 64);
  if ((threadIdx.x & 63) == 0 && flags) __hip_atomic_fetch_or(head + hashgroup::kHeadStatus, flags, MI_RELAXED_AGENT);
}

template <bool HAS_SEL>
__global__ __launch_bounds__(kBlockThreads) void hash_group_rows(const GroupProgram prog, const mi_sel_t* __restrict__ sel_p,
                                                                 const uint32_t* __restrict__ sel_count_p, int64_t nrows,
                                                                 const HashTableDev table) {
  hash_group_rows_body<HAS_SEL, false>(prog, nullptr, sel_p, sel_count_p, nrows, table);
}

// launched only for a program that holds a kOpSumExpr: the expression table rides behind the arguments of hash_group_rows
template <bool HAS_SEL>
__global__ __launch_bounds__(kBlockThreads) void hash_group_rows_expr(const GroupProgram prog, const mi_sel_t* __restrict__ sel_p,
                                                                      const uint32_t* __restrict__ sel_count_p, int64_t nrows,
                                                                      const HashTableDev table, const AggExprTable exprs) {
  hash_group_rows_body<HAS_SEL, true>(prog, &exprs, sel_p, sel_count_p, nrows, table);
}

// ops / classes: 4 bits per aggregate, as PackOpsClasses packs them
__global__ __launch_bounds__(kBlockThreads) void hash_group_collect(const HashTableDev table, int32_t n_aggs, uint32_t ops, uint32_t classes,
                                                                    const HashCollectOut out) {
  const size_t t = static_cast<size_t>(blockIdx.x) * kBlockThreads + threadIdx.x;
  const size_t slots = table.slots;
  const int lane = threadIdx.x & 63;
  gptr<uint32_t> head = GM<uint32_t>(table.head);
  uint64_t key = 0;
  uint32_t is_null = 0;
  bool used = false;
  if (t < slots) {
    key = GC<uint64_t>(table.keys)[t];
    used = key != hashgroup::kEmptyKey;
  } else if (t < slots + hashgroup::kExtraRecords) {
    const uint32_t which = static_cast<uint32_t>(t - slots);
    used = head[hashgroup::kHeadExtra + which] != 0;
    is_null = which == hashgroup::kExtraNull ? 1u : 0u;
    key = is_null ? 0ull : hashgroup::kEmptyKey;
  }
  // the wave's records in use take consecutive indices behind one atomic add (every lane of the wave is here)
  const uint64_t users = __ballot(used);
  if (users == 0) return;   // (uniform over the wave)
  const int leader = __ffsll(static_cast<unsigned long long>(users)) - 1;
  uint32_t base = 0;
  if (lane == leader) base = __hip_atomic_fetch_add(head + hashgroup::kHeadCollected, static_cast<uint32_t>(__popcll(users)), MI_RELAXED_AGENT);
  base = __shfl(base, leader, 64);
  if (!used) return;
  const uint32_t g = base + static_cast<uint32_t>(__popcll(users & ((1ull << lane) - 1ull)));
  if (g >= table.max_groups) return;   // (only when the call has failed with MI_ST_GROUP_LIMIT: the arrays hold max_groups)
  GM<uint64_t>(out.keys)[g] = key;
  GM<uint32_t>(out.nulls)[g] = is_null;
  gptr<const uint64_t> rec = GC<uint64_t>(table.records) + t * static_cast<size_t>(n_aggs) * hashgroup::kRecordWords;
  gptr<Partial> po = GM<Partial>(out.partials) + static_cast<size_t>(g) * n_aggs;
  for (int a = 0; a < n_aggs; a++, rec += hashgroup::kRecordWords) {
    const int op = static_cast<int>((ops >> (4 * a)) & 15u), cls = static_cast<int>((classes >> (4 * a)) & 15u);
    Partial p = {0ull, 0ull, rec[2], 0ull};
    if (p.count != 0 && op != aggmerge::kOpCountStar && op != aggmerge::kOpCount) {
      if (op == aggmerge::kOpMin || op == aggmerge::kOpMax) {
        hashgroup::FromOrderedWord(cls, rec[0], &p.lo, &p.hi);
      } else {
        p.lo = rec[0];
        p.hi = rec[1];
      }
    }
    store_partial(po + a, p);
  }
}

size_t Align16(size_t v) { return (v + 15) & ~static_cast<size_t>(15); }

std::atomic<int64_t> g_hash_launches[2];   // hash_group_rows, hash_group_collect

}  // namespace

void HashGroupLaunchCounts(int64_t out[2]) {
  out[0] = g_hash_launches[0].load();
  out[1] = g_hash_launches[1].load();
}

bool HashGroupProgramIsValid(const GroupProgram& prog, const AggExprTable* exprs) {
  if (prog.n_keys != 1 || !prog.keys[0].data) return false;
  if (!AggProgramIsValid(prog.aggs, exprs)) return false;
  int ops[aggmerge::kMaxAggregates], classes[aggmerge::kMaxAggregates];
  for (int a = 0; a < prog.aggs.n_aggs; a++) {
    ops[a] = prog.aggs.aggs[a].op;
    classes[a] = prog.aggs.aggs[a].a.cls;
  }
  return hashgroup::HashProgramIsValid(prog.keys[0].cls, prog.keys[0].width, prog.aggs.n_aggs, ops, classes);
}

HashTableDev HashTableAt(void* base, uint32_t max_groups, int n_aggs) {
  uint8_t* p = static_cast<uint8_t*>(base);
  HashTableDev t;
  t.slots = hashgroup::SlotsFor(max_groups);
  t.max_groups = max_groups;
  t.head = reinterpret_cast<uint32_t*>(p);
  p += 4 * hashgroup::kHeadWords;
  t.keys = reinterpret_cast<uint64_t*>(p);
  p += 8 * static_cast<size_t>(t.slots);
  t.records = reinterpret_cast<uint64_t*>(p);
  return t;
}

size_t HashCollectBytes(uint32_t max_groups, int n_aggs) {
  const size_t g = max_groups;
  return Align16(g * 8) + g * static_cast<size_t>(n_aggs) * sizeof(aggmerge::Partial) + Align16(g * 4);
}

HashCollectOut HashCollectAt(void* base, uint32_t max_groups, int n_aggs) {
  const size_t g = max_groups;
  uint8_t* p = static_cast<uint8_t*>(base);
  HashCollectOut o;
  o.keys = reinterpret_cast<uint64_t*>(p);
  p += Align16(g * 8);
  o.partials = reinterpret_cast<aggmerge::Partial*>(p);
  p += g * static_cast<size_t>(n_aggs) * sizeof(aggmerge::Partial);
  o.nulls = reinterpret_cast<uint32_t*>(p);
  return o;
}

namespace {
bool TableOk(const HashTableDev& t) {
  return t.head && t.keys && t.records && t.max_groups >= 1 && t.max_groups <= hashgroup::kMaxHashGroups && t.slots == hashgroup::SlotsFor(t.max_groups);
}
uint32_t BlocksOver(const HashTableDev& t) {
  return static_cast<uint32_t>((static_cast<size_t>(t.slots) + hashgroup::kExtraRecords + kBlockThreads - 1) / kBlockThreads);
}
}  // namespace

hipError_t LaunchHashGroupClear(const GroupProgram& prog, const HashTableDev& table, hipStream_t stream) {
  MI_DROP_STALE_ERROR();
  if (!TableOk(table) || prog.aggs.n_aggs < 1 || prog.aggs.n_aggs > aggmerge::kMaxAggregates) return hipErrorInvalidValue;
  uint32_t ops, classes;
  PackOpsClasses(prog.aggs, &ops, &classes);
  hipLaunchKernelGGL(hash_group_clear, dim3(BlocksOver(table)), dim3(kBlockThreads), 0, stream, table, prog.aggs.n_aggs, ops);
  return hipGetLastError();
}

hipError_t LaunchHashGroupRows(const GroupProgram& prog, const mi_sel_t* sel, const uint32_t* sel_count, int64_t nrows,
                               const HashTableDev& table, hipStream_t stream, const AggExprTable* exprs) {
  MI_DROP_STALE_ERROR();
  if (nrows <= 0) return hipSuccess;
  if (!HashGroupProgramIsValid(prog, exprs) || (sel == nullptr) != (sel_count == nullptr) || !TableOk(table)) return hipErrorInvalidValue;
  const int64_t windows = (nrows + kTileRows - 1) / kTileRows;
  if (windows > 0x7FFFFFFFll) return hipErrorInvalidValue;
  const dim3 grid(static_cast<uint32_t>(windows)), block(kBlockThreads);
  if (AggProgramHasExpr(prog.aggs)) {
    if (sel) hipLaunchKernelGGL(hash_group_rows_expr<true>, grid, block, 0, stream, prog, sel, sel_count, nrows, table, *exprs);
    else hipLaunchKernelGGL(hash_group_rows_expr<false>, grid, block, 0, stream, prog, sel, sel_count, nrows, table, *exprs);
  } else if (sel) hipLaunchKernelGGL(hash_group_rows<true>, grid, block, 0, stream, prog, sel, sel_count, nrows, table);
  else hipLaunchKernelGGL(hash_group_rows<false>, grid, block, 0, stream, prog, sel, sel_count, nrows, table);
  g_hash_launches[0]++;
  return hipGetLastError();
}

hipError_t LaunchHashGroupCollect(const GroupProgram& prog, const HashTableDev& table, const HashCollectOut& out, hipStream_t stream) {
  MI_DROP_STALE_ERROR();
  if (!TableOk(table) || prog.aggs.n_aggs < 1 || prog.aggs.n_aggs > aggmerge::kMaxAggregates || !out.keys || !out.partials || !out.nulls)
    return hipErrorInvalidValue;
  uint32_t ops, classes;
  PackOpsClasses(prog.aggs, &ops, &classes);
  hipLaunchKernelGGL(hash_group_collect, dim3(BlocksOver(table)), dim3(kBlockThreads), 0, stream, table, prog.aggs.n_aggs, ops, classes, out);
  g_hash_launches[1]++;
  return hipGetLastError();
}

}  // namespace device
}  // namespace miarrow
