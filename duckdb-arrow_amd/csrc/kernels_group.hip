// kernels_group.hip -- K10: GROUP BY over decoded vectors (mi_scan_group_aggregate, mi_group_aggregate_vectors): up to 4
// key columns, up to 8 aggregates of K9's kinds (the expression sum included) per group, under the selection vectors of the
// pushed-down filter (K6) or over every row.  How a row is read and folded, and how a wave reduces its lanes' partials, is
// kernels_agg_fold.inl, the one place for it, shared with K9; this file keeps the key table, the sort and the ranking.
// Scope: few groups -- at most groupkey::kWindowLimit distinct keys among the selected rows of one 2048-row window,
// groupkey::kMaxGroups in a scan; more raises MI_ST_GROUP_LIMIT.  The rules of a key are group_key.hpp, the rules of a
// merge agg_merge.hpp, both shared with the host.
//
// group_windows: one 256-thread workgroup per 2048-row window, in three steps.
//   1. keys     256 selected rows at a time: a lane normalises the key of its row and finds or inserts it in the window's
//               table in LDS (512 slots, linear probing, the key storage sized by the number of key columns).  A slot is
//               claimed by an LDS compare-and-swap; the claimant writes its key before a barrier, behind it every lane
//               that still looks compares with what the slot holds and either has its slot or steps on.  Which of two
//               different keys wins a slot is left to the hardware: slot numbers mean nothing downstream.
//   2. order    every selected row is the word (slot << 11 | row in window); a bitonic sort in LDS puts a group's rows side
//               by side, ascending.  No row is placed by a ticket: where a row lands is a function of the data.
//   3. fold     wave v takes the local groups v, v + 4, ...: lane l folds the group's rows l, l + 64, ... in ascending
//               order, then the wave reduces by shuffles exactly as agg_windows does.  One Partial per local group and
//               aggregate; the work is selected rows x aggregates + local groups x aggregates, never rows x groups.
//   It writes head[window] = {local groups, flags}, keys[window][g], partials[window][g][aggregate], g the rank of the
//   group's slot among the slots in use.
// group_combine: one workgroup.  Windows in ascending order: lane g finds or inserts local key g in the scan-wide table
//   (HBM: 8192 slots over 4096 key / accumulator records; within a window the keys differ, so two lanes never insert the
//   same one), then the window's partials are merged into those groups' accumulators with aggmerge::Merge.  A group's
//   accumulator therefore takes its windows in ascending order whatever slots the keys won: with the fixed fold above,
//   every double sum has one shape for the same input.
// No atomics between workgroups and no waiting on another workgroup: the launch boundary is the only reduction across
// workgroups.  Status bits travel in the window heads and the table head, ORed; there is no status word.
// No loaded value is an address except a selection index -- the count of a window is clamped to its rows, an index at or
// past them is skipped and raises MI_ST_SEL_RANGE, as in agg_windows -- and a table slot, which is masked to the table.
// A probe sequence is bounded by the table's size.  A string key's length is looked at only to mask its padding and to
// refuse more than 12 bytes (MI_ST_GROUP_KEY_LONG): the pointer of a long string is never followed.
#include "device_common.hpp"
#include "agg_merge.hpp"
#include "group_key.hpp"

#include <atomic>

namespace miarrow {
namespace device {

namespace {

using aggmerge::Partial;
using groupkey::Key;

constexpr int kWinSlots = 2 * groupkey::kWindowLimit;      // the window's table in LDS
constexpr uint32_t kTableSlots = kGroupTableSlots;         // the scan-wide table in HBM
constexpr uint32_t kSlotEmpty = 0xFFFFFFFFu, kSlotBusy = 0xFFFFFFFEu;
constexpr uint32_t kNoRow = 0xFFFFFFFFu;

#include "kernels_agg_fold.inl"

// one part of the key of `row`: 0, MI_ST_GROUP_KEY_LONG for a string that has no inline image, or kPartNull
constexpr uint32_t kPartNull = 1u;
__device__ __forceinline__ uint32_t load_key_part(const GroupKeyColumnDev& c, int64_t row, uint64_t* lo, uint64_t* hi) {
  *lo = 0;
  *hi = 0;
  if (!row_is_valid(c.validity, row)) return kPartNull;   // the bytes under a NULL are not read
  if (c.cls == groupkey::kKeyWide) {
    const u64x2 v = GC<u64x2_a8>(c.data)[row];
    *lo = v.x;
    *hi = v.y;
    return 0;
  }
  if (c.cls == groupkey::kKeyString) {
    const u64x2 v = GC<u64x2_a8>(c.data)[row];
    return groupkey::NormString(v.x, v.y, lo, hi) ? 0u : MI_ST_GROUP_KEY_LONG;
  }
  uint64_t raw;
  switch (c.width) {
    case 1: raw = GC<uint8_t>(c.data)[row]; break;
    case 2: raw = GC<uint16_t>(c.data)[row]; break;
    case 4: raw = GC<uint32_t>(c.data)[row]; break;
    default: raw = GC<uint64_t>(c.data)[row]; break;
  }
  groupkey::NormInteger(c.cls, c.width, raw, lo, hi);
  return 0;
}

// The kernel's text, once.  EXPR: the program may hold kOpSumExpr aggregates and `exprs` is their table; without it the
// branch is not compiled and `exprs` not looked at, so group_windows<HAS_SEL> below is the kernel it was before expressions.
template <bool HAS_SEL, bool EXPR>
__device__ __forceinline__ void group_windows_body(const GroupProgram& prog, const AggExprTable* exprs, const mi_sel_t* __restrict__ sel_p,
                                                   const uint32_t* __restrict__ sel_count_p, int64_t nrows, const GroupWindowsOut& out) {
  extern __shared__ __attribute__((aligned(16))) uint64_t s_keys[];   // [kWinSlots][n_keys]{lo, hi}
  __shared__ uint32_t s_tag[kWinSlots];          // 0: free, else 0x100 | the key's NULL bits
  __shared__ uint32_t s_sort[kTileRows];         // slot << 11 | row in window; kNoRow behind the selected rows
  __shared__ uint16_t s_dense[kWinSlots];        // slot -> rank among the slots in use
  __shared__ uint16_t s_start[groupkey::kWindowLimit + 1];   // rank -> where the group's rows begin in s_sort
  __shared__ uint32_t s_wave[kBlockThreads / 64];
  __shared__ uint32_t s_distinct, s_flags;

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
  const int n_keys = prog.n_keys, n_aggs = prog.aggs.n_aggs;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  for (int i = tid; i < kWinSlots; i += kBlockThreads) s_tag[i] = 0;
  for (int i = tid; i < kTileRows; i += kBlockThreads) s_sort[i] = kNoRow;
  if (tid == 0) {
    s_distinct = 0;
    s_flags = 0;
  }
  __syncthreads();

  // ---- 1. keys
  uint32_t flags = 0;
  bool over = false;
  for (uint32_t base = 0; base < cnt && !over; base += kBlockThreads) {   // (uniform: cnt and `over` are)
    const uint32_t i = base + tid;
    bool pending = i < cnt;
    uint32_t r = i;
    if (HAS_SEL && pending) {
      r = sel[i];
      if (r >= n) {   // not a row of this window: never dereferenced
        flags |= MI_ST_SEL_RANGE;
        pending = false;
      }
    }
    Key key;
    key.nulls = 0;
#pragma unroll
    for (int q = 0; q < groupkey::kMaxKeys; q++) key.lo[q] = key.hi[q] = 0;
    if (pending) {
      const int64_t row = row0 + r;
      uint32_t bad = 0;
      // (one column's descriptor at a time; the part goes to its place by a select, so the key stays in registers)
#pragma clang loop unroll(disable)
      for (int k = 0; k < n_keys; k++) {
        uint64_t lo, hi;
        const uint32_t st = load_key_part(prog.keys[k], row, &lo, &hi);
        if (st == kPartNull) key.nulls |= 1u << k;
        else bad |= st;
#pragma unroll
        for (int q = 0; q < groupkey::kMaxKeys; q++)
          if (q == k) {
            key.lo[q] = lo;
            key.hi[q] = hi;
          }
      }
      if (bad) {   // stays above the scan: the row joins no group, the call fails
        flags |= bad;
        pending = false;
      }
    }
    const uint32_t tag = 0x100u | key.nulls;
    uint32_t h = groupkey::Hash(key, n_keys) & (kWinSlots - 1);
    for (int probe = 0; probe < kWinSlots; probe++) {   // (uniform: every lane leaves at the same barrier)
      if (pending && atomicCAS(&s_tag[h], 0u, tag) == 0u) {
#pragma unroll
        for (int k = 0; k < groupkey::kMaxKeys; k++)
          if (k < n_keys) {
            s_keys[(h * n_keys + k) * 2] = key.lo[k];
            s_keys[(h * n_keys + k) * 2 + 1] = key.hi[k];
          }
        atomicAdd(&s_distinct, 1u);
      }
      __syncthreads();
      if (pending) {
        bool eq = s_tag[h] == tag;
#pragma unroll
        for (int k = 0; k < groupkey::kMaxKeys; k++)
          if (k < n_keys) eq = eq && s_keys[(h * n_keys + k) * 2] == key.lo[k] && s_keys[(h * n_keys + k) * 2 + 1] == key.hi[k];
        if (eq) {
          s_sort[i] = (h << 11) | r;
          pending = false;
        } else {
          h = (h + 1) & (kWinSlots - 1);
        }
      }
      over = s_distinct > static_cast<uint32_t>(groupkey::kWindowLimit);
      if (!__syncthreads_or(pending) || over) break;
    }
  }
  if (flags) atomicOr(&s_flags, flags);
  __syncthreads();
  if (over) {   // the window's work ends here: nothing of it is merged, the call fails
    if (tid == 0) {
      GM<uint32_t>(out.heads)[2 * window] = 0;
      GM<uint32_t>(out.heads)[2 * window + 1] = s_flags | MI_ST_GROUP_LIMIT;
    }
    return;
  }

  // ---- the slots in use, ranked in slot order (two slots per lane, kWinSlots == 2 * kBlockThreads)
  const uint32_t f0 = s_tag[2 * tid] != 0, f1 = s_tag[2 * tid + 1] != 0;
  const uint32_t inc = wave_inclusive_scan_u32(f0 + f1);
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  uint32_t before = inc - (f0 + f1), n_local = 0;
#pragma unroll
  for (int v = 0; v < kBlockThreads / 64; v++) {
    if (v < wave) before += s_wave[v];
    n_local += s_wave[v];
  }
  s_dense[2 * tid] = static_cast<uint16_t>(before);
  s_dense[2 * tid + 1] = static_cast<uint16_t>(before + f0);
  const size_t rec0 = static_cast<size_t>(window) * groupkey::kWindowLimit;
  for (int which = 0; which < 2; which++) {
    const uint32_t slot = 2 * tid + which, g = before + (which ? f0 : 0);
    if (!(which ? f1 : f0)) continue;   // (g < n_local <= kWindowLimit: `over` is false)
    GM<uint32_t>(out.nulls)[rec0 + g] = s_tag[slot] & 0xFFu;
    gptr<u64x2_a8> kout = (gptr<u64x2_a8>)GM<uint64_t>(out.keys) + (rec0 + g) * n_keys;
    for (int k = 0; k < n_keys; k++) {
      const u64x2 v = {s_keys[(slot * n_keys + k) * 2], s_keys[(slot * n_keys + k) * 2 + 1]};
      kout[k] = v;
    }
  }
  if (tid == 0) {
    GM<uint32_t>(out.heads)[2 * window] = n_local;
    GM<uint32_t>(out.heads)[2 * window + 1] = s_flags;
  }
  if (n_local == 0) return;   // (uniform)

  // ---- 2. order: bitonic sort of the first `span` words, span the power of two that holds the selected rows
  uint32_t span = 2;
  while (span < cnt) span <<= 1;
  __syncthreads();
  for (uint32_t k = 2; k <= span; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = tid; t < span / 2; t += kBlockThreads) {
        const uint32_t a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
        const uint32_t x = s_sort[a], y = s_sort[b];
        const bool up = (a & k) == 0;
        if ((x > y) == up) {
          s_sort[a] = y;
          s_sort[b] = x;
        }
      }
      __syncthreads();
    }
  }
  // where every group's rows begin; the words behind the last row are kNoRow
  for (uint32_t j = tid; j < span; j += kBlockThreads) {
    const uint32_t e = s_sort[j];
    if (e == kNoRow) continue;
    const uint32_t slot = e >> 11;
    if (j == 0 || (s_sort[j - 1] >> 11) != slot) s_start[s_dense[slot]] = static_cast<uint16_t>(j);
    if (j + 1 == span || s_sort[j + 1] == kNoRow) s_start[n_local] = static_cast<uint16_t>(j + 1);
  }
  __syncthreads();

  // ---- 3. fold
  gptr<Partial> partials = GM<Partial>(out.partials) + rec0 * n_aggs;
#pragma clang loop unroll(disable)
  for (int a = 0; a < n_aggs; a++) {
    const AggDescDev& d = prog.aggs.aggs[a];
    const int op = d.op, cls = d.a.cls;
#pragma clang loop unroll(disable)
    for (uint32_t g = wave; g < n_local; g += kBlockThreads / 64) {
      const uint32_t begin = s_start[g], end = s_start[g + 1];
      Partial p = {0ull, 0ull, 0ull, 0ull};
      if (EXPR && op == aggmerge::kOpSumExpr) {   // validity, values and the sum: kernels_agg_fold.inl
        const AggExprDev& e = exprs->exprs[a];
        for (uint32_t j = begin + lane; j < end; j += 64) fold_expr_row(e, cls, row0 + (s_sort[j] & (kTileRows - 1)), &p);
      } else {
        for (uint32_t j = begin + lane; j < end; j += 64) fold_row(d, op, cls, row0 + (s_sort[j] & (kTileRows - 1)), &p);
      }
#pragma unroll
      for (int dist = 32; dist >= 1; dist >>= 1) {   // as agg_windows: lane l takes lane l + dist while that lane exists
        const Partial o = shfl_down_partial(p, dist);
        if (lane + dist < 64) aggmerge::Merge<EXPR>(op, cls, &p, o);
      }
      if (lane == 0) store_partial(partials + (static_cast<size_t>(g) * n_aggs + a), p);
    }
  }
}

template <bool HAS_SEL>
__global__ __launch_bounds__(kBlockThreads) void group_windows(const GroupProgram prog, const mi_sel_t* __restrict__ sel_p,
                                                               const uint32_t* __restrict__ sel_count_p, int64_t nrows,
                                                               const GroupWindowsOut out) {
  group_windows_body<HAS_SEL, false>(prog, nullptr, sel_p, sel_count_p, nrows, out);
}

// launched only for a program that holds a kOpSumExpr: the expression table rides behind the arguments of group_windows
template <bool HAS_SEL>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void group_windows_expr(const GroupProgram prog, const mi_sel_t* __restrict__ sel_p,
                                                                    const uint32_t* __restrict__ sel_count_p, int64_t nrows,
                                                                    const GroupWindowsOut out, const AggExprTable exprs) {
  group_windows_body<HAS_SEL, true>(prog, &exprs, sel_p, sel_count_p, nrows, out);
}

__device__ __forceinline__ uint32_t slot_load(uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void slot_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ops / classes: 4 bits per aggregate, as agg_combine takes them
__global__ __launch_bounds__(kBlockThreads) void group_combine(int32_t n_keys, int32_t n_aggs, uint32_t ops, uint32_t classes,
                                                               const GroupWindowsOut in, int64_t n_windows, const GroupTableDev table) {
  __shared__ uint32_t s_gidx[groupkey::kWindowLimit];
  __shared__ uint32_t s_count, s_over;
  const int tid = threadIdx.x;
  gptr<uint32_t> head = GM<uint32_t>(table.head);
  uint32_t flags = head[1];
  if (flags & MI_ST_GROUP_LIMIT) return;   // (uniform) the table is full and the call has failed: nothing more is merged
  if (tid == 0) {
    s_count = head[0];
    s_over = 0;
  }
  __syncthreads();
  gptr<const uint32_t> wheads = GC<uint32_t>(in.heads);
  gptr<u64x2_a8> tkeys = (gptr<u64x2_a8>)GM<uint64_t>(table.keys);
  gptr<uint32_t> tnulls = GM<uint32_t>(table.nulls);
  gptr<Partial> acc = GM<Partial>(table.acc);
  for (int64_t w = 0; w < n_windows; w++) {
    const uint32_t n_local_raw = wheads[2 * w];
    flags |= wheads[2 * w + 1];
    const uint32_t n_local = n_local_raw < static_cast<uint32_t>(groupkey::kWindowLimit) ? n_local_raw : static_cast<uint32_t>(groupkey::kWindowLimit);
    if (n_local == 0) continue;   // (uniform)
    const size_t rec0 = static_cast<size_t>(w) * groupkey::kWindowLimit;
    // ---- find or insert the window's keys
    bool pending = static_cast<uint32_t>(tid) < n_local;
    Key key;
    key.nulls = 0;
#pragma unroll
    for (int k = 0; k < groupkey::kMaxKeys; k++) key.lo[k] = key.hi[k] = 0;
    if (pending) {
      key.nulls = GC<uint32_t>(in.nulls)[rec0 + tid];
      gptr<const u64x2_a8> kin = (gptr<const u64x2_a8>)GC<uint64_t>(in.keys) + (rec0 + tid) * n_keys;
#pragma unroll
      for (int k = 0; k < groupkey::kMaxKeys; k++)
        if (k < n_keys) {
          const u64x2 v = kin[k];
          key.lo[k] = v.x;
          key.hi[k] = v.y;
        }
    }
    uint32_t h = groupkey::Hash(key, n_keys) & (kTableSlots - 1);
    bool over = false;
    for (uint32_t probe = 0; probe < kTableSlots; probe++) {   // (uniform: every lane leaves at the same barrier)
      if (pending && atomicCAS(table.slots + h, kSlotEmpty, kSlotBusy) == kSlotEmpty) {
        const uint32_t g = atomicAdd(&s_count, 1u);
        if (g < static_cast<uint32_t>(groupkey::kMaxGroups)) {
          tnulls[g] = key.nulls;
#pragma unroll
          for (int k = 0; k < groupkey::kMaxKeys; k++)
            if (k < n_keys) {
              const u64x2 v = {key.lo[k], key.hi[k]};
              tkeys[static_cast<size_t>(g) * n_keys + k] = v;
            }
          slot_store(table.slots + h, g);
        } else {
          s_over = 1;
        }
      }
      __syncthreads();
      over = s_over != 0;
      if (pending && !over) {
        const uint32_t g = slot_load(table.slots + h);
        bool eq = g < static_cast<uint32_t>(groupkey::kMaxGroups);   // (a record index, never past the table)
        if (eq) {
          eq = tnulls[g] == key.nulls;
#pragma unroll
          for (int k = 0; k < groupkey::kMaxKeys; k++)
            if (k < n_keys) {
              const u64x2 v = tkeys[static_cast<size_t>(g) * n_keys + k];
              eq = eq && v.x == key.lo[k] && v.y == key.hi[k];
            }
        }
        if (eq) {
          s_gidx[tid] = g;
          pending = false;
        } else {
          h = (h + 1) & (kTableSlots - 1);
        }
      }
      if (!__syncthreads_or(pending && !over)) break;
    }
    if (over) {   // (uniform) more than kMaxGroups keys: this window and what follows stay unmerged, the call fails
      flags |= MI_ST_GROUP_LIMIT;
      break;
    }
    // ---- merge: one lane per (local group, aggregate); the groups of one window differ, so no two lanes share a record
    gptr<const Partial> wparts = GC<Partial>(in.partials) + rec0 * n_aggs;
    for (uint32_t p = tid; p < n_local * static_cast<uint32_t>(n_aggs); p += kBlockThreads) {
      const uint32_t t = p / static_cast<uint32_t>(n_aggs), a = p - t * static_cast<uint32_t>(n_aggs);
      const int op = static_cast<int>((ops >> (4 * a)) & 15u), cls = static_cast<int>((classes >> (4 * a)) & 15u);
      gptr<Partial> rec = acc + (static_cast<size_t>(s_gidx[t]) * n_aggs + a);
      Partial into = load_partial(rec);
      aggmerge::Merge<false>(op, cls, &into, load_partial(wparts + p));
      store_partial(rec, into);
    }
    __syncthreads();   // the next window may meet the same groups, and writes s_gidx again
  }
  if (tid == 0) {
    const uint32_t c = s_count;
    head[0] = c < static_cast<uint32_t>(groupkey::kMaxGroups) ? c : static_cast<uint32_t>(groupkey::kMaxGroups);
    head[1] = flags;
  }
}

bool KeyColumnOk(const GroupKeyColumnDev& c) {
  if (!c.data) return false;
  switch (c.cls) {
    case groupkey::kKeySigned: case groupkey::kKeyUnsigned: return c.width == 1 || c.width == 2 || c.width == 4 || c.width == 8;
    case groupkey::kKeyWide: case groupkey::kKeyString: return c.width == 16;
    default: return false;
  }
}

size_t Align16(size_t v) { return (v + 15) & ~static_cast<size_t>(15); }

std::atomic<int64_t> g_group_launches[2];   // group_windows, group_combine

}  // namespace

void GroupLaunchCounts(int64_t out[2]) {
  out[0] = g_group_launches[0].load();
  out[1] = g_group_launches[1].load();
}

bool GroupProgramIsValid(const GroupProgram& prog, const AggExprTable* exprs) {
  if (prog.n_keys < 1 || prog.n_keys > groupkey::kMaxKeys) return false;
  for (int k = 0; k < prog.n_keys; k++)
    if (!KeyColumnOk(prog.keys[k])) return false;
  return AggProgramIsValid(prog.aggs, exprs);
}

size_t GroupWindowsBytes(int64_t n_windows, int n_keys, int n_aggs) {
  const size_t recs = static_cast<size_t>(n_windows) * groupkey::kWindowLimit;
  return Align16(static_cast<size_t>(n_windows) * 8) + Align16(recs * 4) + recs * static_cast<size_t>(n_keys) * 16 + recs * static_cast<size_t>(n_aggs) * sizeof(aggmerge::Partial);
}

GroupWindowsOut GroupWindowsAt(void* base, int64_t n_windows, int n_keys, int n_aggs) {
  const size_t recs = static_cast<size_t>(n_windows) * groupkey::kWindowLimit;
  uint8_t* p = static_cast<uint8_t*>(base);
  GroupWindowsOut o;
  o.heads = reinterpret_cast<uint32_t*>(p);
  p += Align16(static_cast<size_t>(n_windows) * 8);
  o.nulls = reinterpret_cast<uint32_t*>(p);
  p += Align16(recs * 4);
  o.keys = reinterpret_cast<uint64_t*>(p);
  p += recs * static_cast<size_t>(n_keys) * 16;
  o.partials = reinterpret_cast<aggmerge::Partial*>(p);
  return o;
}

size_t GroupTableBytes(int n_keys, int n_aggs) {
  const size_t g = groupkey::kMaxGroups;
  return 16 + kGroupTableSlots * 4 + g * 4 + g * static_cast<size_t>(n_keys) * 16 + g * static_cast<size_t>(n_aggs) * sizeof(aggmerge::Partial);
}

GroupTableDev GroupTableAt(void* base, int n_keys, int n_aggs) {
  const size_t g = groupkey::kMaxGroups;
  uint8_t* p = static_cast<uint8_t*>(base);
  GroupTableDev t;
  t.head = reinterpret_cast<uint32_t*>(p);
  p += 16;
  t.slots = reinterpret_cast<uint32_t*>(p);
  p += kGroupTableSlots * 4;
  t.nulls = reinterpret_cast<uint32_t*>(p);
  p += g * 4;
  t.keys = reinterpret_cast<uint64_t*>(p);
  p += g * static_cast<size_t>(n_keys) * 16;
  t.acc = reinterpret_cast<aggmerge::Partial*>(p);
  return t;
}

hipError_t GroupTableClear(void* base, int n_keys, int n_aggs, hipStream_t stream) {
  // count 0 is the identity of every merge; every slot free
  hipError_t e = hipMemsetAsync(base, 0, GroupTableBytes(n_keys, n_aggs), stream);
  if (e != hipSuccess) return e;
  return hipMemsetAsync(static_cast<uint8_t*>(base) + 16, 0xFF, kGroupTableSlots * 4, stream);
}

hipError_t LaunchGroupWindows(const GroupProgram& prog, const mi_sel_t* sel, const uint32_t* sel_count, int64_t nrows,
                              const GroupWindowsOut& out, hipStream_t stream, const AggExprTable* exprs) {
  MI_DROP_STALE_ERROR();
  if (nrows <= 0) return hipSuccess;
  if (!GroupProgramIsValid(prog, exprs) || (sel == nullptr) != (sel_count == nullptr) || !out.heads || !out.keys || !out.nulls || !out.partials)
    return hipErrorInvalidValue;
  const int64_t windows = (nrows + kTileRows - 1) / kTileRows;
  if (windows > 0x7FFFFFFFll) return hipErrorInvalidValue;
  const dim3 grid(static_cast<uint32_t>(windows)), block(kBlockThreads);
  const size_t lds = static_cast<size_t>(kWinSlots) * static_cast<size_t>(prog.n_keys) * 16;
  if (AggProgramHasExpr(prog.aggs)) {
    if (sel) hipLaunchKernelGGL(group_windows_expr<true>, grid, block, lds, stream, prog, sel, sel_count, nrows, out, *exprs);
    else hipLaunchKernelGGL(group_windows_expr<false>, grid, block, lds, stream, prog, sel, sel_count, nrows, out, *exprs);
  } else if (sel) hipLaunchKernelGGL(group_windows<true>, grid, block, lds, stream, prog, sel, sel_count, nrows, out);
  else hipLaunchKernelGGL(group_windows<false>, grid, block, lds, stream, prog, sel, sel_count, nrows, out);
  g_group_launches[0]++;
  return hipGetLastError();
}

hipError_t LaunchGroupCombine(const GroupProgram& prog, const GroupWindowsOut& in, int64_t n_windows, const GroupTableDev& table,
                              hipStream_t stream, const AggExprTable* exprs) {
  MI_DROP_STALE_ERROR();
  if (n_windows <= 0) return hipSuccess;
  if (!GroupProgramIsValid(prog, exprs) || !in.heads || !table.head) return hipErrorInvalidValue;
  uint32_t ops, classes;
  PackOpsClasses(prog.aggs, &ops, &classes);
  hipLaunchKernelGGL(group_combine, dim3(1), dim3(kBlockThreads), 0, stream, prog.n_keys, prog.aggs.n_aggs, ops, classes, in, n_windows, table);
  g_group_launches[1]++;
  return hipGetLastError();
}

}  // namespace device
}  // namespace miarrow
