// kernels.hpp -- launch interface of the gfx950 transcode kernels (kernels.hip).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "../../include/mi_arrow_ipc.h"
#include "agg_merge.hpp"
#include "lz4_encode_format.hpp"
#include "task_kind.hpp"

namespace miarrow {
namespace device {

constexpr int kBlockThreads = 256;   // 4 waves of 64
constexpr int kTileRows = 2048;      // rows per tile == DuckDB STANDARD_VECTOR_SIZE: one tile is one output vector
static_assert(kTileRows == kVectorRows, "the plan layout (task_kind.hpp) counts tiles of kVectorRows rows");

// One launch over a device-resident task table slice.  `tile_begin[i]` = first tile of task i within the slice,
// tile_begin[n_tasks] = total_tiles.  `status` accumulates MI_ST_* bits.
// `tile_task[tile]` = task index (within the slice) of every tile of the slice.  One workgroup per tile.
// `kernel_mask`: which kernels of the class have tiles (KernelMaskOfTask, task_kind.hpp).
hipError_t LaunchTranscode(int cls, const mi_col_task* d_tasks, const uint32_t* d_tile_begin, const uint32_t* d_tile_task,
                           int32_t n_tasks, uint32_t total_tiles, uint32_t* d_status, uint32_t kernel_mask, hipStream_t stream);

// Run-end encoded columns (kernels_run_end.hip): MI_K_RUN_END tasks only, one workgroup per 2048-row tile.  Launched after
// every other slice of the plan: the values child must be decoded first.
hipError_t LaunchRunEnd(const mi_col_task* d_tasks, const uint32_t* d_tile_begin, const uint32_t* d_tile_task, int32_t n_tasks,
                        uint32_t total_tiles, uint32_t* d_status, hipStream_t stream);

// Union columns (kernels_union.hip), one workgroup per 2048-row tile.  dense = false: MI_K_UNION tasks (transcode_union, the
// tag pass: tags, the union's validity, one mask per member), launched before anything deeper than they are.  dense = true:
// MI_K_UNION_DENSE tasks (transcode_union_dense), launched with the run-end slices: their members' scratch vectors first.
hipError_t LaunchUnion(bool dense, const mi_col_task* d_tasks, const uint32_t* d_tile_begin, const uint32_t* d_tile_task, int32_t n_tasks,
                       uint32_t total_tiles, uint32_t* d_status, hipStream_t stream);

//! Fused consumer: sum(a * b) over the rows that pass up to 4 conjunctive range filters, straight
//! from the decoded vectors in HBM.  acc = {sum low 64 bits, sum high 64 bits (two's complement), rows selected}.
struct AggSumProductArgs {
  const void* fcol[4];
  const uint64_t* fvalid[4];
  int32_t fwidth[4];
  int64_t lo[4], hi[4];
  int32_t n_filters;
  const void* a;
  const void* b;
  const uint64_t* avalid;
  const uint64_t* bvalid;
  int32_t awidth, bwidth;
  int64_t nrows;
};
hipError_t LaunchAggSumProduct(const AggSumProductArgs& args, unsigned long long* d_acc, int num_cus, hipStream_t stream);

// K8: LZ4_FRAME buffers of one record batch, decompressed in HBM (kernels_lz4.hip).  Positions are 31-bit: a compressed or
// decompressed body of 2 GiB or more takes the host decompressor.
struct Lz4BlockDev {
  uint32_t comp_off, comp_size;   // the block's bytes inside the compressed body
  uint32_t buffer;                // index into Lz4Args::buffers
  uint32_t stored;                // 1 = the block holds its bytes uncompressed
  uint32_t seq_base, seq_cap;     // its slice of the sequence-descriptor scratch, 256 equal parts: LZ4 256 x (ceil(comp_size / 256) / 3 + 2), ZSTD count + 1 rounded up
};
struct Lz4BufferDev {
  uint64_t out_off, out_len;      // where the buffer lies in the decompressed body, and its declared length
  uint32_t first_block, n_blocks;
  uint32_t block_max;             // the frame's maximum block size (BD byte)
  uint32_t independent;           // LZ4 FLG bit 0x20: matches stay inside their block (linked blocks: inside the buffer)
};
struct Lz4Args {
  const uint8_t* comp;            // compressed body (device)
  uint8_t* out;                   // decompressed body (device), out_size bytes
  uint64_t out_size;
  uint64_t max_buffer_len;        // longest decompressed LZ4 buffer: bounds the number of resolve rounds
  const Lz4BlockDev* blocks;
  const Lz4BufferDev* buffers;
  uint32_t n_blocks, n_buffers;
  uint32_t max_block_comp, _pad;  // largest compressed block; _pad: set by the launcher (which parse kernel owns which blocks)
  uint32_t min_block_comp;        // smallest compressed (not stored) block
  uint32_t max_buffer_blocks;     // most blocks any one buffer has
  void* seq;                      // 16 bytes per sequence, in the slices of lz4_parse's 256 lanes per block
  uint32_t* seq_off;              // 4 bytes per sequence
  uint32_t* lane_out;             // per block and lane: output position (inside the block) its slice begins at ...
  uint32_t* lane_nseq;            // ... and its number of sequences
  uint32_t* link;                 // 4 bytes per decompressed byte (rounded up to 16 bytes); no preset needed
  uint32_t* block_out_size;       // per block
  uint32_t* block_nseq;
  uint64_t* block_out_base;
  uint32_t* chunk_base;           // per block (+ 1): first chunk (<= 8 KiB of one block's output) of the block, k8_chunk_map
  uint32_t* buffer_ok;            // per buffer
  uint8_t* mark;                  // one byte per decompressed byte (rounded up to 16), zeroed: 1 = an open word of another tile points here
  uint32_t* skel;                 // the skeleton list: up to one entry per decompressed byte
  uint32_t* round_left;           // 40 words, zeroed
  uint32_t* status;               // MI_ST_DECOMPRESS
  // ZSTD batches (NULL for LZ4): one zstd::BlockInfo per block (zstd_format.hpp); the decoded literals of a block go to
  // literals[BlockInfo::lit_pos ..] -- the same allocation as `comp`, behind the compressed body, so that a sequence's literal
  // source is one position whichever section it came from
  const void* zblocks;
  uint8_t* literals;
  uint32_t* rep_state;            // ZSTD: 4 words per block and slice -- the slice's effect on the repeat offsets, then (zstd_layout) the offsets it starts from
};
inline uint32_t Lz4SeqCapacity(uint32_t comp_size) { return 256u * (((comp_size + 255u) / 256u) / 3u + 2u); }
hipError_t LaunchLz4Decompress(const Lz4Args& args, int num_cus, hipStream_t stream);

// Late materialisation: tasks with mi_col_task.sel decode only the selected rows, compacted per window (kernels_gather.hip)
// d_window_base: total_tiles words of scratch (first output row of every window, filled by the launch)
hipError_t LaunchGather(const mi_col_task* d_tasks, const uint32_t* d_tile_begin, const uint32_t* d_tile_task, int32_t n_tasks,
                        uint32_t total_tiles, int64_t* d_window_base, uint32_t* d_status, hipStream_t stream);

// K6: pushed-down predicate -> one ascending selection vector per 2048-row window (kernels_filter.hip).  The predicate is
// in conjunctive normal form: leaves in clause order, kLeafEndsClause on the last leaf of every clause (a clause is the
// OR of its leaves, the filter the AND of its clauses).
constexpr int kLeafRange = 1;       // lo <= v <= hi on the stored integer (negated with kLeafNegate)
constexpr int kLeafIsNull = 2;
constexpr int kLeafIsNotNull = 3;
constexpr int kLeafIn = 4;          // v is one of in_values[0 .. n_in)
constexpr int kLeafStrIn = 5;       // string_t column: the row equals one of n_in byte strings.  in_values holds 3 words per
                                    // constant: {len | dword1 << 32, dword2 | dword3 << 32, device address of the bytes} where
                                    // dword1..3 are the string_t image (inline bytes, or prefix + 0 + 0 for > 12 bytes)
constexpr int kLeafDictMap = 6;     // dictionary-encoded string column: data = the uint32 selection vector, in_values = one byte per
                                    // dictionary entry (n_in of them; 0 no, 1 yes, 2 NULL entry), lo = 0 match, 1 no match, 2 IS NULL, 3 IS NOT NULL
constexpr int kLeafStrRange = 7;    // string_t column: lower bound <(=) row <(=) upper bound, byte-wise.  in_values: two constants in kLeafStrIn's
                                    // layout (lower, upper); n_in = bit 0 has lower, bit 1 lower inclusive, bit 2 has upper, bit 3 upper inclusive
constexpr int kLeafWideRange = 8;   // 16-byte column (hugeint_t{uint64 lower; int64 upper}: HUGEINT, DECIMAL(19..38)): lo <= v <= hi, `upper`
                                    // signed, then `lower` unsigned.  in_values = {lo.lower, lo.upper, hi.lower, hi.upper}
constexpr int kLeafWideIn = 9;      // 16-byte column: v is one of n_in constants, in_values = {lower, upper} pairs
constexpr int kLeafStrMatch = 10;   // string_t column: contains / ends_with / %-pattern LIKE (like_match.hpp).  in_values: the literal segments in
                                    // kLeafStrIn's layout, in pattern order; n_in = their number (1 .. 8) | anchored at the head << 8 | at the tail << 9
constexpr int kLeafUnsigned = 1;    // flags: the column holds unsigned integers
constexpr int kLeafNegate = 2;      //        NOT (range / in-list); NULL still fails
constexpr int kLeafEndsClause = 4;
constexpr int kLeafBias = 8;        //        uint64 column: values and constants are compared after x ^ 2^63
constexpr int kLeafFloat = 16;      //        FLOAT / DOUBLE column (width 4 / 8): every value goes through filterkey::FloatKey
                                    //        (filter_key.hpp) before the range / IN comparison, whose constants are keys
constexpr int kMaxFilterLeaves = 24;
// The contract of a leaf, held by the program-level suite (mi_filter_program_vectors, tests/test_gpu_filter_programs.py):
//   * data and validity are 8-byte aligned (what the planner hands over for an aliased Arrow buffer), whatever the width;
//   * a NULL row of a string_t vector is sixteen zero bytes: the string leaves may look at any row, valid or not;
//   * kLeafDictMap ignores `validity` (the map knows its NULLs) and takes no kLeafNegate (lo = 1 is its negation);
//   * a program of no leaves keeps every row;
//   * the last leaf of a program carries kLeafEndsClause: a clause left open is dropped.
struct FilterLeafDev {
  const void* data;                 // decoded fixed-width vector (device), NULL for IS [NOT] NULL
  const uint64_t* validity;         // validity words (device) or NULL = all valid
  const int64_t* in_values;         // kLeafIn (device)
  int64_t lo, hi;
  int32_t op, width, flags, n_in;
};
struct FilterProgram {
  int32_t n_leaves;
  int32_t _pad;
  FilterLeafDev leaves[kMaxFilterLeaves];
};
// Two instances of one kernel: programs of the leaves kLeafRange .. kLeafStrRange without kLeafFloat launch filter_program<false>,
// which compiles none of the code of the others; a program that holds a kLeafFloat / kLeafWideRange / kLeafWideIn leaf
// launches filter_program<true>.  A third one, filter_program<true, true>, knows every leaf form and kLeafStrMatch besides; it is
// launched only for a program that holds such a leaf.
hipError_t LaunchFilterProgram(const FilterProgram& prog, int64_t nrows, mi_sel_t* sel_out, uint32_t* count_out, hipStream_t stream);
//! launches of each instance by this process so far: [0] filter_program<false>, [1] filter_program<true>
void FilterLaunchCounts(int64_t out[2]);
//! launches of filter_program<true, true> by this process so far
int64_t FilterPatternLaunches();
// lo <= v < hi on one column (mi_filter_range)
hipError_t LaunchFilterRange(const void* values, int32_t width, const void* validity, int64_t nrows, int64_t lo,
                             int64_t hi, mi_sel_t* sel_out, uint32_t* count_out, hipStream_t stream);

// K9: aggregates over decoded vectors under the filter's selection vectors (kernels_aggregate.hip; the rules of a merge are
// agg_merge.hpp).  The program -- at most aggmerge::kMaxAggregates descriptors -- is a kernel argument, as FilterProgram is.
struct AggColumnDev {
  const void* data;                 // decoded vector (device); may be NULL for COUNT, which reads the validity alone
  const uint64_t* validity;         // validity words (device) or NULL = all valid
  int32_t width;                    // bytes per row
  int32_t cls;                      // aggmerge::kClass*
};
struct AggDescDev {
  AggColumnDev a, b;                // b: the second factor of kOpSumProduct
  int32_t op;                       // aggmerge::kOp*
  int32_t _pad;
};
struct AggProgram {
  int32_t n_aggs;
  int32_t _pad;
  AggDescDev aggs[aggmerge::kMaxAggregates];
};
// The expressions of a program's kOpSumExpr aggregates: a table of its own, a kernel argument of the EXPR instantiations of
// agg_windows / group_windows alone, so a program without an expression launches the kernels it always launched with the
// arguments it always had.  exprs[a] belongs to aggs[a]; for such an aggregate aggs[a].a is the first column factor's
// column (its class is the expression's: what the combine kernels and the host merge by).
struct AggFactorDev {
  AggColumnDev col;                 // cls == aggmerge::kClassAny: a constant factor (`add` alone, nothing is read)
  uint64_t mul, add;                // integer expression: int64 two's complement; float expression: the bits of a double
};
struct AggExprDev {
  int32_t n_factors;                // 1 .. aggmerge::kMaxExprFactors
  int32_t _pad;
  AggFactorDev factors[aggmerge::kMaxExprFactors];
};
struct AggExprTable {
  AggExprDev exprs[aggmerge::kMaxAggregates];
};
//! what the launchers accept: 1 .. 8 aggregates, widths that fit their class, no SUM over 16-byte values, products of two
//! integers or two floats; a kOpSumExpr needs `exprs`: 1 .. 4 factors, at least one column, every column factor with data,
//! width 1 / 2 / 4 / 8 (integers) or 4 / 8 (floats), all integer-like or all floating point, none of 16 bytes
bool AggProgramIsValid(const AggProgram& prog, const AggExprTable* exprs = nullptr);
//! what agg_combine and group_combine take of a valid program: 4 bits per aggregate, the operation its partials merge by (a
//! kOpSumExpr's merge as sums) and the class
void PackOpsClasses(const AggProgram& prog, uint32_t* ops, uint32_t* classes);
//! agg_windows: one partial per window and aggregate to d_partials[window * n_aggs + aggregate].  sel / sel_count in the
//! filter's layout (2048 slots per window, the first sel_count[w] read), or both NULL = every row.  `exprs` is read only
//! when the program holds a kOpSumExpr, and only then the expression instantiation is launched.
hipError_t LaunchAggWindows(const AggProgram& prog, const mi_sel_t* sel, const uint32_t* sel_count, int64_t nrows,
                            aggmerge::Partial* d_partials, hipStream_t stream, const AggExprTable* exprs = nullptr);
//! agg_combine: folds the partials of n_windows windows, in ascending order, into d_acc[0 .. n_aggs)
hipError_t LaunchAggCombine(const AggProgram& prog, const aggmerge::Partial* d_partials, int64_t n_windows, aggmerge::Partial* d_acc,
                            hipStream_t stream, const AggExprTable* exprs = nullptr);
//! whether the program holds a kOpSumExpr (and its launches therefore need the table)
bool AggProgramHasExpr(const AggProgram& prog);

//! launches by this process so far: [0] agg_windows, [1] agg_combine
void AggLaunchCounts(int64_t out[2]);

// K10: GROUP BY over decoded vectors (kernels_group.hip; the rules of a key are group_key.hpp).  Few groups: at most
// groupkey::kWindowLimit distinct keys among the selected rows of one window, groupkey::kMaxGroups in a scan.
struct GroupKeyColumnDev {
  const void* data;                 // decoded vector (device)
  const uint64_t* validity;         // validity words (device) or NULL = all valid
  int32_t width;                    // bytes per row
  int32_t cls;                      // groupkey::kKey*
};
struct GroupProgram {
  int32_t n_keys;
  int32_t _pad;
  GroupKeyColumnDev keys[4];        // groupkey::kMaxKeys
  AggProgram aggs;
};
//! what group_windows writes per window and group_combine reads: heads[2 w] = the window's local groups, heads[2 w + 1] =
//! MI_ST_* bits it raised; record (w * kWindowLimit + g) of nulls / keys (n_keys x {lo, hi}) / partials (n_aggs) is local group g
struct GroupWindowsOut {
  uint32_t* heads;
  uint32_t* nulls;
  uint64_t* keys;
  aggmerge::Partial* partials;
};
size_t GroupWindowsBytes(int64_t n_windows, int n_keys, int n_aggs);
GroupWindowsOut GroupWindowsAt(void* base, int64_t n_windows, int n_keys, int n_aggs);
//! the scan-wide table, in HBM for the whole call: head = {groups, MI_ST_* bits}, kGroupTableSlots slots that name a record,
//! kMaxGroups records of nulls / keys / accumulators
constexpr uint32_t kGroupTableSlots = 8192;
struct GroupTableDev {
  uint32_t* head;
  uint32_t* slots;
  uint32_t* nulls;
  uint64_t* keys;
  aggmerge::Partial* acc;
};
size_t GroupTableBytes(int n_keys, int n_aggs);
GroupTableDev GroupTableAt(void* base, int n_keys, int n_aggs);
//! an empty table (asynchronous)
hipError_t GroupTableClear(void* base, int n_keys, int n_aggs, hipStream_t stream);
//! 1 .. 4 key columns of a class and width that fit, and a valid aggregate program (`exprs` as AggProgramIsValid takes it)
bool GroupProgramIsValid(const GroupProgram& prog, const AggExprTable* exprs = nullptr);
//! group_windows: the local groups of every window of `nrows` rows; sel / sel_count / exprs as LaunchAggWindows takes them
hipError_t LaunchGroupWindows(const GroupProgram& prog, const mi_sel_t* sel, const uint32_t* sel_count, int64_t nrows,
                              const GroupWindowsOut& out, hipStream_t stream, const AggExprTable* exprs = nullptr);
//! group_combine: merges the windows, in ascending order, into the table
hipError_t LaunchGroupCombine(const GroupProgram& prog, const GroupWindowsOut& in, int64_t n_windows, const GroupTableDev& table,
                              hipStream_t stream, const AggExprTable* exprs = nullptr);
//! launches by this process so far: [0] group_windows, [1] group_combine
void GroupLaunchCounts(int64_t out[2]);

// K11: hash GROUP BY over decoded vectors for many groups (kernels_hash_group.hip; the rules of the table are
// hash_group.hpp).  ONE key column of an integer class in prog.keys[0], up to `max_groups` (1 .. hashgroup::kMaxHashGroups)
// distinct keys in a call, and the aggregates whose merge is exact in any order.
//! the table in HBM for the whole call (hashgroup::TableBytes bytes): head words, `slots` key words, the records
struct HashTableDev {
  uint32_t* head;
  uint64_t* keys;
  uint64_t* records;
  uint32_t slots;       // hashgroup::SlotsFor(max_groups)
  uint32_t max_groups;
};
HashTableDev HashTableAt(void* base, uint32_t max_groups, int n_aggs);
//! what hash_group_collect writes: the first head[kHeadCollected] (<= max_groups) entries of keys / nulls / partials (n_aggs each)
struct HashCollectOut {
  uint64_t* keys;
  aggmerge::Partial* partials;
  uint32_t* nulls;
};
size_t HashCollectBytes(uint32_t max_groups, int n_aggs);
HashCollectOut HashCollectAt(void* base, uint32_t max_groups, int n_aggs);
//! one key column that hashgroup::HashProgramIsValid takes, and a valid aggregate program of the operations it takes
bool HashGroupProgramIsValid(const GroupProgram& prog, const AggExprTable* exprs = nullptr);
//! hash_group_clear: every slot free, every record the identity of its operation, the head zero (asynchronous)
hipError_t LaunchHashGroupClear(const GroupProgram& prog, const HashTableDev& table, hipStream_t stream);
//! hash_group_rows: every selected row of `nrows` rows finds or claims its key's slot and applies its aggregates to the
//! slot's records by atomics; sel / sel_count / exprs as LaunchAggWindows takes them
hipError_t LaunchHashGroupRows(const GroupProgram& prog, const mi_sel_t* sel, const uint32_t* sel_count, int64_t nrows,
                               const HashTableDev& table, hipStream_t stream, const AggExprTable* exprs = nullptr);
//! hash_group_collect: the records in use as dense arrays, in no particular order
hipError_t LaunchHashGroupCollect(const GroupProgram& prog, const HashTableDev& table, const HashCollectOut& out, hipStream_t stream);
//! launches by this process so far: [0] hash_group_rows, [1] hash_group_collect
void HashGroupLaunchCounts(int64_t out[2]);

// K7 launches.  The string / list kernel is a single pass (decoupled look-back across the tiles of a column); it needs
// 2 * total_tiles + 1 state words (zeroed by the launch).
// LaunchEncodeFixed: kernel_mask bit 0 = the slice has tiles of encode_fixed, bit 1 = of encode_uuid_text (MI_K_ENC_UUID_TEXT),
// bit 2 = of encode_union (MI_K_ENC_UNION, kernels_encode_union.hip: LaunchEncodeUnion, which it starts before the other two).
hipError_t LaunchEncodeFixed(const mi_col_task* d_tasks, const uint32_t* d_tile_begin, const uint32_t* d_tile_task,
                             int32_t n_tasks, uint32_t total_tiles, int64_t* d_null_counts, uint32_t* d_status, uint32_t kernel_mask,
                             hipStream_t stream);
hipError_t LaunchEncodeUnion(const mi_col_task* d_tasks, const uint32_t* d_tile_begin, const uint32_t* d_tile_task, int32_t n_tasks,
                             uint32_t total_tiles, uint32_t* d_status, hipStream_t stream);
hipError_t LaunchEncodeString(const mi_col_task* d_tasks, const uint32_t* d_tile_begin, const uint32_t* d_tile_task,
                              int32_t n_tasks, uint32_t total_tiles, int64_t* d_tile_state, int64_t* d_null_counts,
                              uint32_t* d_status, bool has_lists, hipStream_t stream);
// MI_K_ENC_STRVIEW tasks only (kernels_encode_view.hip): string_t -> Arrow string views, one workgroup per 2048-row tile, a
// look-back of its own over `total_tiles` state words (zeroed by the launch).  The kind is in no kernel class: a plan stages
// such tasks in a slice of their own, as it does run-end tasks, and launches this kernel only when it has one.
hipError_t LaunchEncodeStringView(const mi_col_task* d_tasks, const uint32_t* d_tile_begin, const uint32_t* d_tile_task, int32_t n_tasks,
                                  uint32_t total_tiles, int64_t* d_tile_state, int64_t* d_null_counts, uint32_t* d_status, hipStream_t stream);

// The writer's LZ4_FRAME compressor (kernels_lz4_encode.hip).  One wave per block of `d_blocks`: block b of the encoded body
// `d_body` is compressed into d_slots + b * lz4enc::kSlotStride and d_words[b] becomes its size word (the compressed size,
// or lz4enc::kStoredFlag | n: the slot holds nothing, the block's bytes are taken from the body).
hipError_t LaunchLz4CompressBlocks(const uint8_t* d_body, const lz4enc::BlockIn* d_blocks, uint32_t n_blocks, uint8_t* d_slots,
                                   uint32_t* d_words, hipStream_t stream);
// Runs the copy table of LayOutCompressedBody (writer_plan.hpp): one workgroup per copy into `d_out`, which the caller zeroed.
hipError_t LaunchCompactBody(const uint8_t* d_body, const uint8_t* d_slots, const lz4enc::BodyCopy* d_copies, uint32_t n_copies,
                             uint8_t* d_out, hipStream_t stream);

}  // namespace device
}  // namespace miarrow
