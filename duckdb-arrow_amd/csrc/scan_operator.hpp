// scan_operator.hpp -- the scan TableFunction body: read_arrow / scan_arrow_ipc on the MI355X path.
//
// Takes the place of what the reference wires together from DuckDB pieces:
//   bind      ArrowFileScan::ArrowFileScan            src/file_scanner/arrow_file_scan.cpp:9-23
//             ScanArrowIPCFunction::ScanArrowIPCBind   src/scanner/scan_arrow_ipc.cpp:20-48
//             ArrowMultiFileInfo::BindReader           src/file_scanner/arrow_multi_file_info.cpp:54-70
//   init      ArrowFileScan::TryInitializeScan         src/file_scanner/arrow_file_scan.cpp:30-67
//             ArrowIPCStreamFactory::Produce (projection)  src/ipc/stream_factory.cpp:14-30
//   scan      ArrowFileScan::Scan -> ArrowTableFunction::ArrowScanFunction   src/file_scanner/arrow_file_scan.cpp:68-72
//             (<= 2048 rows per call, output cardinality 0 = exhausted)
// The per-value work of ArrowToDuckDB runs in the HIP kernels; this class is the pipeline around them:
// record-batch body -> pinned slot -> hipMemcpyAsync H2D (copy stream) -> class kernels (compute stream) ->
// hipMemcpyAsync D2H (copy-back stream) -> DataChunks that alias the pinned output slot.
// What feeds the pipeline and what it is told to keep live beside it:
//   scan_readahead.{hpp,cpp}   ReadAhead: producer threads, their queues and pinned staging buffers (host code only)
//   scan_filter.cpp            pushed-down predicates: normalisation, binding to the scan's columns, constants in HBM,
//                              the per-batch FilterProgram
//   scan_column.hpp            ScanColumn and what its Arrow field says about its values (host code only)
//   scan_aggregate.{hpp,cpp}   the fused aggregates: the methods below that enqueue and drain them, their C ABI, over the
//                              units agg_bind (host code only), agg_result (host code only) and agg_run
//   scan_enqueue.cpp           what a record batch costs the GPU: stage A and stage B of ArrowScan as named steps, the K8
//                              staging, the helpers both stages share
//   scan_k8.{hpp,cpp}          the K8 scratch arena as data: layout, pinned tables, launch arguments (host code only)
//   scan_dictionary.{hpp,cpp}  DictState and the host side of a dictionary version (host code only)
//   scan_multi.cpp             MultiDeviceScan, over ArrowScan's public interface
#pragma once

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <mutex>
#include <memory>
#include <string>
#include <vector>

#include "batch_planner.hpp"
#include "engine.hpp"
#include "ipc_stream_reader.hpp"
#include "scan_aggregate.hpp"
#include "scan_dictionary.hpp"
#include "scan_readahead.hpp"

namespace miarrow {

//! One leaf of a pushed-down predicate after normalisation (scan_filter.cpp): every comparison on an integer-like column
//! is an inclusive range (optionally negated), plus IS [NOT] NULL and IN-lists.
struct FilterLeaf {
  std::string column;
  int32_t op = 0;                 // device::kLeaf*
  int64_t lo = 0, hi = 0;         // kLeafRange: lo <= v <= hi ...
  bool lo_open = true, hi_open = true;  // ... where an open end has no bound at all (uint64 columns reach past INT64_MAX)
  //! kLeafRange from `v > INT64_MAX`: the empty range (1, 0) on every column but a uint64 one, where it keeps the values
  //! >= 2^63 (BoundFilter::Program knows the column's signedness).  Such a leaf is never merged with another range.
  bool above_int64_max = false;
  bool negate = false;
  std::vector<int64_t> in_values;
  bool is_string = false;         // kLeafStrIn: the column is VARCHAR / BLOB, the row passes when it equals one of ...
  std::vector<std::string> str_values;   // ... these byte strings (negate: none of them)
  //! kLeafStrRange: str_values = {lower, upper}; lo_open / hi_open = no such bound, the two below = the bound itself passes
  bool lo_incl = false, hi_incl = false;
  //! kLeafStrMatch (contains / ends_with / %-pattern LIKE, like_match.hpp): str_values = the literal segments in pattern
  //! order, anchored at the head / the tail of the row; negate = NOT LIKE
  bool match_head = false, match_tail = false;
  //! FLOAT / DOUBLE column (width 4 / 8): an integer leaf as above (kLeafRange / kLeafIn) whose lo / hi / in_values are the
  //! order-preserving keys of the constants (filter_key.hpp); the kernel maps every value the same way (kLeafFloat)
  int32_t float_width = 0;
  //! kLeafWideRange / kLeafWideIn: the column is HUGEINT / DECIMAL(19..38), a form of its own as strings are
  bool is_wide = false;
  __int128 wide_lo = 0, wide_hi = 0;     // wide_lo <= v <= wide_hi (negate: outside)
  std::vector<__int128> wide_in;         // sorted, distinct
  int32_t out_col = -1;           // resolved at Init: index into the scan's filter columns
};
//! Conjunctive normal form: every clause is an OR of leaves, the filter is the AND of its clauses.
using FilterCnf = std::vector<std::vector<FilterLeaf>>;
//! `columns` (the scan's bind result) tells what each leaf's constants are compared as: a FLOAT / DOUBLE column takes
//! doubles, a 128-bit one 128-bit integers, and a constant kind that does not fit its column is refused naming the column.
//! Without it (mi_scan_set_filter_range) every constant is a stored int64.
FilterCnf NormaliseFilter(const mi_filter_node* nodes, int32_t n_nodes, int32_t root, const std::vector<ScanColumn>* columns = nullptr);  // scan_filter.cpp
//! what likematch::Compile answered -> nothing, or the refusal mi_scan_set_filter and mi_filter_like_match share (`column` may be empty)
void CheckPattern(int compiled, int32_t op, const std::string& column);

//! A pushed-down filter bound to the columns of a scan (ArrowScan::Init)
struct BoundFilter {
  FilterCnf cnf;
  //! filter column k (FilterLeaf::out_col) -> output column (>= 0) or ~index into `only` (< 0)
  std::vector<int32_t> columns;
  std::vector<ScanColumn> only;          // filter columns outside the projection: decoded, never emitted
  std::vector<DeviceBuffer> d_in_lists;  // per leaf (clause order): its IN-list / string constants in HBM, or empty
  const ScanColumn& Column(size_t k, const std::vector<ScanColumn>& out_columns) const {
    const int32_t wc = columns[k];
    return wc >= 0 ? out_columns[static_cast<size_t>(wc)] : only[static_cast<size_t>(~wc)];
  }
  //! resolves every leaf to a filter column (projected, or decoded for the filter alone) and checks that its type can be
  //! compared on the GPU
  void Resolve(const std::vector<ScanColumn>& all_columns, const std::vector<ScanColumn>& out_columns);
  //! IN-lists and string constants -> HBM, for the lifetime of the scan
  void UploadConstants();
  //! What Program() reads of one record batch in its pipeline slot
  struct Batch {
    const DecodedBatch& batch;
    const std::vector<PlannedNode>& nodes;
    const std::vector<int32_t>& roots;                          // per filter column: planner node of its decoded vector, -1 absent
    const std::vector<std::shared_ptr<DictState>>& node_dict;   // per planner node
    const uint8_t* d_in;                                        // the body in HBM
    const uint8_t* d_out;                                       // the arena of decoded vectors
    const uint8_t* d_empty;                                     // any readable bytes (leaves over absent columns)
  };
  //! The leaves as the filter kernel takes them for this record batch.  Dictionary match maps that the batch's dictionary
  //! versions do not have yet are made here and uploaded on `stream`, in front of the kernel that reads them.
  device::FilterProgram Program(const std::vector<ScanColumn>& out_columns, const Batch& b, hipStream_t stream) const;
};

//! What of a leaf does not depend on the record batch -- form, flags, bounds, the constants UploadConstants put into HBM --
//! as the kernel takes it; the caller binds data, validity and width (BoundFilter::Program, mi_filter_string)
void LeafConstants(const FilterLeaf& leaf, const DeviceBuffer& constants, bool ends_clause, device::FilterLeafDev& L);

//! Vectors of one DataChunk (the storage behind mi_data_chunk.columns)
struct ChunkStorage {
  std::vector<mi_vector> vectors;
  std::vector<mi_vector> child_pool;
  size_t child_pool_used = 0;
};

//! A record batch whose decoded vectors are complete and held for the caller (ArrowScan::AcquireBatch)
struct BatchRef {
  int slot = -1;
  int64_t batch_index = 0;
  int64_t nrows = 0;
  int32_t source = 0;
  int32_t n_windows = 0;     // chunks BuildChunk can produce (compacted batches: of the rows that survived the filter)
  int64_t selected = 0;      // rows passing the pushed-down filter (== nrows without one)
  int64_t chunk_rows = 0;    // rows its chunks hold together: nrows, or `selected` when the batch was compacted
};

//! A decoded top-level column of an acquired record batch where it lies in HBM (the fused COPY reads it there)
struct DeviceColumnView {
  bool flat = false;                  // a leaf vector without dictionary / children; the fields below are set only then
  const uint8_t* d_data = nullptr;    // DuckDB vector data (row 0 of the batch)
  const uint8_t* d_validity = nullptr;  // validity words, NULL when the column has no NULLs
  int32_t kind = 0, width = 0;
  int64_t null_count = 0;
  const uint8_t* d_heap = nullptr;    // string kinds: device copy of the Arrow data buffer ...
  uint64_t ptr_base = 0;              // ... and the pointer value its byte 0 has inside the string_t rows
  const uint8_t* h_offsets = nullptr; // string kinds: the Arrow offsets / validity bitmap in the host body
  const uint8_t* h_validity = nullptr;
  int32_t offset_width = 0;
};

class ScanBase {
 public:
  virtual ~ScanBase() = default;
  virtual const std::vector<ScanColumn>& Bind() = 0;
  virtual void Init(const std::vector<std::string>& projected) = 0;
  virtual void SetFilter(FilterCnf cnf) = 0;
  virtual void Next(mi_data_chunk* out) = 0;
  virtual void Count(int64_t* rows, int64_t* selected, int64_t* chunks) = 0;
  virtual void SumProduct(const std::string& a, const std::string& b, const std::vector<std::string>& filter_columns,
                          const std::vector<int64_t>& lo, const std::vector<int64_t>& hi, mi_sum_product_result* out) = 0;
  //! mi_scan_aggregate: `out` receives one partial per spec (agg_merge.hpp), ops / classes what each is merged by
  virtual void Aggregate(const std::vector<AggSpec>& specs, AggResult* out) = 0;
  //! mi_scan_group_aggregate: the groups of this scan, sorted
  virtual void GroupAggregate(const std::vector<std::string>& keys, const std::vector<AggSpec>& specs, GroupResult* out) = 0;
  //! mi_scan_hash_aggregate: the groups of this scan by one integer key, up to `max_groups` of them, sorted
  virtual void HashAggregate(const std::string& key, const std::vector<AggSpec>& specs, uint32_t max_groups, GroupResult* out) = 0;
  virtual double Progress() = 0;
  virtual void Stats(mi_scan_stats* out) = 0;   // adds to *out
};

constexpr size_t kAlign = 256;   // arrays in HBM start on a multiple of this
inline size_t AlignUp(size_t v, size_t a = kAlign) { return (v + a - 1) / a * a; }

constexpr int kMaxDepth = 16;   // pipeline slots of a scan at most (24 and 32 were measured with 40 hardware queues: slower for both codecs of K8)

class ArrowScan : public ScanBase {
 public:
  ArrowScan(Context* ctx, std::vector<std::string> paths, const mi_scan_options& opts);
  ArrowScan(Context* ctx, std::vector<ArrowIPCBuffer> buffers, const mi_scan_options& opts);
  ~ArrowScan() override;

  //! Bind: schema of the scan (names deduplicated) -- "Provided table/dataframe must have at least one column"
  const std::vector<ScanColumn>& Bind() override;
  //! Init: projection pushdown (column names, output order)
  void Init(const std::vector<std::string>& projected) override;
  //! Predicate pushed into the scan (K6; the reference leaves filters to DuckDB: read_arrow.cpp:47-48)
  void SetFilter(FilterCnf cnf) override;
  //! One DataChunk (<= 2048 rows); size 0 when exhausted
  void Next(mi_data_chunk* out) override;
  void Count(int64_t* rows, int64_t* selected, int64_t* chunks) override;
  double Progress() override;
  void Stats(mi_scan_stats* out) override;
  //! sum(a * b) over rows passing the range filters, all on the GPU; drains the scan (mi_scan_sum_product)
  void SumProduct(const std::string& a, const std::string& b, const std::vector<std::string>& filter_columns,
                  const std::vector<int64_t>& lo, const std::vector<int64_t>& hi, mi_sum_product_result* out) override;

  //! up to 8 aggregates over the rows the pushed-down filter keeps, all on the GPU; drains the scan (mi_scan_aggregate)
  void Aggregate(const std::vector<AggSpec>& specs, AggResult* out) override;
  //! the same aggregates per group of up to 4 key columns, for few groups (mi_scan_group_aggregate)
  void GroupAggregate(const std::vector<std::string>& keys, const std::vector<AggSpec>& specs, GroupResult* out) override;
  //! the aggregates whose merge is exact in any order per group of ONE integer key, for many groups (mi_scan_hash_aggregate)
  void HashAggregate(const std::string& key, const std::vector<AggSpec>& specs, uint32_t max_groups, GroupResult* out) override;

  // ---- batch-level pull (what Next() is built on; the COPY pump and the multi-device scan use it directly) ----
  //! Waits for the next record batch in order; false when the scan is exhausted.  The batch stays valid (its slot is
  //! not recycled) until ReleaseBatch; at most pipeline_depth - 1 batches may be held at once.
  bool AcquireBatch(BatchRef* out);
  //! Chunk `window` (rows [2048 w, 2048 (w+1)) of the batch; fewer when compacted) -> out, vectors in `storage`.
  //! Thread-safe for different batches.
  void BuildChunk(const BatchRef& ref, int32_t window, ChunkStorage* storage, mi_data_chunk* out);
  void ReleaseBatch(const BatchRef& ref);
  //! true once every source is read and no batch is in flight (AcquireBatch returns false both then and when every slot is
  //! held by the caller: release one and ask again)
  bool Exhausted() const { return exhausted && inflight.empty(); }
  void EnsurePipelineDepth(int depth);
  bool HostConsumer() const { return !opts.device_resident; }
  size_t NumOutputColumns() const { return out_columns.size(); }
  const std::vector<ScanColumn>& OutputColumns() const { return out_columns; }
  bool Initialized() const { return initialized; }
  bool HasFilter() const { return has_filter; }
  //! Host consumers only: decoded vectors of the record batches enqueued from now on stay in HBM (no copy into the pinned
  //! output slot) until EnsureHostVectors asks for them -- a consumer that reads them on the GPU (the fused COPY) sets this
  void KeepVectorsOnDevice(bool on) { keep_on_device = on; }
  void EnsureHostVectors(const BatchRef& ref);
  void DeviceColumn(const BatchRef& ref, size_t column, DeviceColumnView* out) const;

 private:
  //! files, or (without any) caller buffers
  ArrowScan(Context* ctx, std::vector<std::string> paths, std::vector<ArrowIPCBuffer> buffers, const mi_scan_options& opts);
  //! What the scan knows of one file beside the read-ahead's reader of it.  The column mapping is written by MapColumns
  //! on the first producer thread before that file's first batch is queued, and read by the pipeline after it took one.
  struct Source {
    std::vector<int32_t> out_to_file_column;   // per output column: index in this file's projected batch, -1 = absent
    std::vector<int32_t> filter_to_file_column;  // per filter-only column (not in the projection)
    std::map<std::string, std::string> hive;   // key -> value parsed from the path
    //! where output column `wc` (>= 0) or filter-only column ~wc (< 0) lies in this file's projected batch, -1 = absent
    int32_t FileColumn(int32_t wc) const { return wc >= 0 ? out_to_file_column[static_cast<size_t>(wc)] : filter_to_file_column[static_cast<size_t>(~wc)]; }
  };
  struct Slot {
    int64_t tr_enqueued_ns = 0;       // MI_SCAN_TRACE: when the batch was submitted
    // one record batch in flight
    DeviceBuffer d_in;                                 // body in HBM
    DeviceBuffer d_out;                                // decoded vectors in HBM
    PinnedBuffer h_out;                                // decoded vectors, pinned
    std::unique_ptr<Plan> plan;                        // full-width decode (all columns, or the filter columns when compacting)
    std::unique_ptr<Plan> gather_plan;                 // compaction: every projected column through the selection vector
    PinnedBuffer h_status;                             // uint32_t: copies of the plans' device status words, K8 counters
    HipEvent h2d_done, compute_done, d2h_done, filter_done;
    bool busy = false;
    DecodedBatch batch;
    int32_t source = 0;
    int64_t batch_index = 0;
    int64_t nrows = 0;
    BatchPlanner planner{PlannerOptions{}};            // layout + tasks of the projected columns
    std::vector<int32_t> col_root;                     // per output column: planner node (-1: absent in this file)
    struct Absent {                                    // the all-NULL vector of an output column absent in this file
      size_t data_off = 0, valid_off = 0;              // in the arena the projected columns are laid out in
      int32_t kind = 0, width = 0;
    };
    std::vector<Absent> absent;                        // per output column
    std::vector<std::shared_ptr<DictState>> node_dict; // per planner node: the dictionary version this batch uses
    PinnedBuffer h_aux;                                // list window tables, string-view buffer tables, filter program
    DeviceBuffer d_aux;
    size_t sel_off = 0, sel_count_off = 0;             // filter outputs (arena offsets)
    std::vector<int32_t> filter_root;                  // per filter column: planner node of its full-width decoded vector
    PinnedBuffer h_counts;                             // uint32_t: rows selected per 2048-row window
    size_t d2h_bytes = 0;                              // bytes that travel back to the host
    size_t stage_a_bytes = 0;                          // arena bytes of the full-width arrays (+ sel, counts)
    bool compact = false;                              // chunks hold only the selected rows (dense arrays behind stage A's)
    bool host_vectors = false;                         // h_out holds the decoded vectors
    // K8: a record batch whose LZ4 buffers are decompressed in HBM (kernels_lz4.hip)
    DeviceBuffer d_comp;                               // the compressed body
    DeviceBuffer d_lz4;                                // block / buffer tables, sequence descriptors, links, counters
    PinnedBuffer h_lz4;                                // pinned copy of the tables
    hipStream_t lz4_stream = nullptr;                  // decompression of this slot overlaps the other slots' copies and kernels;
    HipStream own_lz4_stream;                          // lz4_stream is this one or a lower slot's (borrowed: never destroyed here)
    HipEvent lz4_done;
    PinnedBuffer h_mirror;                             // host consumers: pinned image of the decompressed body; only the
                                                       // string payload buffers are filled (D2H), string_t rows point into it
    bool lz4_counted = true;
    bool needs_stage_b = false;                        // compaction: the gather + copy back wait for the counts
    uint8_t* compact_region = nullptr;                 // device address of the dense arrays
  };

  //! takes the next fetched record batch and enqueues its GPU work; false when nothing could be submitted (no free
  //! slot, nothing fetched yet while `may_block` is false, or every source is exhausted)
  bool SubmitNextBatch(bool may_block);
  //! per-file column mapping by name (ReadAhead::Hooks::project): fills sources[si], returns the reader projection
  std::vector<std::string> MapColumns(size_t si, const ArrowSchemaModel& schema);
  void GrowSlots(size_t n);
  void InitSlot(Slot& s);
  void BuildVector(const Slot& s, int32_t node, size_t window, int64_t compact_rows, uint8_t* base, ChunkStorage* st, mi_vector* out);
  void DecodeDictionary(const DecodedBatch& b);
  // ---- scan_enqueue.cpp: the GPU work of one record batch
  //! stage A: body upload, full-width decode, filter, fused aggregates and -- unless the batch is compacted -- the copy back
  void EnqueueBatch(Slot& s);
  //! stage B of a compacted batch, once the filter's counts are on the host: gather of the selected rows, the copy back
  void EnqueueStageB(Slot& s);
  // the steps of stage A, in the order EnqueueBatch calls them
  bool SetPlannerOptions(Slot& s, size_t in_bytes);
  void LayOutStageA(Slot& s);
  void RefuseAbsentAggregateColumns(const Source& src) const;
  void SizeSlotBuffers(Slot& s);
  void UploadBody(Slot& s, bool mirror);
  void EnqueueLz4(Slot& s);
  void ChooseLz4Stream(Slot& s, int32_t codec);
  void MirrorStringPayload(Slot& s);
  void LaunchStageA(Slot& s);
  void EnqueueSumProduct(Slot& s);
  void CopyBackStageA(Slot& s);
  // what both stages do
  //! every output column that is not a constant into `planner`: decoded from the file's column (its root goes to
  //! s.col_root), or -- absent from this file -- an all-NULL vector of `rows` rows
  void PlanOutputColumns(Slot& s, BatchPlanner& planner, const BatchPlacement& where, int64_t rows);
  //! s.node_dict: the dictionary version every node of `nodes` uses as of now
  void BindNodeDicts(Slot& s, const std::vector<PlannedNode>& nodes);
  //! the status words of the slot's plans travel home behind the results (instead of costing a stream-wide synchronisation),
  //! then d2h_done: stage A has one word (`with_gather` false: word 1 is zeroed), stage B two
  void SendStatusHome(Slot& s, bool with_gather);
  void UploadAux(Slot& s, const std::vector<uint64_t>& aux);
  BatchPlacement MakePlacement(const Slot& s);
  //! H2D on the copy stream: `ranges` ({offset, length}, the same in `from` and `to`) closer than 64 KiB travel as one copy.
  //! align_within >= 0: every copy starts and ends on a multiple of 64 bytes, or at that size.
  void CopyRanges(std::vector<std::pair<int64_t, int64_t>> ranges, const uint8_t* from, uint8_t* to, int64_t align_within);
  //! a column absent from a file (union_by_name): its all-NULL vector of `rows` rows reserved in `planner`'s arena, ...
  void PlanAbsentColumn(Slot& s, BatchPlanner& planner, size_t column, int64_t rows);
  //! ... and zeroed on the compute stream
  void ZeroAbsentColumn(const Slot& s, size_t column, uint8_t* base, int64_t rows);
  void EnsureHostOut(Slot& s, size_t bytes);
  // ----
  Slot* FreeSlot();

  Context* ctx;
  mi_scan_options opts;
  std::vector<Source> sources;
  const bool is_buffers;
  bool bound = false, initialized = false;
  std::vector<ScanColumn> all_columns;   // bind result
  std::vector<ScanColumn> out_columns;   // after projection

  // pipeline
  std::vector<Slot> slots;
  std::deque<int> inflight;              // slot indices in submission order (not yet acquired)
  bool exhausted = false;
  // consumer cursor of Next()
  BatchRef cur_ref;
  bool have_cur = false;
  int32_t cur_window = 0;
  ChunkStorage next_storage;
  // fused aggregate (mi_scan_sum_product): output columns the kernel reads, bounds, device accumulator
  struct Aggregate {
    bool on = false;
    int32_t col_a = -1, col_b = -1;
    std::vector<int32_t> filter_cols;
    std::vector<int64_t> lo, hi;
    DeviceBuffer d_acc;                    // unsigned long long {sum lo, sum hi, rows selected}
    int64_t rows_scanned = 0;
  } agg;
  // fused aggregates (mi_scan_aggregate and its grouped forms): a state of its own beside `agg`
  struct AggregateState {
    bool on = false;
    BoundAggregates plan;                    // what the call reads, over the slots of its projection = the output columns
    int64_t rows_scanned = 0;
    std::unique_ptr<AggRun> run;             // the device side: lives as long as the call
  } aggn;
  // (the methods from here to DrainAggregates are scan_aggregate.cpp's)
  //! the driver of the three calls: DrainAggregates, then the run's read-back; *out is sorted when the plan has keys
  void RunAggregates(BoundAggregates plan, GroupResult* out);
  //! the run's launches over the slot's decoded vectors and selection vectors, behind the filter on the compute stream
  void EnqueueAggregates(Slot& s);
  //! aggn.plan over the slot's decoded vectors as the launches take it; true: `exprs` holds the kOpSumExpr aggregates' expressions
  bool FillAggregatePrograms(const Slot& s, device::GroupProgram* gprog, device::AggExprTable* exprs) const;
  //! runs the scan over aggn.plan.projection with aggn.on: the run's Begin after Init, then every record batch; returns the selected rows
  int64_t DrainAggregates();
  // constant columns (filename / hive): 2048 string_t each per source, host
  std::map<std::pair<int32_t, size_t>, std::vector<mi_string_t>> const_vectors;
  std::mutex const_mu;
  std::vector<mi_validity_t> all_valid;
  // dictionaries by id
  std::map<int64_t, std::shared_ptr<DictState>> dicts;
  bool has_filter = false;
  BoundFilter filter;
  // Buffers a slot has outgrown.  Freeing a buffer waits for the device to go idle -- with the other slots' record batches
  // in flight that is a pipeline stall of milliseconds -- so they are kept until the scan closes (growth is geometric: at
  // most twice the final sizes in all).
  std::vector<DeviceBuffer> retired_device;
  std::vector<PinnedBuffer> retired_host;
  void Retire(DeviceBuffer b) { if (b) retired_device.push_back(std::move(b)); }   // (the pipeline thread alone)
  void Retire(PinnedBuffer b) { if (b) retired_host.push_back(std::move(b)); }
  bool compact = false;
  bool keep_on_device = false;
  mi_scan_stats stats{};
  // MI_SCAN_TRACE: where the host threads' time went (seconds), printed when the scan closes (diagnostics only)
  bool trace = false;
  int64_t tr_latency_ns = 0, tr_inflight_sum = 0, tr_k8_prep_ns = 0, tr_k8_launch_ns = 0, tr_enqueue_ns = 0, tr_fetch_wait_ns = 0, tr_event_wait_ns = 0, tr_poll_ns = 0;
  // Last member, so the first to go: its queues and readers release their staging leases while everything above is
  // still there, and its pinned buffers are freed after ~ArrowScan's body has synchronised the streams.
  ReadAhead readahead;
};

//! read_arrow over several GPUs of one process: one ArrowScan per context, record batch k of the file list
//! goes to sub-scan k mod N, chunks come back in record-batch order (k-way merge on batch_index).  Draining calls
//! (Count, SumProduct) run every sub-scan on its own thread.
class MultiDeviceScan : public ScanBase {
 public:
  MultiDeviceScan(const std::vector<Context*>& ctxs, std::vector<std::string> paths, const mi_scan_options& opts);
  const std::vector<ScanColumn>& Bind() override;
  void Init(const std::vector<std::string>& projected) override;
  void SetFilter(FilterCnf cnf) override;
  void Next(mi_data_chunk* out) override;
  void Count(int64_t* rows, int64_t* selected, int64_t* chunks) override;
  void SumProduct(const std::string& a, const std::string& b, const std::vector<std::string>& filter_columns,
                  const std::vector<int64_t>& lo, const std::vector<int64_t>& hi, mi_sum_product_result* out) override;
  void Aggregate(const std::vector<AggSpec>& specs, AggResult* out) override;
  void GroupAggregate(const std::vector<std::string>& keys, const std::vector<AggSpec>& specs, GroupResult* out) override;
  void HashAggregate(const std::string& key, const std::vector<AggSpec>& specs, uint32_t max_groups, GroupResult* out) override;
  double Progress() override;
  void Stats(mi_scan_stats* out) override;

 private:
  void ForEachParallel(const std::function<void(size_t)>& fn);
  std::vector<std::unique_ptr<ArrowScan>> subs;
  std::vector<mi_data_chunk> pending;   // one chunk per sub-scan, valid until that sub-scan's next Next()
  std::vector<char> have, done;
  int last_emitted = -1;
};

}  // namespace miarrow
