// scan_multi.cpp -- MultiDeviceScan (see scan_operator.hpp): read_arrow over several GPUs of one process, over the public
// interface of ArrowScan alone.  (Its Aggregate / GroupAggregate are scan_aggregate.cpp's.)
#include "scan_operator.hpp"
#include "io_pool.hpp"

#include <cstring>
#include <exception>
#include <thread>

namespace miarrow {

MultiDeviceScan::MultiDeviceScan(const std::vector<Context*>& ctxs, std::vector<std::string> paths, const mi_scan_options& o) {
  if (ctxs.empty()) throw InvalidInputException("mi_scan_open_files_multi needs at least one context");
  const int32_t n = static_cast<int32_t>(ctxs.size());
  const int32_t outer_world = o.world > 1 ? o.world : 1, outer_rank = o.world > 1 ? o.rank : 0;
  if (outer_rank < 0 || outer_rank >= outer_world) throw InvalidInputException("rank outside [0, world)");
  for (int32_t i = 0; i < n; i++) {
    if (!ctxs[static_cast<size_t>(i)]) throw InvalidInputException("mi_scan_open_files_multi: NULL context");
    mi_scan_options so = o;
    // batch k of the file list belongs to this scan when k mod world == rank; its j-th batch goes to context j mod n:
    // k = rank + world * j  =>  sub-scan i takes the batches with k mod (world * n) == rank + world * i
    so.world = outer_world * n;
    so.rank = outer_rank + outer_world * i;
    subs.push_back(std::make_unique<ArrowScan>(ctxs[static_cast<size_t>(i)], paths, so));
  }
  EnsureIoThreads(8 * n);  // every device reads its own record batches out of the page cache
  pending.resize(subs.size());
  have.assign(subs.size(), 0);
  done.assign(subs.size(), 0);
}

const std::vector<ScanColumn>& MultiDeviceScan::Bind() {
  for (size_t i = 1; i < subs.size(); i++) subs[i]->Bind();
  return subs[0]->Bind();
}

void MultiDeviceScan::Init(const std::vector<std::string>& projected) {
  for (auto& s : subs) s->Init(projected);
}

void MultiDeviceScan::SetFilter(FilterCnf cnf) {
  for (auto& s : subs) s->SetFilter(cnf);
}

void MultiDeviceScan::ForEachParallel(const std::function<void(size_t)>& fn) {
  std::vector<std::thread> threads;
  std::vector<std::exception_ptr> errors(subs.size());
  for (size_t i = 0; i < subs.size(); i++)
    threads.emplace_back([&, i] {
      try {
        fn(i);
      } catch (...) {
        errors[i] = std::current_exception();
      }
    });
  for (auto& t : threads) t.join();
  for (auto& e : errors)
    if (e) std::rethrow_exception(e);
}

// k-way merge on the record-batch ordinal: every sub-scan yields its own batches in ascending order, so the chunk to emit
// is the pending one with the smallest batch_index.  A pending chunk stays valid until its sub-scan is pulled again, which
// happens only after the consumer has come back for the next chunk.
void MultiDeviceScan::Next(mi_data_chunk* out) {
  if (last_emitted >= 0) {
    have[static_cast<size_t>(last_emitted)] = 0;
    last_emitted = -1;
  }
  int best = -1;
  for (size_t i = 0; i < subs.size(); i++) {
    if (!have[i] && !done[i]) {
      subs[i]->Next(&pending[i]);
      if (pending[i].size == 0) done[i] = 1;
      else have[i] = 1;
    }
    if (have[i] && (best < 0 || pending[i].batch_index < pending[static_cast<size_t>(best)].batch_index)) best = static_cast<int>(i);
  }
  if (best < 0) {
    std::memset(out, 0, sizeof(*out));
    out->n_columns = static_cast<int32_t>(subs[0]->NumOutputColumns());
    return;
  }
  *out = pending[static_cast<size_t>(best)];
  last_emitted = best;
}

void MultiDeviceScan::Count(int64_t* rows, int64_t* selected, int64_t* chunks) {
  std::vector<int64_t> r(subs.size(), 0), s(subs.size(), 0), c(subs.size(), 0);
  ForEachParallel([&](size_t i) { subs[i]->Count(&r[i], &s[i], &c[i]); });
  int64_t tr = 0, ts = 0, tc = 0;
  for (size_t i = 0; i < subs.size(); i++) {
    tr += r[i];
    ts += s[i];
    tc += c[i];
  }
  if (rows) *rows = tr;
  if (selected) *selected = ts;
  if (chunks) *chunks = tc;
}

void MultiDeviceScan::SumProduct(const std::string& a, const std::string& b, const std::vector<std::string>& filter_columns,
                                 const std::vector<int64_t>& lo, const std::vector<int64_t>& hi, mi_sum_product_result* out) {
  std::vector<mi_sum_product_result> parts(subs.size());
  for (auto& p : parts) std::memset(&p, 0, sizeof(p));
  ForEachParallel([&](size_t i) { subs[i]->SumProduct(a, b, filter_columns, lo, hi, &parts[i]); });
  unsigned __int128 sum = 0;
  std::memset(out, 0, sizeof(*out));
  for (auto& p : parts) {
    sum += (static_cast<unsigned __int128>(static_cast<uint64_t>(p.sum_hi)) << 64) | p.sum_lo;  // two's complement: wraps like the device
    out->rows_scanned += p.rows_scanned;
    out->rows_selected += p.rows_selected;
  }
  out->sum_lo = static_cast<uint64_t>(sum);
  out->sum_hi = static_cast<int64_t>(static_cast<uint64_t>(sum >> 64));
}

void MultiDeviceScan::Stats(mi_scan_stats* out) {
  for (auto& s : subs) s->Stats(out);
}

double MultiDeviceScan::Progress() {
  double p = 0;
  for (auto& s : subs) p += s->Progress();
  return p / static_cast<double>(subs.size());
}

}  // namespace miarrow
