// writer_plan_check.cpp -- the writer's planning unit (duckdb-arrow_amd/csrc/writer_plan.cpp) without a GPU, under
// AddressSanitizer + UBSan and under ThreadSanitizer (test infrastructure, never shipped).
//
//   g++ -std=c++17 -O1 -g -fsanitize=thread -I include tests/sanitize/writer_plan_check.cpp
//       duckdb-arrow_amd/csrc/writer_plan.cpp -lpthread -o writer_plan_check
//
// Layout: for 0, 1, 7, 8, 9, 2048 and 2049 rows, every leaf kind, a list over a string child and a struct of two leaves
// get the buffers the Arrow columnar format prescribes, ascending, apart and on multiples of 64.  Cut rule: the cutter's
// row groups equal a naive restatement (append 2048-row chunks, close after the one that reaches the limit).  Ledger: four
// threads close pieces in random order while this thread holds, cuts and releases; every batch goes back once, on this
// thread, after it is fully cut and closed; ReleaseAll gives back the rest after a failure.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../duckdb-arrow_amd/csrc/writer_plan.hpp"

using namespace miarrow;

namespace {
int g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                    \
  do {                                      \
    g_checks++;                             \
    if (!(cond)) {                          \
      std::fprintf(stderr, "FAILED: ");     \
      std::fprintf(stderr, __VA_ARGS__);    \
      std::fprintf(stderr, "\n");           \
      g_failed++;                           \
    }                                       \
  } while (0)

// ------------------------------------------------------------------------------------------------ layout
// buffer lengths of a node as the Arrow columnar format lists them ("Buffer Listing for Each Layout")
std::vector<int64_t> FormatLengths(const EncodeNode& c) {
  const int64_t n = c.rows, bitmap = (n + 7) / 8, offsets = (n + 1) * (c.large_offsets ? 8 : 4);
  switch (c.kind) {
    case MI_K_ENC_COPY: return {bitmap, n * c.param};
    case MI_K_ENC_DEC128: return {bitmap, n * 16};
    case MI_K_ENC_BOOL: return {bitmap, bitmap};
    case MI_K_ENC_STR32: return {bitmap, offsets, c.payload_bytes};
    case MI_K_ENC_LIST32: return {bitmap, offsets};
    default: return {bitmap};
  }
}

void CheckLayout(const char* what, const std::vector<EncodeNode>& nodes) {
  BodyLayout lay;
  LayOutBody(nodes, &lay);
  std::vector<int64_t> want;
  CHECK(lay.first_span.size() == nodes.size(), "%s: first_span has %zu entries", what, lay.first_span.size());
  for (size_t i = 0; i < nodes.size(); i++) {
    CHECK(lay.first_span[i] == static_cast<int32_t>(want.size()), "%s: node %zu starts at span %d, not %zu", what, i, lay.first_span[i], want.size());
    for (int64_t len : FormatLengths(nodes[i])) want.push_back(len);
  }
  CHECK(lay.spans.size() == want.size(), "%s: %zu spans, the format has %zu", what, lay.spans.size(), want.size());
  if (lay.spans.size() != want.size()) return;
  int64_t end = 0;
  for (size_t k = 0; k < want.size(); k++) {
    const mi_buffer_span& s = lay.spans[k];
    CHECK(s.length == want[k], "%s: span %zu is %lld bytes, not %lld", what, k, (long long)s.length, (long long)want[k]);
    CHECK(s.offset % 64 == 0, "%s: span %zu starts at %lld", what, k, (long long)s.offset);
    CHECK(s.offset >= end, "%s: span %zu at %lld overlaps the one before (ends %lld)", what, k, (long long)s.offset, (long long)end);
    end = s.offset + s.length;
  }
  CHECK(lay.body_size == (end + 63) / 64 * 64, "%s: body of %lld bytes, last span ends at %lld", what, (long long)lay.body_size, (long long)end);
}

void CheckLayouts() {
  for (int64_t n : {0, 1, 7, 8, 9, 2048, 2049}) {
    const std::string rows = " of " + std::to_string(n) + " rows";
    for (int64_t width : {1, 2, 4, 8, 16}) CheckLayout(("copy" + rows).c_str(), {EncodeNode{MI_K_ENC_COPY, width, false, n, 0}});
    for (int64_t width : {2, 4, 8}) CheckLayout(("decimal" + rows).c_str(), {EncodeNode{MI_K_ENC_DEC128, width, false, n, 0}});
    CheckLayout(("bool" + rows).c_str(), {EncodeNode{MI_K_ENC_BOOL, 1, false, n, 0}});
    for (bool large : {false, true}) {
      CheckLayout(("string" + rows).c_str(), {EncodeNode{MI_K_ENC_STR32, 0, large, n, n * 5 + (n ? 3 : 0)}});
      // a list over a string child: 3 child rows per list
      CheckLayout(("list" + rows).c_str(), {EncodeNode{MI_K_ENC_LIST32, 0, large, n, 3 * n}, EncodeNode{MI_K_ENC_STR32, 0, large, 3 * n, 21 * n}});
    }
    CheckLayout(("struct" + rows).c_str(),
                {EncodeNode{MI_K_ENC_VALIDITY, 0, false, n, 0}, EncodeNode{MI_K_ENC_COPY, 4, false, n, 0}, EncodeNode{MI_K_ENC_BOOL, 1, false, n, 0},
                 EncodeNode{MI_K_ENC_COPY, 8, false, n, 0}});
  }
  // int32 offsets end at INT32_MAX (no buffer of that size is made: the layout is arithmetic)
  const int64_t big = 2147483648ll;
  BodyLayout lay;
  std::string message;
  try {
    LayOutBody({EncodeNode{MI_K_ENC_STR32, 0, false, 10, big}}, &lay);
  } catch (const InvalidInputException& e) {
    message = e.what();
  }
  CHECK(message == "Arrow Appender: The maximum total string size for regular string buffers is 2147483647 but the offset of 2147483648 exceeds "
                   "this.\n* SET arrow_large_buffer_size=true to use large string buffers",
        "2 GiB of strings behind int32 offsets: \"%s\"", message.c_str());
  LayOutBody({EncodeNode{MI_K_ENC_STR32, 0, false, 10, big - 1}}, &lay);
  CHECK(lay.spans.size() == 3 && lay.spans[2].length == big - 1, "INT32_MAX string bytes behind int32 offsets");
  LayOutBody({EncodeNode{MI_K_ENC_STR32, 0, true, 10, big}}, &lay);
  CHECK(lay.spans.size() == 3 && lay.spans[1].length == 88 && lay.spans[2].length == big, "2 GiB of strings behind int64 offsets");

  // the task of a string node points where the layout says
  uint8_t* body = reinterpret_cast<uint8_t*>(uintptr_t{1} << 40);
  const uint8_t in[4] = {0, 0, 0, 0};
  const EncodeNode str{MI_K_ENC_STR32, 0, true, 9, 77};
  LayOutBody({EncodeNode{MI_K_ENC_COPY, 8, false, 9, 0}, str}, &lay);
  const mi_col_task t = EncodeTask(str, &lay.spans[static_cast<size_t>(lay.first_span[1])], EncodeInput{in, in + 1, in + 2, 4096}, body);
  CHECK(t.kind == MI_K_ENC_STR32 && t.nrows == 9 && t.flags == 1 && t.buf1 == in && t.validity == in + 1 && t.buf2 == in + 2 && t.ptr_base == 4096 &&
            t.buf2_len == 77 && t.out_validity == body + lay.spans[2].offset && t.out_data == body + lay.spans[3].offset &&
            t.out_aux == body + lay.spans[4].offset,
        "encode task of a string node");
}

// ------------------------------------------------------------------------------------------------ cut rule
std::vector<int64_t> NaiveGroups(const std::vector<int64_t>& batches, int64_t max_rows, int64_t row_bytes, int64_t max_bytes) {
  std::vector<int64_t> groups;
  int64_t cur = 0;
  for (int64_t rows : batches) {
    for (int64_t r = 0; r < rows; r += MI_VECTOR_SIZE) {
      cur += std::min<int64_t>(MI_VECTOR_SIZE, rows - r);
      if (cur >= max_rows || cur * row_bytes >= max_bytes) {
        groups.push_back(cur);
        cur = 0;
      }
    }
  }
  if (cur > 0) groups.push_back(cur);
  return groups;
}

void CheckCut(const char* what, const std::vector<int64_t>& batches, int64_t max_rows, int64_t row_bytes, int64_t max_bytes) {
  mi_write_options o;
  std::memset(&o, 0, sizeof(o));
  o.row_group_size = max_rows;
  o.row_group_size_bytes = max_bytes;
  RowGroupCutter cutter(RowsPerGroup(o, row_bytes));
  std::vector<int64_t> groups;
  int64_t cur = 0;
  for (int64_t rows : batches) {
    int32_t next_window = 0;
    for (const CutPiece& pc : cutter.Cut(rows)) {
      CHECK(pc.window0 == next_window && pc.window1 > pc.window0, "%s: piece [%d, %d) after window %d", what, pc.window0, pc.window1, next_window);
      CHECK(pc.starts_group == (cur == 0), "%s: starts_group %d with %lld rows open", what, pc.starts_group, (long long)cur);
      next_window = pc.window1;
      cur += std::min<int64_t>(rows, static_cast<int64_t>(pc.window1) * MI_VECTOR_SIZE) - static_cast<int64_t>(pc.window0) * MI_VECTOR_SIZE;
      if (pc.closes_group) {
        groups.push_back(cur);
        cur = 0;
      }
    }
    CHECK(next_window == (rows + MI_VECTOR_SIZE - 1) / MI_VECTOR_SIZE, "%s: a batch of %lld rows cut up to window %d", what, (long long)rows, next_window);
    CHECK(cutter.OpenRows() == cur, "%s: %lld rows open, the cutter says %lld", what, (long long)cur, (long long)cutter.OpenRows());
  }
  if (cur > 0) groups.push_back(cur);
  const std::vector<int64_t> want = NaiveGroups(batches, max_rows, row_bytes, max_bytes);
  CHECK(groups == want, "%s: %zu row groups, the naive cut has %zu", what, groups.size(), want.size());
  int64_t total = 0, sum = 0;
  for (int64_t r : batches) total += r;
  for (int64_t g : groups) sum += g;
  CHECK(sum == total, "%s: row groups hold %lld of %lld rows", what, (long long)sum, (long long)total);
}

std::vector<int64_t> Batches(int64_t total, int64_t chunk) {
  std::vector<int64_t> out;
  for (int64_t r = 0; r < total; r += chunk) out.push_back(std::min(chunk, total - r));
  return out;
}

void CheckCuts() {
  const int64_t pairs[5][2] = {{9000, 9000}, {25000, 8192}, {3000, 10000}, {7001, 5000}, {70000, 20000}};
  for (auto& p : pairs) CheckCut(("70000 rows in batches of " + std::to_string(p[0])).c_str(), Batches(70000, p[0]), p[1], 40, p[1] * 1024);
  CheckCut("130 batches of 1000 rows", Batches(130000, 1000), 40960, 28, 40960 * 1024);
  // row_group_size_bytes binds: 28-byte rows reach 100000 bytes at 3572 rows
  CheckCut("bytes bound", {12000, 12000, 6000}, 122880, 28, 100000);
  CHECK(NaiveGroups({12000, 12000, 6000}, 122880, 28, 100000) == (std::vector<int64_t>{4096, 4096, 3808, 4096, 4096, 3808, 4096, 1904}), "bytes bound: naive groups");
  CheckCut("empty batches in between", {0, 5000, 0, 0, 100, 4096, 0}, 4096, 8, 1 << 30);
}

// ------------------------------------------------------------------------------------------------ ledger
struct LedgerRun {
  static constexpr int kTokens = 400;
  std::mutex mu;
  std::condition_variable cv;
  std::exception_ptr error;
  std::vector<int> work;     // tokens of open pieces the closers may take (under mu)
  bool done = false;
  std::atomic<int> open[kTokens];
  std::atomic<bool> cut[kTokens];
  std::atomic<int> released[kTokens];
  std::atomic<int> wrong_thread{0}, too_early{0};
  const std::thread::id pump = std::this_thread::get_id();
  BatchLedger<int> ledger{mu, cv, error, [this](const int& ref) {
                            const int tok = ref / 7;
                            if (std::this_thread::get_id() != pump) wrong_thread++;
                            if (!cut[tok] || open[tok] != 0) too_early++;
                            released[tok]++;
                          }};
  std::vector<std::thread> closers;

  LedgerRun() {
    for (int i = 0; i < kTokens; i++) {
      open[i] = 0;
      cut[i] = false;
      released[i] = 0;
    }
  }
  void StartClosers() {
    for (int t = 0; t < 4; t++) {
      closers.emplace_back([this, t] {
        std::mt19937 rng(static_cast<unsigned>(100 + t));
        while (true) {
          int tok;
          {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return done || !work.empty(); });
            if (work.empty()) return;
            const size_t k = rng() % work.size();   // any open piece, not the oldest
            tok = work[k];
            work[k] = work.back();
            work.pop_back();
          }
          open[tok]--;
          ledger.ClosePiece(tok);
        }
      });
    }
  }
  //! holds token `tok` and cuts it into `pieces` pieces, `offered` of which the closers get to see
  void HoldAndCut(int tok, int pieces, int offered) {
    const int got = ledger.Hold(tok * 7);
    CHECK(got == tok && ledger.RefOf(tok) == tok * 7, "token %d held as %d", tok, got);
    for (int p = 0; p < pieces; p++) {
      open[tok]++;
      ledger.OpenPiece(tok);
      if (p >= offered) continue;
      {
        std::lock_guard<std::mutex> lk(mu);
        work.push_back(tok);
      }
      cv.notify_all();
    }
    cut[tok] = true;
    ledger.MarkFullyCut(tok);
  }
  void JoinClosers() {
    {
      std::lock_guard<std::mutex> lk(mu);
      done = true;
    }
    cv.notify_all();
    for (auto& t : closers) t.join();
  }
};

void CheckLedger() {
  {
    LedgerRun run;
    run.StartClosers();
    std::mt19937 rng(7);
    for (int tok = 0; tok < LedgerRun::kTokens; tok++) {
      const int pieces = static_cast<int>(rng() % 4);
      run.HoldAndCut(tok, pieces, pieces);
      run.ledger.ReleaseReady(false);
      while (run.ledger.Unreleased() > 8) run.ledger.ReleaseReady(true);   // a scan with 8 slots
    }
    while (run.ledger.Unreleased() > 0) run.ledger.ReleaseReady(true);
    run.JoinClosers();
    int not_once = 0;
    for (int tok = 0; tok < LedgerRun::kTokens; tok++) not_once += run.released[tok] != 1;
    CHECK(not_once == 0, "ledger: %d of %d batches not released exactly once", not_once, LedgerRun::kTokens);
    CHECK(run.wrong_thread == 0, "ledger: %d releases off the pump thread", run.wrong_thread.load());
    CHECK(run.too_early == 0, "ledger: %d batches released before they were fully cut and closed", run.too_early.load());
    run.ledger.ReleaseAll();
    for (int tok = 0; tok < LedgerRun::kTokens; tok++) not_once += run.released[tok] != 1;
    CHECK(not_once == 0, "ledger: ReleaseAll released %d batches again", not_once);
  }
  {
    // a failure with pieces still open: ReleaseReady rethrows it, ReleaseAll gives back what is left
    LedgerRun run;
    run.StartClosers();
    for (int tok = 0; tok < 40; tok++) run.HoldAndCut(tok, 2, tok % 3);   // one in three closes completely ...
    run.ledger.Hold(40 * 7);                                             // ... and one is not even cut
    {
      std::lock_guard<std::mutex> lk(run.mu);
      run.error = std::make_exception_ptr(IOException("disk full"));
    }
    run.cv.notify_all();
    std::string message;
    try {
      run.ledger.ReleaseReady(true);
    } catch (const IOException& e) {
      message = e.what();
    }
    CHECK(message == "disk full", "ledger: ReleaseReady after a failure threw \"%s\"", message.c_str());
    run.JoinClosers();
    for (int tok = 0; tok <= 40; tok++) {   // the way out: whatever is open counts as closed
      run.open[tok] = 0;
      run.cut[tok] = true;
    }
    run.ledger.ReleaseAll();
    int not_once = 0;
    for (int tok = 0; tok <= 40; tok++) not_once += run.released[tok] != 1;
    CHECK(not_once == 0, "ledger: after a failure %d of 41 batches not released exactly once", not_once);
    CHECK(run.wrong_thread == 0 && run.ledger.Unreleased() == 0, "ledger: after a failure %lld batches still held", (long long)run.ledger.Unreleased());
  }
}
}  // namespace

int main() {
  CheckLayouts();
  CheckCuts();
  CheckLedger();
  std::printf("writer_plan_check: %d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
