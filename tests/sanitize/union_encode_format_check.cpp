// union_encode_format_check.cpp -- the encode rules of union_format.hpp (EncodeRow, WithPadBits) alone, under ASan + UBSan:
// g++ -std=c++17 -fsanitize=address,undefined -I duckdb-arrow_amd/csrc tests/sanitize/union_encode_format_check.cpp
// Every (tag, m, validity) combination against the rule spelled out here, and whole unions run the way encode_union runs
// them -- member index from EncodeRow alone, masks in arrays of exactly m x words, so a tag used unclamped is a heap overflow.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "union_format.hpp"

using namespace miarrow::unionfmt;

static int failed = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (failed++ < 20) {                                 \
        std::fprintf(stderr, "FAILED %s: ", #cond);        \
        std::fprintf(stderr, __VA_ARGS__);                 \
        std::fprintf(stderr, "\n");                        \
      }                                                    \
    }                                                      \
  } while (0)

static void CheckEveryRow() {
  for (int m = 1; m <= kMaxMembers; m++) {
    for (int tag = 0; tag < 256; tag++) {
      for (int valid = 0; valid < 2; valid++) {
        const EncodedRow r = EncodeRow(tag, m, valid != 0);
        CHECK(r.member >= 0 && r.member < m, "member %d of %d for tag %d", r.member, m, tag);
        CHECK(r.type_id >= 0 && r.type_id < m, "type id %d of %d for tag %d", r.type_id, m, tag);
        if (!valid) {
          CHECK(r.type_id == 0 && !r.selects && r.status == 0u, "a NULL row: id %d selects %d status %u", r.type_id, r.selects, r.status);
        } else if (tag >= m) {
          CHECK(r.type_id == 0 && r.member == 0 && !r.selects && r.status == kStBadTag, "tag %d of %d members", tag, m);
        } else {
          CHECK(r.type_id == tag && r.member == tag && r.selects && r.status == 0u, "tag %d of %d members", tag, m);
        }
      }
    }
  }
  for (int tag : {-1, -128, 256, 1 << 20}) {
    const EncodedRow r = EncodeRow(tag, 3, true);
    CHECK(r.member == 0 && r.type_id == 0 && !r.selects && r.status == kStBadTag, "tag %d", tag);
  }
}

static void CheckPadBits() {
  CHECK(WithPadBits(0, 64, 0) == 0 && WithPadBits(5, 128, 1) == 5, "whole words keep their bits");
  CHECK(WithPadBits(0, 1, 0) == ~1ull && WithPadBits(1, 1, 0) == ~0ull, "one row");
  CHECK(WithPadBits(0, 63, 0) == 1ull << 63 && WithPadBits(0, 65, 1) == ~1ull, "63 and 65 rows");
  CHECK(WithPadBits(0, 64, 1) == ~0ull && WithPadBits(7, 0, 0) == ~0ull, "a word behind the last row is all pad");
  for (int64_t n : {1, 63, 64, 65, 2047, 2048, 2049}) {
    const int64_t words = (n + 63) / 64;
    int64_t zeros = 0;
    for (int64_t j = 0; j < words; j++) zeros += 64 - __builtin_popcountll(WithPadBits(0, n, j));
    CHECK(zeros == n, "%lld rows leave %lld zero bits", (long long)n, (long long)zeros);
  }
}

// a whole union the way the kernel and the writer's staging go through it
static void CheckWholeUnions() {
  std::mt19937_64 rng(42);
  for (int m : {1, 2, 5, 32}) {
    for (int64_t n : {1, 63, 64, 65, 2049, 4097}) {
      for (int damaged = 0; damaged < 2; damaged++) {
        const int64_t words = (n + 63) / 64;
        std::vector<uint8_t> tags(static_cast<size_t>(n));
        std::vector<uint64_t> uw(static_cast<size_t>(words));
        std::vector<std::vector<uint64_t>> own(static_cast<size_t>(m), std::vector<uint64_t>(static_cast<size_t>(words)));
        for (auto& t : tags) t = static_cast<uint8_t>(damaged && rng() % 50 == 0 ? m + rng() % (256 - m) : rng() % m);
        for (auto& w : uw) w = rng() | rng();
        for (auto& o : own)
          for (auto& w : o) w = rng() | rng();
        std::vector<int8_t> ids(static_cast<size_t>(n));
        std::vector<uint64_t> masks(static_cast<size_t>(m * words));   // exactly: an unclamped member index leaves it
        for (int k = 0; k < m; k++)
          for (int64_t j = 0; j < words; j++) masks[static_cast<size_t>(k * words + j)] = WithPadBits(0, n, j);
        uint32_t status = 0;
        for (int64_t r = 0; r < n; r++) {
          const bool valid = (uw[static_cast<size_t>(r >> 6)] >> (r & 63)) & 1;
          const EncodedRow row = EncodeRow(tags[static_cast<size_t>(r)], m, valid);
          ids[static_cast<size_t>(r)] = static_cast<int8_t>(row.type_id);
          status |= row.status;
          const bool bit = row.selects && ((own[static_cast<size_t>(row.member)][static_cast<size_t>(r >> 6)] >> (r & 63)) & 1);
          if (bit) masks[static_cast<size_t>(row.member * words + (r >> 6))] |= 1ull << (r & 63);
        }
        // every row is in one mask at most, and only in the mask of its type id; the masks' zero bits are the members' NULLs
        int64_t set = 0, bad = 0;
        for (int64_t r = 0; r < n; r++) {
          int in = 0;
          for (int k = 0; k < m; k++) {
            const bool bit = (masks[static_cast<size_t>(k * words + (r >> 6))] >> (r & 63)) & 1;
            in += bit;
            if (bit) CHECK(ids[static_cast<size_t>(r)] == k && tags[static_cast<size_t>(r)] == k, "row %lld in mask %d has id %d", (long long)r, k, ids[static_cast<size_t>(r)]);
          }
          CHECK(in <= 1, "row %lld is in %d masks", (long long)r, in);
          set += in;
          const bool valid = (uw[static_cast<size_t>(r >> 6)] >> (r & 63)) & 1;
          bad += valid && tags[static_cast<size_t>(r)] >= m;
          if (!valid || tags[static_cast<size_t>(r)] >= m) CHECK(in == 0 && ids[static_cast<size_t>(r)] == 0, "row %lld", (long long)r);
        }
        CHECK((status == kStBadTag) == (bad > 0), "status %u with %lld damaged rows", status, (long long)bad);
        CHECK(set <= n, "%lld bits", (long long)set);
      }
    }
  }
}

int main() {
  CheckEveryRow();
  CheckPadBits();
  CheckWholeUnions();
  if (failed) {
    std::fprintf(stderr, "union_encode_format: %d checks failed\n", failed);
    return 1;
  }
  std::printf("union_encode_format: ok\n");
  return 0;
}
