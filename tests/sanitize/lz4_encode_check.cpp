// lz4_encode_check.cpp -- the writer's LZ4 compressor without a GPU, under AddressSanitizer + UBSan (test infrastructure,
// never shipped).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I include tests/sanitize/lz4_encode_check.cpp
//       duckdb-arrow_amd/csrc/{writer_plan,ipc_format,io_pool,host_codec,frame_walk,batch_slice,ipc_stream_reader}.cpp -ldl -lpthread -o lz4_encode_check
//
// Runs the serial restatement of the compress kernel (lz4_encode_format.hpp: CompressBlockSerial, CompressBufferSerial)
// and the body layout (writer_plan.cpp: BlocksOfBody, LayOutCompressedBody) over buffers of every length at which the
// format changes its mind and of every content that reaches one of its rules.  For every case: each block's output is
// within its bound, obeys the end-of-block rules and liblz4's block decoder turns it back into the block (alone: a match
// across a block boundary cannot decode); liblz4's frame decoder turns the buffer's frame back into the buffer; the buffer
// sits in the laid-out body where its span says, on a multiple of 8, with zero padding, equal to CompressBufferSerial's
// bytes; and the host reader (IPCBufferStreamReader -> DecompressBody) reads the record batch back.
#include <dlfcn.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../duckdb-arrow_amd/csrc/ipc_stream_reader.hpp"
#include "../../duckdb-arrow_amd/csrc/writer_plan.hpp"

using namespace miarrow;
using namespace miarrow::lz4enc;

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

struct Lz4Lib {
  int (*block)(const char*, char*, int, int) = nullptr;
  size_t (*create)(void**, unsigned) = nullptr;
  size_t (*free_ctx)(void*) = nullptr;
  size_t (*decompress)(void*, void*, size_t*, const void*, size_t*, const void*) = nullptr;
  unsigned (*is_error)(size_t) = nullptr;
} g_lz4;

bool LoadLz4() {
  void* h = dlopen("liblz4.so.1", RTLD_NOW | RTLD_LOCAL);
  if (!h) return false;
  g_lz4.block = reinterpret_cast<int (*)(const char*, char*, int, int)>(dlsym(h, "LZ4_decompress_safe"));
  g_lz4.create = reinterpret_cast<size_t (*)(void**, unsigned)>(dlsym(h, "LZ4F_createDecompressionContext"));
  g_lz4.free_ctx = reinterpret_cast<size_t (*)(void*)>(dlsym(h, "LZ4F_freeDecompressionContext"));
  g_lz4.decompress = reinterpret_cast<size_t (*)(void*, void*, size_t*, const void*, size_t*, const void*)>(dlsym(h, "LZ4F_decompress"));
  g_lz4.is_error = reinterpret_cast<unsigned (*)(size_t)>(dlsym(h, "LZ4F_isError"));
  return g_lz4.block && g_lz4.create && g_lz4.free_ctx && g_lz4.decompress && g_lz4.is_error;
}

bool FrameDecodesTo(const uint8_t* frame, size_t frame_len, const std::vector<uint8_t>& want) {
  void* ctx = nullptr;
  if (g_lz4.is_error(g_lz4.create(&ctx, 100))) return false;
  std::vector<uint8_t> got(want.size() + 1);
  size_t produced = 0, consumed = 0, rc = 1;
  while (rc != 0) {
    size_t dn = got.size() - produced, sn = frame_len - consumed;
    rc = g_lz4.decompress(ctx, got.data() + produced, &dn, frame + consumed, &sn, nullptr);
    if (g_lz4.is_error(rc) || (dn == 0 && sn == 0)) break;
    produced += dn;
    consumed += sn;
  }
  g_lz4.free_ctx(ctx);
  return rc == 0 && consumed == frame_len && produced == want.size() && std::memcmp(got.data(), want.data(), want.size()) == 0;
}

struct Rng {
  uint64_t s;
  uint32_t Next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<uint32_t>(s >> 33);
  }
  uint8_t Byte() { return static_cast<uint8_t>(Next() >> 7); }
};

// the sequences of a compressed block: literal counts and {start, length} of the matches; false when it is malformed
struct Parsed {
  std::vector<uint32_t> literals;
  std::vector<std::pair<uint32_t, uint32_t>> matches;
};
bool ParseBlock(const uint8_t* p, uint32_t size, uint32_t n, Parsed* out) {
  uint32_t at = 0, pos = 0;
  while (true) {
    if (at >= size) return false;
    const uint8_t token = p[at++];
    uint32_t lit = token >> 4;
    if (lit == 15) {
      uint8_t b;
      do {
        if (at >= size) return false;
        b = p[at++];
        lit += b;
      } while (b == 255);
    }
    out->literals.push_back(lit);
    at += lit;
    pos += lit;
    if (at > size) return false;
    if (at == size) return pos == n && (token & 15) == 0;   // the last sequence is literals only
    if (at + 2 > size) return false;
    const uint32_t offset = p[at] | p[at + 1] << 8;
    at += 2;
    uint32_t len = (token & 15) + kMinMatch;
    if ((token & 15) == 15) {
      uint8_t b;
      do {
        if (at >= size) return false;
        b = p[at++];
        len += b;
      } while (b == 255);
    }
    if (offset == 0 || offset > pos) return false;
    out->matches.push_back({pos, len});
    pos += len;
  }
}

struct Totals {
  int cases = 0, blocks = 0, stored = 0, raw_buffers = 0, framed_buffers = 0;
  std::set<uint32_t> literal_runs, match_lengths;
} g_totals;

enum Expect { kAny, kRaw, kFramed };

void CheckBuffer(const std::string& what, const std::vector<uint8_t>& data, Expect expect) {
  g_totals.cases++;
  const int64_t n = static_cast<int64_t>(data.size());
  std::vector<uint32_t> table(kHashSize);
  // ---- block by block
  std::vector<uint32_t> words;
  std::vector<uint8_t> slots(static_cast<size_t>(BlocksOf(n)) * kSlotStride);
  for (int64_t b = 0; b < BlocksOf(n); b++) {
    const uint8_t* src = data.data() + b * kBlockSize;
    const uint32_t bn = static_cast<uint32_t>(std::min<int64_t>(kBlockSize, n - b * kBlockSize));
    std::vector<uint8_t> out(BlockBound(bn));   // exactly the bound: ASan sees a byte past it
    const uint32_t word = CompressBlockSerial(src, bn, out.data(), table.data());
    words.push_back(word);
    g_totals.blocks++;
    if (word & kStoredFlag) {
      g_totals.stored++;
      CHECK((word & ~kStoredFlag) == bn, "%s block %lld: stored size %u of %u", what.c_str(), (long long)b, word & ~kStoredFlag, bn);
      continue;
    }
    CHECK(word < bn && word <= BlockBound(bn), "%s block %lld: %u bytes from %u", what.c_str(), (long long)b, word, bn);
    CHECK(!TooShort(bn), "%s block %lld: %u bytes compressed", what.c_str(), (long long)b, bn);
    std::vector<uint8_t> back(bn);
    const int got = g_lz4.block(reinterpret_cast<const char*>(out.data()), reinterpret_cast<char*>(back.data()), static_cast<int>(word), static_cast<int>(bn));
    CHECK(got == static_cast<int>(bn) && std::memcmp(back.data(), src, bn) == 0, "%s block %lld: liblz4 gives %d bytes", what.c_str(), (long long)b, got);
    Parsed seq;
    CHECK(ParseBlock(out.data(), word, bn, &seq), "%s block %lld: malformed sequences", what.c_str(), (long long)b);
    for (auto& m : seq.matches) {
      CHECK(m.first + kMatchStartGap <= bn, "%s block %lld: match starts at %u of %u", what.c_str(), (long long)b, m.first, bn);
      CHECK(m.first + m.second + kLastLiterals <= bn, "%s block %lld: match ends at %u of %u", what.c_str(), (long long)b, m.first + m.second, bn);
      g_totals.match_lengths.insert(m.second);
    }
    for (size_t i = 0; i + 1 < seq.literals.size(); i++) g_totals.literal_runs.insert(seq.literals[i]);
    std::memcpy(slots.data() + static_cast<size_t>(b) * kSlotStride, out.data(), word);
  }
  // ---- the buffer as the file holds it
  std::vector<uint8_t> buf(static_cast<size_t>(BufferBound(n)));
  std::vector<uint8_t> block_out(BlockBound(kBlockSize));
  CHECK(CompressBufferSerial(data.data(), n, buf.data(), static_cast<int64_t>(buf.size()) - 1, block_out.data(), table.data()) == (n ? -1 : 0),
        "%s: a short output buffer is not refused", what.c_str());
  const int64_t size = CompressBufferSerial(data.data(), n, buf.data(), static_cast<int64_t>(buf.size()), block_out.data(), table.data());
  bool raw = false;
  if (n == 0) {
    CHECK(size == 0, "%s: empty buffer takes %lld bytes", what.c_str(), (long long)size);
  } else {
    int64_t prefix;
    std::memcpy(&prefix, buf.data(), 8);
    raw = prefix == -1;
    if (raw) {
      g_totals.raw_buffers++;
      CHECK(size == 8 + n && std::memcmp(buf.data() + 8, data.data(), data.size()) == 0, "%s: raw form differs", what.c_str());
      CHECK(FrameSize(words.data(), static_cast<int64_t>(words.size())) >= n, "%s: raw although the frame is smaller", what.c_str());
    } else {
      g_totals.framed_buffers++;
      CHECK(prefix == n && size < 8 + n, "%s: prefix %lld, %lld bytes for %lld", what.c_str(), (long long)prefix, (long long)size, (long long)n);
      CHECK(FrameDecodesTo(buf.data() + 8, static_cast<size_t>(size - 8), data), "%s: liblz4 does not read the frame back", what.c_str());
      const uint8_t head[7] = {0x04, 0x22, 0x4D, 0x18, 0x60, 0x40, 0x82};
      CHECK(std::memcmp(buf.data() + 8, head, 7) == 0, "%s: frame header", what.c_str());
    }
    CHECK(expect == kAny || (expect == kRaw) == raw, "%s: expected %s", what.c_str(), expect == kRaw ? "raw" : "a frame");
    if (expect == kRaw)
      for (uint32_t w : words) CHECK(w & kStoredFlag, "%s: a block of it is not stored", what.c_str());
  }
  // ---- a record batch of one BLOB row holding it: layout, compaction (restated with memcpy), and the host reader
  std::vector<EncodeNode> nodes = {EncodeNode{MI_K_ENC_STR32, 0, false, 1, n}, EncodeNode{MI_K_ENC_COPY, 1, false, n, 0}};
  BodyLayout plain;
  LayOutBody(nodes, &plain);
  std::vector<uint8_t> body(static_cast<size_t>(plain.body_size), 0);
  body[static_cast<size_t>(plain.spans[0].offset)] = 1;
  const int32_t offsets[2] = {0, static_cast<int32_t>(n)};
  std::memcpy(body.data() + plain.spans[1].offset, offsets, 8);
  if (n) std::memcpy(body.data() + plain.spans[2].offset, data.data(), data.size());
  if (n) std::memset(body.data() + plain.spans[3].offset, 0xFF, static_cast<size_t>(plain.spans[3].length));
  if (n) std::memcpy(body.data() + plain.spans[4].offset, data.data(), data.size());   // the same bytes as an int8 column
  const std::vector<BlockIn> blocks = BlocksOfBody(plain);
  std::vector<uint32_t> body_words;
  std::vector<uint8_t> body_slots(blocks.size() * static_cast<size_t>(kSlotStride));
  for (size_t b = 0; b < blocks.size(); b++) {
    CHECK(blocks[b].n >= 1 && blocks[b].n <= kBlockSize && blocks[b].in_off % 64 == 0 && blocks[b].in_off + blocks[b].n <= body.size(),
          "%s: block %zu lies at %llu + %u", what.c_str(), b, (unsigned long long)blocks[b].in_off, blocks[b].n);
    body_words.push_back(CompressBlockSerial(body.data() + blocks[b].in_off, blocks[b].n, body_slots.data() + b * kSlotStride, table.data()));
  }
  CompressedBodyLayout packed;
  LayOutCompressedBody(plain, body_words, &packed);
  CHECK(packed.body_size % 8 == 0 && packed.spans.size() == plain.spans.size(), "%s: body of %lld bytes", what.c_str(), (long long)packed.body_size);
  std::vector<uint8_t> out(static_cast<size_t>(packed.body_size), 0);
  std::vector<uint8_t> covered(out.size(), 0);
  for (const BodyCopy& c : packed.copies) {
    CHECK(c.dst >= 0 && c.dst + c.len <= packed.body_size, "%s: copy to %lld + %u", what.c_str(), (long long)c.dst, c.len);
    if (c.dst < 0 || c.dst + c.len > packed.body_size) continue;
    if (c.from == kFromImmediate) {
      CHECK(c.len <= 8, "%s: immediate of %u bytes", what.c_str(), c.len);
      for (uint32_t i = 0; i < c.len && i < 8; i++) out[static_cast<size_t>(c.dst) + i] = static_cast<uint8_t>(c.imm >> (8 * i));
    } else {
      const std::vector<uint8_t>& from = c.from == kFromSlots ? body_slots : body;
      CHECK(c.src >= 0 && static_cast<size_t>(c.src) + c.len <= from.size() && c.len <= kBlockSize, "%s: copy from %lld + %u", what.c_str(), (long long)c.src, c.len);
      if (c.src >= 0 && static_cast<size_t>(c.src) + c.len <= from.size()) std::memcpy(out.data() + c.dst, from.data() + c.src, c.len);
    }
    for (uint32_t i = 0; i < c.len; i++) covered[static_cast<size_t>(c.dst) + i]++;
  }
  int64_t end = 0;
  for (size_t i = 0; i < packed.spans.size(); i++) {
    const mi_buffer_span& sp = packed.spans[i];
    CHECK(sp.offset % 8 == 0 && sp.offset >= end && SpanInside(sp.offset, sp.length, packed.body_size), "%s: buffer %zu at %lld + %lld", what.c_str(), i,
          (long long)sp.offset, (long long)sp.length);
    CHECK((sp.length == 0) == (plain.spans[i].length == 0), "%s: buffer %zu: %lld bytes from %lld", what.c_str(), i, (long long)sp.length, (long long)plain.spans[i].length);
    bool once = true;
    for (int64_t k = 0; k < sp.length; k++) once &= covered[static_cast<size_t>(sp.offset + k)] == 1;
    CHECK(once, "%s: buffer %zu is not written exactly once", what.c_str(), i);
    end = sp.offset + sp.length;
  }
  bool padding_zero = true;
  for (size_t k = 0; k < out.size(); k++) padding_zero &= covered[k] != 0 || out[k] == 0;
  CHECK(padding_zero && end <= packed.body_size && packed.body_size - end < 8, "%s: padding", what.c_str());
  for (int which : {2, 4}) {   // the BLOB's data buffer and the int8 column's: CompressBufferSerial's bytes
    const mi_buffer_span& sp = packed.spans[static_cast<size_t>(which)];
    CHECK(sp.length == size && (size == 0 || std::memcmp(out.data() + sp.offset, buf.data(), static_cast<size_t>(size)) == 0),
          "%s: buffer %d of the body differs from the buffer compressed alone", what.c_str(), which);
  }
  ArrowSchemaModel schema;
  schema.fields = {FieldFromDuckType("b", "BLOB"), FieldFromDuckType("t", "TINYINT")};
  // the reader takes one length per record batch: the int8 column rides along in a batch of its own
  for (int which = 0; which < 2; which++) {
    ArrowSchemaModel one;
    one.fields = {schema.fields[static_cast<size_t>(which)]};
    std::vector<uint8_t> s1 = EncodeSchemaMessage(one);
    const size_t first = which == 0 ? 0 : 3, count = which == 0 ? 3 : 2;
    std::vector<mi_buffer_span> spans(packed.spans.begin() + static_cast<long>(first), packed.spans.begin() + static_cast<long>(first + count));
    const int64_t rows = which == 0 ? 1 : n;
    const std::vector<uint8_t> msg = EncodeRecordBatchMessage(rows, {{rows, 0}}, spans, packed.body_size, 0);
    s1.insert(s1.end(), msg.begin(), msg.end());
    s1.insert(s1.end(), out.begin(), out.end());
    const uint8_t eos[8] = {0xFF, 0xFF, 0xFF, 0xFF, 0, 0, 0, 0};
    s1.insert(s1.end(), eos, eos + 8);
    try {
      IPCBufferStreamReader reader({ArrowIPCBuffer(reinterpret_cast<uint64_t>(s1.data()), s1.size())});
      DecodedBatch batch;
      const bool got = reader.GetNextBatch(&batch);
      CHECK(got && batch.length == rows && batch.compression == -1, "%s: the reader returns no batch", what.c_str());
      if (got) {
        const mi_buffer_span& sp = batch.buffers[which == 0 ? 2 : 1];
        CHECK(sp.length == n && (n == 0 || std::memcmp(batch.body + sp.offset, data.data(), data.size()) == 0), "%s: the reader's bytes differ (column %d)",
              what.c_str(), which);
      }
      CHECK(!reader.GetNextBatch(&batch), "%s: a second batch", what.c_str());
    } catch (const std::exception& e) {
      CHECK(false, "%s: the reader throws: %s", what.c_str(), e.what());
    }
  }
}

std::vector<uint8_t> Periodic(size_t n, size_t period, Rng& rng) {
  std::vector<uint8_t> unit(period), v(n);
  for (auto& b : unit) b = rng.Byte();
  for (size_t i = 0; i < n; i++) v[i] = unit[i % period];
  return v;
}
std::vector<uint8_t> Random(size_t n, Rng& rng) {
  std::vector<uint8_t> v(n);
  for (auto& b : v) b = rng.Byte();
  return v;
}
std::vector<uint8_t> Text(size_t n, Rng& rng) {
  const char* words[] = {"carefully", "final", "deposits", "furiously", "quickly", "express", "packages", "sleep", "blithely", "regular"};
  std::vector<uint8_t> v;
  while (v.size() < n) {
    const char* w = words[rng.Next() % 10];
    v.insert(v.end(), w, w + std::strlen(w));
    v.push_back(' ');
  }
  v.resize(n);
  return v;
}
}  // namespace

int main() {
  if (!LoadLz4()) {
    std::printf("liblz4.so.1 not available\n");
    return 77;
  }
  Rng rng{12345};
  const size_t lengths[] = {0, 1, 4, 5, 12, 13, 14, 64, 65, 65535, 65536, 65537, 3 * 65536 + 7};
  for (size_t n : lengths) {
    const std::string tag = " of " + std::to_string(n);
    CheckBuffer("zeros" + tag, std::vector<uint8_t>(n, 0), n >= 128 ? kFramed : kAny);
    // (a period of 65535 repeats one byte inside a 64 KiB block: the blocks are independent, nothing can match)
    for (size_t period : {2, 3, 4, 7, 65535})
      CheckBuffer("period " + std::to_string(period) + tag, Periodic(n, period, rng), period == 65535 ? (n ? kRaw : kAny) : n >= 128 ? kFramed : kAny);
    CheckBuffer("random" + tag, Random(n, rng), n ? kRaw : kAny);
    CheckBuffer("text" + tag, Text(n, rng), n >= 65535 ? kFramed : kAny);
  }
  // match lengths around the token's 15 and the first two extension bytes: the match of an all-zero block starts at 64
  // (the first group has no candidates) and ends 5 bytes before the block does
  for (uint32_t len : {18, 19, 20, 273, 274, 275, 528, 529, 530}) {
    g_totals.match_lengths.clear();
    CheckBuffer("zeros with a match of " + std::to_string(len), std::vector<uint8_t>(64 + len + 5, 0), kAny);
    CHECK(g_totals.match_lengths.count(len) == 1, "no match of %u bytes in the all-zero block", len);
  }
  // literal runs of exactly 14, 15, 269 and 270 bytes between two matches: copies of one 40-byte phrase with fresh bytes
  // between them.  A match runs on into what follows the copy it refers to, so every run starts with a byte of its own.
  {
    const std::vector<uint8_t> phrase = Random(40, rng);
    std::vector<uint8_t> v = Random(200, rng);
    v.insert(v.end(), phrase.begin(), phrase.end());
    uint8_t first = 0x10;
    for (size_t run : {30, 14, 15, 269, 270}) {
      std::vector<uint8_t> fresh = Random(run, rng);
      fresh[0] = first++;
      v.insert(v.end(), fresh.begin(), fresh.end());
      v.insert(v.end(), phrase.begin(), phrase.end());
    }
    const std::vector<uint8_t> tail = Random(64, rng);
    v.insert(v.end(), tail.begin(), tail.end());
    g_totals.literal_runs.clear();
    g_totals.match_lengths.clear();
    CheckBuffer("literal runs", v, kAny);
    for (uint32_t run : {14u, 15u, 269u, 270u}) CHECK(g_totals.literal_runs.count(run) == 1, "no literal run of %u bytes", run);
    CHECK(g_totals.match_lengths == std::set<uint32_t>{40}, "the copies of the phrase are not matches of 40 bytes");
  }
  // a repeat that begins inside the last 12 bytes: the only match there is must be refused, so the block is stored
  {
    std::vector<uint8_t> v = Random(300, rng);
    std::memcpy(v.data() + 300 - 10, v.data() + 20, 10);
    CheckBuffer("match in the last 12 bytes", v, kRaw);
    // the same repeat 40 bytes earlier is taken, and stops 5 bytes before the end
    std::vector<uint8_t> u = Random(300, rng);
    std::memcpy(u.data() + 300 - 60, u.data() + 20, 60);
    g_totals.match_lengths.clear();
    CheckBuffer("match into the last bytes", u, kFramed);
    CHECK(g_totals.match_lengths.count(55) == 1, "the match does not end 5 bytes before the block");
  }
  // repeats that straddle a multiple of 64 positions (the groups of the match finder), at every phase
  for (size_t phase = 0; phase < 8; phase++) {
    std::vector<uint8_t> v = Random(1000, rng);
    std::memcpy(v.data() + 64 * 9 - 9 + phase * 3, v.data() + 100 + phase, 30);
    CheckBuffer("repeat across a group boundary, phase " + std::to_string(phase), v, kAny);
  }
  // repeats that straddle a block boundary: blocks are independent
  {
    std::vector<uint8_t> v = Random(2 * 65536, rng);
    const std::vector<uint8_t> phrase = Text(4000, rng);
    std::memcpy(v.data() + 65536 - 2000, phrase.data(), 4000);       // one phrase over the boundary
    std::memcpy(v.data() + 65536 + 30000, phrase.data(), 4000);      // and again inside the second block: only its second half can match
    std::memcpy(v.data() + 1000, phrase.data(), 2000);               // the first half repeats inside the first block
    CheckBuffer("repeat across a block boundary", v, kAny);
    CheckBuffer("zeros then text across blocks", [&] { std::vector<uint8_t> z(65536 + 500, 0); std::memcpy(z.data() + 65536 - 100, phrase.data(), 600); return z; }(), kFramed);
  }
  std::printf("%d cases, %d blocks (%d stored), %d framed and %d raw buffers, %d checks, %d failed\n", g_totals.cases, g_totals.blocks, g_totals.stored,
              g_totals.framed_buffers, g_totals.raw_buffers, g_checks, g_failed);
  return g_failed ? 1 : 0;
}
