// k8_scratch_check.cpp -- the K8 scratch arena as data (duckdb-arrow_amd/csrc/scan_k8.cpp: LayOutK8Scratch, FillK8Tables,
// FillK8Args) over hand-built DeferredBody descriptions, as a program of its own for g++ -fsanitize=address,undefined.  The
// expected offsets are worked out here from the rule "a region takes round_up(bytes + 16, 256)" and the region order, with
// the element sizes written out; the tables are filled into an allocation of exactly the reported size, so ASan judges every
// write.  No arguments; prints "<checks> checks, <failed> failed" and exits 1 on a failure.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "scan_k8.hpp"

using namespace miarrow;

namespace {
long failed = 0, checks = 0;
std::string current;

void Expect(bool ok, const char* what, long long a = 0, long long b = 0) {
  checks++;
  if (!ok && failed++ < 40) std::fprintf(stderr, "FAILED [%s]: %s (%lld, %lld)\n", current.c_str(), what, a, b);
}

static_assert(sizeof(device::Lz4BlockDev) == 24 && sizeof(device::Lz4BufferDev) == 32 && sizeof(zstd::BlockInfo) == 72, "element sizes the expected offsets below are written with");

size_t RoundUp(size_t v, size_t a) { return (v + a - 1) / a * a; }
uint32_t Lz4SeqCap(uint32_t comp_size) { return 256u * (((comp_size + 255u) / 256u) / 3u + 2u); }   // kernels.hpp, restated

struct Region {
  const char* name;
  size_t offset;    // from the function under test
  size_t bytes;     // what the region must hold, written out here
  bool counter;     // cleared by the one memset per record batch
};

// the regions in their order, sizes from the description alone
std::vector<Region> Regions(const DeferredBody& d, size_t out_size, const K8Layout& l, uint64_t total_seq) {
  const size_t nb = d.blocks.size(), nf = d.buffers.size();
  const bool z = d.codec == 1;
  return {
      {"blocks", l.o_blocks, nb * 24, false},
      {"buffers", l.o_buffers, nf * 32, false},
      {"zblocks", l.o_zblocks, z ? nb * 72 : 0, false},
      {"block_out_size", l.o_bsize, nb * 4, true},
      {"block_nseq", l.o_bnseq, nb * 4, true},
      {"block_out_base", l.o_bbase, nb * 8, true},
      {"chunk_base", l.o_chunk, (nb + 1) * 4, true},
      {"buffer_ok", l.o_bufok, nf * 4, true},
      {"round_left", l.o_round, 40 * 4, true},
      {"status", l.o_status, 4, true},
      {"mark", l.o_mark, out_size + 16, true},
      {"seq", l.o_seq, static_cast<size_t>(total_seq) * 16, false},
      {"seq_off", l.o_seqoff, static_cast<size_t>(total_seq) * 4, false},
      {"lane_out", l.o_lane_out, nb * 256 * 4, false},
      {"lane_nseq", l.o_lane_n, nb * 256 * 4, false},
      {"rep_state", l.o_rep, z ? nb * 256 * 16 : 0, false},
      {"link", l.o_link, out_size * 4 + 16, false},
      {"skel", l.o_skel, out_size * 4 + 16, false},
  };
}

void CheckBody(const std::string& name, const DeferredBody& d, size_t out_size) {
  current = name;
  const size_t nb = d.blocks.size(), nf = d.buffers.size();
  const bool z = d.codec == 1;
  const K8Layout l = LayOutK8Scratch(d, out_size);

  // the sums and extremes, restated
  uint64_t total_seq = 0, max_len = 0;
  uint32_t max_blocks = 0, min_comp = 0xFFFFFFFFu, max_comp = 0;
  std::vector<uint32_t> seq_base(nb), seq_cap(nb);
  for (size_t i = 0; i < nb; i++) {
    seq_cap[i] = z ? d.blocks[i].seq_cap : Lz4SeqCap(d.blocks[i].comp_size);
    seq_base[i] = static_cast<uint32_t>(total_seq);
    total_seq += seq_cap[i];
    if (!d.blocks[i].stored) {
      if (d.blocks[i].comp_size > max_comp) max_comp = d.blocks[i].comp_size;
      if (d.blocks[i].comp_size < min_comp) min_comp = d.blocks[i].comp_size;
    }
  }
  for (const auto& f : d.buffers)
    if (!f.raw) {
      if (static_cast<uint64_t>(f.out_len) > max_len) max_len = static_cast<uint64_t>(f.out_len);
      if (f.n_blocks > max_blocks) max_blocks = f.n_blocks;
    }
  Expect(l.total_seq == total_seq, "total_seq is the end of the running sum of seq_cap", l.total_seq, total_seq);
  Expect(l.max_len == max_len, "max_len is over the buffers that have blocks", l.max_len, max_len);
  Expect(l.max_blocks == max_blocks, "max_blocks is over the buffers that have blocks", l.max_blocks, max_blocks);
  Expect(l.min_block_comp == min_comp && l.max_block_comp == max_comp, "min / max compressed size are over the blocks that are not stored", l.min_block_comp, l.max_block_comp);
  Expect(l.out_size == out_size, "out_size");
  const size_t lit_base = RoundUp(static_cast<size_t>(d.comp_size) + 64, 256);
  Expect(l.lit_base == lit_base, "lit_base", l.lit_base, lit_base);
  Expect(l.comp_need == (z ? lit_base + d.literal_scratch + 64 : static_cast<size_t>(d.comp_size) + 64), "comp_need", l.comp_need);

  // the arena: offsets from the rule, in the declared order
  const std::vector<Region> regions = Regions(d, out_size, l, total_seq);
  size_t at = 0;
  for (size_t i = 0; i < regions.size(); i++) {
    const Region& r = regions[i];
    Expect(r.offset == at, r.name, r.offset, at);
    Expect(r.offset % 256 == 0, "a region starts on a multiple of 256", r.offset);
    const size_t next = i + 1 < regions.size() ? regions[i + 1].offset : l.arena_bytes;
    Expect(r.offset + r.bytes <= next, "a region ends in front of the next one / inside the arena", r.offset + r.bytes, next);
    if (i + 1 < regions.size()) Expect(regions[i + 1].offset > r.offset, "regions lie in the declared order, pairwise disjoint");
    if (std::strcmp(r.name, "zblocks") == 0) Expect(l.tables_bytes == next, "tables_bytes is the end of the last table", l.tables_bytes, next);
    if (std::strcmp(r.name, "mark") == 0) Expect(l.counters_end == next, "counters_end is the end of the marks", l.counters_end, next);
    at += RoundUp(r.bytes + 16, 256);
  }
  Expect(l.arena_bytes == at, "arena total", l.arena_bytes, at);
  for (const Region& r : regions) {
    // (by where a region starts: a region of an empty body holds 0 bytes; that it ends in front of the next one is checked above)
    const bool in_tables = r.offset < l.tables_bytes, in_counters = r.offset >= l.tables_bytes && r.offset < l.counters_end;
    const bool is_table = !std::strcmp(r.name, "blocks") || !std::strcmp(r.name, "buffers") || !std::strcmp(r.name, "zblocks");
    Expect(in_tables == is_table, "exactly the tables lie below tables_bytes", r.offset);
    Expect(in_counters == r.counter, "exactly the counter regions lie in [tables_bytes, counters_end)", r.offset);
  }
  if (!z) {   // the ZSTD-only regions are there for LZ4 too, with the size of take(0)
    Expect(l.tables_bytes - l.o_zblocks == 256, "LZ4: the zblocks region has the size of take(0)", l.tables_bytes - l.o_zblocks);
    Expect(l.o_link - l.o_rep == 256, "LZ4: the rep_state region has the size of take(0)", l.o_link - l.o_rep);
  }

  // the tables, into an allocation of exactly tables_bytes
  uint8_t* tables = static_cast<uint8_t*>(std::malloc(l.tables_bytes));
  std::memset(tables, 0xA5, l.tables_bytes);
  FillK8Tables(d, l, tables);
  for (size_t i = 0; i < nb; i++) {
    device::Lz4BlockDev hb;
    std::memcpy(&hb, tables + l.o_blocks + i * 24, 24);
    Expect(hb.comp_off == d.blocks[i].comp_off && hb.comp_size == d.blocks[i].comp_size && hb.buffer == d.blocks[i].buffer && hb.stored == d.blocks[i].stored,
           "a block's entry repeats its description", static_cast<long long>(i));
    Expect(hb.seq_base == seq_base[i] && hb.seq_cap == seq_cap[i], "seq_base is the running sum of seq_cap", hb.seq_base, seq_base[i]);
  }
  for (size_t i = 0; i < nf; i++) {
    device::Lz4BufferDev hf;
    std::memcpy(&hf, tables + l.o_buffers + i * 32, 32);
    const auto& f = d.buffers[i];
    Expect(hf.out_off == static_cast<uint64_t>(f.out_off) && hf.first_block == f.first_block && hf.block_max == f.block_max && hf.independent == (f.independent ? 1u : 0u),
           "a buffer's entry repeats its description", static_cast<long long>(i));
    if (f.raw) Expect(hf.out_len == 0 && hf.n_blocks == 0, "a raw buffer gets zero length and zero blocks", static_cast<long long>(hf.out_len), hf.n_blocks);
    else Expect(hf.out_len == static_cast<uint64_t>(f.out_len) && hf.n_blocks == f.n_blocks, "a compressed buffer keeps its length and blocks", static_cast<long long>(i));
  }
  if (z)
    for (size_t i = 0; i < nb; i++) {
      zstd::BlockInfo hz;
      std::memcpy(&hz, tables + l.o_zblocks + i * 72, 72);
      const zstd::BlockInfo& in = d.zblocks[i];
      const bool rebased = in.type == 1 || (in.type == 2 && (in.lit_type == 1 || in.lit_type == 2 || in.lit_type == 3));
      Expect(hz.lit_pos == in.lit_pos + (rebased ? static_cast<uint32_t>(lit_base) : 0u), "lit_pos is rebased for RLE blocks and for compressed blocks whose literals are not raw, only", hz.lit_pos, in.lit_pos);
      zstd::BlockInfo same = hz;
      same.lit_pos = in.lit_pos;
      Expect(std::memcmp(&same, &in, 72) == 0, "nothing else of a BlockInfo changes", static_cast<long long>(i));
    }
  std::free(tables);

  // the launch arguments: every pointer is its base plus the region's offset, inside the arena
  uint8_t* d_lz4 = static_cast<uint8_t*>(std::malloc(l.arena_bytes ? l.arena_bytes : 1));
  uint8_t* d_comp = static_cast<uint8_t*>(std::malloc(l.comp_need));
  uint8_t* d_in = static_cast<uint8_t*>(std::malloc(out_size + 64));
  device::Lz4Args* a = static_cast<device::Lz4Args*>(std::malloc(sizeof(device::Lz4Args)));   // exactly one: ASan sees a write past it
  FillK8Args(d, l, d_lz4, d_comp, d_in, a);
  auto at_region = [&](const void* p, const char* region) {
    for (const Region& r : regions)
      if (!std::strcmp(r.name, region)) return p == d_lz4 + r.offset && r.offset + r.bytes <= l.arena_bytes;
    return false;
  };
  Expect(a->comp == d_comp && a->literals == d_comp && a->out == d_in, "comp, literals and out are the three bases");
  Expect(a->out_size == out_size && a->max_buffer_len == max_len && a->max_buffer_blocks == max_blocks, "sizes in the arguments");
  Expect(a->n_blocks == nb && a->n_buffers == nf && a->min_block_comp == min_comp && a->max_block_comp == max_comp && a->_pad == 0, "counts in the arguments");
  Expect(at_region(a->blocks, "blocks") && at_region(a->buffers, "buffers"), "table pointers");
  Expect(at_region(a->block_out_size, "block_out_size") && at_region(a->block_nseq, "block_nseq") && at_region(a->block_out_base, "block_out_base") &&
             at_region(a->chunk_base, "chunk_base") && at_region(a->buffer_ok, "buffer_ok") && at_region(a->round_left, "round_left") &&
             at_region(a->status, "status") && at_region(a->mark, "mark"),
         "counter pointers");
  Expect(at_region(a->seq, "seq") && at_region(a->seq_off, "seq_off") && at_region(a->lane_out, "lane_out") && at_region(a->lane_nseq, "lane_nseq") &&
             at_region(a->link, "link") && at_region(a->skel, "skel"),
         "scratch pointers");
  if (z) Expect(at_region(a->zblocks, "zblocks") && at_region(a->rep_state, "rep_state"), "ZSTD pointers");
  else Expect(a->zblocks == nullptr && a->rep_state == nullptr, "LZ4: no ZSTD pointers");
  std::free(a);
  std::free(d_in);
  std::free(d_comp);
  std::free(d_lz4);
}

DeferredBody::Buffer Buf(int64_t comp_off, int64_t comp_len, int64_t out_off, int64_t out_len, bool raw, uint32_t first_block, uint32_t n_blocks, bool independent) {
  DeferredBody::Buffer f;
  f.comp_off = comp_off;
  f.comp_len = comp_len;
  f.out_off = out_off;
  f.out_len = out_len;
  f.raw = raw;
  f.first_block = first_block;
  f.n_blocks = n_blocks;
  f.block_max = 65536;
  f.independent = independent;
  return f;
}

// `sizes`: compressed size per block (a negative one = a stored block of that many bytes); buffers of `per_buffer` blocks each,
// with a raw buffer in the second place when `raw_between`
DeferredBody Body(int32_t codec, const std::vector<int64_t>& sizes, size_t per_buffer, bool raw_between, size_t* out_size) {
  DeferredBody d;
  d.codec = codec;
  uint32_t comp_at = 64;
  int64_t out_at = 0;
  size_t i = 0;
  bool raw_done = !raw_between;
  while (i < sizes.size() || !raw_done) {
    if (!raw_done && !d.buffers.empty()) {
      // a raw buffer: its bytes themselves, no blocks.  Its out_len and n_blocks are larger than any compressed buffer's, so a
      // rule that let them into max_len / max_blocks, or into the table, shows.
      d.buffers.push_back(Buf(comp_at, 900000, out_at, 900000, true, static_cast<uint32_t>(d.blocks.size()), 7777, false));
      comp_at += 900000;
      out_at += (900000 + 63) / 64 * 64;
      raw_done = true;
      continue;
    }
    const size_t first = d.blocks.size();
    const uint32_t buffer = static_cast<uint32_t>(d.buffers.size());
    const int64_t frame_off = comp_at;
    int64_t out_len = 0;
    for (size_t k = 0; k < per_buffer && i < sizes.size(); k++, i++) {
      DeferredBody::Block blk;
      blk.stored = sizes[i] < 0 ? 1 : 0;
      blk.comp_size = static_cast<uint32_t>(sizes[i] < 0 ? -sizes[i] : sizes[i]);
      blk.comp_off = comp_at + 4;
      blk.buffer = buffer;
      blk.seq_cap = codec == 1 ? 256u * static_cast<uint32_t>(1 + (i * 7) % 5) : 0xDEADu;   // LZ4 derives it from comp_size
      comp_at += 4 + blk.comp_size;
      out_len += blk.stored ? blk.comp_size : 3 * static_cast<int64_t>(blk.comp_size) + 1;
      d.blocks.push_back(blk);
      if (codec == 1) {
        zstd::BlockInfo zi;
        std::memset(&zi, 0, sizeof(zi));
        zi.comp_off = blk.comp_off;
        zi.comp_size = blk.comp_size;
        zi.type = static_cast<uint32_t>(i % 3);           // raw, RLE, compressed
        zi.lit_type = static_cast<uint32_t>((i / 3) % 4);   // raw, RLE, Huffman, Huffman with an earlier table
        zi.lit_pos = 1000 + static_cast<uint32_t>(i);
        zi.nseq = static_cast<uint32_t>(i);
        zi.huf_src = zi.ll_src = zi.of_src = zi.ml_src = static_cast<uint32_t>(i);
        d.zblocks.push_back(zi);
      }
    }
    d.buffers.push_back(Buf(frame_off, comp_at - frame_off, out_at, out_len, false, static_cast<uint32_t>(first), static_cast<uint32_t>(d.blocks.size() - first), buffer % 2 == 0));
    out_at += (out_len + 63) / 64 * 64;
  }
  d.comp_size = comp_at;
  d.literal_scratch = codec == 1 ? 12345 : 0;
  *out_size = static_cast<size_t>(out_at);
  return d;
}

}  // namespace

int main() {
  for (int32_t codec = 0; codec < 2; codec++) {
    const std::string c = codec == 1 ? "zstd" : "lz4";
    size_t out_size = 0;
    {   // an empty body: no buffer, no block, nothing to decompress
      DeferredBody d;
      d.codec = codec;
      CheckBody(c + " empty body", d, 0);
    }
    {   // one buffer without a block (an LZ4 frame that holds only its end mark)
      DeferredBody d;
      d.codec = codec;
      d.comp_size = 19;
      d.buffers.push_back(Buf(0, 19, 0, 0, false, 0, 0, true));
      CheckBody(c + " 0 blocks", d, 0);
    }
    {
      const DeferredBody d = Body(codec, {1}, 1, false, &out_size);   // one block of one byte
      CheckBody(c + " 1 block of 1 byte", d, out_size);
    }
    {
      const DeferredBody d = Body(codec, {-1}, 1, false, &out_size);   // one stored block: min / max stay at their start values
      CheckBody(c + " 1 stored block", d, out_size);
    }
    {
      const DeferredBody d = Body(codec, {4 << 20}, 1, false, &out_size);
      CheckBody(c + " 1 block of 4 MiB", d, out_size);
    }
    {   // 300 blocks in buffers of 64, a raw buffer between the first two, stored blocks, a 1-byte and a 4 MiB block among them
      std::vector<int64_t> sizes;
      for (int i = 0; i < 300; i++) sizes.push_back(i % 11 == 3 ? -(200 + i) : 100 + 37 * i);
      sizes[5] = 1;
      sizes[130] = 4 << 20;
      sizes[131] = -(5 << 20);   // stored and larger than every compressed block: not the maximum
      sizes[6] = -1;             // stored and smaller: not the minimum
      const DeferredBody d = Body(codec, sizes, 64, true, &out_size);
      CheckBody(c + " 300 blocks, raw buffer between compressed ones", d, out_size);
    }
  }
  std::printf("%ld checks, %ld failed\n", checks, failed);
  return failed ? 1 : 0;
}
