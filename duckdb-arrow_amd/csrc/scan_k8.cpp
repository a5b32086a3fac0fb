// scan_k8.cpp -- see scan_k8.hpp.
#include "scan_k8.hpp"

#include <algorithm>
#include <cstring>

namespace miarrow {

namespace {
size_t RoundUp256(size_t v) { return (v + 255) / 256 * 256; }
}  // namespace

K8Layout LayOutK8Scratch(const DeferredBody& d, size_t out_size) {
  K8Layout l;
  const size_t nb = d.blocks.size(), nf = d.buffers.size();
  const bool is_zstd = d.codec == 1;
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t o = at; at += RoundUp256(bytes + 16); return o; };
  l.out_size = out_size;
  for (const auto& blk : d.blocks) {
    l.total_seq += is_zstd ? blk.seq_cap : device::Lz4SeqCapacity(blk.comp_size);
    if (!blk.stored) {   // LZ4: which token walk fits; ZSTD: how much LDS the staged block takes
      l.max_block_comp = std::max(l.max_block_comp, blk.comp_size);
      l.min_block_comp = std::min(l.min_block_comp, blk.comp_size);
    }
  }
  // a raw buffer (length prefix -1: Arrow C++ with min_space_savings, arrow-rs, Arrow Java) has no blocks
  for (const auto& f : d.buffers)
    if (!f.raw) {
      l.max_len = std::max<uint64_t>(l.max_len, static_cast<uint64_t>(f.out_len));
      l.max_blocks = std::max<uint32_t>(l.max_blocks, f.n_blocks);
    }
  // ZSTD: the decoded literals of every block lie behind the compressed body, in the same allocation
  l.lit_base = RoundUp256(static_cast<size_t>(d.comp_size) + 64);
  l.comp_need = is_zstd ? l.lit_base + d.literal_scratch + 64 : static_cast<size_t>(d.comp_size) + 64;

  l.o_blocks = take(nb * sizeof(device::Lz4BlockDev));
  l.o_buffers = take(nf * sizeof(device::Lz4BufferDev));
  l.o_zblocks = take(is_zstd ? nb * sizeof(zstd::BlockInfo) : 0);
  l.tables_bytes = at;
  l.o_bsize = take(nb * 4);
  l.o_bnseq = take(nb * 4);
  l.o_bbase = take(nb * 8);
  l.o_chunk = take((nb + 1) * 4);
  l.o_bufok = take(nf * 4);
  l.o_round = take(40 * 4);
  l.o_status = take(4);
  l.o_mark = take(out_size + 16);
  l.counters_end = at;
  l.o_seq = take(static_cast<size_t>(l.total_seq) * 16);
  l.o_seqoff = take(static_cast<size_t>(l.total_seq) * 4);
  l.o_lane_out = take(nb * 256 * 4);
  l.o_lane_n = take(nb * 256 * 4);
  l.o_rep = take(is_zstd ? nb * 256 * 16 : 0);
  l.o_link = take(out_size * 4 + 16);
  l.o_skel = take(out_size * 4 + 16);
  l.arena_bytes = at;
  return l;
}

void FillK8Tables(const DeferredBody& d, const K8Layout& l, uint8_t* tables) {
  const size_t nb = d.blocks.size(), nf = d.buffers.size();
  const bool is_zstd = d.codec == 1;
  auto* hb = reinterpret_cast<device::Lz4BlockDev*>(tables + l.o_blocks);
  auto* hf = reinterpret_cast<device::Lz4BufferDev*>(tables + l.o_buffers);
  uint32_t seq_at = 0;
  for (size_t i = 0; i < nb; i++) {
    const auto& blk = d.blocks[i];
    hb[i].comp_off = blk.comp_off;
    hb[i].comp_size = blk.comp_size;
    hb[i].buffer = blk.buffer;
    hb[i].stored = blk.stored;
    hb[i].seq_base = seq_at;
    hb[i].seq_cap = is_zstd ? blk.seq_cap : device::Lz4SeqCapacity(blk.comp_size);
    seq_at += hb[i].seq_cap;
  }
  if (is_zstd) {
    auto* hz = reinterpret_cast<zstd::BlockInfo*>(tables + l.o_zblocks);
    for (size_t i = 0; i < nb; i++) {
      hz[i] = d.zblocks[i];
      const bool in_scratch = hz[i].type == 1 || (hz[i].type == 2 && hz[i].lit_type != 0);
      if (in_scratch) hz[i].lit_pos += static_cast<uint32_t>(l.lit_base);
    }
  }
  for (size_t i = 0; i < nf; i++) {
    const auto& f = d.buffers[i];
    hf[i].out_off = static_cast<uint64_t>(f.out_off);
    // a raw buffer has no blocks: the layout kernels check "sum of the block sizes == out_len", which for it is 0 == 0; its
    // bytes are copied by the caller
    hf[i].out_len = f.raw ? 0 : static_cast<uint64_t>(f.out_len);
    hf[i].first_block = f.first_block;
    hf[i].n_blocks = f.raw ? 0 : f.n_blocks;
    hf[i].block_max = f.block_max;
    hf[i].independent = f.independent ? 1u : 0u;
  }
}

void FillK8Args(const DeferredBody& d, const K8Layout& l, uint8_t* d_lz4, uint8_t* d_comp, uint8_t* d_in, device::Lz4Args* out) {
  const bool is_zstd = d.codec == 1;
  device::Lz4Args& a = *out;
  std::memset(&a, 0, sizeof(a));
  a.comp = d_comp;
  a.out = d_in;
  a.out_size = l.out_size;
  a.max_buffer_len = l.max_len;
  a.max_buffer_blocks = l.max_blocks;
  a.blocks = reinterpret_cast<const device::Lz4BlockDev*>(d_lz4 + l.o_blocks);
  a.buffers = reinterpret_cast<const device::Lz4BufferDev*>(d_lz4 + l.o_buffers);
  a.n_blocks = static_cast<uint32_t>(d.blocks.size());
  a.n_buffers = static_cast<uint32_t>(d.buffers.size());
  a.min_block_comp = l.min_block_comp;
  a.max_block_comp = l.max_block_comp;
  a.seq = d_lz4 + l.o_seq;
  a.seq_off = reinterpret_cast<uint32_t*>(d_lz4 + l.o_seqoff);
  a.lane_out = reinterpret_cast<uint32_t*>(d_lz4 + l.o_lane_out);
  a.lane_nseq = reinterpret_cast<uint32_t*>(d_lz4 + l.o_lane_n);
  a.link = reinterpret_cast<uint32_t*>(d_lz4 + l.o_link);
  a.block_out_size = reinterpret_cast<uint32_t*>(d_lz4 + l.o_bsize);
  a.block_nseq = reinterpret_cast<uint32_t*>(d_lz4 + l.o_bnseq);
  a.block_out_base = reinterpret_cast<uint64_t*>(d_lz4 + l.o_bbase);
  a.chunk_base = reinterpret_cast<uint32_t*>(d_lz4 + l.o_chunk);
  a.buffer_ok = reinterpret_cast<uint32_t*>(d_lz4 + l.o_bufok);
  a.round_left = reinterpret_cast<uint32_t*>(d_lz4 + l.o_round);
  a.mark = d_lz4 + l.o_mark;
  a.skel = reinterpret_cast<uint32_t*>(d_lz4 + l.o_skel);
  a.status = reinterpret_cast<uint32_t*>(d_lz4 + l.o_status);
  a.zblocks = is_zstd ? d_lz4 + l.o_zblocks : nullptr;
  a.literals = d_comp;
  a.rep_state = is_zstd ? reinterpret_cast<uint32_t*>(d_lz4 + l.o_rep) : nullptr;
}

}  // namespace miarrow
