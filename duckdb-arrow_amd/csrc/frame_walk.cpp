// frame_walk.cpp -- see frame_walk.hpp.
#include "frame_walk.hpp"

#include <algorithm>
#include <cstring>

namespace miarrow {

bool WalkLz4Frame(const uint8_t* body, int64_t frame_off, int64_t frame_len, uint32_t buffer_index, DeferredBody::Buffer* buf,
                  std::vector<DeferredBody::Block>* blocks) {
  const uint8_t* p = body + frame_off;
  int64_t at = 0;
  auto u32 = [&](int64_t o) { uint32_t v; std::memcpy(&v, p + o, 4); return v; };
  if (frame_len < 7 || u32(0) != 0x184D2204u) return false;
  const uint8_t flg = p[4], bd = p[5];
  if ((flg >> 6) != 1 || (flg & 0x02) || (flg & 0x01)) return false;   // version 01; reserved bit; dictionary id
  const bool block_checksum = (flg & 0x10) != 0, content_size = (flg & 0x08) != 0, content_checksum = (flg & 0x04) != 0;
  const int bsid = (bd >> 4) & 7;
  if (bsid < 4 || (bd & 0x8F)) return false;
  buf->block_max = 1u << (8 + 2 * bsid);   // 4: 64 KiB, 5: 256 KiB, 6: 1 MiB, 7: 4 MiB
  buf->independent = (flg & 0x20) != 0;    // block independence: liblz4 decodes every block without the ones before it
  at = 6 + (content_size ? 8 : 0) + 1;     // + header checksum
  if (at > frame_len) return false;
  buf->first_block = static_cast<uint32_t>(blocks->size());
  while (true) {
    if (at + 4 > frame_len) return false;
    const uint32_t word = u32(at);
    at += 4;
    if (word == 0) break;   // end mark
    const uint32_t size = word & 0x7FFFFFFFu;
    if (size > buf->block_max || at + size + (block_checksum ? 4 : 0) > frame_len) return false;
    DeferredBody::Block b;
    b.comp_off = static_cast<uint32_t>(frame_off + at);
    b.comp_size = size;
    b.buffer = buffer_index;
    b.stored = word >> 31;
    blocks->push_back(b);
    at += size + (block_checksum ? 4 : 0);
  }
  if (content_checksum && at + 4 > frame_len) return false;
  buf->n_blocks = static_cast<uint32_t>(blocks->size()) - buf->first_block;
  return true;
}

bool WalkZstdFrame(const uint8_t* body, int64_t frame_off, int64_t frame_len, uint32_t buffer_index, int64_t declared_len,
                   DeferredBody::Buffer* buf, std::vector<DeferredBody::Block>* blocks, std::vector<zstd::BlockInfo>* infos,
                   uint32_t* literal_scratch) {
  const uint8_t* p = body + frame_off;
  if (frame_len < 9 || p[0] != 0x28 || p[1] != 0xB5 || p[2] != 0x2F || p[3] != 0xFD) return false;
  const uint8_t fhd = p[4];
  const int fcs_flag = fhd >> 6;
  const bool single_segment = (fhd & 0x20) != 0;
  if ((fhd & 0x08) || (fhd & 0x04) || (fhd & 0x03)) return false;   // reserved bit; content checksum; dictionary id
  int64_t at = 5;
  uint64_t window = 0;
  if (!single_segment) {
    const uint8_t wd = p[at++];
    const uint64_t base = uint64_t(1) << (10 + (wd >> 3));
    window = base + (base >> 3) * (wd & 7u);
  }
  const int fcs_bytes = fcs_flag == 0 ? (single_segment ? 1 : 0) : fcs_flag == 1 ? 2 : fcs_flag == 2 ? 4 : 8;
  if (at + fcs_bytes > frame_len) return false;
  if (fcs_bytes) {
    uint64_t fcs = 0;
    std::memcpy(&fcs, p + at, static_cast<size_t>(fcs_bytes));   // little-endian host (the extension's platforms)
    if (fcs_bytes == 2) fcs += 256;
    if (fcs != static_cast<uint64_t>(declared_len)) return false;   // the host path words the error
    if (single_segment) window = fcs;
    at += fcs_bytes;
  }
  const uint64_t block_max = std::min<uint64_t>(std::max<uint64_t>(window, 1), zstd::kBlockMax);
  buf->block_max = zstd::kBlockMax;
  buf->first_block = static_cast<uint32_t>(blocks->size());
  const uint32_t none = ~0u;
  uint32_t last_huf = none, last_tbl[3] = {none, none, none};
  for (bool last = false; !last;) {
    if (at + 3 > frame_len) return false;
    const uint32_t h = static_cast<uint32_t>(p[at]) | (static_cast<uint32_t>(p[at + 1]) << 8) | (static_cast<uint32_t>(p[at + 2]) << 16);
    at += 3;
    last = (h & 1u) != 0;
    const uint32_t type = (h >> 1) & 3u, size = h >> 3;
    if (type == 3) return false;
    const uint32_t stored = type == 1 ? 1u : size;
    if ((type != 1 && size > block_max) || (type == 1 && size > block_max) || at + stored > frame_len) return false;
    const uint32_t self = static_cast<uint32_t>(blocks->size());
    DeferredBody::Block b;
    b.comp_off = static_cast<uint32_t>(frame_off + at);
    b.comp_size = stored;
    b.buffer = buffer_index;
    b.stored = type == 0;
    zstd::BlockInfo z;
    std::memset(&z, 0, sizeof(z));
    z.comp_off = b.comp_off;
    z.comp_size = stored;
    z.type = type;
    z.huf_src = z.ll_src = z.of_src = z.ml_src = self;
    const uint8_t* c = p + at;
    if (type == 1) {
      z.regen = size;
      z.lit_pos = *literal_scratch;   // its one byte, written to the scratch like a literal
      *literal_scratch += 1;
      b.seq_cap = 256;
    } else if (type == 2) {
      if (size < 2) return false;
      // literals section header
      z.lit_type = c[0] & 3u;
      const uint32_t fmt = (c[0] >> 2) & 3u;
      if (z.lit_type < 2) {
        if (!(fmt & 1u)) { z.lit_hdr = 1; z.lit_regen = c[0] >> 3; }
        else if (fmt == 1) { z.lit_hdr = 2; z.lit_regen = (c[0] >> 4) | (static_cast<uint32_t>(c[1]) << 4); }
        else {
          if (size < 3) return false;
          z.lit_hdr = 3;
          z.lit_regen = (c[0] >> 4) | (static_cast<uint32_t>(c[1]) << 4) | (static_cast<uint32_t>(c[2]) << 12);
        }
        z.lit_comp = z.lit_type == 0 ? z.lit_regen : 1;
        z.lit_streams = 1;
      } else {
        if (size < 5) return false;
        const uint64_t v = static_cast<uint64_t>(c[0]) | (static_cast<uint64_t>(c[1]) << 8) | (static_cast<uint64_t>(c[2]) << 16) |
                           (static_cast<uint64_t>(c[3]) << 24) | (static_cast<uint64_t>(c[4]) << 32);
        if (fmt <= 1) { z.lit_hdr = 3; z.lit_regen = (v >> 4) & 0x3FFu; z.lit_comp = (v >> 14) & 0x3FFu; }
        else if (fmt == 2) { z.lit_hdr = 4; z.lit_regen = (v >> 4) & 0x3FFFu; z.lit_comp = (v >> 18) & 0x3FFFu; }
        else { z.lit_hdr = 5; z.lit_regen = (v >> 4) & 0x3FFFFu; z.lit_comp = (v >> 22) & 0x3FFFFu; }
        z.lit_streams = fmt == 0 ? 1 : 4;
        if (z.lit_type == 3) {
          if (last_huf == none) return false;
          z.huf_src = last_huf;
        } else {
          last_huf = self;
        }
        if (z.lit_comp == 0 || z.lit_regen == 0) return false;
      }
      if (z.lit_regen > zstd::kBlockMax || static_cast<uint64_t>(z.lit_hdr) + z.lit_comp + 1 > size) return false;
      if (z.lit_type == 0) {
        z.lit_pos = b.comp_off + z.lit_hdr;
      } else {
        z.lit_pos = *literal_scratch;
        *literal_scratch += (z.lit_regen + 3u) & ~3u;
      }
      // sequences section: the count, then (count > 0) the modes of the three tables
      z.seq_pos = z.lit_hdr + z.lit_comp;
      const uint8_t* q = c + z.seq_pos;
      const uint32_t left = size - z.seq_pos;
      if (q[0] == 0) { z.seq_hdr = 1; z.nseq = 0; }
      else if (q[0] < 128) { z.seq_hdr = 1; z.nseq = q[0]; }
      else if (q[0] < 255) {
        if (left < 2) return false;
        z.seq_hdr = 2;
        z.nseq = ((static_cast<uint32_t>(q[0]) - 128u) << 8) + q[1];
      } else {
        if (left < 3) return false;
        z.seq_hdr = 3;
        z.nseq = static_cast<uint32_t>(q[1]) + (static_cast<uint32_t>(q[2]) << 8) + 0x7F00u;
      }
      if (z.nseq == 0) {
        if (left != z.seq_hdr) return false;
      } else {
        if (left < z.seq_hdr + 2) return false;
        const uint32_t modes = q[z.seq_hdr];
        if (modes & 3u) return false;
        uint32_t* src[3] = {&z.ll_src, &z.of_src, &z.ml_src};
        for (int t = 0; t < 3; t++) {
          if (((modes >> (6 - 2 * t)) & 3u) == 3u) {
            if (last_tbl[t] == none) return false;
            *src[t] = last_tbl[t];
          } else {
            last_tbl[t] = self;
          }
        }
      }
      b.seq_cap = 256u * ((z.nseq + 1u + 255u) / 256u);
    }
    blocks->push_back(b);
    infos->push_back(z);
    at += stored;
  }
  if (at != frame_len) return false;   // a second frame, a skippable frame, trailing bytes: the host library's business
  buf->n_blocks = static_cast<uint32_t>(blocks->size()) - buf->first_block;
  return true;
}

}  // namespace miarrow
