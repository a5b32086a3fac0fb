// scan_k8.hpp -- the host arithmetic of the K8 staging (ArrowScan::EnqueueLz4, scan_enqueue.cpp): where every table, counter
// and scratch array of one compressed record batch lies in the slot's scratch arena, what goes into the three pinned tables,
// and the device::Lz4Args the launch takes.  Plain functions of a DeferredBody: no HIP call, no device, nothing allocated.
#pragma once

#include <cstddef>
#include <cstdint>

#include "frame_walk.hpp"
#include "kernels.hpp"

namespace miarrow {

//! The scratch arena of one compressed record batch (Slot::d_lz4).  Every region starts on a multiple of 256 and takes
//! RoundUp(bytes + 16, 256); the regions lie in the order of the members, without gaps:
//!   [0, tables_bytes)              the tables the host fills (Slot::h_lz4 holds the same bytes) and uploads
//!   [tables_bytes, counters_end)   what the ONE memset per record batch clears: counters, status, marks
//!   [counters_end, arena_bytes)    scratch that needs no preset: every word a stage reads was written by the stage before
struct K8Layout {
  size_t o_blocks = 0;     // nb x device::Lz4BlockDev
  size_t o_buffers = 0;    // nf x device::Lz4BufferDev
  size_t o_zblocks = 0;    // ZSTD: nb x zstd::BlockInfo; LZ4: 0 bytes (the region is still there)
  size_t tables_bytes = 0;
  size_t o_bsize = 0;      // block_out_size: nb x 4
  size_t o_bnseq = 0;      // block_nseq: nb x 4
  size_t o_bbase = 0;      // block_out_base: nb x 8
  size_t o_chunk = 0;      // chunk_base: (nb + 1) x 4
  size_t o_bufok = 0;      // buffer_ok: nf x 4
  size_t o_round = 0;      // round_left: 40 x 4
  size_t o_status = 0;     // status: 4
  size_t o_mark = 0;       // mark: out_size + 16
  size_t counters_end = 0;
  size_t o_seq = 0;        // seq: total_seq x 16
  size_t o_seqoff = 0;     // seq_off: total_seq x 4
  size_t o_lane_out = 0;   // lane_out: nb x 256 x 4
  size_t o_lane_n = 0;     // lane_nseq: nb x 256 x 4
  size_t o_rep = 0;        // ZSTD: rep_state, nb x 256 x 16; LZ4: 0 bytes
  size_t o_link = 0;       // link: out_size x 4 + 16
  size_t o_skel = 0;       // skel: out_size x 4 + 16
  size_t arena_bytes = 0;
  // the compressed body in HBM (Slot::d_comp): comp_need bytes; ZSTD keeps the decoded literals of every block behind the
  // compressed bytes, from lit_base on
  size_t comp_need = 0, lit_base = 0;
  size_t out_size = 0;           // the decompressed body
  uint64_t total_seq = 0;        // sequence descriptors of all blocks (the end of the running sum Lz4BlockDev::seq_base)
  uint64_t max_len = 0;          // longest decompressed buffer that has blocks (a raw buffer has none)
  uint32_t max_blocks = 0;       // most blocks any one such buffer has
  uint32_t min_block_comp = 0xFFFFFFFFu, max_block_comp = 0;   // over the blocks that are not stored
};
K8Layout LayOutK8Scratch(const DeferredBody& d, size_t out_size);

//! The Lz4BlockDev, Lz4BufferDev and (ZSTD) zstd::BlockInfo tables into `tables`, which holds l.tables_bytes bytes.
void FillK8Tables(const DeferredBody& d, const K8Layout& l, uint8_t* tables);

//! The launch arguments: the arena at `d_lz4`, the compressed body at `d_comp`, the decompressed one at `d_in`.
void FillK8Args(const DeferredBody& d, const K8Layout& l, uint8_t* d_lz4, uint8_t* d_comp, uint8_t* d_in, device::Lz4Args* a);

}  // namespace miarrow
