// frame_walk.hpp -- the host half of the K8 kernels (kernels_lz4.hip, kernels_zstd.inl): the frame, block and section headers
// of an LZ4_FRAME / ZSTD buffer parsed into the tables the kernels consume.  Pure byte parsing: nothing here reads a file,
// starts a thread or loads a library.
#pragma once

#include <cstdint>
#include <vector>

#include "zstd_format.hpp"

namespace miarrow {

//! A record-batch body whose LZ4_FRAME / ZSTD buffers are still compressed (IPCStreamReader::SetDeferLz4 / SetDeferZstd): the
//! frames were walked on the host (frame header, block headers), the bytes are decompressed in HBM by the K8 kernels.
struct DeferredBody {
  struct Buffer {
    int64_t comp_off = 0, comp_len = 0;   // raw: the bytes themselves; else the frame, inside the compressed body
    int64_t out_off = 0, out_len = 0;     // place in the decompressed body
    bool raw = false;                     // stored uncompressed (length prefix -1)
    uint32_t first_block = 0, n_blocks = 0, block_max = 0;
    bool independent = false;             // LZ4: FLG bit 0x20, a match may not reach in front of its own block
  };
  struct Block {
    uint32_t comp_off = 0, comp_size = 0, buffer = 0, stored = 0;
    uint32_t seq_cap = 0;                 // ZSTD: sequence descriptors the block needs (LZ4: derived from comp_size)
  };
  const uint8_t* comp = nullptr;          // the compressed body as it was read (kept alive by DecodedBatch::owner)
  int64_t comp_size = 0;
  std::vector<Buffer> buffers;            // the needed, non-empty buffers of the message
  std::vector<Block> blocks;              // every block of every non-raw buffer, buffer by buffer
  int32_t codec = 0;                      // 0 LZ4_FRAME, 1 ZSTD
  std::vector<zstd::BlockInfo> zblocks;   // ZSTD: one per entry of `blocks`
  uint32_t literal_scratch = 0;           // ZSTD: bytes of decoded literals (BlockInfo::lit_pos of non-raw literals counts from 0)
};

//! Walks one LZ4 frame (lz4_Frame_format.md: magic, FLG, BD, [content size], [dict id], HC, blocks, end mark) without
//! touching the block data: appends its blocks to `blocks`.  false = something the GPU path does not take (skippable or
//! legacy frames, a dictionary id, a damaged header): the caller decompresses the record batch on the host instead, which
//! also produces the reference's error text for damaged input.
bool WalkLz4Frame(const uint8_t* body, int64_t frame_off, int64_t frame_len, uint32_t buffer_index, DeferredBody::Buffer* buf,
                  std::vector<DeferredBody::Block>* blocks);
//! Walks one ZSTD frame (one IPC buffer) from its headers.  false = a frame the device path does not take (dictionary,
//! content checksum, several frames, anything malformed): the host decompressor handles it and reports what is wrong.
bool WalkZstdFrame(const uint8_t* body, int64_t frame_off, int64_t frame_len, uint32_t buffer_index, int64_t declared_len,
                   DeferredBody::Buffer* buf, std::vector<DeferredBody::Block>* blocks, std::vector<zstd::BlockInfo>* infos,
                   uint32_t* literal_scratch);

}  // namespace miarrow
