// writer_compress.cpp -- BodyCompressor (writer.hpp): the steps between the K7 encode and the D2H of a compressed body.
#include <hip/hip_runtime.h>

#include <cstring>

#include "kernels.hpp"
#include "writer.hpp"
#include "writer_internal.hpp"

namespace miarrow {

template <typename Buffer>
void BodyCompressor::Keep(Buffer& buf, std::vector<Buffer>& retired, size_t need) {
  Buffer old = Grow(buf, need, GrownCapacity(need, buf.size(), 1 << 16));
  if (old) retired.push_back(std::move(old));
}

void BodyCompressor::Run(const BodyLayout& plain, const uint8_t* d_body, hipStream_t s) {
  using namespace lz4enc;
  const std::vector<BlockIn> blocks = BlocksOfBody(plain);
  const size_t n_blocks = blocks.size();
  // an uncompressed body is the worst case but for the prefixes, frame headers and size words: per buffer 8 + 7 + 4 and
  // 8 of padding, per block 4.  The copy table has at most 4 entries per buffer and 2 per block.
  const size_t out_cap = static_cast<size_t>(plain.body_size) + 32 * plain.spans.size() + 4 * n_blocks + 64;
  const size_t max_copies = 4 * plain.spans.size() + 2 * n_blocks;
  const size_t words_at = RoundUp(n_blocks * sizeof(BlockIn), 64), copies_at = words_at + RoundUp(n_blocks * 4, 64);
  const size_t tables = copies_at + max_copies * sizeof(BodyCopy) + 64;
  Keep(d_tables, retired_device, tables);
  Keep(h_tables, retired_pinned, tables);
  Keep(d_slots, retired_device, n_blocks * static_cast<size_t>(kSlotStride) + 64);
  Keep(d_out, retired_device, out_cap);

  uint8_t* h = h_tables.get();
  uint8_t* d = d_tables.get();
  std::vector<uint32_t> words(n_blocks);
  if (n_blocks) {
    std::memcpy(h, blocks.data(), n_blocks * sizeof(BlockIn));
    MI_HIP_CHECK(hipMemcpyAsync(d, h, n_blocks * sizeof(BlockIn), hipMemcpyHostToDevice, s));
    MI_HIP_CHECK(device::LaunchLz4CompressBlocks(d_body, reinterpret_cast<const BlockIn*>(d), static_cast<uint32_t>(n_blocks), d_slots.get(),
                                                 reinterpret_cast<uint32_t*>(d + words_at), s));
    MI_HIP_CHECK(hipMemcpyAsync(h + words_at, d + words_at, n_blocks * 4, hipMemcpyDeviceToHost, s));
    MI_HIP_CHECK(hipStreamSynchronize(s));
    std::memcpy(words.data(), h + words_at, n_blocks * 4);
  }
  LayOutCompressedBody(plain, words, &layout);
  if (static_cast<size_t>(layout.body_size) > out_cap || layout.copies.size() > max_copies)
    throw InternalException("compressed body larger than its bound");
  MI_HIP_CHECK(hipMemsetAsync(d_out.get(), 0, static_cast<size_t>(layout.body_size), s));   // padding between buffers
  if (!layout.copies.empty()) {
    std::memcpy(h + copies_at, layout.copies.data(), layout.copies.size() * sizeof(BodyCopy));
    MI_HIP_CHECK(hipMemcpyAsync(d + copies_at, h + copies_at, layout.copies.size() * sizeof(BodyCopy), hipMemcpyHostToDevice, s));
    MI_HIP_CHECK(device::LaunchCompactBody(d_body, d_slots.get(), reinterpret_cast<const BodyCopy*>(d + copies_at),
                                           static_cast<uint32_t>(layout.copies.size()), d_out.get(), s));
  }
}

}  // namespace miarrow

// ---- the verification hook of include/mi_arrow_ipc.h: the serial restatement, no GPU
namespace miarrow {
int WrapC(const std::function<void()>& f);  // c_api.cpp
}

extern "C" int mi_lz4_frame_compress_host(const uint8_t* in, int64_t n, uint8_t* out, int64_t cap, int64_t* size) {
  using namespace miarrow;
  return WrapC([&] {
    if (!size || n < 0 || (!in && n)) throw InvalidInputException("mi_lz4_frame_compress_host: bad argument");
    *size = lz4enc::BufferBound(n);
    if (!out || cap < *size) return;   // *size = the room a call needs
    std::vector<uint8_t> block_out(lz4enc::BlockBound(lz4enc::kBlockSize));
    std::vector<uint32_t> table(lz4enc::kHashSize);
    *size = lz4enc::CompressBufferSerial(in, n, out, cap, block_out.data(), table.data());
  });
}
