// host_codec.hpp -- the host decompressors of compressed IPC bodies: the system's libzstd.so.1 and liblz4.so.1, bound at run
// time (no headers in the image).  `codec` is BodyCompression.codec: 0 LZ4_FRAME, 1 ZSTD.
#pragma once

#include <cstdint>

namespace miarrow {

//! The library of `codec` was found on this host, with every function the reader needs
bool HostCodecAvailable(int32_t codec);
//! The content size the header of a ZSTD frame declares; false when libzstd cannot tell (no such function in the library,
//! a frame without the field, a damaged header)
bool ZstdFrameContentSize(const uint8_t* frame, int64_t frame_len, uint64_t* content_size);
//! One frame of `codec` -> exactly n bytes at dst; IOException (with the decompressor's error name) otherwise
void HostDecompressFrame(int32_t codec, uint8_t* dst, int64_t n, const uint8_t* src, int64_t src_len);

}  // namespace miarrow
