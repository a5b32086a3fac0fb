// host_codec.cpp -- see host_codec.hpp.
#include "host_codec.hpp"

#include <dlfcn.h>

#include <memory>
#include <string>

#include "ipc_format.hpp"

namespace miarrow {

// Body compression (Message.fbs BodyCompression, method BUFFER): every buffer is `int64 uncompressed_length` (-1 = the
// bytes that follow are stored raw) + one frame.  The reference decompresses ZSTD on the CPU with DuckDB's bundled zstd
// (DuckDBDecompressZstd, base_stream_reader.cpp:11-32) and registers no LZ4 function (:37-50); here the system's
// libzstd.so.1 is bound at run time (no headers in the image).
namespace {
struct ZstdApi {
  size_t (*decompress)(void*, size_t, const void*, size_t) = nullptr;
  unsigned (*is_error)(size_t) = nullptr;
  const char* (*error_name)(size_t) = nullptr;
  unsigned long long (*frame_content_size)(const void*, size_t) = nullptr;  // optional
  bool ok = false;
};
const ZstdApi& Zstd() {
  static ZstdApi api = [] {
    ZstdApi a;
    void* h = dlopen("libzstd.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("libzstd.so", RTLD_NOW | RTLD_LOCAL);
    if (h) {
      a.decompress = reinterpret_cast<size_t (*)(void*, size_t, const void*, size_t)>(dlsym(h, "ZSTD_decompress"));
      a.is_error = reinterpret_cast<unsigned (*)(size_t)>(dlsym(h, "ZSTD_isError"));
      a.error_name = reinterpret_cast<const char* (*)(size_t)>(dlsym(h, "ZSTD_getErrorName"));
      a.frame_content_size = reinterpret_cast<unsigned long long (*)(const void*, size_t)>(dlsym(h, "ZSTD_getFrameContentSize"));
      a.ok = a.decompress && a.is_error && a.error_name;
    }
    return a;
  }();
  return api;
}
// LZ4_FRAME (codec 0; what Feather V2 files use by default): the reference registers no LZ4 function, so it rejects these
// bodies; here the system's liblz4.so.1 frame API is bound at run time when it exists.
struct Lz4Api {
  size_t (*create)(void**, unsigned) = nullptr;
  size_t (*free_ctx)(void*) = nullptr;
  size_t (*decompress)(void*, void*, size_t*, const void*, size_t*, const void*) = nullptr;
  unsigned (*is_error)(size_t) = nullptr;
  const char* (*error_name)(size_t) = nullptr;
  bool ok = false;
};
const Lz4Api& Lz4() {
  static Lz4Api api = [] {
    Lz4Api a;
    void* h = dlopen("liblz4.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("liblz4.so", RTLD_NOW | RTLD_LOCAL);
    if (h) {
      a.create = reinterpret_cast<size_t (*)(void**, unsigned)>(dlsym(h, "LZ4F_createDecompressionContext"));
      a.free_ctx = reinterpret_cast<size_t (*)(void*)>(dlsym(h, "LZ4F_freeDecompressionContext"));
      a.decompress = reinterpret_cast<size_t (*)(void*, void*, size_t*, const void*, size_t*, const void*)>(dlsym(h, "LZ4F_decompress"));
      a.is_error = reinterpret_cast<unsigned (*)(size_t)>(dlsym(h, "LZ4F_isError"));
      a.error_name = reinterpret_cast<const char* (*)(size_t)>(dlsym(h, "LZ4F_getErrorName"));
      a.ok = a.create && a.free_ctx && a.decompress && a.is_error && a.error_name;
    }
    return a;
  }();
  return api;
}

}  // namespace

bool HostCodecAvailable(int32_t codec) { return codec == 0 ? Lz4().ok : codec == 1 && Zstd().ok; }

bool ZstdFrameContentSize(const uint8_t* frame, int64_t frame_len, uint64_t* content_size) {
  const ZstdApi& z = Zstd();
  if (!z.frame_content_size) return false;
  *content_size = z.frame_content_size(frame, static_cast<size_t>(frame_len));
  return *content_size < 0xFFFFFFFFFFFFFFFEull;   // ZSTD_CONTENTSIZE_UNKNOWN, ZSTD_CONTENTSIZE_ERROR
}

void HostDecompressFrame(int32_t codec, uint8_t* dst, int64_t n, const uint8_t* src, int64_t src_len) {
  if (codec == 1) {
    const ZstdApi& z = Zstd();
    const size_t code = z.decompress(dst, static_cast<size_t>(n), src, static_cast<size_t>(src_len));
    if (z.is_error(code)) {
      throw IOException("ZSTD_decompress([buffer with " + std::to_string(src_len) + " bytes] -> [buffer with " + std::to_string(n) +
                        " bytes]) failed with error '" + z.error_name(code) + "'");
    }
    if (static_cast<int64_t>(code) != n)
      throw IOException("Expected decompressed size of " + std::to_string(n) + " bytes but got " + std::to_string(code) + " bytes");
    return;
  }
  const Lz4Api& z = Lz4();
  void* dctx = nullptr;
  size_t rc = z.create(&dctx, 100 /* LZ4F_VERSION */);
  if (z.is_error(rc)) throw IOException(std::string("LZ4F_createDecompressionContext failed: ") + z.error_name(rc));
  std::shared_ptr<void> guard(dctx, [&z](void* p) { z.free_ctx(p); });
  size_t produced = 0, consumed = 0;
  while (true) {
    size_t dst_size = static_cast<size_t>(n) - produced, src_size = static_cast<size_t>(src_len) - consumed;
    rc = z.decompress(dctx, dst + produced, &dst_size, src + consumed, &src_size, nullptr);
    if (z.is_error(rc)) {
      throw IOException("LZ4F_decompress([buffer with " + std::to_string(src_len) + " bytes] -> [buffer with " + std::to_string(n) +
                        " bytes]) failed with error '" + z.error_name(rc) + "'");
    }
    produced += dst_size;
    consumed += src_size;
    if (rc == 0) break;                             // frame complete
    if (dst_size == 0 && src_size == 0) break;      // no progress: truncated frame or output full
  }
  if (static_cast<int64_t>(produced) != n || rc != 0)
    throw IOException("Expected decompressed size of " + std::to_string(n) + " bytes but got " + std::to_string(produced) + " bytes");
}

}  // namespace miarrow
