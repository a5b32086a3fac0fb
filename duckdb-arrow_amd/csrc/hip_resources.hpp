// hip_resources.hpp -- owners of the HIP resources the host code creates: HBM and pinned buffers, events, streams.
// Move-only; the destructor releases what it owns and ignores the result (a destructor cannot report, and a failed free
// leaves nothing to retry).  An empty owner holds nothing and releases nothing.
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>

#include "ipc_format.hpp"

namespace miarrow {

#define MI_HIP_CHECK(expr)                                                                                  \
  do {                                                                                                      \
    hipError_t _e = (expr);                                                                                 \
    if (_e != hipSuccess) {                                                                                 \
      throw ::miarrow::Exception(_e == hipErrorOutOfMemory ? MI_ENOMEM : MI_EIO,                            \
                                 std::string(#expr) + " failed: " + hipGetErrorString(_e));                 \
    }                                                                                                       \
  } while (0)

//! One hipMalloc (kPinned = false) or hipHostMalloc (true) allocation of size() bytes.
template <bool kPinned>
class HipBuffer {
 public:
  HipBuffer() = default;
  explicit HipBuffer(size_t bytes) {
    if (kPinned) MI_HIP_CHECK(hipHostMalloc(&p_, bytes, hipHostMallocDefault));
    else MI_HIP_CHECK(hipMalloc(&p_, bytes));
    bytes_ = bytes;
  }
  HipBuffer(HipBuffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  HipBuffer& operator=(HipBuffer o) noexcept {   // the allocation held before goes with `o`
    std::swap(p_, o.p_);
    std::swap(bytes_, o.bytes_);
    return *this;
  }
  ~HipBuffer() {
    if (!p_) return;
    if (kPinned) (void)hipHostFree(p_);
    else (void)hipFree(p_);
  }
  template <typename T = uint8_t>
  T* get() const { return static_cast<T*>(p_); }
  size_t size() const { return bytes_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  void* p_ = nullptr;
  size_t bytes_ = 0;
};
using DeviceBuffer = HipBuffer<false>;
using PinnedBuffer = HipBuffer<true>;

//! When `buf` is empty or holds fewer than `need` bytes, it becomes a new allocation of `new_cap` bytes that starts with
//! the first `keep_bytes` of the old one (pinned buffers only), and the old allocation is returned: the caller frees it at
//! once (lets it go) or keeps it.  The returned buffer is empty when nothing grew or there was nothing before.
template <bool kPinned>
HipBuffer<kPinned> Grow(HipBuffer<kPinned>& buf, size_t need, size_t new_cap, size_t keep_bytes = 0) {
  if (buf && need <= buf.size()) return {};
  HipBuffer<kPinned> grown(new_cap);
  if (kPinned && buf && keep_bytes) std::memcpy(grown.get(), buf.get(), std::min(keep_bytes, buf.size()));
  std::swap(buf, grown);
  return grown;   // now the outgrown one
}

//! One event or stream; converts to the raw handle for HIP calls.
template <typename Handle, hipError_t (*Destroy)(Handle)>
class HipHandle {
 public:
  HipHandle() = default;
  HipHandle(HipHandle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  HipHandle& operator=(HipHandle o) noexcept {
    std::swap(h_, o.h_);
    return *this;
  }
  ~HipHandle() {
    if (h_) (void)Destroy(h_);
  }
  operator Handle() const { return h_; }

 protected:
  Handle h_ = nullptr;
};

class HipEvent : public HipHandle<hipEvent_t, hipEventDestroy> {
 public:
  static HipEvent Create() {   // without timing: the library's events only order streams and say "done"
    HipEvent e;
    MI_HIP_CHECK(hipEventCreateWithFlags(&e.h_, hipEventDisableTiming));
    return e;
  }
  static HipEvent CreateTimed() {   // for the entry points that report a kernel time
    HipEvent e;
    MI_HIP_CHECK(hipEventCreate(&e.h_));
    return e;
  }
};

class HipStream : public HipHandle<hipStream_t, hipStreamDestroy> {
 public:
  static HipStream Create() {   // non-blocking: not ordered with the null stream
    HipStream s;
    MI_HIP_CHECK(hipStreamCreateWithFlags(&s.h_, hipStreamNonBlocking));
    return s;
  }
};

}  // namespace miarrow
