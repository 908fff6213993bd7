// HIP helpers shared by the .hip translation units: error plumbing for HIP calls, stream-ordered blocking copies and
// growing device / pinned host buffers.
// HIP only: the .cpp files (built with -x c++) include cc_internal.h, never this header.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "cc_internal.h"

#define CC_HIP(expr)                                                                                         \
  do {                                                                                                       \
    hipError_t e_ = (expr);                                                                                  \
    if (e_ != hipSuccess) return set_error(CC_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                           __FILE__, __LINE__);                                              \
  } while (0)

namespace ccamd {

// Makes `device` the calling thread's device, or says why it cannot be (no device at all, index out of range). Every entry
// point that touches the device starts with it. Defined in cc_detect_api.hip.
cc_status ensure_device(int device);

// A blocking copy that stays off the legacy stream. Plain hipMemcpy / hipMemset are refused while ANY thread of the process
// captures a hipGraph (the detector's single-image path captures one per scale plan) and fail that thread's capture with them;
// stream-ordered copies on a non-blocking stream are not.
inline hipError_t copy_sync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t st) {
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, st);
  return e != hipSuccess ? e : hipStreamSynchronize(st);
}
struct OwnStream {  // for entry points that have no handle to borrow a stream from, and the detector's own streams
  hipStream_t s = nullptr;
  hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
  hipError_t create(int priority) { return hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority); }
  ~OwnStream() {
    if (s) (void)hipStreamDestroy(s);
  }
};
struct OwnEvent {  // move-only: a vector of them may grow
  hipEvent_t e = nullptr;
  OwnEvent() = default;
  OwnEvent(OwnEvent&& o) noexcept : e(o.e) { o.e = nullptr; }
  OwnEvent& operator=(OwnEvent&& o) noexcept { return std::swap(e, o.e), *this; }  // o's destructor ends what this one held
  hipError_t create() { return hipEventCreate(&e); }
  hipError_t create(unsigned flags) { return hipEventCreateWithFlags(&e, flags); }
  ~OwnEvent() {
    if (e) (void)hipEventDestroy(e);
  }
};

// Device buffer of `n` elements. ensure() only grows (contents are not kept); upload() allocates at least one element, so
// that a table's pointer is valid even when the table is empty.
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  hipError_t ensure(size_t count) {
    if (count <= n) return hipSuccess;
    release();
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T));
    if (e == hipSuccess) n = count;
    return e;
  }
  hipError_t upload(const std::vector<T>& v, hipStream_t st) {
    hipError_t e = ensure(std::max<size_t>(v.size(), 1));
    if (e != hipSuccess || v.empty()) return e;
    return hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st);
  }
};

// Pinned host buffer of `bytes` bytes; ensure() only grows (contents are not kept).
struct PinnedBuf {
  void* p = nullptr;
  size_t bytes = 0;
  ~PinnedBuf() {
    if (p) (void)hipHostFree(p);
  }
  hipError_t ensure(size_t b) {
    if (b <= bytes) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
    hipError_t e = hipHostMalloc(&p, b, hipHostMallocDefault);
    if (e == hipSuccess) bytes = b;
    return e;
  }
};

}  // namespace ccamd
