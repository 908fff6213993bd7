// HIP helpers shared by the .hip translation units: error plumbing for HIP calls and stream-ordered blocking copies.
// HIP only: the .cpp files (built with -x c++) include cc_internal.h, never this header.
#pragma once
#include <hip/hip_runtime.h>

#include "cc_internal.h"

#define CC_HIP(expr)                                                                                         \
  do {                                                                                                       \
    hipError_t e_ = (expr);                                                                                  \
    if (e_ != hipSuccess) return set_error(CC_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                           __FILE__, __LINE__);                                              \
  } while (0)

namespace ccamd {

// A blocking copy that stays off the legacy stream. Plain hipMemcpy / hipMemset are refused while ANY thread of the process
// captures a hipGraph (the detector's single-image path captures one per scale plan) and fail that thread's capture with them;
// stream-ordered copies on a non-blocking stream are not.
inline hipError_t copy_sync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t st) {
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, st);
  return e != hipSuccess ? e : hipStreamSynchronize(st);
}
struct OwnStream {  // for entry points that have no handle to borrow a stream from
  hipStream_t s = nullptr;
  hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
  ~OwnStream() {
    if (s) (void)hipStreamDestroy(s);
  }
};

}  // namespace ccamd
