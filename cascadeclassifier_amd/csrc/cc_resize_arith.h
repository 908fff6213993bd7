// The arithmetic of the fixed-point bilinear resize (cv::resize INTER_LINEAR_EXACT), in ONE place: the tap
// of one destination index (host tables of the pyramid, cc_host.cpp; per-sample taps of the sample renderer, cc_samples.hip)
// and the two interpolation steps (k_resize in cc_front.hip, k_sample_render in cc_samples.hip).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIP__)
#define CC_HD __host__ __device__ inline
#else
#define CC_HD inline
#endif

namespace ccamd {

// Left tap and 8.8 weight of the right tap of destination index d: f = scale * (d + 0.5) - 0.5, scale = 1 / ((double)dst / src).
// Outside [0, src - 1) the border pixel is replicated with weight 0. The rounding is cvRound's (half to even).
CC_HD void linear_exact_tap(int src, int dst, int d, int32_t& ofs, uint16_t& w1) {
  const double inv_scale = (double)dst / (double)src;
  const double scale = 1.0 / inv_scale;
  const double f = scale * ((double)d + 0.5) - 0.5;
  const int i = (int)floor(f);
  if (i >= 0 && src > 1 && i < src - 1) {
    ofs = i;
    w1 = (uint16_t)(int)nearbyint((f - (double)i) * 256.0);
  } else {
    ofs = (i >= 0 && src > 1) ? src - 1 : 0;
    w1 = 0;
  }
}

#if defined(__HIP__)  // (only what the compiler itself defines: a host-only HIP compile of cc_host.cpp includes no runtime header)
// Horizontal step: two 8-bit pixels, 8.8 weights w0 + w1 = 256 -> exact in 16 bits.
__device__ inline __attribute__((always_inline)) unsigned resize_lerp_h(unsigned w0, unsigned w1, unsigned a, unsigned b) { return w0 * a + w1 * b; }
// Vertical step on two horizontal results: exact in 32 bits, (v + 2^15) >> 16.
__device__ inline __attribute__((always_inline)) unsigned resize_lerp_v(unsigned w0, unsigned w1, unsigned h0, unsigned h1) {
  return (h0 * w0 + h1 * w1 + (1u << 15)) >> 16;
}
#endif

}  // namespace ccamd
