// The arithmetic of the fixed-point bilinear resize (cv::resize INTER_LINEAR_EXACT), in ONE place: the tap
// of one destination index (host tables of the pyramid, cc_host.cpp; per-sample taps of the sample renderer, cc_samples.hip)
// and the two interpolation steps (k_resize in cc_front.hip, k_sample_render and k_info_render in cc_samples.hip).
// Next to it the per-axis arithmetic of cv::resize INTER_AREA: the scale test and the weight table's entries of one
// destination index (the host table cc_area_tab and the threads of k_info_render, cc_samples.hip).
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

// One axis of cv::resize INTER_AREA (OpenCV 4.6.0 resize.cpp, restated): scale = 1 / ((double)dst / src), the
// same form as above; the axis is integer-ratio iff |scale - (int)scale| < DBL_EPSILON (49 -> 1 is not: 1 / (1. / 49) != 49).
struct AreaAxis {
  double scale;
  int iscale;
  bool integer;
};
CC_HD AreaAxis area_axis(int src, int dst) {
  AreaAxis a;
  a.scale = 1.0 / ((double)dst / (double)src);
  a.iscale = (int)a.scale;
  a.integer = fabs(a.scale - (double)a.iscale) < 2.220446049250313e-16 /* DBL_EPSILON */;
  return a;
}

// The entries of destination index d in computeResizeAreaTab(src, dst, scale), in the table's order: source index s1 - 1 with
// weight a_left when `left`, then s1 .. s2 - 1 with a_mid each, then s2 with a_right when `right`. All in double, one
// rounding to float per weight. Every index is inside 0 .. src - 1: `left` needs s1 > fs1 >= 0, and s2 <= src - 1.
struct AreaCell {
  int s1, s2;
  bool left, right;
  float a_left, a_mid, a_right;
};
CC_HD AreaCell area_cell(int src, double scale, int d) {
  const double fs1 = (double)d * scale;
  const double fs2 = fs1 + scale;
  const double rest = (double)src - fs1;
  const double cell = scale < rest ? scale : rest;
  int s1 = (int)ceil(fs1), s2 = (int)floor(fs2);
  s2 = s2 < src - 1 ? s2 : src - 1;
  s1 = s1 < s2 ? s1 : s2;
  AreaCell c;
  c.s1 = s1, c.s2 = s2;
  c.left = (double)s1 - fs1 > 1e-3;
  c.right = fs2 - (double)s2 > 1e-3;
  c.a_left = (float)(((double)s1 - fs1) / cell);
  c.a_mid = (float)(1.0 / cell);
  double r = fs2 - (double)s2;
  r = r < 1.0 ? r : 1.0;
  r = r < cell ? r : cell;
  c.a_right = (float)(r / cell);
  return c;
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
