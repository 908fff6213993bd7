// HOG device code shared by the evaluator's setImage (cc_hog.hip) and the negative miner's HOG kernel (cc_negmine.hip):
// the per-pixel gradient and bin, the two sequential float passes that turn them into the ten integral planes, and one
// variable's value. Both kernels call these functions, so a mined window's planes and values equal setImage's of that
// window by construction. Every translation unit that includes this is compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <mutex>

namespace ccamd {

// ------------------------------------------------------------------------------------------------
// Per-pixel gradient and orientation bin (HOGfeatures.cpp:209-231). One definition for the device kernels and the host
// mirror: every operation is an IEEE basic operation or an explicit fused multiply-add, so both give the same bits.
// ------------------------------------------------------------------------------------------------
// cv::cartToPolar(..., false) -> hal::fastAtan32f (OpenCV 4.6.0, core/src/mathfuncs_core.simd.hpp): polynomial
// coefficients atan2_p1..p7 pre-scaled to degrees, each product rounded to float.
constexpr float kHogP1 = 0.9997878412794807f * (float)(180 / M_PI);
constexpr float kHogP3 = -0.3258083974640975f * (float)(180 / M_PI);
constexpr float kHogP5 = 0.1555786518463281f * (float)(180 / M_PI);
constexpr float kHogP7 = -0.04432655554792128f * (float)(180 / M_PI);

__host__ __device__ inline float hog_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// dx, dy: integer central differences in [-255, 255]. Writes the magnitude and returns the bin in [0, 9).
__host__ __device__ inline int hog_grad_bin(int dx, int dy, float* mag) {
  const float fx = (float)dx, fy = (float)dy;
  *mag = sqrtf(fx * fx + fy * fy);  // hal::magnitude32f; dx^2 + dy^2 < 2^24 is exact in float
  // v_atan_f32::compute: the SIMD body (v_fma, fused on AVX2 / NEON dispatch) is the form restated here
  const float ax = fabsf(fx), ay = fabsf(fy);
  const float c = fminf(ax, ay) / (fmaxf(ax, ay) + (float)DBL_EPSILON);
  const float cc = c * c;
  float a = hog_fma(hog_fma(hog_fma(cc, kHogP7, kHogP5), cc, kHogP3), cc, kHogP1) * c;
  if (ax < ay) a = 90.f - a;
  if (fx < 0.f) a = 180.f - a;
  if (fy < 0.f) a = 360.f - a;
  const float angle = a * (float)(M_PI / 180);  // fastAtan32f's scale for radians
  // HOGfeatures.cpp:218-226: angleScale = (float)(nbins / CV_PI); cvFloor(angle * angleScale - 0.5f), wrapped once
  const float t = angle * (float)(9 / M_PI) - 0.5f;
  int b = (int)floorf(t);
  if (b < 0)
    b += 9;
  else if (b >= 9)
    b -= 9;
  return b;
}

// operator() of one variable (HOGfeatures.h:84-112) on one sample's interleaved planes. Lattice point (i, j) of the block
// (i, j in 0..2 along x, y) is entry (y + j * ch) * (W + 1) + x + i * cw.
__host__ __device__ inline float hog_value_from(float res, float nf) { return res > 0.001f ? res / (nf + 0.001f) : 0.f; }

__host__ __device__ inline float hog_var_value(const float* planes, int sw, const int32_t* blk /* x, y, cw, ch */, int comp) {
  const int cell = comp / 9, bin = comp % 9;
  const int x = blk[0], y = blk[1], cw = blk[2], ch = blk[3];
  const int cx = x + (cell & 1) * cw, cy = y + (cell >> 1) * ch;
  auto at = [&](int px, int py, int chn) { return planes[((size_t)py * sw + px) * 10 + chn]; };
  const float res = ((at(cx, cy, bin) - at(cx + cw, cy, bin)) - at(cx, cy + ch, bin)) + at(cx + cw, cy + ch, bin);
  // normFactor: fastRect[0].p0 - fastRect[1].p1 - fastRect[2].p2 + fastRect[3].p3, the block's outer corners
  const float nf = ((at(x, y, 9) - at(x + 2 * cw, y, 9)) - at(x, y + 2 * ch, 9)) + at(x + 2 * cw, y + 2 * ch, 9);
  return hog_value_from(res, nf);
}

// ------------------------------------------------------------------------------------------------
// LDS of the two kernels that build a window's planes (host). A workgroup gets kHogLdsDefault bytes of dynamic LDS without
// asking and at most kHogLdsMax (the LDS of one CU of gfx950) after the kernel has opted in.
// ------------------------------------------------------------------------------------------------
constexpr size_t kHogLdsDefault = 64 * 1024, kHogLdsMax = 160 * 1024;

struct HogLdsPlan {
  int planes_per_pass;  // k_hog_set_images: planes that go through LDS together; 0: the window is refused
  int set_budget_kib;   // the budget that count was chosen under: 64 or 160
  size_t set_bytes;     // k_hog_set_images' dynamic LDS with that count (of one plane per pass where the window is refused)
  size_t mine_bytes;    // k_negmine_hog's dynamic LDS; cc_negminer_create refuses more than kHogLdsMax
};

// k_hog_set_images: magnitudes [H][W] float, the row sums of P planes [P][H][W + 1] float, bins [H][W] bytes.
// k_negmine_hog: planes [10][H + 1][W + 1] float, magnitudes [H][W] float, bins [H][W] bytes.
// Planes per setImage pass: all ten within 64 KB where they fit, else as many as fit there (no opt-in, several workgroups
// per CU), else as many as 160 KB (one workgroup per CU) holds.
inline HogLdsPlan hog_lds_plan(int W, int H) {
  auto set_lds = [&](int P) { return (size_t)W * H * 4 + (size_t)P * H * (W + 1) * 4 + (size_t)W * H; };
  HogLdsPlan p{0, 0, 0, (size_t)10 * (W + 1) * (H + 1) * 4 + (size_t)W * H * 5};
  for (size_t budget : {kHogLdsDefault, kHogLdsMax}) {
    int P = 10;
    while (P > 0 && set_lds(P) > budget) P--;
    p.planes_per_pass = P;
    p.set_budget_kib = (int)(budget / 1024);
    if (P > 0) break;
  }
  p.set_bytes = set_lds(std::max(p.planes_per_pass, 1));
  return p;
}

// A kernel's opt-in to more than kHogLdsDefault bytes of dynamic LDS is an attribute of the kernel on a device, shared by
// every object that launches it. It is only ever raised: an object created later with a smaller window must not take away
// what an earlier one launches with. One instance per kernel; `device` is the calling thread's current device.
class LdsOptIn {
 public:
  hipError_t raise(const void* kernel, int device, size_t bytes) {
    if (bytes <= kHogLdsDefault) return hipSuccess;
    std::lock_guard<std::mutex> lk(mu_);
    const bool known = device >= 0 && device < kDevices;
    if (known && set_[device] >= bytes) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess && known) set_[device] = bytes;
    return e;
  }

 private:
  static constexpr int kDevices = 64;
  std::mutex mu_;
  size_t set_[kDevices] = {};
};

// ------------------------------------------------------------------------------------------------
// setImage of one window by a workgroup (HOGfeatures.cpp:163-256). The caller places __syncthreads between the steps.
// ------------------------------------------------------------------------------------------------
// Step 1: gradient magnitude and bin of every pixel of the W x H window at px (rows `pitch` bytes apart) into mag / bins
// ([H][W]). BORDER_REPLICATE inside the window: neighbour indices are clamped to the window, as integralHistogram does
// on the copy NegReader::get makes.
__device__ inline void hog_window_grad(const uint8_t* px, size_t pitch, int W, int H, float* mag, uint8_t* bins, int tid, int nthr) {
  for (int i = tid; i < W * H; i += nthr) {
    const int y = i / W, x = i - y * W;
    const int xl = max(x - 1, 0), xr = min(x + 1, W - 1), yu = max(y - 1, 0), yd = min(y + 1, H - 1);
    const int dx = (int)px[(size_t)y * pitch + xr] - (int)px[(size_t)y * pitch + xl];
    const int dy = (int)px[(size_t)yd * pitch + x] - (int)px[(size_t)yu * pitch + x];
    float m;
    bins[i] = (uint8_t)hog_grad_bin(dx, dy, &m);
    mag[i] = m;
  }
}

// Step 2, planes [c0, c0 + P): one lane per (plane, row), the running row sum in float strictly left to right (the
// reference's `strSum += mag`; a parallel scan would reassociate). Row y of plane c goes to
// rp + (c - c0) * plane_stride + y * (W + 1), entries 0 (= 0) .. W.
__device__ inline void hog_row_pass(const float* mag, const uint8_t* bins, int W, int H, int c0, int P, float* rp, size_t plane_stride,
                                    int tid, int nthr) {
  const int sw = W + 1;
  for (int t = tid; t < P * H; t += nthr) {
    const int y = t / P, c = c0 + t % P;
    float* row = rp + (size_t)(c - c0) * plane_stride + (size_t)y * sw;
    const float* mrow = mag + y * W;
    const uint8_t* brow = bins + y * W;
    float s = 0.f;
    row[0] = 0.f;
    if (c == 9) {
      for (int x = 0; x < W; x++) {
        s += mrow[x];
        row[x + 1] = s;
      }
    } else {
      for (int x = 0; x < W; x++) {
        if (brow[x] == c) s += mrow[x];
        row[x + 1] = s;
      }
    }
  }
}

// Step 3, planes [c0, c0 + P): one lane per (plane, column), integral(y + 1, x) = integral(y, x) + rowsum(y, x) top to
// bottom (the reference's `histBuf[x] = histBuf[-histStep + x] + strSum`). out(c, x, y) is the address of entry (x, y),
// y in [0, H], of plane c; it may alias the row sums of step 2 one row down (each lane reads an entry before it writes it).
template <class Out>
__device__ inline void hog_col_pass(const float* rp, size_t plane_stride, int W, int H, int c0, int P, Out out, int tid, int nthr) {
  const int sw = W + 1;
  for (int t = tid; t < P * sw; t += nthr) {
    const int x = t / P, c = c0 + t % P;
    const float* col = rp + (size_t)(c - c0) * plane_stride + x;
    float acc = 0.f;
    *out(c, x, 0) = 0.f;
    for (int y = 0; y < H; y++) {
      acc = acc + col[(size_t)y * sw];
      *out(c, x, y + 1) = acc;
    }
  }
}

}  // namespace ccamd
