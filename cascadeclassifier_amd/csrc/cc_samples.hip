// Sample synthesis (section 8 of the header): the positives of the trainer from one object image, as the reference's
// createsamples tool makes them (tools/createsamples/utility.cpp). Two halves:
//   host    cc_sample_plan: cv::RNG, icvRandomQuad with Rodrigues, the 8x8 LU solve of cvGetPerspectiveTransform, the
//           scanline walk of cvWarpPerspective (row spans), the rectangle arithmetic of icvPlaceDistortedSample and the
//           background reader. Serial in the reference too, a few hundred flops per sample.
//   device  k_sampler_prepare (mask, border extension), k_sample_render (warp, blur, resize and blend of a batch of samples,
//           one thread per output pixel), k_warp_dense (the warp alone, cc_warp_perspective_u8).
// The tool's test mode (cvCreateTestSamples: one sample blended into a random rectangle of each background image) adds
// cc_testset_plan on the host and k_testset_render on the device; placement and pixel arithmetic are shared with the above.
// The reference warps image and mask into a (w + 2 (w/2)) x (h + 2 (h/2)) canvas, blurs the mask canvas and resizes a
// rectangle of both to the window. INTER_LINEAR_EXACT reads a 2x2 neighbourhood per output pixel whatever the ratio, so of
// the canvas only 4 image pixels and the 4x4 mask pixels under the blur of those 4 are ever read: the kernel evaluates
// exactly these and the canvas does not exist. A canvas pixel is a pure function of (x, y), the coefficients and the span of
// row y; the spans are the one sequential part (x_min += k_left, row after row) and come from the host.
// The tool's -info mode (cvCreateTrainingSamplesFromInfo: annotated rectangles cut out and resized to the window) has no
// random draw and no plan: cc_area_tab states one axis of INTER_AREA on the host, k_info_render resizes a batch of
// rectangles of any sizes (copy, exact bilinear, integer-ratio and general area) with one thread per window pixel.
// This translation unit is compiled with -ffp-contract=off: a fused multiply-add in the warp or in the area sums changes bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>

#include "cc_detect_internal.h"
#include "cc_resize_arith.h"

namespace ccamd {

// ------------------------------------------------------------------------------------------------
// Host plan
// ------------------------------------------------------------------------------------------------
struct CvRng {  // cv::RNG: multiply-with-carry
  uint64_t state;
  unsigned next() {
    state = (uint64_t)(unsigned)state * 4164903690U + (state >> 32);
    return (unsigned)state;
  }
  int uniform(int a, int b) { return a == b ? a : (int)(next() % (unsigned)(b - a) + (unsigned)a); }
  double uniform(double a, double b) {
    const unsigned t = next();
    const double d = (double)(((uint64_t)t << 32) | next()) * 5.4210108624275221700372640043497e-20;
    return d * (b - a) + a;
  }
  // the float overload: ONE draw, (float)next() scaled by 2^-32 in float, every operation rounded to float
  float uniform(float a, float b) {
    const float f = (float)next() * 2.3283064365386962890625e-10f;
    return f * (b - a) + a;
  }
};

// cvRound: half to even; a value that does not fit an int32 converts to INT_MIN, as cvtsd2si does.
static inline int cv_round(double v) {
  const double r = std::nearbyint(v);
  return (r >= -2147483648.0 && r <= 2147483647.0) ? (int)r : INT_MIN;
}

// cv::Rodrigues of a rotation vector (calib3d, OpenCV 4.6.0): c I + (1 - c) r r^T + s [r]x, r normalised by 1 / theta.
static void rodrigues(const double v[3], double R[9]) {
  const double theta = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  if (theta < DBL_EPSILON) {
    for (int i = 0; i < 9; i++) R[i] = i % 4 == 0 ? 1.0 : 0.0;
    return;
  }
  const double c = std::cos(theta), s = std::sin(theta), c1 = 1.0 - c, it = 1.0 / theta;
  const double r[3] = {v[0] * it, v[1] * it, v[2] * it};
  const double rx[9] = {0, -r[2], r[1], r[2], 0, -r[0], -r[1], r[0], 0};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R[i * 3 + j] = (c * (i == j ? 1.0 : 0.0) + c1 * (r[i] * r[j])) + s * rx[i * 3 + j];
}

// icvRandomQuad (utility.cpp:419-466): four draws, the corners rotated and projected from distance d.
static void random_quad(CvRng& rng, int width, int height, double maxx, double maxy, double maxz, double quad[4][2]) {
  double rv[3], R[9];
  rv[0] = rng.uniform(-maxx, maxx);
  rv[1] = (maxy - std::fabs(rv[0])) * rng.uniform(-1.0, 1.0);
  rv[2] = rng.uniform(-maxz, maxz);
  const double d = (3.0 + 1.0 * rng.uniform(-1.0, 1.0)) * width;
  rodrigues(rv, R);
  const double halfw = 0.5 * width, halfh = 0.5 * height;
  const double corner[4][2] = {{-halfw, -halfh}, {halfw, -halfh}, {halfw, halfh}, {-halfw, halfh}};
  for (int i = 0; i < 4; i++) {
    double v[3];  // cv::gemm's 3x3 by 3x1 case: a[0] b[0] + a[1] b[1] + a[2] b[2], left to right
    for (int k = 0; k < 3; k++) v[k] = (R[k * 3] * corner[i][0] + R[k * 3 + 1] * corner[i][1]) + R[k * 3 + 2] * 0.0;
    quad[i][0] = v[0] * d / (d + v[2]) + halfw;
    quad[i][1] = v[1] * d / (d + v[2]) + halfh;
  }
}

// cvGetPerspectiveTransform (utility.cpp:180-223): the 8x8 system, solved as cv::solve does (hal::LU64f: partial pivoting,
// the first largest |a| wins, rows eliminated with alpha = a[j][i] * (-1 / a[i][i]), back substitution s -= a[i][k] b[k]).
static bool perspective_coeffs(int sw, int sh, const double quad[4][2], double c[9]) {
  double a[8][8], b[8];
  memset(a, 0, sizeof(a));
  memset(b, 0, sizeof(b));
  for (int i = 0; i < 4; i++) {
    a[i][0] = a[i + 4][3] = quad[i][0];
    a[i][1] = a[i + 4][4] = quad[i][1];
    a[i][2] = a[i + 4][5] = 1;
  }
  const int u = sw - 1, v = sh - 1;
  for (int i = 1; i <= 2; i++) a[i][6] = -quad[i][0] * u, a[i][7] = -quad[i][1] * u, b[i] = u;
  for (int i = 2; i <= 3; i++) a[i + 4][6] = -quad[i][0] * v, a[i + 4][7] = -quad[i][1] * v, b[i + 4] = v;
  const int m = 8;
  for (int i = 0; i < m; i++) {
    int k = i;
    for (int j = i + 1; j < m; j++)
      if (std::fabs(a[j][i]) > std::fabs(a[k][i])) k = j;
    if (std::fabs(a[k][i]) < DBL_EPSILON * 100) return false;
    if (k != i) {
      for (int j = i; j < m; j++) std::swap(a[i][j], a[k][j]);
      std::swap(b[i], b[k]);
    }
    const double d = -1 / a[i][i];
    for (int j = i + 1; j < m; j++) {
      const double alpha = a[j][i] * d;
      for (int kk = i + 1; kk < m; kk++) a[j][kk] += alpha * a[i][kk];
      b[j] += alpha * b[i];
    }
  }
  for (int i = m - 1; i >= 0; i--) {
    double s = b[i];
    for (int k = i + 1; k < m; k++) s -= a[i][k] * b[k];
    b[i] = s / a[i][i];
  }
  for (int i = 0; i < 8; i++) c[i] = b[i];
  c[8] = 1;
  return true;
}

// The scanline walk of cvWarpPerspective (utility.cpp:255-416) without its pixels: spans[y] = {ix_min, ix_max} of every row
// the walk visits, {0, -1} elsewhere. The walk accumulates x_min += k_left row after row; that rounding sequence is the
// definition, so it is repeated here and not replaced by a closed form. A row is never visited twice (each segment starts
// one past the rounded end of the one before). false: nonconvex or degenerate (:274-276).
static bool row_spans(const double quad[4][2], int cols, int rows, int32_t* spans) {
  int direction = 0;
  for (int i = 0; i < 4; i++) {
    const int ni = i == 3 ? 0 : i + 1, pi = i == 0 ? 3 : i - 1;
    const double d =
        (quad[i][0] - quad[pi][0]) * (quad[ni][1] - quad[i][1]) - (quad[i][1] - quad[pi][1]) * (quad[ni][0] - quad[i][0]);
    const int cur = d > 0 ? 1 : d < 0 ? -1 : 0;
    if (direction == 0)
      direction = cur;
    else if (direction * cur < 0) {
      direction = 0;
      break;
    }
  }
  if (direction == 0) return false;
  int left = 0;
  for (int i = 1; i < 4; i++)
    if (quad[i][1] < quad[left][1] || (quad[i][1] == quad[left][1] && quad[i][0] < quad[left][0])) left = i;
  double q[4][2];  // clockwise from the topmost (leftmost of two) vertex
  for (int k = 0; k < 4; k++) {
    const int i = direction > 0 ? (left + k) % 4 : (left - k + 4) % 4;
    q[k][0] = quad[i][0];
    q[k][1] = quad[i][1];
  }
  for (int y = 0; y < rows; y++) spans[2 * y] = 0, spans[2 * y + 1] = -1;
  left = 0;
  int right = q[0][1] == q[1][1] ? 1 : 0;
  int next_left = 3, next_right = right + 1;
  double y_min = q[left][1] - 1;
  double k_left, b_left, k_right, b_right;
  auto edge = [&](int a, int b, double& k, double& bb) {
    k = (q[a][0] - q[b][0]) / (q[a][1] - q[b][1]);
    bb = (q[a][1] * q[b][0] - q[a][0] * q[b][1]) / (q[a][1] - q[b][1]);
  };
  edge(left, next_left, k_left, b_left);
  edge(right, next_right, k_right, b_right);
  for (;;) {
    const double y_max = std::min(q[next_left][1], q[next_right][1]);
    const int iy_min = std::max(cv_round(y_min), 0) + 1;
    const int iy_max = std::min(cv_round(y_max), rows - 1);
    double x_min = k_left * iy_min + b_left;
    double x_max = k_right * iy_min + b_right;
    for (int y = iy_min; y <= iy_max; y++) {
      spans[2 * y] = std::max(cv_round(x_min), 0);
      spans[2 * y + 1] = std::min(cv_round(x_max), cols - 1);
      x_min += k_left;
      x_max += k_right;
    }
    if (next_left == next_right || (next_left + 1 == next_right && q[next_left][1] == q[next_right][1])) break;
    if (y_max == q[next_left][1]) {
      left = next_left;
      next_left = left - 1;
      edge(left, next_left, k_left, b_left);
    }
    if (y_max == q[next_right][1]) {
      right = next_right;
      next_right = right + 1;
      edge(right, next_right, k_right, b_right);
    }
    y_min = y_max;
  }
  return true;
}

// icvGetNextFromBackgroundData (utility.cpp:765-831) over image sizes: the pick, the round / offset rule, the first scale.
static bool bg_next_image(cc_sample_bg_reader& r, CvRng& rng, int win_w, int win_h) {
  int ox = 0, oy = 0;
  bool found = false;
  for (int i = 0; i < r.n_images && !found; i++) {
    const int round = r.round;
    r.last = rng.uniform(0, 2147483647 /* RAND_MAX */) % r.n_images;
    r.round += r.last / r.n_images;
    r.round = r.round % (win_w * win_h);
    ox = std::min(round % win_w, r.sizes[2 * r.last] - win_w);
    oy = std::min(round / win_w, r.sizes[2 * r.last + 1] - win_h);
    found = ox >= 0 && oy >= 0;
  }
  if (!found) return false;
  const int w = r.sizes[2 * r.last], h = r.sizes[2 * r.last + 1];
  r.off_x = r.pt_x = ox;
  r.off_y = r.pt_y = oy;
  r.scale = std::max(((float)win_w + r.pt_x) / ((float)w), ((float)win_h + r.pt_y) / ((float)h));
  r.cur_w = (int)(r.scale * w + 0.5F);
  r.cur_h = (int)(r.scale * h + 0.5F);
  r.have = 1;
  return true;
}

// icvGetBackgroundImage (utility.cpp:852-886): the window, then the step to the next one (x, then y, then the scale ladder
// with factor sqrt 2 in float, then a new image).
static bool bg_take(cc_sample_bg_reader& r, CvRng& rng, int win_w, int win_h, cc_sample_record& rec) {
  const float stepfactor = 0.5F, scalefactor = 1.4142135623730950488016887242097F;
  if (!r.have && !bg_next_image(r, rng, win_w, win_h)) return false;
  rec.bg_image = r.last, rec.bg_w = r.cur_w, rec.bg_h = r.cur_h, rec.bg_x = r.pt_x, rec.bg_y = r.pt_y;
  if ((int)(r.pt_x + (1.0F + stepfactor) * win_w) < r.cur_w) {
    r.pt_x += (int)(stepfactor * win_w);
  } else {
    r.pt_x = r.off_x;
    if ((int)(r.pt_y + (1.0F + stepfactor) * win_h) < r.cur_h) {
      r.pt_y += (int)(stepfactor * win_h);
    } else {
      r.pt_y = r.off_y;
      r.scale *= scalefactor;
      if (r.scale <= 1.0F) {
        r.cur_w = (int)(r.scale * r.sizes[2 * r.last]);
        r.cur_h = (int)(r.scale * r.sizes[2 * r.last + 1]);
      } else if (!bg_next_image(r, rng, win_w, win_h)) {
        return false;
      }
    }
  }
  return true;
}

// Limits of the plan and the kernels: source sides 2..8192 (the canvas then has sides up to 16384 and every coordinate
// product fits an int32; a side of 1 has no reflected neighbour for the blur), window sides 1..4096.
constexpr int SAMPLE_SRC_MIN = 2, SAMPLE_SRC_MAX = 8192, SAMPLE_WIN_MAX = 4096;
static bool sample_sizes_ok(int src_w, int src_h, int out_w, int out_h) {
  return src_w >= SAMPLE_SRC_MIN && src_h >= SAMPLE_SRC_MIN && src_w <= SAMPLE_SRC_MAX && src_h <= SAMPLE_SRC_MAX && out_w >= 1 &&
         out_h >= 1 && out_w <= SAMPLE_WIN_MAX && out_h <= SAMPLE_WIN_MAX;
}

// icvPlaceDistortedSample without its pixels (utility.cpp:596-605, :615-648, :658), for a background of out_w x out_h: the
// quad, its coefficients and row spans, the source rectangle, forecolordev. Shared by the training mode (cc_sample_plan)
// and the test mode (cc_testset_plan). R keeps its bg_* fields. Returns why the sample is refused, or nullptr.
static const char* place_sample(int src_w, int src_h, int out_w, int out_h, const cc_sample_params& P, CvRng& rng, int inverse,
                                cc_sample_record& R, int32_t* spans) {
  const int dx = src_w / 2, dy = src_h / 2, cw = src_w + 2 * dx, ch = src_h + 2 * dy;
  double quad[4][2];
  random_quad(rng, src_w, src_h, P.maxxangle, P.maxyangle, P.maxzangle, quad);
  for (int i = 0; i < 4; i++) quad[i][0] += (double)dx, quad[i][1] += (double)dy;
  memcpy(R.quad, quad, sizeof(quad));
  if (!perspective_coeffs(src_w, src_h, quad, R.coeffs)) return "singular system";
  if (!row_spans(quad, cw, ch, spans)) return "Quadrangle is nonconvex or degenerated.";
  // icvPlaceDistortedSample (utility.cpp:615-648): doubles up to the random scale, then float
  int cx = dx, cy = dy, cwid = src_w, chei = src_h;
  if (P.inscribe) {
    cx = (int)std::min(quad[0][0], quad[3][0]);
    cy = (int)std::min(quad[0][1], quad[1][1]);
    cwid = (int)(std::max(quad[1][0], quad[2][0]) + 0.5F) - cx;
    chei = (int)(std::max(quad[2][1], quad[3][1]) + 0.5F) - cy;
  }
  const double xshift = rng.uniform(0., P.maxshift);
  const double yshift = rng.uniform(0., P.maxshift);
  cx -= (int)(xshift * cwid);
  cy -= (int)(yshift * chei);
  cwid = (int)((1.0 + P.maxshift) * cwid);
  chei = (int)((1.0 + P.maxshift) * chei);
  const double randscale = rng.uniform(0., P.maxscale);
  cx -= (int)(0.5 * randscale * cwid);
  cy -= (int)(0.5 * randscale * chei);
  cwid = (int)((1.0 + randscale) * cwid);
  chei = (int)((1.0 + randscale) * chei);
  const float scale = std::max(((float)cwid) / out_w, ((float)chei) / out_h);
  const int rx = (int)(-0.5F * (scale * out_w - cwid) + cx);
  const int ry = (int)(-0.5F * (scale * out_h - chei) + cy);
  const int rw = (int)(scale * out_w), rh = (int)(scale * out_h);
  // roi & Rect(0, 0, canvas)
  const int x0 = std::max(rx, 0), y0 = std::max(ry, 0);
  const int x1 = (int)std::min<int64_t>((int64_t)rx + rw, cw), y1 = (int)std::min<int64_t>((int64_t)ry + rh, ch);
  if (x1 <= x0 || y1 <= y0) return "its source rectangle misses the canvas";
  R.roi_x = x0, R.roi_y = y0, R.roi_w = x1 - x0, R.roi_h = y1 - y0;
  R.inverse = inverse;
  R.forecolordev = rng.uniform(-P.maxintensitydev, P.maxintensitydev);
  return nullptr;
}

// ------------------------------------------------------------------------------------------------
// Device
// ------------------------------------------------------------------------------------------------
// One destination pixel of cvWarpPerspective (utility.cpp:351-387): three dot products and TWO divisions in double (no
// reciprocal: it rounds differently), floor, four taps that read 0 outside the source under four separate range conditions,
// i0 + (i1 - i0) * delta_y truncated to a byte. Coordinates far outside the source (|.| beyond int range included) have all
// four taps out of range; they are folded to -2 before the conversion so that it is defined.
struct WarpCoord {
  int ix, iy;
  double dx, dy;
};
__device__ __forceinline__ WarpCoord warp_coord(const double* __restrict__ c, int x, int y, int sw, int sh) {
  const double div = (c[6] * x + c[7] * y) + c[8];
  const double src_x = ((c[0] * x + c[1] * y) + c[2]) / div;
  const double src_y = ((c[3] * x + c[4] * y) + c[5]) / div;
  const double fx = floor(src_x), fy = floor(src_y);
  WarpCoord w;
  w.ix = (fx >= -2.0 && fx <= (double)sw) ? (int)fx : -2;
  w.iy = (fy >= -2.0 && fy <= (double)sh) ? (int)fy : -2;
  w.dx = src_x - fx;
  w.dy = src_y - fy;
  return w;
}
__device__ __forceinline__ unsigned warp_sample(const uint8_t* __restrict__ src, int sw, int sh, size_t stride, const WarpCoord& w) {
  const bool x_in = w.ix >= 0 && w.ix < sw, x1_in = w.ix >= -1 && w.ix + 1 < sw;
  const bool y_in = w.iy >= 0 && w.iy < sh, y1_in = w.iy >= -1 && w.iy + 1 < sh;
  const uint8_t* r0 = src + (size_t)(y_in ? w.iy : 0) * stride;
  const uint8_t* r1 = src + (size_t)(y1_in ? w.iy + 1 : 0) * stride;
  const int i00 = (x_in && y_in) ? r0[w.ix] : 0, i10 = (x1_in && y_in) ? r0[w.ix + 1] : 0;
  const int i01 = (x_in && y1_in) ? r1[w.ix] : 0, i11 = (x1_in && y1_in) ? r1[w.ix + 1] : 0;
  const double i0 = i00 + (i10 - i00) * w.dx;
  const double i1 = i01 + (i11 - i01) * w.dx;
  return (unsigned)(int)(i0 + (i1 - i0) * w.dy) & 255u;
}

// The byte a canvas or a window without a background is filled with: Mat = Scalar saturates (utility.cpp:607, :992), so
// a bgcolor of 300 fills with 255 and -5 with 0. The mask test and de / dd below take the int as it is (:536-537, :555-556).
__host__ __device__ __forceinline__ unsigned sample_fill(int bgcolor) { return bgcolor < 0 ? 0u : bgcolor > 255 ? 255u : (unsigned)bgcolor; }

// icvStartSampleDistortion (utility.cpp:533-565), one thread per pixel: mask, 3x3 minimum / maximum over the pixels inside
// the image (cv::erode / cv::dilate leave the outside out), border extension with the reference's (uchar) wrap-around.
__global__ __launch_bounds__(256) void k_sampler_prepare(const uint8_t* __restrict__ img, int w, int h, size_t stride, int bgcolor,
                                                         int bgthreshold, uint8_t* __restrict__ src, uint8_t* __restrict__ mask) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  const int p = img[(size_t)y * stride + x];
  const bool bg = bgcolor - bgthreshold <= p && p <= bgcolor + bgthreshold;
  int lo = 255, hi = 0;
  for (int yy = max(y - 1, 0); yy <= min(y + 1, h - 1); yy++)
    for (int xx = max(x - 1, 0); xx <= min(x + 1, w - 1); xx++) {
      const int v = img[(size_t)yy * stride + xx];
      lo = min(lo, v);
      hi = max(hi, v);
    }
  int v = p;
  if (bg) {
    const int de = (bgcolor - lo) & 255, dd = (hi - bgcolor) & 255;
    if (de >= dd && de > bgthreshold) v = lo;
    if (dd > de && dd > bgthreshold) v = hi;
  }
  src[(size_t)y * w + x] = (uint8_t)v;
  mask[(size_t)y * w + x] = bg ? 0 : 255;
}

// BORDER_REFLECT_101 at the canvas edge, then clamped (a canvas side is at least 4, so the clamp only meets coordinates
// whose weight is 0).
__device__ __forceinline__ int reflect101(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * n - 2 - i : i;
  return min(max(i, 0), n - 1);
}

// One output pixel (ox, oy) of a sample placed into an out_w x out_h window whose pixel there is bg: the one pixel
// arithmetic of both render kernels. sp: the sample's row spans.
// The pixel's resize taps (x0, x0 + 1) x (y0, y0 + 1) in the sample's rectangle give the canvas patch of columns
// rx + x0 - 1 .. rx + x0 + 2 and as many rows: the inner 2x2 are the image taps, the 3x3 around each of them the support of
// the blurred mask taps (1-2-1 both ways, (S + 8) >> 4). A tap the resize clamps to the border (x1 == x0) has weight 0, so
// the patch column it gets does not matter. Each patch pixel costs one coordinate evaluation, shared by image and mask.
__device__ __forceinline__ uint8_t sample_pixel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ mask, int sw, int sh,
                                                unsigned fill, const cc_sample_record& R, const int2* __restrict__ sp, int out_w,
                                                int out_h, int ox, int oy, int bg) {
  const int cw = sw + 2 * (sw / 2), ch = sh + 2 * (sh / 2);
  int32_t x0, y0;
  uint16_t wx1, wy1;
  linear_exact_tap(R.roi_w, out_w, ox, x0, wx1);
  linear_exact_tap(R.roi_h, out_h, oy, y0, wy1);
  unsigned iv[2][2], mv[4][4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int y = reflect101(R.roi_y + y0 - 1 + j, ch);
    const int2 span = sp[y];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int x = reflect101(R.roi_x + x0 - 1 + i, cw);
      const bool inside = x >= span.x && x <= span.y;
      const bool centre = (i == 1 || i == 2) && (j == 1 || j == 2);
      unsigned m = 0, v = fill;
      if (inside) {
        const WarpCoord w = warp_coord(R.coeffs, x, y, sw, sh);
        m = warp_sample(mask, sw, sh, sw, w);
        if (centre) v = warp_sample(src, sw, sh, sw, w);
      }
      mv[j][i] = m;
      if (centre) iv[j - 1][i - 1] = v;
    }
  }
  unsigned bl[2][2];  // the blurred mask at the four taps
#pragma unroll
  for (int j = 0; j < 2; j++)
#pragma unroll
    for (int i = 0; i < 2; i++) {
      unsigned acc = 0;
#pragma unroll
      for (int dj = 0; dj < 3; dj++) {
        const unsigned hz = mv[j + dj][i] + 2 * mv[j + dj][i + 1] + mv[j + dj][i + 2];
        acc += (dj == 1 ? 2 : 1) * hz;
      }
      bl[j][i] = (acc + 8) >> 4;
    }
  const unsigned wx0 = 256u - wx1, wy0 = 256u - wy1;
  const unsigned img = resize_lerp_v(wy0, wy1, resize_lerp_h(wx0, wx1, iv[0][0], iv[0][1]), resize_lerp_h(wx0, wx1, iv[1][0], iv[1][1]));
  const unsigned alpha = resize_lerp_v(wy0, wy1, resize_lerp_h(wx0, wx1, bl[0][0], bl[0][1]), resize_lerp_h(wx0, wx1, bl[1][0], bl[1][1]));
  // blend (utility.cpp:660-671)
  int t = min(max(R.forecolordev + (int)img, 0), 255);
  if (R.inverse) t ^= 0xFF;
  return (uint8_t)((t * (int)alpha + (255 - (int)alpha) * bg) / 255);
}

// A batch of samples of one window size: block = 256 output pixels of one sample (blockIdx.y), thread = one output pixel.
__global__ __launch_bounds__(256) void k_sample_render(const uint8_t* __restrict__ src, const uint8_t* __restrict__ mask, int sw, int sh,
                                                       int bgcolor, const cc_sample_record* __restrict__ recs,
                                                       const int2* __restrict__ spans, int out_w, int out_h,
                                                       const uint8_t* __restrict__ backgrounds, uint8_t* __restrict__ out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= out_w * out_h) return;
  const int s = blockIdx.y, oy = p / out_w, ox = p - oy * out_w;
  const int ch = sh + 2 * (sh / 2);
  const unsigned fill = sample_fill(bgcolor);
  const size_t o = (size_t)s * out_w * out_h + p;
  const int bg = backgrounds ? backgrounds[o] : (int)fill;
  out[o] = sample_pixel(src, mask, sw, sh, fill, recs[s], spans + (size_t)s * ch, out_w, out_h, ox, oy, bg);
}

// One test image's rectangle in a batch (cc_sampler_render_testset): where its image copy starts in the batch's output,
// that copy's row pitch in bytes, and the rectangle the sample is blended into.
struct TestsetSlot {
  size_t offset;
  int32_t pitch, x, y, w, h, pad;
};

// A batch of test images whose rectangles differ in size: block = one 256-pixel tile of one rectangle, tiles[blockIdx.x] =
// (sample, first pixel of the tile in the rectangle's row-major order); thread = one rectangle pixel, which it reads from
// the image copy and writes back blended (nobody else touches that byte). The grid has exactly as many blocks as tiles.
__global__ __launch_bounds__(256) void k_testset_render(const uint8_t* __restrict__ src, const uint8_t* __restrict__ mask, int sw, int sh,
                                                        int bgcolor, const cc_sample_record* __restrict__ recs,
                                                        const int2* __restrict__ spans, const TestsetSlot* __restrict__ slots,
                                                        const int2* __restrict__ tiles, uint8_t* out) {
  const int2 tile = tiles[blockIdx.x];
  const int s = tile.x;
  const TestsetSlot L = slots[s];
  const int p = tile.y + threadIdx.x;
  if (p >= L.w * L.h) return;
  const int oy = p / L.w, ox = p - oy * L.w;
  const int ch = sh + 2 * (sh / 2);
  uint8_t* px = out + L.offset + (size_t)(L.y + oy) * L.pitch + (L.x + ox);
  *px = sample_pixel(src, mask, sw, sh, sample_fill(bgcolor), recs[s], spans + (size_t)s * ch, L.w, L.h, ox, oy, (int)*px);
}

// The warp alone into an existing image: thread = one destination pixel, written only inside its row's span.
__global__ __launch_bounds__(256) void k_warp_dense(const uint8_t* __restrict__ src, int sw, int sh, size_t sstride, const double* __restrict__ c,
                                                    const int2* __restrict__ spans, uint8_t* __restrict__ dst, int dw, int dh, size_t dstride) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= dw || y >= dh) return;
  const int2 span = spans[y];
  if (x < span.x || x > span.y) return;
  dst[(size_t)y * dstride + x] = (uint8_t)warp_sample(src, sw, sh, sstride, warp_coord(c, x, y, sw, sh));
}

// ------------------------------------------------------------------------------------------------
// The -info mode (cvCreateTrainingSamplesFromInfo, utility.cpp:1125-1232): annotated rectangles resized to the window
// ------------------------------------------------------------------------------------------------
// How resize(src(Rect), sample, Size(dw, dh), 0, 0, sw >= dw && sh >= dh ? INTER_AREA : INTER_LINEAR_EXACT) treats one
// rectangle (:1205-1208, and cv::resize's own same-size copy and integer-ratio fast path).
enum InfoMode { INFO_COPY = 0, INFO_LINEAR = 1, INFO_AREA_FAST = 2, INFO_AREA = 3 };

// One record of a batch: the first byte of its rectangle in the batch's image buffer, that image's row pitch in bytes, the
// rectangle's sides and its InfoMode. The rectangle alone is the source: nothing outside it is read.
struct InfoSlot {
  size_t src;
  int32_t pitch, w, h, mode;
};

__device__ __forceinline__ uint8_t saturate_round_u8(float v) {  // saturate_cast<uchar>(cvRound(v)): half to even
  return (uint8_t)min(max(__float2int_rn(v), 0), 255);
}

// One window pixel (dx, dy) of an sw x sh rectangle at S.
__device__ __forceinline__ uint8_t info_pixel(const uint8_t* __restrict__ S, size_t pitch, int sw, int sh, int dw, int dh, int mode, int dx,
                                              int dy) {
  if (mode == INFO_COPY) return S[(size_t)dy * pitch + dx];
  if (mode == INFO_LINEAR) {  // two taps per axis, the border replicated at the rectangle's edge
    int32_t x0, y0;
    uint16_t wx1, wy1;
    linear_exact_tap(sw, dw, dx, x0, wx1);
    linear_exact_tap(sh, dh, dy, y0, wy1);
    const int x1 = min(x0 + 1, sw - 1), y1 = min(y0 + 1, sh - 1);
    const uint8_t* r0 = S + (size_t)y0 * pitch;
    const uint8_t* r1 = S + (size_t)y1 * pitch;
    const unsigned wx0 = 256u - wx1, wy0 = 256u - wy1;
    return (uint8_t)resize_lerp_v(wy0, wy1, resize_lerp_h(wx0, wx1, r0[x0], r0[x1]), resize_lerp_h(wx0, wx1, r1[x0], r1[x1]));
  }
  const AreaAxis ax = area_axis(sw, dw), ay = area_axis(sh, dh);
  if (mode == INFO_AREA_FAST) {  // sw == iscale_x * dw and sh == iscale_y * dh (checked on the host): the block is inside
    const int kx = ax.iscale, ky = ay.iscale;
    const uint8_t* p = S + (size_t)(dy * ky) * pitch + (size_t)(dx * kx);
    if (kx == 2 && ky == 2) return (uint8_t)((p[0] + p[1] + p[pitch] + p[pitch + 1] + 2) >> 2);
    int sum = 0;  // below 2^31: the host refuses iscale_x * iscale_y * 255 >= 2^31
    for (int j = 0; j < ky; j++) {
      const uint8_t* r = p + (size_t)j * pitch;
      for (int i = 0; i < kx; i++) sum += r[i];
    }
    const float scale = 1.f / (float)(kx * ky);
    return saturate_round_u8((float)sum * scale);
  }
  // General path, float, in the table's order: per y entry the left-to-right sum over the x entries, then sum += beta * buf.
  // (The first y entry assigns beta * buf; adding it to 0 gives the same float.)
  const AreaCell cx = area_cell(sw, ax.scale, dx), cy = area_cell(sh, ay.scale, dy);
  float sum = 0.f;
  auto add_row = [&](int sy, float beta) {
    const uint8_t* r = S + (size_t)sy * pitch;
    float buf = 0.f;
    if (cx.left) buf += (float)r[cx.s1 - 1] * cx.a_left;
    for (int sx = cx.s1; sx < cx.s2; sx++) buf += (float)r[sx] * cx.a_mid;
    if (cx.right) buf += (float)r[cx.s2] * cx.a_right;
    sum += beta * buf;
  };
  if (cy.left) add_row(cy.s1 - 1, cy.a_left);
  for (int sy = cy.s1; sy < cy.s2; sy++) add_row(sy, cy.a_mid);
  if (cy.right) add_row(cy.s2, cy.a_right);
  return saturate_round_u8(sum);
}

// A batch of rectangles of different sizes and modes: block = one 256-pixel tile of one record's window, tiles[blockIdx.x] =
// (record, first pixel of the tile in the window's row-major order); thread = one window pixel, lanes along dx. The grid has
// exactly as many blocks as tiles.
__global__ __launch_bounds__(256) void k_info_render(const uint8_t* __restrict__ images, const InfoSlot* __restrict__ slots,
                                                     const int2* __restrict__ tiles, int dw, int dh, uint8_t* __restrict__ out) {
  const int2 tile = tiles[blockIdx.x];
  const int p = tile.y + threadIdx.x;
  if (p >= dw * dh) return;
  const InfoSlot L = slots[tile.x];
  const int dy = p / dw, dx = p - dy * dw;
  out[(size_t)tile.x * dw * dh + p] = info_pixel(images + L.src, (size_t)L.pitch, L.w, L.h, dw, dh, L.mode, dx, dy);
}

// Limits of the -info mode: image and rectangle sides 1..8192, window sides 1..4096 (a window has at most 2^24 pixels and
// 65536 tiles; every index product fits an int32).
constexpr int INFO_SIDE_MAX = 8192;

// The InfoMode of an sw x sh rectangle for a dw x dh window, or -1 with *why set.
static int info_mode(int sw, int sh, int dw, int dh, const char** why) {
  if (sw == dw && sh == dh) return INFO_COPY;
  if (!(sw >= dw && sh >= dh)) return INFO_LINEAR;
  const AreaAxis ax = area_axis(sw, dw), ay = area_axis(sh, dh);
  if (!(ax.integer && ay.integer)) return INFO_AREA;
  // the fast path sums a block into an int: the reference's sum would overflow from iscale_x * iscale_y * 255 = 2^31 on
  if ((int64_t)ax.iscale * ay.iscale * 255 >= ((int64_t)1 << 31)) {
    *why = "the integer-ratio block sum passes 2^31";
    return -1;
  }
  // an integer scale of sides this small means an exact multiple; the kernel's block reads rely on it
  if ((int64_t)ax.iscale * dw != sw || (int64_t)ay.iscale * dh != sh) {
    *why = "integer ratio without an exact multiple";
    return -1;
  }
  return INFO_AREA_FAST;
}

static thread_local double g_info_ms[3] = {0.0, 0.0, 0.0};  // upload, kernel, copy back of the thread's last call

}  // namespace ccamd

using namespace ccamd;

struct cc_sampler {
  int device = 0, w = 0, h = 0, bgcolor = 0, bgthreshold = 0;
  OwnStream st;
  DevBuf<uint8_t> src, mask;  // border-extended image and mask, w bytes per row
  struct BgImage {
    int w = 0, h = 0;
    size_t pitch = 0;
    DevBuf<uint8_t> px;
  };
  std::vector<BgImage> bgs;
  // per batch
  DevBuf<cc_sample_record> recs;
  DevBuf<int2> spans;
  DevBuf<uint8_t> bgwin, out, scaled;
  DevBuf<TestsetSlot> slots;  // test mode
  DevBuf<int2> tiles;
};

// One background image at the size a record names, through the pyramid's exact resize (k_resize); the result has
// *pitch bytes per row. Blocks until the kernel has run: the tap tables it reads die with T.
static cc_status scale_background(cc_sampler* s, const cc_sampler::BgImage& b, int dw, int dh, size_t* pitch) {
  FrontTables T;
  T.L = front_layout(b.w, b.h, {make_int2(dw, dh)}, false);
  CC_HIP(T.upload(s->st.s));
  CC_HIP(s->scaled.ensure(T.L.pyr_frame_bytes));
  FrontIO io;
  io.src = b.px.p;
  io.row_stride = b.pitch;
  io.pyr = s->scaled.p;
  launch_front(s->st.s, T, io, 1, FRONT_RESIZE);
  CC_HIP(hipGetLastError());
  CC_HIP(hipStreamSynchronize(s->st.s));
  *pitch = (size_t)T.L.sd[0].pitch8;
  return CC_OK;
}

extern "C" {

cc_status cc_sample_plan(int src_w, int src_h, int out_w, int out_h, const cc_sample_params* params, uint64_t* rng_state,
                         cc_sample_bg_reader* bg, int n, cc_sample_record* records, int32_t* spans) {
  if (!params || !rng_state || !records || n < 0 || !sample_sizes_ok(src_w, src_h, out_w, out_h))
    return set_error(CC_ERR_INVALID_ARG, "cc_sample_plan: bad argument (source sides %d..%d, window sides 1..%d)", SAMPLE_SRC_MIN,
                     SAMPLE_SRC_MAX, SAMPLE_WIN_MAX);
  if (bg && (!bg->sizes || bg->n_images < 1)) return set_error(CC_ERR_INVALID_ARG, "cc_sample_plan: background reader without images");
  const int ch = src_h + 2 * (src_h / 2);
  CvRng rng{*rng_state};
  cc_sample_bg_reader reader;
  if (bg) reader = *bg;
  std::vector<int32_t> own_spans(spans ? 0 : 2 * (size_t)ch);
  for (int s = 0; s < n; s++) {
    cc_sample_record& R = records[s];
    memset(&R, 0, sizeof(R));
    R.bg_image = -1;
    if (bg && !bg_take(reader, rng, out_w, out_h, R))
      return set_error(CC_ERR_INVALID_ARG, "cc_sample_plan: no background image holds a %d x %d window", out_w, out_h);
    int inverse = params->invert;
    if (params->invert == CC_SAMPLE_RANDOM_INVERT) inverse = rng.uniform(0, 2);
    const char* why = place_sample(src_w, src_h, out_w, out_h, *params, rng, inverse, R, spans ? spans + 2 * (size_t)s * ch : own_spans.data());
    if (why) return set_error(CC_ERR_INVALID_ARG, "cc_sample_plan: sample %d: %s", s, why);
  }
  *rng_state = rng.state;
  if (bg) *bg = reader;
  return CC_OK;
}

cc_status cc_testset_plan(int src_w, int src_h, int win_w, int win_h, const cc_sample_params* params, uint64_t* rng_state,
                          cc_sample_bg_reader* bg, double* maxscale, int32_t* iterations_done, int num, int32_t* n_emitted,
                          cc_testset_item* items, cc_sample_record* records, int32_t* spans) {
  if (!params || !rng_state || !bg || !maxscale || !iterations_done || !n_emitted || num < 0 || *iterations_done < 0 ||
      (num && (!items || !records)) || !sample_sizes_ok(src_w, src_h, win_w, win_h))
    return set_error(CC_ERR_INVALID_ARG, "cc_testset_plan: bad argument (source sides %d..%d, window sides 1..%d)", SAMPLE_SRC_MIN,
                     SAMPLE_SRC_MAX, SAMPLE_WIN_MAX);
  if (!bg->sizes || bg->n_images < 1) return set_error(CC_ERR_INVALID_ARG, "cc_testset_plan: background reader without images");
  cc_sample_params P = *params;  // icvPlaceDistortedSample(..., 1, 0.0, 0.0, &data) (utility.cpp:1099-1101)
  P.inscribe = 1, P.maxshift = 0.0, P.maxscale = 0.0;
  const int ch = src_h + 2 * (src_h / 2);
  CvRng rng{*rng_state};
  cc_sample_bg_reader reader = *bg;
  double ms = *maxscale;
  const int first = *iterations_done;
  const int last = (int)std::min<int64_t>((int64_t)first + num, reader.n_images);  // count = MIN(count, cvbgdata->count)
  std::vector<int32_t> own_spans(spans ? 0 : 2 * (size_t)ch);
  int n = 0;
  for (int i = first; i < last; i++) {
    if (!bg_next_image(reader, rng, 10, 10))  // icvInitBackgroundReaders(bgfilename, Size(10, 10)) (:1055)
      return set_error(CC_ERR_INVALID_ARG, "cc_testset_plan: iteration %d: no background image has both sides of 10 or more", i + 1);
    const int cols = reader.sizes[2 * reader.last], rows = reader.sizes[2 * reader.last + 1];
    if (ms < 0.0) ms = std::min(0.7F * cols / win_w, 0.7F * rows / win_h);  // float, assigned once (:1082-1085)
    if (ms < 1.0F) continue;
    const float scale = rng.uniform(1.0F, (float)ms);
    const float fw = scale * win_w, fh = scale * win_h;
    if (!(fw >= 1.0F && fw < SAMPLE_WIN_MAX + 1.0F && fh >= 1.0F && fh < SAMPLE_WIN_MAX + 1.0F))
      return set_error(CC_ERR_INVALID_ARG, "cc_testset_plan: iteration %d: rectangle sides outside 1..%d", i + 1, SAMPLE_WIN_MAX);
    const int width = (int)fw, height = (int)fh;
    const int x = (int)(rng.uniform(0.1, 0.8) * (cols - width));
    const int y = (int)(rng.uniform(0.1, 0.8) * (rows - height));
    if (x < 0 || y < 0 || width > cols - x || height > rows - y)  // the reference's src(Rect(x, y, width, height)) asserts
      return set_error(CC_ERR_INVALID_ARG, "cc_testset_plan: iteration %d: rectangle %d x %d at (%d, %d) leaves its %d x %d image", i + 1,
                       width, height, x, y, cols, rows);
    int inverse = P.invert;
    if (P.invert == CC_SAMPLE_RANDOM_INVERT) inverse = rng.uniform(0, 2);
    cc_sample_record& R = records[n];
    memset(&R, 0, sizeof(R));
    R.bg_image = -1;  // the record's own background fields belong to the training mode's reader
    const char* why = place_sample(src_w, src_h, width, height, P, rng, inverse, R, spans ? spans + 2 * (size_t)n * ch : own_spans.data());
    if (why) return set_error(CC_ERR_INVALID_ARG, "cc_testset_plan: iteration %d: %s", i + 1, why);
    items[n] = cc_testset_item{i + 1, reader.last, x, y, width, height};
    n++;
  }
  *rng_state = rng.state;
  *bg = reader;
  *maxscale = ms;
  *iterations_done = std::max(first, last);
  *n_emitted = n;
  return CC_OK;
}

cc_status cc_sampler_create(int device, const uint8_t* img, int w, int h, size_t stride, int bgcolor, int bgthreshold, cc_sampler** out) {
  if (!out) return set_error(CC_ERR_INVALID_ARG, "cc_sampler_create: out is NULL");
  *out = nullptr;
  // source sides 2..8192: see SAMPLE_SRC_MIN / SAMPLE_SRC_MAX
  if (!img || w < SAMPLE_SRC_MIN || h < SAMPLE_SRC_MIN || w > SAMPLE_SRC_MAX || h > SAMPLE_SRC_MAX || stride < (size_t)w)
    return set_error(CC_ERR_INVALID_ARG, "cc_sampler_create: bad argument (sides %d..%d)", SAMPLE_SRC_MIN, SAMPLE_SRC_MAX);
  cc_status st = ensure_device(device);
  if (st != CC_OK) return st;
  std::unique_ptr<cc_sampler> s(new cc_sampler);
  s->device = device, s->w = w, s->h = h, s->bgcolor = bgcolor, s->bgthreshold = bgthreshold;
  CC_HIP(s->st.create());
  DevBuf<uint8_t> raw;
  const size_t n = (size_t)w * h;
  CC_HIP(raw.ensure(n));
  CC_HIP(s->src.ensure(n));
  CC_HIP(s->mask.ensure(n));
  CC_HIP(hipMemcpy2DAsync(raw.p, w, img, stride, w, h, hipMemcpyHostToDevice, s->st.s));
  hipLaunchKernelGGL(k_sampler_prepare, dim3((w + 63) / 64, (h + 3) / 4), dim3(256), 0, s->st.s, raw.p, w, h, (size_t)w, bgcolor,
                     bgthreshold, s->src.p, s->mask.p);
  CC_HIP(hipGetLastError());
  CC_HIP(hipStreamSynchronize(s->st.s));
  *out = s.release();
  return CC_OK;
}

void cc_sampler_destroy(cc_sampler* s) {
  if (!s) return;
  (void)ensure_device(s->device);
  delete s;
}

cc_status cc_sampler_set_backgrounds(cc_sampler* s, const uint8_t* const* images, const int32_t* widths, const int32_t* heights,
                                     int n_images) {
  // image sides 1..16384 (the pyramid's limit for a source frame is wider); at most 65536 images
  if (!s || n_images < 0 || n_images > 65536 || (n_images && (!images || !widths || !heights)))
    return set_error(CC_ERR_INVALID_ARG, "cc_sampler_set_backgrounds: bad argument");
  for (int i = 0; i < n_images; i++)
    if (!images[i] || widths[i] < 1 || heights[i] < 1 || widths[i] > 16384 || heights[i] > 16384)
      return set_error(CC_ERR_INVALID_ARG, "cc_sampler_set_backgrounds: image %d: sides 1..16384", i);
  cc_status st = ensure_device(s->device);
  if (st != CC_OK) return st;
  std::vector<cc_sampler::BgImage> bgs(n_images);
  for (int i = 0; i < n_images; i++) {
    cc_sampler::BgImage& b = bgs[i];
    b.w = widths[i], b.h = heights[i];
    b.pitch = (size_t)align_up(b.w, 4);
    CC_HIP(b.px.ensure(b.pitch * b.h));
    CC_HIP(hipMemcpy2DAsync(b.px.p, b.pitch, images[i], b.w, b.w, b.h, hipMemcpyHostToDevice, s->st.s));
  }
  CC_HIP(hipStreamSynchronize(s->st.s));
  s->bgs.swap(bgs);
  return CC_OK;
}

cc_status cc_sampler_render(cc_sampler* s, const cc_sample_record* records, const int32_t* spans, int n, int out_w, int out_h,
                            const uint8_t* backgrounds, int max_batch, uint8_t* out) {
  if (!s || n < 0 || (n && (!records || !spans || !out)) || !sample_sizes_ok(s->w, s->h, out_w, out_h))
    return set_error(CC_ERR_INVALID_ARG, "cc_sampler_render: bad argument (window sides 1..%d)", SAMPLE_WIN_MAX);
  const int cw = s->w + 2 * (s->w / 2), ch = s->h + 2 * (s->h / 2);
  const size_t area = (size_t)out_w * out_h;
  bool reader_bg = false;
  for (int i = 0; i < n; i++) {
    const cc_sample_record& R = records[i];
    // the kernel indexes the spans by canvas row and the source by guarded coordinates: the rectangle is what must be inside
    if (R.roi_x < 0 || R.roi_y < 0 || R.roi_w < 1 || R.roi_h < 1 || R.roi_x > cw - R.roi_w || R.roi_y > ch - R.roi_h)
      return set_error(CC_ERR_INVALID_ARG, "cc_sampler_render: record %d: rectangle outside the %d x %d canvas", i, cw, ch);
    if (!backgrounds && R.bg_image != -1) {
      if (R.bg_image < 0 || (size_t)R.bg_image >= s->bgs.size())
        return set_error(CC_ERR_INVALID_ARG, "cc_sampler_render: record %d: background image %d of %zu", i, R.bg_image, s->bgs.size());
      const cc_sampler::BgImage& b = s->bgs[R.bg_image];
      if (R.bg_w < 1 || R.bg_h < 1 || R.bg_w > b.w || R.bg_h > b.h || R.bg_x < 0 || R.bg_y < 0 || R.bg_x > R.bg_w - out_w ||
          R.bg_y > R.bg_h - out_h)
        return set_error(CC_ERR_INVALID_ARG, "cc_sampler_render: record %d: window outside its background", i);
      reader_bg = true;
    }
  }
  cc_status st = ensure_device(s->device);
  if (st != CC_OK) return st;
  if (n == 0) return CC_OK;
  // Batch: a quarter of the free memory over the bytes a sample needs (record, spans, window, output), at most 32768 samples
  // (the sample index is the grid's y, limit 65535) and at most max_batch when the caller gives one.
  const bool with_bg = backgrounds || reader_bg;
  const size_t per_sample = sizeof(cc_sample_record) + (size_t)ch * sizeof(int2) + area * (with_bg ? 2 : 1);
  size_t free_b = 0, total_b = 0;
  CC_HIP(hipMemGetInfo(&free_b, &total_b));
  size_t batch = std::min<size_t>(std::max<size_t>(free_b / 4 / per_sample, 1), 32768);
  batch = std::min<size_t>(batch, (size_t)n);
  if (max_batch > 0) batch = std::min<size_t>(batch, (size_t)max_batch);
  hipStream_t q = s->st.s;
  CC_HIP(s->recs.ensure(batch));
  CC_HIP(s->spans.ensure(batch * ch));
  CC_HIP(s->out.ensure(batch * area));
  if (with_bg) CC_HIP(s->bgwin.ensure(batch * area));
  for (size_t first = 0; first < (size_t)n; first += batch) {
    const size_t nb = std::min(batch, (size_t)n - first);
    CC_HIP(hipMemcpyAsync(s->recs.p, records + first, nb * sizeof(cc_sample_record), hipMemcpyHostToDevice, q));
    CC_HIP(hipMemcpyAsync(s->spans.p, spans + 2 * first * ch, nb * ch * sizeof(int2), hipMemcpyHostToDevice, q));
    if (backgrounds) {
      CC_HIP(hipMemcpyAsync(s->bgwin.p, backgrounds + first * area, nb * area, hipMemcpyHostToDevice, q));
    } else if (reader_bg) {
      // consecutive records share a scaled image until the reader moves on: one resize per run of equal (image, size)
      int cur_i = -2, cur_w = 0, cur_h = 0;
      size_t pitch = 0;
      for (size_t i = 0; i < nb; i++) {
        const cc_sample_record& R = records[first + i];
        uint8_t* slot = s->bgwin.p + i * area;
        if (R.bg_image == -1) {
          CC_HIP(hipMemsetAsync(slot, (int)sample_fill(s->bgcolor), area, q));
          continue;
        }
        if (R.bg_image != cur_i || R.bg_w != cur_w || R.bg_h != cur_h) {
          st = scale_background(s, s->bgs[R.bg_image], R.bg_w, R.bg_h, &pitch);
          if (st != CC_OK) return st;
          cur_i = R.bg_image, cur_w = R.bg_w, cur_h = R.bg_h;
        }
        CC_HIP(hipMemcpy2DAsync(slot, out_w, s->scaled.p + (size_t)R.bg_y * pitch + R.bg_x, pitch, out_w, out_h,
                                hipMemcpyDeviceToDevice, q));
      }
    }
    hipLaunchKernelGGL(k_sample_render, dim3((unsigned)((area + 255) / 256), (unsigned)nb), dim3(256), 0, q, s->src.p, s->mask.p, s->w,
                       s->h, s->bgcolor, s->recs.p, s->spans.p, out_w, out_h, with_bg ? s->bgwin.p : nullptr, s->out.p);
    CC_HIP(hipGetLastError());
    CC_HIP(copy_sync(out + first * area, s->out.p, nb * area, hipMemcpyDeviceToHost, q));
  }
  return CC_OK;
}

cc_status cc_sampler_render_testset(cc_sampler* s, const cc_testset_item* items, const cc_sample_record* records, const int32_t* spans,
                                    int n, int max_batch, uint8_t* const* out_host, void* out_device, size_t frame_stride) {
  if (!s || n < 0 || (n && (!items || !records || !spans || (!out_host && !out_device))))
    return set_error(CC_ERR_INVALID_ARG, "cc_sampler_render_testset: bad argument");
  const int cw = s->w + 2 * (s->w / 2), ch = s->h + 2 * (s->h / 2);
  for (int i = 0; i < n; i++) {
    const cc_testset_item& I = items[i];
    const cc_sample_record& R = records[i];
    if (I.bg_image < 0 || (size_t)I.bg_image >= s->bgs.size())
      return set_error(CC_ERR_INVALID_ARG, "cc_sampler_render_testset: item %d: background image %d of %zu", i, I.bg_image, s->bgs.size());
    const cc_sampler::BgImage& b = s->bgs[I.bg_image];
    // the kernel writes rows y .. y + height - 1, columns x .. x + width - 1 of the image's copy: all of them must be inside
    if (I.width < 1 || I.height < 1 || I.width > SAMPLE_WIN_MAX || I.height > SAMPLE_WIN_MAX || I.x < 0 || I.y < 0 || I.x > b.w - I.width ||
        I.y > b.h - I.height)
      return set_error(CC_ERR_INVALID_ARG, "cc_sampler_render_testset: item %d: rectangle outside its %d x %d image (sides 1..%d)", i, b.w,
                       b.h, SAMPLE_WIN_MAX);
    if (R.roi_x < 0 || R.roi_y < 0 || R.roi_w < 1 || R.roi_h < 1 || R.roi_x > cw - R.roi_w || R.roi_y > ch - R.roi_h)
      return set_error(CC_ERR_INVALID_ARG, "cc_sampler_render_testset: record %d: rectangle outside the %d x %d canvas", i, cw, ch);
    if (out_host && !out_host[i]) return set_error(CC_ERR_INVALID_ARG, "cc_sampler_render_testset: item %d: output pointer is NULL", i);
    if (out_device) {
      const cc_sampler::BgImage& b0 = s->bgs[items[0].bg_image];
      if (b.w != b0.w || b.h != b0.h)
        return set_error(CC_ERR_INVALID_ARG, "cc_sampler_render_testset: a device output needs backgrounds of one size (item %d: %d x %d, item 0: %d x %d)",
                         i, b.w, b.h, b0.w, b0.h);
    }
  }
  if (out_device && n) {
    const cc_sampler::BgImage& b0 = s->bgs[items[0].bg_image];
    if (frame_stride == 0) frame_stride = (size_t)b0.w * b0.h;
    if (frame_stride < (size_t)b0.w * b0.h) return set_error(CC_ERR_INVALID_ARG, "cc_sampler_render_testset: frame_stride below rows * cols");
  }
  cc_status st = ensure_device(s->device);
  if (st != CC_OK) return st;
  if (n == 0) return CC_OK;
  // Batch: items are added while what the batch allocates (record, spans, slot, tiles and, without a device output, the image
  // copy) stays within a quarter of the free memory, at most 32768 items and 2^24 tiles (a rectangle has at most 65536), and
  // at most max_batch when the caller gives one. One item always goes.
  size_t free_b = 0, total_b = 0;
  CC_HIP(hipMemGetInfo(&free_b, &total_b));
  const size_t budget = free_b / 4, max_tiles = (size_t)1 << 24;
  hipStream_t q = s->st.s;
  std::vector<TestsetSlot> slots;
  std::vector<int2> tiles;
  for (size_t first = 0; first < (size_t)n;) {
    slots.clear();
    tiles.clear();
    size_t bytes = 0, image_bytes = 0;
    while (first + slots.size() < (size_t)n) {
      const size_t i = first + slots.size();
      const cc_testset_item& I = items[i];
      const cc_sampler::BgImage& b = s->bgs[I.bg_image];
      const size_t area = (size_t)b.w * b.h, nt = ((size_t)I.width * I.height + 255) / 256;
      const size_t need = sizeof(cc_sample_record) + (size_t)ch * sizeof(int2) + sizeof(TestsetSlot) + nt * sizeof(int2) + (out_device ? 0 : area);
      if (!slots.empty() && (bytes + need > budget || tiles.size() + nt > max_tiles || slots.size() >= 32768 ||
                             (max_batch > 0 && slots.size() >= (size_t)max_batch)))
        break;
      TestsetSlot L;
      L.offset = out_device ? i * frame_stride : image_bytes;
      L.pitch = b.w, L.x = I.x, L.y = I.y, L.w = I.width, L.h = I.height, L.pad = 0;
      for (size_t t = 0; t < nt; t++) tiles.push_back(make_int2((int)slots.size(), (int)(t * 256)));
      slots.push_back(L);
      bytes += need;
      image_bytes += area;
    }
    const size_t nb = slots.size();
    CC_HIP(s->recs.ensure(nb));
    CC_HIP(s->spans.ensure(nb * ch));
    if (!out_device) CC_HIP(s->out.ensure(image_bytes));
    uint8_t* base = out_device ? (uint8_t*)out_device : s->out.p;
    CC_HIP(hipMemcpyAsync(s->recs.p, records + first, nb * sizeof(cc_sample_record), hipMemcpyHostToDevice, q));
    CC_HIP(hipMemcpyAsync(s->spans.p, spans + 2 * first * ch, nb * ch * sizeof(int2), hipMemcpyHostToDevice, q));
    CC_HIP(s->slots.upload(slots, q));
    CC_HIP(s->tiles.upload(tiles, q));
    for (size_t i = 0; i < nb; i++) {  // a fresh copy per item: two items of one image do not see each other
      const cc_sampler::BgImage& b = s->bgs[items[first + i].bg_image];
      CC_HIP(hipMemcpy2DAsync(base + slots[i].offset, b.w, b.px.p, b.pitch, b.w, b.h, hipMemcpyDeviceToDevice, q));
    }
    hipLaunchKernelGGL(k_testset_render, dim3((unsigned)tiles.size()), dim3(256), 0, q, s->src.p, s->mask.p, s->w, s->h, s->bgcolor,
                       s->recs.p, s->spans.p, s->slots.p, s->tiles.p, base);
    CC_HIP(hipGetLastError());
    if (out_host)
      for (size_t i = 0; i < nb; i++) {
        const cc_sampler::BgImage& b = s->bgs[items[first + i].bg_image];
        CC_HIP(hipMemcpyAsync(out_host[first + i], base + slots[i].offset, (size_t)b.w * b.h, hipMemcpyDeviceToHost, q));
      }
    CC_HIP(hipStreamSynchronize(q));  // slots and tiles are host memory of this frame, the device buffers are reused
    first += nb;
  }
  return CC_OK;
}

cc_status cc_warp_perspective_u8(int device, const uint8_t* src, int sw, int sh, size_t sstride, uint8_t* dst, int dw, int dh,
                                 size_t dstride, const double* quad) {
  // sides 1..16384: coordinates and their products stay far inside an int32
  if (!src || !dst || !quad || sw < 1 || sh < 1 || dw < 1 || dh < 1 || sw > 16384 || sh > 16384 || dw > 16384 || dh > 16384 ||
      sstride < (size_t)sw || dstride < (size_t)dw)
    return set_error(CC_ERR_INVALID_ARG, "cc_warp_perspective_u8: bad argument (sides 1..16384)");
  double q[4][2], c[9];
  memcpy(q, quad, sizeof(q));
  for (int i = 0; i < 8; i++)
    if (!std::isfinite(quad[i])) return set_error(CC_ERR_INVALID_ARG, "cc_warp_perspective_u8: quad is not finite");
  std::vector<int32_t> spans(2 * (size_t)dh);
  if (!row_spans(q, dw, dh, spans.data())) return set_error(CC_ERR_INVALID_ARG, "cc_warp_perspective_u8: Quadrangle is nonconvex or degenerated.");
  if (!perspective_coeffs(sw, sh, q, c)) return set_error(CC_ERR_INVALID_ARG, "cc_warp_perspective_u8: singular system");
  cc_status st = ensure_device(device);
  if (st != CC_OK) return st;
  OwnStream own;  // not the legacy stream: see copy_sync
  CC_HIP(own.create());
  DevBuf<uint8_t> d_src, d_dst;
  DevBuf<double> d_c;
  DevBuf<int2> d_spans;
  CC_HIP(d_src.ensure((size_t)sw * sh));
  CC_HIP(d_dst.ensure((size_t)dw * dh));
  CC_HIP(d_c.ensure(9));
  CC_HIP(d_spans.ensure(dh));
  CC_HIP(hipMemcpy2DAsync(d_src.p, sw, src, sstride, sw, sh, hipMemcpyHostToDevice, own.s));
  CC_HIP(hipMemcpy2DAsync(d_dst.p, dw, dst, dstride, dw, dh, hipMemcpyHostToDevice, own.s));
  CC_HIP(hipMemcpyAsync(d_c.p, c, sizeof(c), hipMemcpyHostToDevice, own.s));
  CC_HIP(hipMemcpyAsync(d_spans.p, spans.data(), spans.size() * sizeof(int32_t), hipMemcpyHostToDevice, own.s));
  hipLaunchKernelGGL(k_warp_dense, dim3((dw + 63) / 64, (dh + 3) / 4), dim3(256), 0, own.s, d_src.p, sw, sh, (size_t)sw, d_c.p, d_spans.p,
                     d_dst.p, dw, dh, (size_t)dw);
  CC_HIP(hipGetLastError());
  CC_HIP(hipMemcpy2DAsync(dst, dstride, d_dst.p, dw, dw, dh, hipMemcpyDeviceToHost, own.s));
  CC_HIP(hipStreamSynchronize(own.s));  // c and spans are host memory of this frame: nothing outlives the call
  return CC_OK;
}

cc_status cc_area_tab(int ssize, int dsize, double* scale, int32_t* iscale, int32_t* is_integer, int32_t* dst_index, int32_t* src_index,
                      float* alpha, int capacity, int32_t* n_entries) {
  // an area resize shrinks or keeps: 1 <= dsize <= ssize <= 8192
  if (ssize < 1 || dsize < 1 || dsize > ssize || ssize > INFO_SIDE_MAX || capacity < 0 || !n_entries ||
      (capacity && (!dst_index || !src_index || !alpha)))
    return set_error(CC_ERR_INVALID_ARG, "cc_area_tab: bad argument (1 <= dsize <= ssize <= %d)", INFO_SIDE_MAX);
  const AreaAxis a = area_axis(ssize, dsize);
  if (scale) *scale = a.scale;
  if (iscale) *iscale = a.iscale;
  if (is_integer) *is_integer = a.integer ? 1 : 0;
  int k = 0;
  auto emit = [&](int d, int s, float w) {
    if (k < capacity) dst_index[k] = d, src_index[k] = s, alpha[k] = w;
    k++;
  };
  for (int d = 0; d < dsize; d++) {
    const AreaCell c = area_cell(ssize, a.scale, d);
    if (c.left) emit(d, c.s1 - 1, c.a_left);
    for (int s = c.s1; s < c.s2; s++) emit(d, s, c.a_mid);
    if (c.right) emit(d, c.s2, c.a_right);
  }
  *n_entries = k;
  if (k > capacity) return set_error(CC_ERR_BUFFER_TOO_SMALL, "cc_area_tab: %d entries, room for %d", k, capacity);
  return CC_OK;
}

cc_status cc_samples_from_info(int device, const uint8_t* const* images, const int32_t* widths, const int32_t* heights,
                               const size_t* strides, int n_images, const cc_info_record* records, int n, int win_w, int win_h,
                               int max_batch, uint8_t* out_host, void* out_device) {
  g_info_ms[0] = g_info_ms[1] = g_info_ms[2] = 0.0;
  if (n < 0 || n_images < 0 || (n_images && (!images || !widths || !heights || !strides)) || (n && (!records || (!out_host && !out_device))))
    return set_error(CC_ERR_INVALID_ARG, "cc_samples_from_info: bad argument");
  // window sides 1..4096
  if (win_w < 1 || win_h < 1 || win_w > SAMPLE_WIN_MAX || win_h > SAMPLE_WIN_MAX)
    return set_error(CC_ERR_INVALID_ARG, "cc_samples_from_info: window sides 1..%d", SAMPLE_WIN_MAX);
  // image sides 1..8192, and with them a rectangle's
  for (int i = 0; i < n_images; i++)
    if (!images[i] || widths[i] < 1 || heights[i] < 1 || widths[i] > INFO_SIDE_MAX || heights[i] > INFO_SIDE_MAX || strides[i] < (size_t)widths[i])
      return set_error(CC_ERR_INVALID_ARG, "cc_samples_from_info: image %d: sides 1..%d, stride at least the width", i, INFO_SIDE_MAX);
  std::vector<int32_t> modes((size_t)n);
  for (int i = 0; i < n; i++) {
    const cc_info_record& R = records[i];
    if (R.image < 0 || R.image >= n_images)
      return set_error(CC_ERR_INVALID_ARG, "cc_samples_from_info: record %d: image %d of %d", i, R.image, n_images);
    // the kernel reads rows y .. y + height - 1, columns x .. x + width - 1 of the image: all of them must be inside
    const int iw = widths[R.image], ih = heights[R.image];
    if (R.width < 1 || R.height < 1 || R.x < 0 || R.y < 0 || R.x > iw - R.width || R.y > ih - R.height)
      return set_error(CC_ERR_INVALID_ARG, "cc_samples_from_info: record %d: rectangle %d x %d at (%d, %d) leaves its %d x %d image", i,
                       R.width, R.height, R.x, R.y, iw, ih);
    const char* why = nullptr;
    modes[i] = info_mode(R.width, R.height, win_w, win_h, &why);
    if (modes[i] < 0)
      return set_error(CC_ERR_INVALID_ARG, "cc_samples_from_info: record %d: %d x %d to %d x %d: %s", i, R.width, R.height, win_w, win_h, why);
  }
  cc_status st = ensure_device(device);
  if (st != CC_OK) return st;
  if (n == 0) return CC_OK;
  OwnStream own;
  CC_HIP(own.create());
  hipStream_t q = own.s;
  OwnEvent ev[4];
  for (OwnEvent& e : ev) CC_HIP(e.create());
  // Batch: consecutive records are added while what the batch allocates (each image it names once, slot, tiles and, without
  // a device output, the windows) stays within a quarter of the free memory, at most 2^20 records and 2^24 tiles (a window
  // has at most 65536), and at most max_batch records when the caller gives one. One record always goes.
  size_t free_b = 0, total_b = 0;
  CC_HIP(hipMemGetInfo(&free_b, &total_b));
  const size_t budget = free_b / 4, max_tiles = (size_t)1 << 24, max_records = (size_t)1 << 20;
  const size_t area = (size_t)win_w * win_h, nt = (area + 255) / 256;
  DevBuf<uint8_t> d_images, d_out;
  DevBuf<InfoSlot> d_slots;
  DevBuf<int2> d_tiles;
  std::vector<InfoSlot> slots;
  std::vector<int2> tiles;
  std::vector<int64_t> where((size_t)n_images, -1);  // an image's offset in this batch's buffer
  std::vector<int> used;
  for (size_t first = 0; first < (size_t)n;) {
    slots.clear();
    tiles.clear();
    for (int i : used) where[i] = -1;
    used.clear();
    size_t bytes = 0, image_bytes = 0;
    while (first + slots.size() < (size_t)n) {
      const size_t i = first + slots.size();
      const cc_info_record& R = records[i];
      const size_t img = where[R.image] < 0 ? (size_t)widths[R.image] * heights[R.image] : 0;
      const size_t need = img + sizeof(InfoSlot) + nt * sizeof(int2) + (out_device ? 0 : area);
      if (!slots.empty() && (bytes + need > budget || tiles.size() + nt > max_tiles || slots.size() >= max_records ||
                             (max_batch > 0 && slots.size() >= (size_t)max_batch)))
        break;
      if (where[R.image] < 0) {
        where[R.image] = (int64_t)image_bytes;
        used.push_back(R.image);
        image_bytes += img;
      }
      InfoSlot L;
      L.pitch = widths[R.image];  // the device copy is dense
      L.src = (size_t)where[R.image] + (size_t)R.y * L.pitch + R.x;
      L.w = R.width, L.h = R.height, L.mode = modes[i];
      for (size_t t = 0; t < nt; t++) tiles.push_back(make_int2((int)slots.size(), (int)(t * 256)));
      slots.push_back(L);
      bytes += need;
    }
    const size_t nb = slots.size();
    CC_HIP(d_images.ensure(image_bytes));
    if (!out_device) CC_HIP(d_out.ensure(nb * area));
    uint8_t* base = out_device ? (uint8_t*)out_device + first * area : d_out.p;
    CC_HIP(hipEventRecord(ev[0].e, q));
    for (int i : used)
      CC_HIP(hipMemcpy2DAsync(d_images.p + where[i], widths[i], images[i], strides[i], widths[i], heights[i], hipMemcpyHostToDevice, q));
    CC_HIP(d_slots.upload(slots, q));
    CC_HIP(d_tiles.upload(tiles, q));
    CC_HIP(hipEventRecord(ev[1].e, q));
    hipLaunchKernelGGL(k_info_render, dim3((unsigned)tiles.size()), dim3(256), 0, q, d_images.p, d_slots.p, d_tiles.p, win_w, win_h, base);
    CC_HIP(hipGetLastError());
    CC_HIP(hipEventRecord(ev[2].e, q));
    if (out_host) CC_HIP(hipMemcpyAsync(out_host + first * area, base, nb * area, hipMemcpyDeviceToHost, q));
    CC_HIP(hipEventRecord(ev[3].e, q));
    CC_HIP(hipStreamSynchronize(q));  // slots and tiles are host memory of this frame, the device buffers are reused
    for (int k = 0; k < 3; k++) {
      float ms = 0.f;
      CC_HIP(hipEventElapsedTime(&ms, ev[k].e, ev[k + 1].e));
      g_info_ms[k] += (double)ms;
    }
    first += nb;
  }
  return CC_OK;
}

cc_status cc_samples_from_info_last_ms(double* upload_ms, double* kernel_ms, double* download_ms) {
  if (upload_ms) *upload_ms = g_info_ms[0];
  if (kernel_ms) *kernel_ms = g_info_ms[1];
  if (download_ms) *download_ms = g_info_ms[2];
  return CC_OK;
}

cc_status cc_resize_area_u8(int device, const uint8_t* src, int w, int h, size_t stride, uint8_t* dst, int dw, int dh) {
  // INTER_AREA proper: the window is no larger than the source on either axis (cv::resize would interpolate otherwise)
  if (!src || !dst || w < 1 || h < 1 || dw < 1 || dh < 1 || dw > w || dh > h)
    return set_error(CC_ERR_INVALID_ARG, "cc_resize_area_u8: bad argument (1 <= dw <= w, 1 <= dh <= h)");
  const int32_t iw = w, ih = h;
  const cc_info_record whole = {0, 0, 0, w, h};
  return cc_samples_from_info(device, &src, &iw, &ih, &stride, 1, &whole, 1, dw, dh, 0, dst, nullptr);
}

}  // extern "C"
