// Negative mining for cascade training on gfx950 (the reference's NegReader): every window of a background image's scale
// ladder is run through the cascade trained so far, and the windows that pass are copied out as new negatives. The ladder
// levels come from the shared front end (cc_front.hip); the window kernels read the integral images from global memory
// (k_negmine_windows, k_negmine_wave) or build HOG planes per window in LDS (k_negmine_hog). Entry points cc_negminer_*.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <future>
#include <memory>

#include "cc_detect_internal.h"
#include "cc_hog_device.h"
#include "cc_train_device.h"

namespace ccamd {

// ------------------------------------------------------------------------------------------------
// Negative mining (training side): one thread per window of the reader's stream; integrals are read from global
// memory (windows sit half a window apart, there is little to share), geometry -> offsets on the fly because every
// ladder level has its own row pitch. Arithmetic is the trainer's: value = calc / normfactor, `<=` goes left.
// ------------------------------------------------------------------------------------------------
struct MineLevel {
  int w, h, pitchI, nx, ny;
  long long int_ofs, img_ofs;
  long long win_first;
  int pitch8;
  int pad;
};
struct MineNode {  // a tree node with its feature's geometry
  int r[3][4];
  float w[3];
  int tilted;
  float thr;
  int left, right;  // child > 0: node index inside the tree; child <= 0: leaf index -child
  int subset[8];
  int pad;
};
struct MineArgs {
  const int32_t* integ;  // channels: 0 sum, 1 sqsum (Haar), 2 tilted (if any)
  size_t chan_elems;
  const MineLevel* levels;
  int n_levels;
  long long n_windows;
  int W0, H0, ox, oy, sx, sy;
  WalkTables walk;
  const MineNode* nodes;
  uint8_t* pass;   // [image][n_windows]
  int nchan;       // channels per image in integ: image f starts at integ + f * nchan * chan_elems (blockIdx.y = image)
};

// Window i of the stream: its ladder level, and in (x, y) its top-left corner in that level.
__device__ __forceinline__ MineLevel mine_window(const MineLevel* levels, int n_levels, long long i, int ox, int oy, int sx, int sy, int& x,
                                                 int& y) {
  int l = 0;
  while (l + 1 < n_levels && levels[l + 1].win_first <= i) l++;
  const MineLevel L = levels[l];
  const int k = (int)(i - L.win_first);
  const int gy = k / L.nx, gx = k - gy * L.nx;
  x = ox + gx * sx;
  y = oy + gy * sy;
  return L;
}

// calcNormFactor, features.cpp:13-25 (the 4-corner difference of the wrapped squared sums is exact)
__device__ __forceinline__ float mine_norm_factor(const int32_t* sum, const unsigned* sq, size_t base, int P, int W0, int H0) {
  const int nw = W0 - 2, nh = H0 - 2;
  const size_t q = base + P + 1;
  const int vs = sum[q] - sum[q + nw] - sum[q + (size_t)nh * P] + sum[q + (size_t)nh * P + nw];
  const unsigned vq = sq[q] - sq[q + nw] - sq[q + (size_t)nh * P] + sq[q + (size_t)nh * P + nw];
  const double area = (double)(nw * nh);
  return (float)sqrt((double)(area * (double)vq - (double)vs * (double)vs));
}

// What the window kernels know of their window: its level's integrals and their pitch, its base in them, its norm factor.
struct MineWindow {
  const int32_t *sum, *til;
  size_t base;
  int P;
  float nf;
};

// The child node n chooses for window w. Haar: value = calc / normfactor, `<=` goes left; LBP: a code in the node's subset
// goes left. The offsets come from the node's geometry and the level's pitch.
template <bool HAAR>
__device__ __forceinline__ int mine_child(const MineNode& n, const MineWindow& w) {
  const int P = w.P;
  if (HAAR) {
    const int32_t* b = (n.tilted ? w.til : w.sum) + w.base;
    HaarFeatDev F;
    F.tilted = n.tilted;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const int rx = n.r[j][0], ry = n.r[j][1], rw = n.r[j][2], rh = n.r[j][3];
      F.w[j] = n.w[j];
      if (!n.tilted) {  // CV_SUM_OFFSETS
        F.p[j][0] = rx + P * ry;
        F.p[j][1] = rx + rw + P * ry;
        F.p[j][2] = rx + P * (ry + rh);
        F.p[j][3] = rx + rw + P * (ry + rh);
      } else {  // CV_TILTED_OFFSETS
        F.p[j][0] = rx + P * ry;
        F.p[j][1] = rx - rh + P * (ry + rh);
        F.p[j][2] = rx + rw + P * (ry + rw);
        F.p[j][3] = rx + rw - rh + P * (ry + rw + rh);
      }
    }
    return haar_value(haar_sum(F, [&](int o) { return b[o]; }), w.nf) <= n.thr ? n.left : n.right;
  }
  const int32_t* b = w.sum + w.base;
  LbpFeatDev F;
#pragma unroll
  for (int rr = 0; rr < 4; rr++)
#pragma unroll
    for (int cc = 0; cc < 4; cc++) F.p[4 * rr + cc] = (n.r[0][0] + cc * n.r[0][2]) + P * (n.r[0][1] + rr * n.r[0][3]);
  const int code = lbp_code_at(F, [&](int o) { return b[o]; });
  return (n.subset[code >> 5] & (1 << (code & 31))) != 0 ? n.left : n.right;
}

template <bool HAAR>
__device__ __forceinline__ MineWindow mine_window_integrals(const MineArgs& A, long long i, int image) {
  int x, y;
  const MineLevel L = mine_window(A.levels, A.n_levels, i, A.ox, A.oy, A.sx, A.sy, x, y);
  const int32_t* integ = A.integ + (size_t)image * A.nchan * A.chan_elems;
  MineWindow w;
  w.sum = integ + L.int_ofs;
  w.til = integ + 2 * A.chan_elems + L.int_ofs;
  w.P = L.pitchI;
  w.base = (size_t)y * w.P + x;
  w.nf = HAAR ? mine_norm_factor(w.sum, reinterpret_cast<const unsigned*>(integ + A.chan_elems + L.int_ofs), w.base, w.P, A.W0, A.H0) : 1.f;
  return w;
}

template <bool HAAR>
__global__ __launch_bounds__(256) void k_negmine_windows(MineArgs A) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n_windows) return;
  const MineWindow w = mine_window_integrals<HAAR>(A, i, blockIdx.y);
  A.pass[(size_t)blockIdx.y * A.n_windows + i] = walk_stages(A.walk, [&](int n) { return mine_child<HAAR>(A.nodes[n], w); });
}

// Same stream, one WAVEFRONT per window: the 64 lanes take the stumps of a stage (stump t = first + lane, + 64, ...), their
// votes meet in a DPP wave sum. A background image yields only ~10^4 stream windows (13 584 for 1920x1080): one thread per
// window leaves most of the chip idle while a few hundred threads walk every stage serially. Used for stump cascades whose
// stage sums are exact in double whatever the order (stage_sums_order_independent), so the parallel sum equals the
// trainer's sequential one bit for bit; other cascades keep k_negmine_windows.
template <bool HAAR>
__global__ __launch_bounds__(256) void k_negmine_wave(MineArgs A) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (i >= A.n_windows) return;  // wave-uniform
  const MineWindow w = mine_window_integrals<HAAR>(A, i, blockIdx.y);
  const bool pass = walk_stages_wave(A.walk, lane, [&](int n) { return mine_child<HAAR>(A.nodes[n], w); });
  if (lane == 0) A.pass[(size_t)blockIdx.y * A.n_windows + i] = pass;
}

// copies the pixels of selected stream windows out of the ladder: one block per window
__global__ __launch_bounds__(64) void k_negmine_gather(const uint8_t* __restrict__ pyr, size_t pyr_image_bytes, long long n_windows,
                                                       const MineLevel* __restrict__ levels, int n_levels,
                                                       const long long* __restrict__ keep, int W0, int H0, int ox, int oy, int sx, int sy,
                                                       uint8_t* __restrict__ out) {
  const long long gi = keep[blockIdx.x];  // image * n_windows + stream index
  const long long img = gi / n_windows, i = gi - img * n_windows;
  pyr += (size_t)img * pyr_image_bytes;
  int x, y;
  const MineLevel L = mine_window(levels, n_levels, i, ox, oy, sx, sy, x, y);
  const uint8_t* src = pyr + L.img_ofs + (size_t)y * L.pitch8 + x;
  for (int e = threadIdx.x; e < W0 * H0; e += 64) {
    const int yy = e / W0, xx = e - yy * W0;
    out[(size_t)blockIdx.x * W0 * H0 + e] = src[(size_t)yy * L.pitch8 + xx];
  }
}

// HOG cascades. NegReader::get copies each window out of its ladder level and setImage takes its border from that copy
// (HOGfeatures.cpp:173-183), so the outer ring of every window has gradients of its own: planes cannot be shared between
// overlapping windows or computed once per level. One workgroup per stream window builds the window's ten integral planes
// in LDS with the evaluator's setImage code (cc_hog_device.h) and walks the trained stages on them.
struct HogMineNode {  // a tree node with its variable as LDS offsets into the window's planes
  int cell[4];  // bin plane at the cell's corners: top-left, top-right, bottom-left, bottom-right
  int norm[4];  // norm plane at the block's outer corners, same order
  float thr;
  int left, right;  // child > 0: node index inside the tree; child <= 0: leaf index -child
  int pad;
};
struct HogMineArgs {
  const uint8_t* pyr;  // ladder levels, image f at pyr + f * pyr_image_bytes (blockIdx.y = image)
  size_t pyr_image_bytes;
  const MineLevel* levels;
  int n_levels;
  long long n_windows;
  int W0, H0, ox, oy, sx, sy;
  WalkTables walk;
  const HogMineNode* nodes;
  uint8_t* pass;  // [image][n_windows]
  int wave;       // 1: stumps of a stage across the lanes of wavefront 0 (order-independent sums); 0: one lane walks
};
constexpr int HOG_MINE_THREADS = 256;

// operator() of one variable (hog_var_value's arithmetic, corners already resolved to LDS offsets)
__device__ __forceinline__ float hog_mine_value(const float* P, const HogMineNode& n) {
  const float res = ((P[n.cell[0]] - P[n.cell[1]]) - P[n.cell[2]]) + P[n.cell[3]];
  const float nf = ((P[n.norm[0]] - P[n.norm[1]]) - P[n.norm[2]]) + P[n.norm[3]];
  return hog_value_from(res, nf);
}

// LDS: planes [10][H0 + 1][W0 + 1] float, magnitudes [H0][W0] float, bins [H0][W0] bytes (hog_lds_plan, cc_hog_device.h)
__global__ __launch_bounds__(HOG_MINE_THREADS) void k_negmine_hog(HogMineArgs A) {
  extern __shared__ float hog_lds[];
  const long long i = blockIdx.x;
  int x, y;
  const MineLevel L = mine_window(A.levels, A.n_levels, i, A.ox, A.oy, A.sx, A.sy, x, y);
  const int W = A.W0, H = A.H0, sw = W + 1;
  const size_t plane = (size_t)sw * (H + 1);
  float* planes = hog_lds;
  float* mag = planes + 10 * plane;
  uint8_t* bins = reinterpret_cast<uint8_t*>(mag + (size_t)W * H);
  const uint8_t* px = A.pyr + (size_t)blockIdx.y * A.pyr_image_bytes + L.img_ofs + (size_t)y * L.pitch8 + x;
  hog_window_grad(px, (size_t)L.pitch8, W, H, mag, bins, threadIdx.x, HOG_MINE_THREADS);
  __syncthreads();
  // row sums go to rows 1..H of each plane; the column pass turns them into the integral in place
  hog_row_pass(mag, bins, W, H, 0, 10, planes + sw, plane, threadIdx.x, HOG_MINE_THREADS);
  __syncthreads();
  hog_col_pass(planes + sw, plane, W, H, 0, 10, [=](int c, int xx, int yy) { return planes + c * plane + (size_t)yy * sw + xx; },
               threadIdx.x, HOG_MINE_THREADS);
  __syncthreads();
  if (threadIdx.x >= 64) return;  // wavefront 0 walks the stages
  const int lane = threadIdx.x;
  auto child = [&](int k) {
    const HogMineNode& n = A.nodes[k];
    return hog_mine_value(planes, n) <= n.thr ? n.left : n.right;
  };
  bool pass = true;
  if (A.wave)
    pass = walk_stages_wave(A.walk, lane, child);
  else if (lane == 0)
    pass = walk_stages(A.walk, child);
  if (lane == 0) A.pass[(size_t)blockIdx.y * A.n_windows + i] = pass;
}

static LdsOptIn g_negmine_hog_lds;  // k_negmine_hog's opt-in, shared by every HOG miner

}  // namespace ccamd

using namespace ccamd;

struct cc_negminer {
  Cascade m;
  bool empty = false;  // no trained stage (cc_negminer_create_empty): every window passes, no window kernel runs
  int device = 0;
  OwnStream stream;
  WalkTablesDev walk;
  DevBuf<MineNode> d_nodes;
  DevBuf<HogMineNode> d_hog_nodes;  // HOG cascades (k_negmine_hog)
  size_t hog_lds = 0;               // k_negmine_hog's dynamic LDS per workgroup
  // per-image workspace
  DevBuf<uint8_t> d_src, d_pyr, d_pass, d_pix;
  DevBuf<int32_t> d_integ, d_hbuf, d_diag, d_tseg;
  DevBuf<long long> d_keep;
  // The tables below depend on (image size, offset) only: consecutive images of a background set share them, so they are
  // built and uploaded when that key changes, not per call.
  FrontTables front;  // the ladder's levels
  DevBuf<MineLevel> d_levels;
  struct Plan {
    int width = -1, height = -1, ox = -1, oy = -1;
    long long wins = 0;
  } plan;
  PinnedBuf h_src;   // the images of a call, tight rows of align4(width)
  PinnedBuf h_pass;  // pass flags on their way back
  OwnStream copy_stream;               // the images' way to the device, piece by piece, under the kernels of the piece before
  std::vector<OwnEvent> piece_landed;  // one per piece of a call (grown on demand)
  FillWork fill;                       // cc_negminer_fill's selection
};

extern "C" {

namespace {

struct MineGeom {
  int w, h, nx, ny;
};

// The reader's scale ladder and window grid for one image (imagestorage.cpp:57-126), in its float arithmetic.
void mine_ladder(int W0, int H0, int cols, int rows, int ox, int oy, std::vector<MineGeom>& out) {
  out.clear();
  const float scaleFactor = 1.4142135623730950488016887242097F, stepFactor = 0.5F;
  float scale = std::max(((float)W0 + ox) / ((float)cols), ((float)H0 + oy) / ((float)rows));
  int lw = (int)(scale * cols + 0.5F), lh = (int)(scale * rows + 0.5F);
  for (;;) {
    MineGeom g{lw, lh, 0, 0};
    int x = ox;
    g.nx = 1;
    while ((int)(x + (1.0F + stepFactor) * W0) < lw) {
      x += (int)(stepFactor * W0);
      g.nx++;
    }
    int y = oy;
    g.ny = 1;
    while ((int)(y + (1.0F + stepFactor) * H0) < lh) {
      y += (int)(stepFactor * H0);
      g.ny++;
    }
    out.push_back(g);
    scale *= scaleFactor;
    if (!(scale <= 1.0F) || out.size() > 64) break;
    lw = (int)(scale * cols);
    lh = (int)(scale * rows);
  }
}

cc_status mine_check(const cc_negminer* m, int width, int height, int ox, int oy, const char* who) {
  if (!m) return set_error(CC_ERR_INVALID_ARG, "%s: null miner", who);
  if (width < 1 || height < 1 || width > 32768 || height > 32768) return set_error(CC_ERR_INVALID_ARG, "%s: bad image size", who);
  // NegReader::nextImg only accepts offsets with 0 <= ox <= cols - W, 0 <= oy <= rows - H
  if (ox < 0 || oy < 0 || ox > width - m->m.win_w || oy > height - m->m.win_h)
    return set_error(CC_ERR_INVALID_ARG, "%s: offset (%d,%d) does not leave room for a %dx%d window in a %dx%d image", who, ox, oy,
                     m->m.win_w, m->m.win_h, width, height);
  return CC_OK;
}

}  // namespace

cc_status cc_negminer_create_empty(int feature_type, int win_w, int win_h, int device, cc_negminer** out) {
  if (!out) return set_error(CC_ERR_INVALID_ARG, "cc_negminer_create_empty: null argument");
  *out = nullptr;
  if (feature_type != CC_FEATURE_HAAR && feature_type != CC_FEATURE_LBP && feature_type != CC_FEATURE_HOG)
    return set_error(CC_ERR_UNSUPPORTED, "cc_negminer_create_empty: feature type %d", feature_type);
  if (win_w < 2 || win_h < 2 || win_w > 4096 || win_h > 4096)  // half a window is the stream's step: at least one pixel
    return set_error(CC_ERR_INVALID_ARG, "cc_negminer_create_empty: window %dx%d", win_w, win_h);
  cc_status st = ensure_device(device);
  if (st != CC_OK) return st;
  std::unique_ptr<cc_negminer> m(new cc_negminer());
  m->m.feature_type = feature_type;
  m->m.win_w = win_w;
  m->m.win_h = win_h;
  m->empty = true;
  m->device = device;
  CC_HIP(m->stream.create());
  CC_HIP(m->copy_stream.create());
  *out = m.release();
  return CC_OK;
}

cc_status cc_negminer_create(const cc_cascade* c, int device, cc_negminer** out) {
  if (!c || !out) return set_error(CC_ERR_INVALID_ARG, "cc_negminer_create: null argument");
  *out = nullptr;
  cc_status st = ensure_device(device);
  if (st != CC_OK) return st;
  std::unique_ptr<cc_negminer> m(new cc_negminer());
  m->m = c->m;
  m->device = device;
  CC_HIP(m->stream.create());
  CC_HIP(m->copy_stream.create());
  const Cascade& M = m->m;
  const bool haar = M.feature_type == CC_FEATURE_HAAR, hog = M.feature_type == CC_FEATURE_HOG;
  if (!haar && !hog && M.feature_type != CC_FEATURE_LBP)
    return set_error(CC_ERR_UNSUPPORTED, "cc_negminer_create: feature type %d", M.feature_type);
  if (hog) {
    m->hog_lds = hog_lds_plan(M.win_w, M.win_h).mine_bytes;
    if (m->hog_lds > kHogLdsMax)
      return set_error(CC_ERR_UNSUPPORTED, "cc_negminer_create: HOG window %dx%d needs %zu bytes of LDS per window (limit %zu)", M.win_w,
                       M.win_h, m->hog_lds, kHogLdsMax);
    CC_HIP(g_negmine_hog_lds.raise(reinterpret_cast<const void*>(&k_negmine_hog), device, m->hog_lds));
    const int sw = M.win_w + 1, plane = sw * (M.win_h + 1);
    std::vector<HogMineNode> hn(M.node_feature.size());
    for (size_t i = 0; i < hn.size(); i++) {
      HogMineNode& n = hn[i];
      std::memset(&n, 0, sizeof(n));
      // the block lies inside the window (checked at load), so every offset is inside the planes
      const int32_t* f = &M.hog_feats[(size_t)M.node_feature[i] * 5];
      const int x = f[0], y = f[1], cw = f[2], ch = f[3], cell = f[4] / 9, bin = f[4] % 9;
      const int cx = x + (cell & 1) * cw, cy = y + (cell >> 1) * ch;
      n.cell[0] = bin * plane + cy * sw + cx;
      n.cell[1] = bin * plane + cy * sw + cx + cw;
      n.cell[2] = bin * plane + (cy + ch) * sw + cx;
      n.cell[3] = bin * plane + (cy + ch) * sw + cx + cw;
      n.norm[0] = 9 * plane + y * sw + x;
      n.norm[1] = 9 * plane + y * sw + x + 2 * cw;
      n.norm[2] = 9 * plane + (y + 2 * ch) * sw + x;
      n.norm[3] = 9 * plane + (y + 2 * ch) * sw + x + 2 * cw;
      n.thr = M.node_threshold[i];
      n.left = M.node_left[i];
      n.right = M.node_right[i];
    }
    CC_HIP(m->d_hog_nodes.upload(hn, m->stream.s));
    CC_HIP(hipStreamSynchronize(m->stream.s));  // `hn` ends here
  }
  std::vector<MineNode> nodes(hog ? 0 : M.node_feature.size());
  for (size_t i = 0; i < nodes.size(); i++) {
    MineNode& n = nodes[i];
    std::memset(&n, 0, sizeof(n));
    const int fi = M.node_feature[i];
    if (haar) {
      bool used = true;
      for (int j = 0; j < 3; j++) {
        const float wt = M.haar_weights[(size_t)fi * 3 + j];
        if (wt == 0.0f) used = false;  // offsets stay 0 from the first zero weight on (haarfeatures.cpp:292-308)
        if (!used) continue;
        n.w[j] = wt;
        for (int k = 0; k < 4; k++) n.r[j][k] = M.haar_rects[(size_t)fi * 12 + j * 4 + k];
      }
      n.tilted = M.haar_tilted[fi];
      n.thr = M.node_threshold[i];
    } else {
      for (int k = 0; k < 4; k++) n.r[0][k] = M.lbp_rects[(size_t)fi * 4 + k];
      for (int j = 0; j < 8; j++) n.subset[j] = M.node_subset[i * 8 + j];
    }
    n.left = M.node_left[i];
    n.right = M.node_right[i];
  }
  CC_HIP(m->d_nodes.upload(nodes, m->stream.s));
  CC_HIP(m->walk.upload(M, m->stream.s));
  CC_HIP(hipStreamSynchronize(m->stream.s));
  *out = m.release();
  return CC_OK;
}

void cc_negminer_destroy(cc_negminer* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  delete m;
}

cc_status cc_negminer_plan(const cc_negminer* m, int width, int height, int ox, int oy, int32_t* lw, int32_t* lh, int32_t* nx,
                           int32_t* ny, int cap, int* n_levels, int64_t* n_windows) {
  cc_status st = mine_check(m, width, height, ox, oy, "cc_negminer_plan");
  if (st != CC_OK) return st;
  if (!n_levels || !n_windows) return set_error(CC_ERR_INVALID_ARG, "cc_negminer_plan: null output");
  std::vector<MineGeom> g;
  mine_ladder(m->m.win_w, m->m.win_h, width, height, ox, oy, g);
  *n_levels = (int)g.size();
  *n_windows = 0;
  for (size_t i = 0; i < g.size(); i++) {
    *n_windows += (int64_t)g[i].nx * g[i].ny;
    if ((int)i < cap) {
      if (lw) lw[i] = g[i].w;
      if (lh) lh[i] = g[i].h;
      if (nx) nx[i] = g[i].nx;
      if (ny) ny[i] = g[i].ny;
    }
  }
  return CC_OK;
}

// Tables of one (image size, offset): ladder geometry, resize taps, kernel block maps. Cached in m->plan.
static cc_status mine_plan(cc_negminer* m, int width, int height, int ox, int oy, const char* who) {
  cc_negminer::Plan& P = m->plan;
  if (P.width == width && P.height == height && P.ox == ox && P.oy == oy) return CC_OK;
  P.width = -1;  // invalid until everything below has succeeded
  const Cascade& M = m->m;
  std::vector<MineGeom> g;
  mine_ladder(M.win_w, M.win_h, width, height, ox, oy, g);
  const int nl = (int)g.size();
  std::vector<int2> sizes((size_t)nl);
  for (int i = 0; i < nl; i++) {
    if (g[i].w < M.win_w + ox || g[i].h < M.win_h + oy)
      return set_error(CC_ERR_INVALID_ARG, "%s: ladder level %d (%dx%d) smaller than window + offset", who, i, g[i].w, g[i].h);
    sizes[(size_t)i] = make_int2(g[i].w, g[i].h);
  }
  m->front.L = front_layout(width, height, sizes, M.feature_type == CC_FEATURE_HAAR && M.has_tilted);
  std::vector<MineLevel> lv((size_t)nl);
  long long wins = 0;
  for (int i = 0; i < nl; i++) {
    const ScaleDev& S = m->front.L.sd[(size_t)i];
    MineLevel& L = lv[(size_t)i];
    L.w = S.w;
    L.h = S.h;
    L.pitchI = S.pitchI;
    L.pitch8 = S.pitch8;
    L.nx = g[i].nx;
    L.ny = g[i].ny;
    L.int_ofs = S.int_ofs;
    L.img_ofs = S.img_ofs;
    L.win_first = wins;
    L.pad = 0;
    wins += (long long)g[i].nx * g[i].ny;
  }
  CC_HIP(m->d_levels.upload(lv, m->stream.s));
  CC_HIP(m->front.upload(m->stream.s));  // synchronises: `lv` ends here
  P.wins = wins;
  P.ox = ox;
  P.oy = oy;
  P.height = height;
  P.width = width;
  return CC_OK;
}

// One call of mine_images: the arguments its parts share, and what mine_begin derives from them and the plan.
struct MineCall {
  cc_negminer* m;
  const uint8_t* const* images;
  int K, width, height;
  size_t row_stride;
  int ox, oy;
  const char* who;
  bool to_host;  // the flags go back to the caller (cc_negminer_run*); cc_negminer_fill keeps them on the device
  bool haar, tilt, hog, wave_mode;
  bool pixels_only;  // the window kernels read pixels (HOG) or nothing (no stages): no integral images
  int nchan, sx, sy;
  long long wins;
  size_t chan_elems, spitch, src_bytes;
};

// Checks and plan. *n_windows is set as soon as the plan is known, also when the capacity is too small.
static cc_status mine_begin(MineCall& C, uint8_t* pass, int64_t cap, int64_t* n_windows, uint8_t* pixels, int64_t* keep_index, int max_keep,
                            int* n_keep) {
  cc_negminer* m = C.m;
  const char* who = C.who;
  cc_status st = mine_check(m, C.width, C.height, C.ox, C.oy, who);
  if (st != CC_OK) return st;
  if (!C.images || C.K < 1 || (C.to_host && !pass) || !n_windows || C.row_stride < (size_t)C.width)
    return set_error(CC_ERR_INVALID_ARG, "%s: bad argument", who);
  for (int k = 0; k < C.K; k++)
    if (!C.images[k]) return set_error(CC_ERR_INVALID_ARG, "%s: image %d is null", who, k);
  if (pixels && (!keep_index || !n_keep || max_keep < 0)) return set_error(CC_ERR_INVALID_ARG, "%s: bad keep buffers", who);
  st = ensure_device(m->device);
  if (st != CC_OK) return st;
  st = mine_plan(m, C.width, C.height, C.ox, C.oy, who);
  if (st != CC_OK) return st;
  const Cascade& M = m->m;
  C.haar = M.feature_type == CC_FEATURE_HAAR;
  C.tilt = C.haar && M.has_tilted;
  C.hog = M.feature_type == CC_FEATURE_HOG;
  C.pixels_only = C.hog || m->empty;
  C.wins = m->plan.wins;
  *n_windows = C.wins;
  if (C.to_host && C.wins * C.K > cap)
    return set_error(CC_ERR_BUFFER_TOO_SMALL, "%s: %lld windows (%d images), capacity %lld", who, C.wins * C.K, C.K, (long long)cap);
  C.nchan = C.haar ? (C.tilt ? 3 : 2) : 1;
  C.chan_elems = m->front.L.int_frame_elems;
  C.spitch = (size_t)align_up(C.width, 4);
  C.src_bytes = C.spitch * (size_t)C.height;
  C.sx = (int)(0.5F * M.win_w);
  C.sy = (int)(0.5F * M.win_h);
  // one wavefront per window where the parallel stage sum is exact (stumps, order-independent sums); else one thread per window
  C.wave_mode = !m->empty && M.max_nodes_per_tree == 1 && stage_sums_order_independent(M);
  return CC_OK;
}

// The per-call workspace, sized for all K images.
static cc_status mine_workspace(const MineCall& C) {
  cc_negminer* m = C.m;
  const FrontLayout& FL = m->front.L;
  const size_t K = (size_t)C.K;
  CC_HIP(m->d_src.ensure(C.src_bytes * K));
  CC_HIP(m->d_pyr.ensure(FL.pyr_frame_bytes * K));
  if (!C.pixels_only) {  // HOG windows build their planes from the levels' pixels: no integral images
    CC_HIP(m->d_integ.ensure(C.chan_elems * (size_t)C.nchan * K));
    CC_HIP(m->d_hbuf.ensure(std::max<size_t>(FL.h_frame_elems * (size_t)C.nchan * K, 4)));
  }
  CC_HIP(m->d_pass.ensure((size_t)std::max<long long>(C.wins * C.K, 1)));
  CC_HIP(m->h_src.ensure(C.src_bytes * K));
  if (C.to_host) CC_HIP(m->h_pass.ensure((size_t)std::max<long long>(C.wins * C.K, 1)));
  if (C.tilt) {
    CC_HIP(m->d_diag.ensure(C.chan_elems * 2 * K));
    CC_HIP(m->d_tseg.ensure(std::max<size_t>(FL.tseg_frame_elems * K, 1)));
  }
  return CC_OK;
}

// Every kernel over the images [k0, k0 + n): the front-end kernels and the window kernels take the image as blockIdx.y.
static void mine_launch_images(const MineCall& C, int k0, int n) {
  cc_negminer* m = C.m;
  const FrontLayout& FL = m->front.L;
  const Cascade& M = m->m;
  hipStream_t s = m->stream.s;
  const long long wins = C.wins;
  FrontIO io;
  io.src = m->d_src.p + (size_t)k0 * C.src_bytes;
  io.row_stride = C.spitch;
  io.frame_stride = C.src_bytes;
  io.pyr = m->d_pyr.p + (size_t)k0 * FL.pyr_frame_bytes;
  if (!C.pixels_only) {
    io.integ = m->d_integ.p + (size_t)k0 * C.nchan * C.chan_elems;
    io.hbuf = m->d_hbuf.p + (size_t)k0 * C.nchan * FL.h_frame_elems;
  }
  if (C.tilt) {
    io.diag = m->d_diag.p + (size_t)k0 * 2 * C.chan_elems;
    io.tseg = m->d_tseg.p + (size_t)k0 * FL.tseg_frame_elems;
  }
  io.nchan = C.nchan;
  io.sq = C.haar;
  launch_front(s, m->front, io, n, C.pixels_only ? FRONT_RESIZE : FRONT_RESIZE | FRONT_INTEGRALS);
  if (wins == 0) return;
  if (m->empty) {
    (void)hipMemsetAsync(m->d_pass.p + (size_t)k0 * (size_t)wins, 1, (size_t)n * (size_t)wins, s);
    return;
  }
  if (C.hog) {
    HogMineArgs H;
    H.pyr = io.pyr;
    H.pyr_image_bytes = FL.pyr_frame_bytes;
    H.levels = m->d_levels.p;
    H.n_levels = (int)FL.sd.size();
    H.n_windows = wins;
    H.W0 = M.win_w;
    H.H0 = M.win_h;
    H.ox = C.ox;
    H.oy = C.oy;
    H.sx = C.sx;
    H.sy = C.sy;
    H.walk = m->walk.tables();
    H.nodes = m->d_hog_nodes.p;
    H.pass = m->d_pass.p + (size_t)k0 * (size_t)wins;
    H.wave = C.wave_mode ? 1 : 0;
    hipLaunchKernelGGL(k_negmine_hog, dim3((unsigned)wins, n), dim3(HOG_MINE_THREADS), m->hog_lds, s, H);
    return;
  }
  MineArgs B;
  B.integ = io.integ;
  B.chan_elems = C.chan_elems;
  B.nchan = C.nchan;
  B.levels = m->d_levels.p;
  B.n_levels = (int)FL.sd.size();
  B.n_windows = wins;
  B.W0 = M.win_w;
  B.H0 = M.win_h;
  B.ox = C.ox;
  B.oy = C.oy;
  B.sx = C.sx;
  B.sy = C.sy;
  B.walk = m->walk.tables();
  B.nodes = m->d_nodes.p;
  B.pass = m->d_pass.p + (size_t)k0 * (size_t)wins;
  if (C.wave_mode) {
    const unsigned nb = (unsigned)((wins + 3) / 4);
    if (C.haar)
      hipLaunchKernelGGL(k_negmine_wave<true>, dim3(nb, n), dim3(256), 0, s, B);
    else
      hipLaunchKernelGGL(k_negmine_wave<false>, dim3(nb, n), dim3(256), 0, s, B);
  } else {
    const unsigned nb = (unsigned)((wins + 255) / 256);
    if (C.haar)
      hipLaunchKernelGGL(k_negmine_windows<true>, dim3(nb, n), dim3(256), 0, s, B);
    else
      hipLaunchKernelGGL(k_negmine_windows<false>, dim3(nb, n), dim3(256), 0, s, B);
  }
}

// Pageable rows -> pinned, tight rows, then asynchronous transfers on the copy stream: the images travel in pieces of >= 8 MB;
// a piece's copy is issued as soon as it is staged (it runs under the staging of the next piece) and its kernels are queued
// behind it on the compute stream (they run under the next piece's copy). A Full-HD background is 2 MB for 13 584 windows:
// the image's way to the device is most of what a call costs. Large pieces are staged by up to 4 threads.
static cc_status mine_pieces(const MineCall& C) {
  cc_negminer* m = C.m;
  const char* who = C.who;
  const uint8_t* const* images = C.images;
  const int K = C.K, width = C.width, height = C.height;
  const size_t row_stride = C.row_stride, spitch = C.spitch, src_bytes = C.src_bytes;
  hipStream_t s = m->stream.s;
  uint8_t* const h_src = static_cast<uint8_t*>(m->h_src.p);
  auto stage = [&](int ka, int kb) {
    for (int k = ka; k < kb; k++) {
      uint8_t* dst = h_src + (size_t)k * src_bytes;
      if (row_stride == spitch)
        std::memcpy(dst, images[k], (size_t)(height - 1) * spitch + (size_t)width);
      else
        for (int y = 0; y < height; y++) std::memcpy(dst + (size_t)y * spitch, images[k] + (size_t)y * row_stride, (size_t)width);
    }
  };
  const int per_piece = (int)std::max<size_t>(1, ((size_t)8 << 20) / std::max<size_t>(src_bytes, 1));
  const size_t n_pieces = ((size_t)K + per_piece - 1) / per_piece;
  while (m->piece_landed.size() < n_pieces) {
    OwnEvent ev;
    CC_HIP(ev.create(hipEventDisableTiming));
    m->piece_landed.push_back(std::move(ev));
  }
  size_t piece = 0;
  for (int k0 = 0; k0 < K; k0 += per_piece, piece++) {
    const int k1 = std::min(K, k0 + per_piece), n = k1 - k0;
    const int nt = std::min({4, n, (int)std::max<size_t>(1, ((size_t)n * src_bytes) >> 21)});
    if (nt <= 1) {
      stage(k0, k1);
    } else {
      std::vector<std::future<void>> jobs;
      try {
        for (int t = 1; t < nt; t++) jobs.push_back(std::async(std::launch::async, stage, k0 + (int)((long long)n * t / nt), k0 + (int)((long long)n * (t + 1) / nt)));
        stage(k0, k0 + n / nt);
        for (auto& j : jobs) j.get();
      } catch (const std::exception& e) {
        for (auto& j : jobs)
          if (j.valid()) j.wait();
        (void)hipStreamSynchronize(m->copy_stream.s);
        (void)hipStreamSynchronize(s);
        return set_error(CC_ERR_HIP, "%s: staging the images: %s", who, e.what());
      }
    }
    CC_HIP(hipMemcpyAsync(m->d_src.p + (size_t)k0 * src_bytes, h_src + (size_t)k0 * src_bytes, (size_t)n * src_bytes, hipMemcpyHostToDevice,
                          m->copy_stream.s));
    CC_HIP(hipEventRecord(m->piece_landed[piece].e, m->copy_stream.s));
    CC_HIP(hipStreamWaitEvent(s, m->piece_landed[piece].e, 0));
    mine_launch_images(C, k0, n);
  }
  CC_HIP(hipGetLastError());
  return CC_OK;
}

// The flags of all K images back to `pass`; the compute stream is idle afterwards.
static cc_status mine_fetch_flags(const MineCall& C, uint8_t* pass) {
  cc_negminer* m = C.m;
  hipStream_t s = m->stream.s;
  const long long wins = C.wins;
  const int K = C.K;
  if (wins > 0) CC_HIP(hipMemcpyAsync(m->h_pass.p, m->d_pass.p, (size_t)(wins * K), hipMemcpyDeviceToHost, s));
  CC_HIP(hipStreamSynchronize(s));
  if (wins > 0) std::memcpy(pass, m->h_pass.p, (size_t)(wins * K));
  return CC_OK;
}

// The pixels of the first max_keep windows that passed, out of the ladders still on the device.
static cc_status mine_gather_kept(const MineCall& C, const uint8_t* pass, uint8_t* pixels, int64_t* keep_index, int max_keep, int* n_keep) {
  cc_negminer* m = C.m;
  hipStream_t s = m->stream.s;
  const FrontLayout& FL = m->front.L;
  const int W0 = m->m.win_w, H0 = m->m.win_h, nl = (int)FL.sd.size(), K = C.K;
  const long long wins = C.wins;
  std::vector<long long> keep;
  for (long long i = 0; i < wins * K && (int)keep.size() < max_keep; i++)
    if (pass[i]) keep.push_back(i);
  *n_keep = (int)keep.size();
  if (!keep.empty()) {
    const size_t wsz = (size_t)W0 * H0;
    CC_HIP(m->d_keep.upload(keep, s));
    CC_HIP(m->d_pix.ensure(keep.size() * wsz));
    hipLaunchKernelGGL(k_negmine_gather, dim3((unsigned)keep.size()), dim3(64), 0, s, m->d_pyr.p, FL.pyr_frame_bytes, wins, m->d_levels.p, nl,
                       m->d_keep.p, W0, H0, C.ox, C.oy, C.sx, C.sy, m->d_pix.p);
    CC_HIP(hipGetLastError());
    CC_HIP(hipMemcpyAsync(pixels, m->d_pix.p, keep.size() * wsz, hipMemcpyDeviceToHost, s));
    CC_HIP(hipStreamSynchronize(s));
    for (size_t i = 0; i < keep.size(); i++) keep_index[i] = keep[i];
  }
  return CC_OK;
}

// n_images images of one size, consumed with one offset: ONE copy to the device, one launch of every kernel over all of
// them (the front-end kernels and the window kernels take the image as blockIdx.y, like the detector's frames), one copy back.
static cc_status mine_images(cc_negminer* m, const uint8_t* const* images, int n_images, int width, int height, size_t row_stride, int ox,
                             int oy, uint8_t* pass, int64_t cap, int64_t* n_windows, uint8_t* pixels, int64_t* keep_index, int max_keep,
                             int* n_keep, const char* who) {
  MineCall C{};
  C.m = m;
  C.images = images;
  C.K = n_images;
  C.width = width;
  C.height = height;
  C.row_stride = row_stride;
  C.ox = ox;
  C.oy = oy;
  C.who = who;
  C.to_host = true;
  cc_status st = mine_begin(C, pass, cap, n_windows, pixels, keep_index, max_keep, n_keep);
  if (st == CC_OK) st = mine_workspace(C);
  if (st == CC_OK) st = mine_pieces(C);
  if (st == CC_OK) st = mine_fetch_flags(C, pass);
  if (st == CC_OK && pixels) st = mine_gather_kept(C, pass, pixels, keep_index, max_keep, n_keep);
  return st;
}

cc_status cc_negminer_run(cc_negminer* m, const uint8_t* gray, int width, int height, size_t row_stride, int ox, int oy, uint8_t* pass,
                          int64_t cap, int64_t* n_windows, uint8_t* pixels, int64_t* keep_index, int max_keep, int* n_keep) {
  if (!m) return set_error(CC_ERR_INVALID_ARG, "cc_negminer_run: null miner");
  return mine_images(m, &gray, 1, width, height, row_stride, ox, oy, pass, cap, n_windows, pixels, keep_index, max_keep, n_keep, "cc_negminer_run");
}

cc_status cc_negminer_run_batch(cc_negminer* m, const uint8_t* const* images, int n_images, int width, int height, size_t row_stride, int ox,
                                int oy, uint8_t* pass, int64_t cap, int64_t* n_windows, uint8_t* pixels, int64_t* keep_index, int max_keep,
                                int* n_keep) {
  if (!m) return set_error(CC_ERR_INVALID_ARG, "cc_negminer_run_batch: null miner");
  if (n_images > 256) return set_error(CC_ERR_INVALID_ARG, "cc_negminer_run_batch: at most 256 images per call (%d given)", n_images);
  return mine_images(m, images, n_images, width, height, row_stride, ox, oy, pass, cap, n_windows, pixels, keep_index, max_keep, n_keep,
                     "cc_negminer_run_batch");
}

// fillPassedSamples' negative branch over the stream of the images (section 6c): the window kernels as in mine_images, then
// the selection on the flags where they are (cc_fill.hip), the kept windows' pixels out of the ladders, and the evaluator's
// setImage on them. What crosses to the host is the selection's record and, on request, the kept positions.
cc_status cc_negminer_fill(cc_negminer* m, cc_evaluator* e, const uint8_t* const* images, int n_images, int width, int height,
                           size_t row_stride, int ox, int oy, int64_t start, int first_idx, int want, int64_t got_before,
                           int64_t consumed_before, double min_acceptance_ratio, int* n_filled, int64_t* n_consumed, int* stop,
                           int64_t* keep_index) {
  const char* who = "cc_negminer_fill";
  if (!m || !e || !n_filled || !n_consumed || !stop) return set_error(CC_ERR_INVALID_ARG, "%s: null argument", who);
  if (e->device != m->device || e->type != m->m.feature_type || e->W != m->m.win_w || e->H != m->m.win_h)
    return set_error(CC_ERR_INVALID_ARG, "%s: miner (device %d, feature type %d, %dx%d) and evaluator (device %d, feature type %d, %dx%d) differ",
                     who, m->device, m->m.feature_type, m->m.win_w, m->m.win_h, e->device, e->type, e->W, e->H);
  if (n_images < 1 || n_images > 256) return set_error(CC_ERR_INVALID_ARG, "%s: 1 to 256 images per call (%d given)", who, n_images);
  if (first_idx < 0 || want < 0 || (long long)first_idx + want > e->max_samples)
    return set_error(CC_ERR_OUT_OF_RANGE, "%s: samples [%d, %lld) exceed max_samples %d", who, first_idx, (long long)first_idx + want,
                     e->max_samples);
  if (got_before < 0 || consumed_before < 0) return set_error(CC_ERR_INVALID_ARG, "%s: negative counts", who);
  MineCall C{};
  C.m = m;
  C.images = images;
  C.K = n_images;
  C.width = width;
  C.height = height;
  C.row_stride = row_stride;
  C.ox = ox;
  C.oy = oy;
  C.who = who;
  C.to_host = false;
  int64_t wins = 0;
  cc_status st = mine_begin(C, nullptr, 0, &wins, nullptr, nullptr, 0, nullptr);
  if (st != CC_OK) return st;
  const long long total = C.wins * C.K;
  if (start < 0 || start > total) return set_error(CC_ERR_INVALID_ARG, "%s: start %lld outside the stream [0, %lld]", who, (long long)start, total);
  st = mine_workspace(C);
  if (st == CC_OK) st = mine_pieces(C);
  if (st != CC_OK) return st;
  hipStream_t s = m->stream.s;
  FillResult R;
  st = fill_select(m->fill, m->d_pass.p, total, start, want, got_before, consumed_before, min_acceptance_ratio, s, &R);
  if (st != CC_OK) return st;
  if (R.n_filled > 0) {
    const FrontLayout& FL = m->front.L;
    const int W0 = m->m.win_w, H0 = m->m.win_h;
    CC_HIP(m->d_pix.ensure((size_t)R.n_filled * W0 * H0));
    hipLaunchKernelGGL(k_negmine_gather, dim3((unsigned)R.n_filled), dim3(64), 0, s, m->d_pyr.p, FL.pyr_frame_bytes, C.wins, m->d_levels.p,
                       (int)FL.sd.size(), m->fill.d_keep.p, W0, H0, C.ox, C.oy, C.sx, C.sy, m->d_pix.p);
    CC_HIP(hipGetLastError());
    if (keep_index) CC_HIP(hipMemcpyAsync(keep_index, m->fill.d_keep.p, (size_t)R.n_filled * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    CC_HIP(hipStreamSynchronize(s));  // the evaluator's stream reads d_pix
    st = eval_set_images_device(e, m->d_pix.p, R.n_filled, first_idx, 0.f);
    if (st != CC_OK) return st;
  }
  *n_filled = R.n_filled;
  *n_consumed = R.n_consumed;
  *stop = R.stop;
  return CC_OK;
}

}  // extern "C"
