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
  int nstages;
  const int* stage_first;
  const int* stage_ntrees;
  const float* stage_thr;
  const MineNode* nodes;
  const int* tree_root;
  const int* tree_leaf0;
  const float* leaves;
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

// Node n's decision for the window at `base` of a level with integral pitch P. Haar: value = calc / normfactor, `<=` goes left;
// LBP: the 3x3-cell code is in the node's subset.
template <bool HAAR>
__device__ __forceinline__ bool mine_go_left(const MineNode* n, const int32_t* sum, const int32_t* til, size_t base, int P, float nf) {
  if (HAAR) {
    const int32_t* b = (n->tilted ? til : sum) + base;
    float ret = 0.f;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      if (j == 2 && n->w[2] == 0.0f) break;
      const int rx = n->r[j][0], ry = n->r[j][1], rw = n->r[j][2], rh = n->r[j][3];
      int p0, p1, p2, p3;
      if (!n->tilted) {  // CV_SUM_OFFSETS
        p0 = rx + P * ry;
        p1 = rx + rw + P * ry;
        p2 = rx + P * (ry + rh);
        p3 = rx + rw + P * (ry + rh);
      } else {  // CV_TILTED_OFFSETS
        p0 = rx + P * ry;
        p1 = rx - rh + P * (ry + rh);
        p2 = rx + rw + P * (ry + rw);
        p3 = rx + rw - rh + P * (ry + rw + rh);
      }
      const float term = n->w[j] * (float)(b[p0] - b[p1] - b[p2] + b[p3]);
      ret = j == 0 ? term : ret + term;
    }
    const float val = nf == 0.0f ? 0.0f : ret / nf;
    return val <= n->thr;
  }
  const int32_t* b = sum + base;
  int p[16];
#pragma unroll
  for (int rr = 0; rr < 4; rr++)
#pragma unroll
    for (int cc = 0; cc < 4; cc++) p[4 * rr + cc] = b[(n->r[0][0] + cc * n->r[0][2]) + P * (n->r[0][1] + rr * n->r[0][3])];
  const int c = p[5] - p[6] - p[9] + p[10];
  const int code = (p[0] - p[1] - p[4] + p[5] >= c ? 128 : 0) | (p[1] - p[2] - p[5] + p[6] >= c ? 64 : 0) |
                   (p[2] - p[3] - p[6] + p[7] >= c ? 32 : 0) | (p[6] - p[7] - p[10] + p[11] >= c ? 16 : 0) |
                   (p[10] - p[11] - p[14] + p[15] >= c ? 8 : 0) | (p[9] - p[10] - p[13] + p[14] >= c ? 4 : 0) |
                   (p[8] - p[9] - p[12] + p[13] >= c ? 2 : 0) | (p[4] - p[5] - p[8] + p[9] >= c ? 1 : 0);
  return (n->subset[code >> 5] & (1 << (code & 31))) != 0;
}

template <bool HAAR>
__global__ __launch_bounds__(256) void k_negmine_windows(MineArgs A) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n_windows) return;
  int x, y;
  const MineLevel L = mine_window(A.levels, A.n_levels, i, A.ox, A.oy, A.sx, A.sy, x, y);
  const int32_t* integ = A.integ + (size_t)blockIdx.y * A.nchan * A.chan_elems;
  const int32_t* sum = integ + L.int_ofs;
  const int32_t* til = integ + 2 * A.chan_elems + L.int_ofs;
  const int P = L.pitchI;
  const size_t base = (size_t)y * P + x;
  const float nf = HAAR ? mine_norm_factor(sum, reinterpret_cast<const unsigned*>(integ + A.chan_elems + L.int_ofs), base, P, A.W0, A.H0) : 1.f;
  uint8_t pass = 1;
  for (int st = 0; st < A.nstages && pass; st++) {
    double acc = 0;
    const int first = A.stage_first[st], nt = A.stage_ntrees[st];
    for (int t = first; t < first + nt; t++) {
      int idx = 0;
      const int root = A.tree_root[t];
      do {
        const MineNode* n = A.nodes + root + idx;
        idx = mine_go_left<HAAR>(n, sum, til, base, P, nf) ? n->left : n->right;
      } while (idx > 0);
      acc += (double)A.leaves[A.tree_leaf0[t] - idx];
    }
    if (acc < (double)A.stage_thr[st]) pass = 0;
  }
  A.pass[(size_t)blockIdx.y * A.n_windows + i] = pass;
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
  int x, y;
  const MineLevel L = mine_window(A.levels, A.n_levels, i, A.ox, A.oy, A.sx, A.sy, x, y);
  const int32_t* integ = A.integ + (size_t)blockIdx.y * A.nchan * A.chan_elems;
  const int32_t* sum = integ + L.int_ofs;
  const int32_t* til = integ + 2 * A.chan_elems + L.int_ofs;
  const int P = L.pitchI;
  const size_t base = (size_t)y * P + x;
  const float nf = HAAR ? mine_norm_factor(sum, reinterpret_cast<const unsigned*>(integ + A.chan_elems + L.int_ofs), base, P, A.W0, A.H0) : 1.f;
  uint8_t pass = 1;
  for (int st = 0; st < A.nstages; st++) {
    const int first = A.stage_first[st], nt = A.stage_ntrees[st];
    double part = 0;
    for (int t = first + lane; t < first + nt; t += 64) {
      const MineNode* n = A.nodes + A.tree_root[t];
      const bool go_left = mine_go_left<HAAR>(n, sum, til, base, P, nf);
      part += (double)A.leaves[A.tree_leaf0[t] - (go_left ? n->left : n->right)];
    }
    if (wave_sum_f64(part) < (double)A.stage_thr[st]) {
      pass = 0;
      break;
    }
  }
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
  int nstages;
  const int* stage_first;
  const int* stage_ntrees;
  const float* stage_thr;
  const HogMineNode* nodes;
  const int* tree_root;
  const int* tree_leaf0;
  const float* leaves;
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

// LDS: planes [10][H0 + 1][W0 + 1] float, magnitudes [H0][W0] float, bins [H0][W0] bytes (hog_mine_lds_bytes)
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
  uint8_t pass = 1;
  if (A.wave) {
    for (int st = 0; st < A.nstages; st++) {
      const int first = A.stage_first[st], nt = A.stage_ntrees[st];
      double part = 0;
      for (int t = first + lane; t < first + nt; t += 64) {
        const HogMineNode& n = A.nodes[A.tree_root[t]];
        part += (double)A.leaves[A.tree_leaf0[t] - (hog_mine_value(planes, n) <= n.thr ? n.left : n.right)];
      }
      if (wave_sum_f64(part) < (double)A.stage_thr[st]) {
        pass = 0;
        break;
      }
    }
  } else if (lane == 0) {
    for (int st = 0; st < A.nstages && pass; st++) {
      double acc = 0;
      const int first = A.stage_first[st], nt = A.stage_ntrees[st];
      for (int t = first; t < first + nt; t++) {
        const int root = A.tree_root[t];
        int idx = 0;
        do {
          const HogMineNode& n = A.nodes[root + idx];
          idx = hog_mine_value(planes, n) <= n.thr ? n.left : n.right;
        } while (idx > 0);
        acc += (double)A.leaves[A.tree_leaf0[t] - idx];
      }
      if (acc < (double)A.stage_thr[st]) pass = 0;
    }
  }
  if (lane == 0) A.pass[(size_t)blockIdx.y * A.n_windows + i] = pass;
}

static size_t hog_mine_lds_bytes(int W, int H) { return (size_t)10 * (W + 1) * (H + 1) * 4 + (size_t)W * H * 5; }

}  // namespace ccamd

using namespace ccamd;

struct cc_negminer {
  Cascade m;
  int device = 0;
  hipStream_t stream = nullptr;
  DevBuf<MineNode> d_nodes;
  DevBuf<HogMineNode> d_hog_nodes;  // HOG cascades (k_negmine_hog)
  size_t hog_lds = 0;               // k_negmine_hog's dynamic LDS per workgroup
  DevBuf<int> d_stage_first, d_stage_ntrees, d_tree_root, d_tree_leaf0;
  DevBuf<float> d_stage_thr, d_leaves;
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
  hipStream_t copy_stream = nullptr;      // the images' way to the device, piece by piece, under the kernels of the piece before
  std::vector<hipEvent_t> piece_landed;   // one per piece of a call (grown on demand)
  ~cc_negminer() {
    for (hipEvent_t e : piece_landed) (void)hipEventDestroy(e);
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
    if (stream) (void)hipStreamDestroy(stream);
  }
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

cc_status cc_negminer_create(const cc_cascade* c, int device, cc_negminer** out) {
  if (!c || !out) return set_error(CC_ERR_INVALID_ARG, "cc_negminer_create: null argument");
  *out = nullptr;
  cc_status st = ensure_device(device);
  if (st != CC_OK) return st;
  std::unique_ptr<cc_negminer> m(new cc_negminer());
  m->m = c->m;
  m->device = device;
  CC_HIP(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
  CC_HIP(hipStreamCreateWithFlags(&m->copy_stream, hipStreamNonBlocking));
  const Cascade& M = m->m;
  const bool haar = M.feature_type == CC_FEATURE_HAAR, hog = M.feature_type == CC_FEATURE_HOG;
  if (!haar && !hog && M.feature_type != CC_FEATURE_LBP)
    return set_error(CC_ERR_UNSUPPORTED, "cc_negminer_create: feature type %d", M.feature_type);
  if (hog) {
    m->hog_lds = hog_mine_lds_bytes(M.win_w, M.win_h);
    if (m->hog_lds > 160 * 1024)
      return set_error(CC_ERR_UNSUPPORTED, "cc_negminer_create: HOG window %dx%d needs %zu bytes of LDS per window (limit %d)", M.win_w,
                       M.win_h, m->hog_lds, 160 * 1024);
    if (m->hog_lds > 64 * 1024)
      CC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_negmine_hog), hipFuncAttributeMaxDynamicSharedMemorySize, (int)m->hog_lds));
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
    CC_HIP(m->d_hog_nodes.upload(hn, m->stream));
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
  std::vector<int> sfirst(M.stage_first.begin(), M.stage_first.end()), sn(M.stage_ntrees.begin(), M.stage_ntrees.end());
  std::vector<int> root(M.tree_first_node.begin(), M.tree_first_node.end()), leaf0(M.tree_first_leaf.begin(), M.tree_first_leaf.end());
  CC_HIP(m->d_nodes.upload(nodes, m->stream));
  CC_HIP(m->d_stage_first.upload(sfirst, m->stream));
  CC_HIP(m->d_stage_ntrees.upload(sn, m->stream));
  CC_HIP(m->d_stage_thr.upload(M.stage_threshold, m->stream));  // already threshold - 1e-5f (CV_THRESHOLD_EPS)
  CC_HIP(m->d_tree_root.upload(root, m->stream));
  CC_HIP(m->d_tree_leaf0.upload(leaf0, m->stream));
  CC_HIP(m->d_leaves.upload(M.leaves, m->stream));
  CC_HIP(hipStreamSynchronize(m->stream));
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
  CC_HIP(m->d_levels.upload(lv, m->stream));
  CC_HIP(m->front.upload(m->stream));  // synchronises: `lv` ends here
  P.wins = wins;
  P.ox = ox;
  P.oy = oy;
  P.height = height;
  P.width = width;
  return CC_OK;
}

// n_images images of one size, consumed with one offset: ONE copy to the device, one launch of every kernel over all of
// them (the front-end kernels and the window kernels take the image as blockIdx.y, like the detector's frames), one copy back.
static cc_status mine_images(cc_negminer* m, const uint8_t* const* images, int n_images, int width, int height, size_t row_stride, int ox,
                             int oy, uint8_t* pass, int64_t cap, int64_t* n_windows, uint8_t* pixels, int64_t* keep_index, int max_keep,
                             int* n_keep, const char* who) {
  cc_status st = mine_check(m, width, height, ox, oy, who);
  if (st != CC_OK) return st;
  if (!images || n_images < 1 || !pass || !n_windows || row_stride < (size_t)width) return set_error(CC_ERR_INVALID_ARG, "%s: bad argument", who);
  for (int k = 0; k < n_images; k++)
    if (!images[k]) return set_error(CC_ERR_INVALID_ARG, "%s: image %d is null", who, k);
  if (pixels && (!keep_index || !n_keep || max_keep < 0)) return set_error(CC_ERR_INVALID_ARG, "%s: bad keep buffers", who);
  st = ensure_device(m->device);
  if (st != CC_OK) return st;
  st = mine_plan(m, width, height, ox, oy, who);
  if (st != CC_OK) return st;
  const cc_negminer::Plan& P = m->plan;
  const FrontLayout& FL = m->front.L;
  const Cascade& M = m->m;
  const int W0 = M.win_w, H0 = M.win_h, nl = (int)FL.sd.size(), K = n_images;
  const bool haar = M.feature_type == CC_FEATURE_HAAR, tilt = haar && M.has_tilted, hog = M.feature_type == CC_FEATURE_HOG;
  const long long wins = P.wins;
  *n_windows = wins;
  if (wins * K > cap) return set_error(CC_ERR_BUFFER_TOO_SMALL, "%s: %lld windows (%d images), capacity %lld", who, wins * K, K, (long long)cap);
  hipStream_t s = m->stream;
  const int nchan = haar ? (tilt ? 3 : 2) : 1;
  const size_t chan_elems = FL.int_frame_elems, spitch = (size_t)align_up(width, 4), src_bytes = spitch * (size_t)height;
  CC_HIP(m->d_src.ensure(src_bytes * K));
  CC_HIP(m->d_pyr.ensure(FL.pyr_frame_bytes * K));
  if (!hog) {  // HOG windows build their planes from the levels' pixels: no integral images
    CC_HIP(m->d_integ.ensure(chan_elems * (size_t)nchan * K));
    CC_HIP(m->d_hbuf.ensure(std::max<size_t>(FL.h_frame_elems * (size_t)nchan * K, 4)));
  }
  CC_HIP(m->d_pass.ensure((size_t)std::max<long long>(wins * K, 1)));
  CC_HIP(m->h_src.ensure(src_bytes * K));
  CC_HIP(m->h_pass.ensure((size_t)std::max<long long>(wins * K, 1)));
  uint8_t* const h_src = static_cast<uint8_t*>(m->h_src.p);
  MineArgs A;
  A.integ = m->d_integ.p;
  A.chan_elems = chan_elems;
  A.nchan = nchan;
  A.levels = m->d_levels.p;
  A.n_levels = nl;
  A.n_windows = wins;
  A.W0 = W0;
  A.H0 = H0;
  A.ox = ox;
  A.oy = oy;
  A.sx = (int)(0.5F * W0);
  A.sy = (int)(0.5F * H0);
  A.nstages = (int)M.stage_ntrees.size();
  A.stage_first = m->d_stage_first.p;
  A.stage_ntrees = m->d_stage_ntrees.p;
  A.stage_thr = m->d_stage_thr.p;
  A.nodes = m->d_nodes.p;
  A.tree_root = m->d_tree_root.p;
  A.tree_leaf0 = m->d_tree_leaf0.p;
  A.leaves = m->d_leaves.p;
  A.pass = m->d_pass.p;
  if (tilt) {
    CC_HIP(m->d_diag.ensure(chan_elems * 2 * K));
    CC_HIP(m->d_tseg.ensure(std::max<size_t>(FL.tseg_frame_elems * K, 1)));
  }
  // one wavefront per window where the parallel stage sum is exact (stumps, order-independent sums); else one thread per window
  const bool wave_mode = M.max_nodes_per_tree == 1 && stage_sums_order_independent(M);
  // Every kernel over the images [k0, k0 + n): the front-end kernels and the window kernels take the image as blockIdx.y.
  auto launch_images = [&](int k0, int n) {
    FrontIO io;
    io.src = m->d_src.p + (size_t)k0 * src_bytes;
    io.row_stride = spitch;
    io.frame_stride = src_bytes;
    io.pyr = m->d_pyr.p + (size_t)k0 * FL.pyr_frame_bytes;
    if (!hog) {
      io.integ = m->d_integ.p + (size_t)k0 * nchan * chan_elems;
      io.hbuf = m->d_hbuf.p + (size_t)k0 * nchan * FL.h_frame_elems;
    }
    if (tilt) {
      io.diag = m->d_diag.p + (size_t)k0 * 2 * chan_elems;
      io.tseg = m->d_tseg.p + (size_t)k0 * FL.tseg_frame_elems;
    }
    io.nchan = nchan;
    io.sq = haar;
    launch_front(s, m->front, io, n, hog ? FRONT_RESIZE : FRONT_RESIZE | FRONT_INTEGRALS);
    if (wins == 0) return;
    if (hog) {
      HogMineArgs H;
      H.pyr = io.pyr;
      H.pyr_image_bytes = FL.pyr_frame_bytes;
      H.levels = A.levels;
      H.n_levels = A.n_levels;
      H.n_windows = wins;
      H.W0 = W0;
      H.H0 = H0;
      H.ox = ox;
      H.oy = oy;
      H.sx = A.sx;
      H.sy = A.sy;
      H.nstages = A.nstages;
      H.stage_first = A.stage_first;
      H.stage_ntrees = A.stage_ntrees;
      H.stage_thr = A.stage_thr;
      H.nodes = m->d_hog_nodes.p;
      H.tree_root = A.tree_root;
      H.tree_leaf0 = A.tree_leaf0;
      H.leaves = A.leaves;
      H.pass = m->d_pass.p + (size_t)k0 * (size_t)wins;
      H.wave = wave_mode ? 1 : 0;
      hipLaunchKernelGGL(k_negmine_hog, dim3((unsigned)wins, n), dim3(HOG_MINE_THREADS), m->hog_lds, s, H);
      return;
    }
    MineArgs B = A;
    B.integ = io.integ;
    B.pass = m->d_pass.p + (size_t)k0 * (size_t)wins;
    if (wave_mode) {
      const unsigned nb = (unsigned)((wins + 3) / 4);
      if (haar)
        hipLaunchKernelGGL(k_negmine_wave<true>, dim3(nb, n), dim3(256), 0, s, B);
      else
        hipLaunchKernelGGL(k_negmine_wave<false>, dim3(nb, n), dim3(256), 0, s, B);
    } else {
      const unsigned nb = (unsigned)((wins + 255) / 256);
      if (haar)
        hipLaunchKernelGGL(k_negmine_windows<true>, dim3(nb, n), dim3(256), 0, s, B);
      else
        hipLaunchKernelGGL(k_negmine_windows<false>, dim3(nb, n), dim3(256), 0, s, B);
    }
  };
  // Pageable rows -> pinned, tight rows, then asynchronous transfers on the copy stream: the images travel in pieces of >= 8 MB;
  // a piece's copy is issued as soon as it is staged (it runs under the staging of the next piece) and its kernels are queued
  // behind it on the compute stream (they run under the next piece's copy). A Full-HD background is 2 MB for 13 584 windows:
  // the image's way to the device is most of what a call costs. Large pieces are staged by up to 4 threads.
  {
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
      hipEvent_t ev = nullptr;
      CC_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      m->piece_landed.push_back(ev);
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
          (void)hipStreamSynchronize(m->copy_stream);
          (void)hipStreamSynchronize(s);
          return set_error(CC_ERR_HIP, "%s: staging the images: %s", who, e.what());
        }
      }
      CC_HIP(hipMemcpyAsync(m->d_src.p + (size_t)k0 * src_bytes, h_src + (size_t)k0 * src_bytes, (size_t)n * src_bytes, hipMemcpyHostToDevice,
                            m->copy_stream));
      CC_HIP(hipEventRecord(m->piece_landed[piece], m->copy_stream));
      CC_HIP(hipStreamWaitEvent(s, m->piece_landed[piece], 0));
      launch_images(k0, n);
    }
  }
  CC_HIP(hipGetLastError());
  if (wins > 0) CC_HIP(hipMemcpyAsync(m->h_pass.p, m->d_pass.p, (size_t)(wins * K), hipMemcpyDeviceToHost, s));
  CC_HIP(hipStreamSynchronize(s));
  if (wins > 0) std::memcpy(pass, m->h_pass.p, (size_t)(wins * K));
  if (pixels) {
    std::vector<long long> keep;
    for (long long i = 0; i < wins * K && (int)keep.size() < max_keep; i++)
      if (pass[i]) keep.push_back(i);
    *n_keep = (int)keep.size();
    if (!keep.empty()) {
      const size_t wsz = (size_t)W0 * H0;
      CC_HIP(m->d_keep.upload(keep, s));
      CC_HIP(m->d_pix.ensure(keep.size() * wsz));
      hipLaunchKernelGGL(k_negmine_gather, dim3((unsigned)keep.size()), dim3(64), 0, s, m->d_pyr.p, FL.pyr_frame_bytes, wins, m->d_levels.p, nl,
                         m->d_keep.p, W0, H0, ox, oy, A.sx, A.sy, m->d_pix.p);
      CC_HIP(hipGetLastError());
      CC_HIP(hipMemcpyAsync(pixels, m->d_pix.p, keep.size() * wsz, hipMemcpyDeviceToHost, s));
      CC_HIP(hipStreamSynchronize(s));
      for (size_t i = 0; i < keep.size(); i++) keep_index[i] = keep[i];
    }
  }
  return CC_OK;
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

}  // extern "C"
