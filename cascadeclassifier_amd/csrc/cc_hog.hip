// HOG feature evaluator on gfx950: batched setImage (gradient, orientation bin, ten float integral planes per sample) and
// bulk operator() over (variable range x samples). Replaces CvHOGEvaluator (traincascade/lib/include/HOGfeatures.h:43-112,
// traincascade/lib/src/HOGfeatures.cpp:16-256) behind section 4 of the C ABI.
//
// Plane layout in HBM: [max_samples][(W+1)*(H+1)][10] float, the ten planes of one integral entry side by side: channels
// 0..8 are the per-bin integral histograms (`hist[bin]`), channel 9 is the magnitude integral (`normSum`). 40 * (W+1)(H+1)
// bytes per sample (43 560 at 32x32). A variable reads one bin at the four corners of a cell; the 36 variables of a block
// read the 9 bins at the block's 3x3 corner lattice plus the norm at its 4 outer corners, so one (sample, block) is 9
// lattice points x 40 contiguous bytes: 45 eight-byte loads per lane instead of 288 scattered reads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>

#include "cc_hog_device.h"
#include "cc_train_device.h"

namespace ccamd {

// ------------------------------------------------------------------------------------------------
// setImage for a batch: one block per sample.
//   1. gradient magnitude and bin of every pixel into LDS (BORDER_REPLICATE: indices clamped);
//   2. row pass, one lane per (plane, row): the running row sum in float, strictly left to right (the reference's
//      `strSum += mag`; a parallel scan would reassociate), into LDS;
//   3. column pass, one lane per (plane, column): integral(y + 1, x) = integral(y, x) + rowsum(y, x), top to bottom,
//      written to HBM. Lanes of a wavefront cover consecutive (column, plane) pairs: contiguous stores.
// Planes go through LDS `planes_per_pass` at a time (all ten up to ~40x40 windows at the 64 KB budget).
// ------------------------------------------------------------------------------------------------
constexpr int HOG_SET_THREADS = 256;

__global__ __launch_bounds__(HOG_SET_THREADS) void k_hog_set_images(const uint8_t* __restrict__ imgs, int W, int H, int first_idx,
                                                                    int planes_per_pass, float* __restrict__ planes) {
  extern __shared__ float lds_f[];
  const int sw = W + 1, cols = sw * (H + 1);
  float* mag = lds_f;                                              // [H][W]
  float* rp = lds_f + (size_t)W * H;                               // [P][H][W + 1], column 0 = 0
  uint8_t* bins = reinterpret_cast<uint8_t*>(rp + (size_t)planes_per_pass * H * sw);  // [H][W]
  const uint8_t* img = imgs + (size_t)blockIdx.x * W * H;
  float* out = planes + (size_t)(first_idx + blockIdx.x) * cols * 10;
  hog_window_grad(img, W, W, H, mag, bins, threadIdx.x, HOG_SET_THREADS);
  __syncthreads();
  for (int c0 = 0; c0 < 10; c0 += planes_per_pass) {
    const int P = min(planes_per_pass, 10 - c0);
    hog_row_pass(mag, bins, W, H, c0, P, rp, (size_t)H * sw, threadIdx.x, HOG_SET_THREADS);
    __syncthreads();
    // lanes of a wavefront cover consecutive (column, plane) pairs: contiguous stores
    hog_col_pass(rp, (size_t)H * sw, W, H, c0, P, [=](int c, int x, int y) { return out + ((size_t)y * sw + x) * 10 + c; }, threadIdx.x,
                 HOG_SET_THREADS);
    __syncthreads();  // rp is rewritten by the next group of planes
  }
}

// ------------------------------------------------------------------------------------------------
// Bulk operator(): a wavefront owns 64 samples (lanes) and walks feature blocks; per block it loads the 3x3 lattice (9 x 10
// floats) once and emits the block's variables that fall in [vi_begin, vi_end) to out[(vi - vi_begin) * pitch + s]:
// for a fixed variable the 64 lanes store 256 contiguous bytes.
// ------------------------------------------------------------------------------------------------
constexpr int HOG_EVAL_THREADS = 256;

struct HogBatchArgs {
  const float* planes;
  const int32_t* blocks;      // [num_blocks][4]: x, y, cell w, cell h
  const int32_t* sample_idx;  // optional
  int n_samples, sw, cols;
  int vi_begin, vi_end;
  int blk_begin, blk_end;     // blocks overlapping [vi_begin, vi_end)
  int blks_per_chunk;
  float* out;
  size_t out_pitch;
};

__global__ __launch_bounds__(HOG_EVAL_THREADS) void k_hog_eval_batch(HogBatchArgs A) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  constexpr int WAVES = HOG_EVAL_THREADS / 64;
  const int s = blockIdx.x * 64 + lane;
  const bool valid = s < A.n_samples;
  const int si = valid ? (A.sample_idx ? A.sample_idx[s] : s) : 0;
  const float* base = A.planes + (size_t)si * A.cols * 10;
  const int b0 = A.blk_begin + blockIdx.y * A.blks_per_chunk;
  const int b1 = min(b0 + A.blks_per_chunk, A.blk_end);
  float* out = A.out + s;
  for (int b = b0 + wave; b < b1; b += WAVES) {
    const int x = A.blocks[4 * b], y = A.blocks[4 * b + 1], cw = A.blocks[4 * b + 2], ch = A.blocks[4 * b + 3];
    float h[9][10];  // lattice point (i, j) -> h[j * 3 + i][channel]
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
      for (int i = 0; i < 3; i++) {
        const float2* p = reinterpret_cast<const float2*>(base + ((size_t)(y + j * ch) * A.sw + x + i * cw) * 10);
#pragma unroll
        for (int k = 0; k < 5; k++) {
          const float2 v = p[k];
          h[j * 3 + i][2 * k] = v.x;
          h[j * 3 + i][2 * k + 1] = v.y;
        }
      }
    const float nf = ((h[0][9] - h[2][9]) - h[6][9]) + h[8][9];
    const int v0 = b * 36;
#pragma unroll
    for (int cell = 0; cell < 4; cell++) {
      const int q = (cell >> 1) * 3 + (cell & 1);  // lattice index of the cell's top-left corner
#pragma unroll
      for (int bin = 0; bin < 9; bin++) {
        const int vi = v0 + cell * 9 + bin;
        if (vi < A.vi_begin || vi >= A.vi_end) continue;  // wave-uniform: ranges that start or end inside a block
        const float res = ((h[q][bin] - h[q + 1][bin]) - h[q + 3][bin]) + h[q + 4][bin];
        if (valid) out[(size_t)(vi - A.vi_begin) * A.out_pitch] = hog_value_from(res, nf);
      }
    }
  }
}

// operator()(vi[k], one stored sample): one thread per list entry.
__global__ void k_hog_eval_list(const float* __restrict__ planes, const int32_t* __restrict__ blocks, int sw,
                                const int32_t* __restrict__ list, int n, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int vi = list[i];
  out[i] = hog_var_value(planes, sw, blocks + 4 * (vi / 36), vi % 36);
}

// CvCascadeClassifier::predict on stored samples: one thread per sample walks the stages (walk_stages, cc_train_device.h)
// on the sample's planes; a variable's value is operator()'s (hog_var_value), an ordered split goes left on `<=`.
struct HogNodeDev {
  int32_t blk[4];  // x, y, cell w, cell h of the block
  int32_t comp;
  float thr;
  int32_t left, right;  // child > 0: node index inside the tree; child <= 0: leaf index -child
};

struct HogPredictArgs {
  const float* planes;
  int sw, cols;
  const int32_t* sample_idx;  // optional
  int n_samples;
  WalkTables walk;
  const HogNodeDev* nodes;
  uint8_t* out;
};

__global__ __launch_bounds__(64) void k_hog_predict(HogPredictArgs A) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= A.n_samples) return;
  const int si = A.sample_idx ? A.sample_idx[s] : s;
  const float* planes = A.planes + (size_t)si * A.cols * 10;
  A.out[s] = walk_stages(A.walk, [&](int i) {
    const HogNodeDev& n = A.nodes[i];
    return hog_var_value(planes, A.sw, n.blk, n.comp) <= n.thr ? n.left : n.right;
  });
}

// Bin and magnitude of every (dx, dy) in [-255, 255]^2, pair (dx, dy) at (dy + 255) * 511 + dx + 255.
__global__ void k_hog_bins(uint8_t* __restrict__ bin, float* __restrict__ mag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 511 * 511) return;
  const int dy = i / 511 - 255, dx = i % 511 - 255;
  float m;
  bin[i] = (uint8_t)hog_grad_bin(dx, dy, &m);
  mag[i] = m;
}

// ------------------------------------------------------------------------------------------------
// Host side
// ------------------------------------------------------------------------------------------------
// hog_catalog: cc_host.cpp, beside the Haar and LBP catalogs (cc_cascade_from_stumps needs it without a device).
static LdsOptIn g_set_images_lds;  // k_hog_set_images' opt-in, shared by every HOG evaluator

cc_status hog_init(cc_evaluator* e) {
  hog_catalog(e->W, e->H, e->hog_blocks);
  e->nfeat = (int)(e->hog_blocks.size() / 4) * 36;  // the trainer's variable space (o_cvcascadeboosttraindata.cpp:246-247)
  const HogLdsPlan plan = hog_lds_plan(e->W, e->H);
  e->hog_planes_per_pass = plan.planes_per_pass;
  e->hog_set_lds = plan.set_bytes;
  if (e->hog_planes_per_pass == 0)
    return set_error(CC_ERR_UNSUPPORTED, "cc_eval_create: HOG window %dx%d too large for the setImage kernel's LDS", e->W, e->H);
  CC_HIP(g_set_images_lds.raise(reinterpret_cast<const void*>(&k_hog_set_images), e->device, plan.set_bytes));
  CC_HIP(e->samples.hog.ensure((size_t)e->max_samples * e->cols * 10));
  CC_HIP(hipMemsetAsync(e->samples.hog.p, 0, (size_t)e->max_samples * e->cols * 10 * 4, e->stream.s));
  CC_HIP(e->d_hog_blocks.ensure(std::max<size_t>(e->hog_blocks.size(), 4)));
  if (!e->hog_blocks.empty())
    CC_HIP(copy_sync(e->d_hog_blocks.p, e->hog_blocks.data(), e->hog_blocks.size() * 4, hipMemcpyHostToDevice, e->stream.s));
  return CC_OK;
}

cc_status hog_launch_set_images(cc_evaluator* e, const SampleTables& t, const uint8_t* d_imgs, int n, int first_idx) {
  hipLaunchKernelGGL(k_hog_set_images, dim3(n), dim3(HOG_SET_THREADS), e->hog_set_lds, e->stream.s, d_imgs, e->W, e->H, first_idx,
                     e->hog_planes_per_pass, t.hog.p);
  CC_HIP(hipGetLastError());
  return CC_OK;
}

cc_status hog_launch_batch(cc_evaluator* e, int vb, int ve, const int32_t* d_idx, int ns, float* d_out, size_t out_pitch) {
  HogBatchArgs A;
  A.planes = e->samples.hog.p;
  A.blocks = e->d_hog_blocks.p;
  A.sample_idx = d_idx;
  A.n_samples = ns;
  A.sw = e->W + 1;
  A.cols = e->cols;
  A.vi_begin = vb;
  A.vi_end = ve;
  A.blk_begin = vb / 36;
  A.blk_end = (ve + 35) / 36;
  A.out = d_out;
  A.out_pitch = out_pitch ? out_pitch : (size_t)ns;
  const int nblk = A.blk_end - A.blk_begin, tiles = (ns + 63) / 64;
  // chunks of blocks: enough workgroups for a few rounds over the chip, at least one block per wavefront
  int chunks = std::max(1, std::min((nblk + 3) / 4, (256 * 8 + tiles - 1) / std::max(tiles, 1)));
  A.blks_per_chunk = (nblk + chunks - 1) / chunks;
  chunks = (nblk + A.blks_per_chunk - 1) / A.blks_per_chunk;
  (void)hipEventRecord(e->ev_a.e, e->stream.s);
  hipLaunchKernelGGL(k_hog_eval_batch, dim3(tiles, chunks), dim3(HOG_EVAL_THREADS), 0, e->stream.s, A);
  (void)hipEventRecord(e->ev_b.e, e->stream.s);
  CC_HIP(hipGetLastError());
  return CC_OK;
}

cc_status hog_launch_list(cc_evaluator* e, const int32_t* d_list, int n, int si, float* d_out) {
  hipLaunchKernelGGL(k_hog_eval_list, dim3((n + 255) / 256), dim3(256), 0, e->stream.s, e->samples.hog.p + (size_t)si * e->cols * 10,
                     e->d_hog_blocks.p, e->W + 1, d_list, n, d_out);
  CC_HIP(hipGetLastError());
  return CC_OK;
}

cc_status hog_predict(cc_evaluator* e, const SampleTables& t, const Cascade& m, const int32_t* d_idx, int ns, uint8_t* out) {
  std::vector<HogNodeDev> nodes(m.node_feature.size());
  for (size_t i = 0; i < nodes.size(); i++) {
    const int32_t* f = &m.hog_feats[(size_t)m.node_feature[i] * 5];  // validated inside the window at load
    HogNodeDev& n = nodes[i];
    for (int k = 0; k < 4; k++) n.blk[k] = f[k];
    n.comp = f[4];
    n.thr = m.node_threshold[i];
    n.left = m.node_left[i];
    n.right = m.node_right[i];
  }
  // declared after `nodes`: on an early return these go first, and hipFree waits for the queued copies that read it and m
  WalkTablesDev walk;
  DevBuf<HogNodeDev> d_nodes;
  CC_HIP(walk.upload(m, e->stream.s));
  CC_HIP(d_nodes.upload(nodes, e->stream.s));
  CC_HIP(e->d_pred.ensure((size_t)ns));
  HogPredictArgs A;
  A.planes = t.hog.p;
  A.sw = e->W + 1;
  A.cols = e->cols;
  A.sample_idx = d_idx;
  A.n_samples = ns;
  A.walk = walk.tables();
  A.nodes = d_nodes.p;
  A.out = e->d_pred.p;
  hipLaunchKernelGGL(k_hog_predict, dim3((ns + 63) / 64), dim3(64), 0, e->stream.s, A);
  CC_HIP(hipGetLastError());
  if (out) CC_HIP(hipMemcpyAsync(out, e->d_pred.p, (size_t)ns, hipMemcpyDeviceToHost, e->stream.s));
  CC_HIP(hipStreamSynchronize(e->stream.s));  // the tables and `nodes` above are freed on return
  return CC_OK;
}

// The ten planes of one window on the host, entry for entry what k_hog_set_images writes (same per-pixel function, same
// sequential float sums; this translation unit is compiled with -ffp-contract=off).
void hog_host_planes(const cc_evaluator* e, const uint8_t* px, std::vector<float>& planes) {
  const int W = e->W, H = e->H, sw = W + 1;
  std::vector<float> mag((size_t)W * H);
  std::vector<uint8_t> bins((size_t)W * H);
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++) {
      const int xl = std::max(x - 1, 0), xr = std::min(x + 1, W - 1), yu = std::max(y - 1, 0), yd = std::min(y + 1, H - 1);
      const int dx = (int)px[y * W + xr] - (int)px[y * W + xl];
      const int dy = (int)px[yd * W + x] - (int)px[yu * W + x];
      bins[(size_t)y * W + x] = (uint8_t)hog_grad_bin(dx, dy, &mag[(size_t)y * W + x]);
    }
  planes.assign((size_t)e->cols * 10, 0.f);
  for (int c = 0; c < 10; c++)
    for (int y = 0; y < H; y++) {
      float s = 0.f;
      for (int x = 0; x < W; x++) {
        if (c == 9 || bins[(size_t)y * W + x] == c) s += mag[(size_t)y * W + x];
        planes[((size_t)(y + 1) * sw + x + 1) * 10 + c] = planes[((size_t)y * sw + x + 1) * 10 + c] + s;
      }
    }
}

float hog_host_value(const cc_evaluator* e, const float* planes, int vi) {
  return hog_var_value(planes, e->W + 1, &e->hog_blocks[(size_t)(vi / 36) * 4], vi % 36);
}

}  // namespace ccamd

using namespace ccamd;

extern "C" {

cc_status cc_eval_hog_feature_geometry(const cc_evaluator* e, int feature_idx, int32_t* cells) {
  if (!e || !cells) return set_error(CC_ERR_INVALID_ARG, "cc_eval_hog_feature_geometry: null argument");
  if (e->type != CC_FEATURE_HOG) return set_error(CC_ERR_INVALID_ARG, "cc_eval_hog_feature_geometry: evaluator is not HOG");
  const int nb = (int)(e->hog_blocks.size() / 4);
  if (feature_idx < 0 || feature_idx >= nb)
    return set_error(CC_ERR_OUT_OF_RANGE, "cc_eval_hog_feature_geometry: feature %d out of range (%d)", feature_idx, nb);
  const int32_t* b = &e->hog_blocks[(size_t)feature_idx * 4];
  for (int c = 0; c < 4; c++) {  // HOGfeatures.cpp:120-131: 0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right
    cells[4 * c] = b[0] + (c & 1) * b[2];
    cells[4 * c + 1] = b[1] + (c >> 1) * b[3];
    cells[4 * c + 2] = b[2];
    cells[4 * c + 3] = b[3];
  }
  return CC_OK;
}

cc_status cc_eval_get_hog_sample(cc_evaluator* e, int idx, float* hist, float* norm) {
  if (!e) return set_error(CC_ERR_INVALID_ARG, "cc_eval_get_hog_sample: null evaluator");
  if (e->type != CC_FEATURE_HOG) return set_error(CC_ERR_INVALID_ARG, "cc_eval_get_hog_sample: evaluator is not HOG");
  if (idx < 0 || idx >= e->max_samples) return set_error(CC_ERR_OUT_OF_RANGE, "cc_eval_get_hog_sample: idx %d out of range", idx);
  cc_status st = eval_device(e);
  if (st != CC_OK) return st;
  std::lock_guard<std::mutex> lk(e->mu);
  st = flush_pending_images(e);  // the device's copy is what this call reports, also for a sample set a moment ago
  if (st != CC_OK) return st;
  std::vector<float> v((size_t)e->cols * 10);
  CC_HIP(copy_sync(v.data(), e->samples.hog.p + (size_t)idx * e->cols * 10, v.size() * 4, hipMemcpyDeviceToHost, e->stream.s));
  for (int p = 0; p < e->cols; p++) {
    if (hist)
      for (int b = 0; b < 9; b++) hist[(size_t)b * e->cols + p] = v[(size_t)p * 10 + b];
    if (norm) norm[p] = v[(size_t)p * 10 + 9];
  }
  return CC_OK;
}

cc_status cc_debug_hog_lds(int win_w, int win_h, int* planes_per_pass, int* set_budget_kib, int64_t* set_bytes, int64_t* mine_bytes) {
  if (win_w < 1 || win_h < 1 || win_w > 4096 || win_h > 4096) return set_error(CC_ERR_INVALID_ARG, "cc_debug_hog_lds: window %dx%d", win_w, win_h);
  const HogLdsPlan p = hog_lds_plan(win_w, win_h);
  if (planes_per_pass) *planes_per_pass = p.planes_per_pass;
  if (set_budget_kib) *set_budget_kib = p.set_budget_kib;
  if (set_bytes) *set_bytes = (int64_t)p.set_bytes;
  if (mine_bytes) *mine_bytes = (int64_t)p.mine_bytes;
  return CC_OK;
}

cc_status cc_debug_hog_bins(int device, int32_t* n, uint8_t* bin, float* mag) {
  if (!n || !bin || !mag) return set_error(CC_ERR_INVALID_ARG, "cc_debug_hog_bins: null output");
  if (cc_status st = ensure_device(device); st != CC_OK) return st;
  constexpr int N = 511 * 511;
  DevBuf<uint8_t> d_bin;
  DevBuf<float> d_mag;
  CC_HIP(d_bin.ensure(N));
  CC_HIP(d_mag.ensure(N));
  OwnStream own;  // not the legacy stream: see copy_sync
  CC_HIP(own.create());
  CC_HIP(hipMemsetAsync(d_bin.p, 0xFF, N, own.s));
  CC_HIP(hipMemsetAsync(d_mag.p, 0, (size_t)N * 4, own.s));
  hipLaunchKernelGGL(k_hog_bins, dim3((N + 255) / 256), dim3(256), 0, own.s, d_bin.p, d_mag.p);
  CC_HIP(hipGetLastError());
  CC_HIP(copy_sync(bin, d_bin.p, N, hipMemcpyDeviceToHost, own.s));
  CC_HIP(copy_sync(mag, d_mag.p, (size_t)N * 4, hipMemcpyDeviceToHost, own.s));
  *n = N;
  return CC_OK;
}

}  // extern "C"
