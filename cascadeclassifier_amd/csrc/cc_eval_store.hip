// Training-side feature evaluator on gfx950, the evaluator's life and its samples: create / destroy, batched setImage
// (per-sample integral / tilted integral / norm factor), the queue and the host mirror of images set one at a time.
// Bulk operator() is in cc_eval_calc.hip, cascade predict in cc_eval_predict.hip, HOG in cc_hog.hip. Replaces
// CvHaarEvaluator / CvLBPEvaluator (traincascade/lib/include/haarfeatures.h:61-122, lbpfeatures.h:37-83,
// traincascade/lib/src/haarfeatures.cpp:89-114, lbpfeatures.cpp:15-28) behind section 4 of the C ABI.
//
// Data layout in HBM: sum / tilted are [max_samples][(W+1)*(H+1)] int32, one sample per row exactly like the
// reference's `sum` / `tilted` Mats; normfactor is [max_samples] float.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>

#include "cc_train_device.h"

namespace ccamd {

// ------------------------------------------------------------------------------------------------
// setImage for a batch: one 64-thread block per sample.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_set_images(const uint8_t* __restrict__ imgs, int W, int H, int first_idx,
                                                   int32_t* __restrict__ sum, int32_t* __restrict__ tilted,
                                                   float* __restrict__ normfactor, int want_norm) {
  extern __shared__ int32_t lds[];  // row prefix sums [H][W+1]
  const int cols = (W + 1) * (H + 1), sw = W + 1;
  const int i = blockIdx.x;
  const uint8_t* img = imgs + (size_t)i * W * H;
  int32_t* s = sum + (size_t)(first_idx + i) * cols;
  for (int y = threadIdx.x; y < H; y += 64) {
    int acc = 0;
    lds[y * sw] = 0;
    for (int x = 0; x < W; x++) {
      acc += img[y * W + x];
      lds[y * sw + x + 1] = acc;
    }
  }
  __syncthreads();
  for (int x = threadIdx.x; x <= W; x += 64) {
    int acc = 0;
    s[x] = 0;
    for (int y = 0; y < H; y++) {
      acc += lds[y * sw + x];
      s[(y + 1) * sw + x] = acc;
    }
  }
  if (tilted) {
    int32_t* t = tilted + (size_t)(first_idx + i) * cols;
    for (int e = threadIdx.x; e < cols; e += 64) {
      const int Y = e / sw, X = e - Y * sw;
      int acc = 0;
      for (int y = 0; y < Y; y++) {
        const int half = Y - y - 1;
        const int x0 = max(X - 1 - half, 0), x1 = min(X - 1 + half, W - 1);
        if (x1 >= x0) acc += lds[y * sw + x1 + 1] - lds[y * sw + x0];
      }
      t[e] = acc;
    }
  }
  if (want_norm) {
    // calcNormFactor (features.cpp:13-25): sums over normrect (1,1,W-2,H-2); the reference's double sqsum integral
    // holds exact integers, so the 4-corner difference equals the exact integer sum of squares computed here.
    long long sq = 0;
    int sm = 0;
    for (int e = threadIdx.x; e < (W - 2) * (H - 2); e += 64) {
      const int y = 1 + e / (W - 2), x = 1 + e % (W - 2);
      const int p = img[y * W + x];
      sm += p;
      sq += p * p;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      sm += __shfl_xor(sm, d);
      sq += __shfl_xor(sq, d);
    }
    if (threadIdx.x == 0) {
      const double area = (double)((W - 2) * (H - 2));
      normfactor[first_idx + i] = (float)sqrt((double)(area * (double)sq - (double)sm * (double)sm));
    }
  }
}

cc_status eval_device(cc_evaluator* e) { return ensure_device(e->device); }

cc_status launch_set_images(cc_evaluator* e, const SampleTables& t, const uint8_t* d_imgs, int n, int first_idx) {
  if (e->type == CC_FEATURE_HOG) return hog_launch_set_images(e, t, d_imgs, n, first_idx);
  const size_t lds = (size_t)e->H * (e->W + 1) * 4;
  hipLaunchKernelGGL(k_set_images, dim3(n), dim3(64), lds, e->stream.s, d_imgs, e->W, e->H, first_idx, t.sum.p,
                     e->use_tilted ? t.tilted.p : nullptr, t.nf.p, e->type == CC_FEATURE_HAAR ? 1 : 0);
  CC_HIP(hipGetLastError());
  return CC_OK;
}

// setImage of n > 0 windows into the stored samples [first_idx, first_idx + n): pending queue first, generation, host
// mirror, the pixels to the device unless they are there (on_device), launch, synchronise. Caller holds e->mu and sets
// the labels.
static cc_status set_images(cc_evaluator* e, const uint8_t* imgs, bool on_device, int n, int first_idx) {
  cc_status st = flush_pending_images(e);  // images set earlier, one at a time, must not land on top of these
  if (st != CC_OK) return st;
  e->generation++;
  if (e->mirror_idx >= first_idx && e->mirror_idx < first_idx + n) e->mirror_idx = -1;
  if (!on_device) {
    const size_t bytes = (size_t)n * e->W * e->H;
    CC_HIP(e->d_imgs.ensure(bytes));
    CC_HIP(hipMemcpyAsync(e->d_imgs.p, imgs, bytes, hipMemcpyHostToDevice, e->stream.s));
    imgs = e->d_imgs.p;
  }
  st = launch_set_images(e, e->samples, imgs, n, first_idx);
  if (st != CC_OK) return st;
  CC_HIP(hipStreamSynchronize(e->stream.s));
  return CC_OK;
}

cc_status eval_set_images_device(cc_evaluator* e, const uint8_t* d_imgs, int n, int first_idx, float label) {
  if (n == 0) return CC_OK;
  std::lock_guard<std::mutex> lk(e->mu);
  if (cc_status st = set_images(e, d_imgs, true, n, first_idx); st != CC_OK) return st;
  for (int i = 0; i < n; i++) e->cls[(size_t)first_idx + i] = label;
  return CC_OK;
}

cc_status flush_pending_images(cc_evaluator* e) {
  const int n = (int)e->pend_idx.size();
  if (n == 0) return CC_OK;
  const size_t px = (size_t)e->W * e->H;
  // upload in sample order so that consecutive indices become one launch
  std::vector<int> order((size_t)n);
  for (int i = 0; i < n; i++) order[(size_t)i] = i;
  std::sort(order.begin(), order.end(), [&](int a, int b) { return e->pend_idx[(size_t)a] < e->pend_idx[(size_t)b]; });
  CC_HIP(e->pin_in.ensure((size_t)n * px));
  uint8_t* host = static_cast<uint8_t*>(e->pin_in.p);
  for (int i = 0; i < n; i++) std::memcpy(host + (size_t)i * px, e->pend_px.data() + (size_t)order[(size_t)i] * px, px);
  CC_HIP(e->d_imgs.ensure((size_t)n * px));
  CC_HIP(hipMemcpyAsync(e->d_imgs.p, host, (size_t)n * px, hipMemcpyHostToDevice, e->stream.s));
  for (int i = 0; i < n;) {
    int j = i + 1;
    while (j < n && e->pend_idx[(size_t)order[(size_t)j]] == e->pend_idx[(size_t)order[(size_t)j - 1]] + 1) j++;
    if (cc_status st = launch_set_images(e, e->samples, e->d_imgs.p + (size_t)i * px, j - i, e->pend_idx[(size_t)order[(size_t)i]]); st != CC_OK)
      return st;
    i = j;
  }
  CC_HIP(hipStreamSynchronize(e->stream.s));
  for (int32_t idx : e->pend_idx) e->pend_slot[(size_t)idx] = -1;
  e->pend_idx.clear();
  e->pend_px.clear();
  return CC_OK;
}

// The integral(s) and the norm factor of one W x H window on the host, entry for entry what k_set_images writes
// (haarfeatures.cpp:100-114, features.cpp:13-25, lbpfeatures.cpp:22-28): sum(y + 1, x + 1) = pixels above and to the left
// incl.; tilted(Y, X) = pixels of rows y < Y within |x - (X - 1)| <= Y - y - 1; norm factor from the exact integer sums over
// normrect (1, 1, W - 2, H - 2). Integer arithmetic throughout, one correctly rounded double sqrt at the end.
static void host_window_integrals(const cc_evaluator* e, const uint8_t* px, std::vector<int32_t>& sum, std::vector<int32_t>& tilted, float& nf) {
  const int W = e->W, H = e->H, sw = W + 1;
  sum.assign((size_t)e->cols, 0);
  for (int y = 0; y < H; y++) {
    int acc = 0;
    for (int x = 0; x < W; x++) {
      acc += px[y * W + x];
      sum[(size_t)(y + 1) * sw + x + 1] = sum[(size_t)y * sw + x + 1] + acc;
    }
  }
  if (e->use_tilted) {
    // row prefix sums r[y][x + 1] = px[y][0..x]; then the kernel's row-by-row clipped spans
    std::vector<int32_t> rp((size_t)H * sw, 0);
    for (int y = 0; y < H; y++)
      for (int x = 0; x < W; x++) rp[(size_t)y * sw + x + 1] = rp[(size_t)y * sw + x] + px[y * W + x];
    tilted.assign((size_t)e->cols, 0);
    for (int Y = 0; Y <= H; Y++)
      for (int X = 0; X <= W; X++) {
        int acc = 0;
        for (int y = 0; y < Y; y++) {
          const int half = Y - y - 1;
          const int x0 = std::max(X - 1 - half, 0), x1 = std::min(X - 1 + half, W - 1);
          if (x1 >= x0) acc += rp[(size_t)y * sw + x1 + 1] - rp[(size_t)y * sw + x0];
        }
        tilted[(size_t)Y * sw + X] = acc;
      }
  }
  nf = 0.f;
  if (e->type == CC_FEATURE_HAAR) {
    long long sq = 0;
    int sm = 0;
    for (int y = 1; y < H - 1; y++)
      for (int x = 1; x < W - 1; x++) {
        const int p = px[y * W + x];
        sm += p;
        sq += p * p;
      }
    const double area = (double)((W - 2) * (H - 2));
    nf = (float)std::sqrt((double)(area * (double)sq - (double)sm * (double)sm));
  }
}

// operator()(fi) on the mirrored window: the functions k_eval_list calls (haarfeatures.h:108-122, lbpfeatures.h:70-83).
// Built with -ffp-contract=off; float division on the host is the correctly rounded quotient the device kernels produce.
static inline float host_mirror_value(const cc_evaluator* e, int fi) {
  if (e->type == CC_FEATURE_HAAR) {
    const HaarFeatDev& F = e->h_haar[(size_t)fi];
    const int32_t* b = F.tilted ? e->mirror_tilted.data() : e->mirror_sum.data();
    return haar_value(haar_sum(F, [&](int o) { return b[o]; }), e->mirror_nf);
  }
  const int32_t* s = e->mirror_sum.data();
  return (float)lbp_code_at(e->h_lbp[(size_t)fi], [&](int o) { return s[o]; });
}
// The plain-offset catalog (row stride W + 1) of the host mirror, built once; cc_eval_calc_list uploads one from a temporary.
static void host_catalog(cc_evaluator* e) {
  std::call_once(e->host_catalog_once, [e]() {
    if (e->type == CC_FEATURE_HAAR)
      e->h_haar = haar_catalog_dev(e->haar, e->W);
    else
      e->h_lbp = lbp_catalog_dev(e->lbp, e->W);
  });
}
bool mirror_answer(cc_evaluator* e, int si, const int32_t* feats, int n, float* out) {
  if (e->type == CC_FEATURE_HOG) {
    std::lock_guard<std::mutex> lk(e->mu);
    if (si != e->mirror_idx) return false;
    for (int i = 0; i < n; i++) out[i] = hog_host_value(e, e->mirror_hog.data(), feats[i]);
    return true;
  }
  if (si != e->mirror_idx) return false;
  host_catalog(e);
  for (int i = 0; i < n; i++) out[i] = host_mirror_value(e, feats[i]);
  return true;
}

}  // namespace ccamd

using namespace ccamd;

extern "C" {

cc_status cc_eval_create(int feature_type, int haar_mode, int win_w, int win_h, int max_samples, int device, cc_evaluator** out) {
  if (!out) return set_error(CC_ERR_INVALID_ARG, "cc_eval_create: null output");
  *out = nullptr;
  if (feature_type != CC_FEATURE_HAAR && feature_type != CC_FEATURE_LBP && feature_type != CC_FEATURE_HOG) return set_error(CC_ERR_INVALID_ARG, "cc_eval_create: unknown feature type %d", feature_type);
  if (max_samples <= 0) return set_error(CC_ERR_INVALID_ARG, "cc_eval_create: maxSampleCount must be > 0");  // features.cpp:75
  if (win_w < 3 || win_h < 3 || win_w > 256 || win_h > 256) return set_error(CC_ERR_INVALID_ARG, "cc_eval_create: window %dx%d out of range", win_w, win_h);
  if (feature_type == CC_FEATURE_HAAR && (haar_mode < CC_HAAR_BASIC || haar_mode > CC_HAAR_ALL))
    return set_error(CC_ERR_INVALID_ARG, "cc_eval_create: unknown Haar mode %d", haar_mode);
  std::unique_ptr<cc_evaluator> e(new cc_evaluator());
  e->type = feature_type;
  e->mode = haar_mode;
  e->W = win_w;
  e->H = win_h;
  e->max_samples = max_samples;
  e->device = device;
  e->cols = (win_w + 1) * (win_h + 1);
  e->use_tilted = feature_type == CC_FEATURE_HAAR && haar_mode == CC_HAAR_ALL;
  cc_status st = eval_device(e.get());
  if (st != CC_OK) return st;
  e->cls.assign((size_t)max_samples, 0.f);
  CC_HIP(e->stream.create());
  CC_HIP(e->ev_a.create());
  CC_HIP(e->ev_b.create());
  if (feature_type == CC_FEATURE_HOG) {  // haar_mode is ignored; planes and catalog in cc_hog.hip
    st = hog_init(e.get());
    if (st != CC_OK) return st;
    CC_HIP(hipStreamSynchronize(e->stream.s));
    *out = e.release();
    return CC_OK;
  }
  // samples per LDS tile: largest power of two (<= 32) that keeps the tile within 80 KB (two blocks per CU). With 32
  // samples per tile each 32-lane half of a wavefront is one feature over 32 consecutive samples: LDS reads are
  // conflict-free and every output store is a full 128-byte line.
  const size_t per_sample = (size_t)e->cols * 4 * (e->use_tilted ? 2 : 1);
  const size_t budget = 80 * 1024;
  int S = 32;
  while (S > 1 && per_sample * S > budget) S >>= 1;
  if (per_sample * S > budget) return set_error(CC_ERR_UNSUPPORTED, "cc_eval_create: window %dx%d too large for the LDS tile", win_w, win_h);
  // the wide tile (64 samples, the whole 160 KB of a CU, k_eval_batch_wide) where it fits and no tilted tile is needed
  if (!e->use_tilted && per_sample * 64 <= 160 * 1024) S = 64;
  e->S = S;
  if (per_sample * S > 64 * 1024)
    if (st = batch_kernels_allow_lds((int)(per_sample * S)); st != CC_OK) return st;
  // k_set_images keeps the row prefix sums of one sample, H * (W + 1) words, in dynamic LDS: past 64 KB (128x128 LBP asks
  // for 66 048 bytes) the attribute is raised as for the batch kernels above (a runtime that enforces it refuses the launch)
  if (const size_t set_lds = (size_t)win_h * (win_w + 1) * 4; set_lds > 64 * 1024)
    CC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_set_images), hipFuncAttributeMaxDynamicSharedMemorySize, (int)set_lds));
  CC_HIP(e->samples.sum.ensure((size_t)max_samples * e->cols));
  CC_HIP(hipMemsetAsync(e->samples.sum.p, 0, (size_t)max_samples * e->cols * 4, e->stream.s));
  if (e->use_tilted) {
    CC_HIP(e->samples.tilted.ensure((size_t)max_samples * e->cols));
    CC_HIP(hipMemsetAsync(e->samples.tilted.p, 0, (size_t)max_samples * e->cols * 4, e->stream.s));
  }
  CC_HIP(e->samples.nf.ensure((size_t)max_samples));
  CC_HIP(hipMemsetAsync(e->samples.nf.p, 0, (size_t)max_samples * 4, e->stream.s));
  if (feature_type == CC_FEATURE_HAAR) {
    haar_catalog(win_w, win_h, haar_mode, e->haar);
    e->nfeat = (int)e->haar.size();
    const std::vector<HaarFeatDev> dev = haar_catalog_dev(e->haar, win_w, e->S, e->use_tilted ? e->cols * e->S * 4 : 0);
    CC_HIP(e->d_haar.ensure(std::max<size_t>(dev.size(), 1)));
    CC_HIP(copy_sync(e->d_haar.p, dev.data(), dev.size() * sizeof(HaarFeatDev), hipMemcpyHostToDevice, e->stream.s));
  } else {
    lbp_catalog(win_w, win_h, e->lbp);
    e->nfeat = (int)(e->lbp.size() / 4);
    const std::vector<LbpFeatDev> dev = lbp_catalog_dev(e->lbp, win_w, e->S);
    CC_HIP(e->d_lbp.ensure(std::max<size_t>(dev.size(), 1)));
    CC_HIP(copy_sync(e->d_lbp.p, dev.data(), dev.size() * sizeof(LbpFeatDev), hipMemcpyHostToDevice, e->stream.s));
  }
  CC_HIP(hipStreamSynchronize(e->stream.s));
  *out = e.release();
  return CC_OK;
}

void cc_eval_destroy(cc_evaluator* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  (void)hipStreamSynchronize(e->stream.s);  // nothing is in flight when the members go, in whatever order
  delete e;
}

int cc_eval_num_features(const cc_evaluator* e) {
  if (!e) return 0;
  return e->type == CC_FEATURE_HOG ? (int)(e->hog_blocks.size() / 4) : e->nfeat;  // HOG: blocks (HOGfeatures.cpp:105)
}
int cc_debug_eval_tile_samples(const cc_evaluator* e) { return e && e->type != CC_FEATURE_HOG ? e->S : 0; }
int cc_eval_max_cat_count(const cc_evaluator* e) { return e && e->type == CC_FEATURE_LBP ? 256 : 0; }
int cc_eval_feature_size(const cc_evaluator* e) { return e ? (e->type == CC_FEATURE_HOG ? 36 : 1) : 0; }  // N_BINS * N_CELLS
const float* cc_eval_labels(const cc_evaluator* e) { return e ? e->cls.data() : nullptr; }

cc_status cc_eval_feature_geometry(const cc_evaluator* e, int fi, int32_t* rects, float* weights, int* tilted) {
  if (!e || !rects) return set_error(CC_ERR_INVALID_ARG, "cc_eval_feature_geometry: null argument");
  if (e->type == CC_FEATURE_HOG)  // four cells do not fit the 3-rect output: cc_eval_hog_feature_geometry
    return set_error(CC_ERR_INVALID_ARG, "cc_eval_feature_geometry: HOG evaluator, use cc_eval_hog_feature_geometry");
  if (fi < 0 || fi >= e->nfeat) return set_error(CC_ERR_OUT_OF_RANGE, "cc_eval_feature_geometry: feature %d out of range (%d)", fi, e->nfeat);
  if (e->type == CC_FEATURE_HAAR) {
    std::memcpy(rects, e->haar[fi].r, sizeof(int32_t) * 12);
    if (weights) std::memcpy(weights, e->haar[fi].w, sizeof(float) * 3);
    if (tilted) *tilted = e->haar[fi].tilted;
  } else
    std::memcpy(rects, &e->lbp[(size_t)fi * 4], sizeof(int32_t) * 4);
  return CC_OK;
}

cc_status cc_eval_set_images(cc_evaluator* e, const uint8_t* imgs, int n, int first_idx, const uint8_t* labels) {
  if (!e || (!imgs && n > 0)) return set_error(CC_ERR_INVALID_ARG, "cc_eval_set_images: null argument");
  if (n < 0 || first_idx < 0 || first_idx + n > e->max_samples)  // features.cpp:87: idx < cls.rows
    return set_error(CC_ERR_OUT_OF_RANGE, "cc_eval_set_images: samples [%d, %d) exceed max_samples %d", first_idx, first_idx + n, e->max_samples);
  cc_status st = eval_device(e);
  if (st != CC_OK) return st;
  if (n == 0) return CC_OK;
  std::lock_guard<std::mutex> lk(e->mu);
  st = set_images(e, imgs, false, n, first_idx);
  if (st != CC_OK) return st;
  if (labels)
    for (int i = 0; i < n; i++) e->cls[(size_t)first_idx + i] = (float)labels[i];
  return CC_OK;
}

// setImage for ONE window (haarfeatures.cpp:100-114, lbpfeatures.cpp:22-28) -- the call the trainer's negative-mining loop
// makes for every candidate window (cascadeclassifier.cpp:340-347), 10^5..10^6 times per late stage, each followed by a
// few operator() calls for the same sample. A launch per window would cost more than the window's arithmetic
// (round 3: 15.7 k windows/s through two launches per window), so this call does no device work: it queues the pixels
// (a later image for the same sample replaces the queued one; the queue goes to the device, runs of consecutive samples
// per launch, before anything reads stored samples there) and keeps a host mirror of THIS window's integral(s) and norm
// factor, from which cc_eval_calc / cc_eval_calc_list answer for this sample ("scalar, host-mirror fast
// path"). The mirror's values are bit-identical to the device's (tests/test_gpu_eval.py compares every catalog feature).
cc_status cc_eval_set_image(cc_evaluator* e, const uint8_t* img, size_t row_stride, uint8_t cls_label, int idx) {
  if (!e || !img) return set_error(CC_ERR_INVALID_ARG, "cc_eval_set_image: null argument");
  if (row_stride < (size_t)e->W) return set_error(CC_ERR_INVALID_ARG, "cc_eval_set_image: row stride smaller than the window width");
  if (idx < 0 || idx >= e->max_samples) return set_error(CC_ERR_OUT_OF_RANGE, "cc_eval_set_image: idx %d out of range (%d)", idx, e->max_samples);
  const size_t px = (size_t)e->W * e->H;
  constexpr int kMaxQueued = 4096;
  std::lock_guard<std::mutex> lk(e->mu);
  e->generation++;
  if ((int)e->pend_idx.size() >= kMaxQueued && (e->pend_slot.empty() || e->pend_slot[(size_t)idx] < 0)) {
    cc_status st = eval_device(e);
    if (st == CC_OK) st = flush_pending_images(e);
    if (st != CC_OK) return st;
  }
  if (e->pend_slot.empty()) e->pend_slot.assign((size_t)e->max_samples, -1);
  int slot = e->pend_slot[(size_t)idx];
  if (slot < 0) {
    slot = (int)e->pend_idx.size();
    e->pend_idx.push_back(idx);
    e->pend_px.resize((size_t)(slot + 1) * px);
    e->pend_slot[(size_t)idx] = slot;
  }
  uint8_t* dst = e->pend_px.data() + (size_t)slot * px;
  for (int y = 0; y < e->H; y++) std::memcpy(dst + (size_t)y * e->W, img + (size_t)y * row_stride, (size_t)e->W);
  e->mirror_idx = -1;
  if (e->type == CC_FEATURE_HOG)
    hog_host_planes(e, dst, e->mirror_hog);
  else
    host_window_integrals(e, dst, e->mirror_sum, e->mirror_tilted, e->mirror_nf);
  e->mirror_idx = idx;
  e->cls[(size_t)idx] = (float)cls_label;
  return CC_OK;
}

cc_status cc_eval_get_sample(cc_evaluator* e, int idx, int32_t* sum, int32_t* tilted, float* normfactor) {
  if (!e) return set_error(CC_ERR_INVALID_ARG, "cc_eval_get_sample: null evaluator");
  if (idx < 0 || idx >= e->max_samples) return set_error(CC_ERR_OUT_OF_RANGE, "cc_eval_get_sample: idx %d out of range", idx);
  if (e->type == CC_FEATURE_HOG) return set_error(CC_ERR_INVALID_ARG, "cc_eval_get_sample: HOG evaluator, use cc_eval_get_hog_sample");
  cc_status st = eval_device(e);
  if (st != CC_OK) return st;
  std::lock_guard<std::mutex> lk(e->mu);
  st = flush_pending_images(e);  // the device's copy is what this call reports, also for a sample set a moment ago
  if (st != CC_OK) return st;
  if (sum) CC_HIP(copy_sync(sum, e->samples.sum.p + (size_t)idx * e->cols, (size_t)e->cols * 4, hipMemcpyDeviceToHost, e->stream.s));
  if (tilted) {
    if (!e->use_tilted) return set_error(CC_ERR_INVALID_ARG, "cc_eval_get_sample: evaluator keeps no tilted integrals (mode != ALL)");
    CC_HIP(copy_sync(tilted, e->samples.tilted.p + (size_t)idx * e->cols, (size_t)e->cols * 4, hipMemcpyDeviceToHost, e->stream.s));
  }
  if (normfactor) {
    if (e->type != CC_FEATURE_HAAR) return set_error(CC_ERR_INVALID_ARG, "cc_eval_get_sample: LBP evaluator has no norm factor");
    CC_HIP(copy_sync(normfactor, e->samples.nf.p + idx, 4, hipMemcpyDeviceToHost, e->stream.s));
  }
  return CC_OK;
}

}  // extern "C"
