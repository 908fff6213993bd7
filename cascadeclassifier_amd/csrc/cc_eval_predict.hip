// Training-side cascade predict on gfx950: CvCascadeClassifier::predict of a trained cascade on rows of sample tables
// (cc_eval_store.hip), Haar and LBP; HOG cascades go to cc_hog.hip.
#include <hip/hip_runtime.h>

#include <mutex>

#include "cc_train_device.h"

namespace ccamd {

// ------------------------------------------------------------------------------------------------
// Training-side cascade predict: one thread per stored sample walks the stages (walk_stages); LBP stumps are one-node
// trees, Haar stump cascades take k_predict_haar_stumps below.
// ------------------------------------------------------------------------------------------------
struct PredictArgs {
  const int32_t* sum;
  const int32_t* tilted;
  const float* normfactor;
  const int32_t* sample_idx;
  int n_samples, cols;
  WalkTables walk;
  const void* nodes;  // HaarPredictNode / LbpPredictNode per tree node
  uint8_t* out;
};

template <bool HAAR>
__global__ __launch_bounds__(64) void k_predict(PredictArgs A) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= A.n_samples) return;
  const int si = A.sample_idx ? A.sample_idx[s] : s;
  const int32_t* img = A.sum + (size_t)si * A.cols;
  bool pass;
  if (HAAR) {  // ordered split: `<=` goes left
    const int32_t* timg = A.tilted ? A.tilted + (size_t)si * A.cols : img;
    const float nf = A.normfactor[si];
    pass = walk_stages(A.walk, [&](int n) {
      const HaarPredictNode& N = reinterpret_cast<const HaarPredictNode*>(A.nodes)[n];
      const int32_t* b = N.f.tilted ? timg : img;
      return haar_value(haar_sum(N.f, [&](int o) { return b[o]; }), nf) <= N.thr ? N.left : N.right;
    });
  } else {  // categorical split: a code whose bit is set goes left
    pass = walk_stages(A.walk, [&](int n) {
      const LbpPredictNode& N = reinterpret_cast<const LbpPredictNode*>(A.nodes)[n];
      const int code = lbp_code_at(N.f, [&](int o) { return img[o]; });
      return (N.subset[code >> 5] & (1 << (code & 31))) != 0 ? N.left : N.right;
    });
  }
  A.out[s] = pass;
}

// Haar STUMP cascades are not on the shared walk: this is the stump loop and (predict_haar_stumps) the upload from before
// cc_train_device.h, kept as they were. Through walk_stages the same call measured 12.5 % slower, through stump records
// handed to the walk still 2.9 %, cause of the rest not found (profiles/EXPERIMENTS.md 3.18). k is wave-uniform here.
struct StumpPredictArgs {
  const int32_t* sum;
  const int32_t* tilted;
  const float* normfactor;
  const int32_t* sample_idx;
  int n_samples, cols;
  int nstages;
  const int* stage_ntrees;
  const float* stage_thr;  // threshold - CV_THRESHOLD_EPS
  const HaarFeatDev* feats;  // per stump, fastRect offsets
  const float* stump_thr;
  const float* stump_left;
  const float* stump_right;
  uint8_t* out;
};

__global__ __launch_bounds__(64) void k_predict_haar_stumps(StumpPredictArgs A) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= A.n_samples) return;
  const int si = A.sample_idx ? A.sample_idx[s] : s;
  const int32_t* img = A.sum + (size_t)si * A.cols;
  const int32_t* timg = A.tilted ? A.tilted + (size_t)si * A.cols : img;
  const float nf = A.normfactor[si];
  int k = 0;
  uint8_t pass = 1;
  for (int st = 0; st < A.nstages && pass; st++) {
    double acc = 0;
    const int nt = A.stage_ntrees[st];
    for (int i = 0; i < nt; i++, k++) {
      const HaarFeatDev F = A.feats[k];
      const int32_t* b = F.tilted ? timg : img;
      const float val = haar_value(haar_sum(F, [&](int o) { return b[o]; }), nf);
      acc += (double)(val <= A.stump_thr[k] ? A.stump_left[k] : A.stump_right[k]);
    }
    if (acc < (double)A.stage_thr[st]) pass = 0;
  }
  A.out[s] = pass;
}

static const char* feature_type_name(int t) {
  return t == CC_FEATURE_HAAR ? "HAAR" : t == CC_FEATURE_LBP ? "LBP" : t == CC_FEATURE_HOG ? "HOG" : "unknown";
}

// Haar stump cascade m on rows of t as before the shared walk (see k_predict_haar_stumps). Caller holds e->mu.
static cc_status predict_haar_stumps(cc_evaluator* e, const SampleTables& t, const Cascade& m, const int32_t* d_idx, int n_samples, uint8_t* out) {
  const size_t ns = m.stump_feature.size(), nst = m.stage_ntrees.size();
  std::vector<HaarFeatDev> dev(ns);
  for (size_t i = 0; i < ns; i++) haar_feature_to_dev(m, m.stump_feature[i], dev[i]);
  DevBuf<HaarFeatDev> dh;
  DevBuf<int> d_ntrees;
  DevBuf<float> d_sthr, d_thr, d_left, d_right;
  auto put = [&](auto& buf, const auto& v) {  // as before: allocate, then a blocking copy
    const hipError_t err = buf.ensure(v.size());
    return err != hipSuccess ? err : copy_sync(buf.p, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice, e->stream.s);
  };
  CC_HIP(put(dh, dev));
  CC_HIP(put(d_ntrees, m.stage_ntrees));
  CC_HIP(put(d_sthr, m.stage_threshold));
  CC_HIP(put(d_thr, m.stump_threshold));
  CC_HIP(put(d_left, m.stump_left));
  CC_HIP(put(d_right, m.stump_right));
  CC_HIP(e->d_pred.ensure((size_t)n_samples));
  const StumpPredictArgs A{t.sum.p, e->use_tilted ? t.tilted.p : nullptr, t.nf.p, d_idx, n_samples, e->cols, (int)nst,
                           d_ntrees.p, d_sthr.p, dh.p, d_thr.p, d_left.p, d_right.p, e->d_pred.p};
  hipLaunchKernelGGL(k_predict_haar_stumps, dim3((n_samples + 63) / 64), dim3(64), 0, e->stream.s, A);
  CC_HIP(hipGetLastError());
  if (out) CC_HIP(hipMemcpyAsync(out, e->d_pred.p, (size_t)n_samples, hipMemcpyDeviceToHost, e->stream.s));
  CC_HIP(hipStreamSynchronize(e->stream.s));
  return CC_OK;
}

cc_status predict_check(const cc_evaluator* e, const Cascade& m, const char* who) {
  if (m.feature_type != e->type || m.win_w != e->W || m.win_h != e->H)
    return set_error(CC_ERR_INVALID_ARG, "%s: cascade (%s %dx%d) does not match the evaluator (%s %dx%d)", who,
                     feature_type_name(m.feature_type), m.win_w, m.win_h, feature_type_name(e->type), e->W, e->H);
  if (m.has_tilted && !e->use_tilted)
    return set_error(CC_ERR_INVALID_ARG, "%s: cascade has tilted features but the evaluator keeps no tilted integrals", who);
  return CC_OK;
}

cc_status predict_stored(cc_evaluator* e, const SampleTables& t, const Cascade& m, const int32_t* d_idx, int n_samples, uint8_t* out) {
  if (e->type == CC_FEATURE_HOG) return hog_predict(e, t, m, d_idx, n_samples, out);
  if (e->type != CC_FEATURE_HAAR && e->type != CC_FEATURE_LBP)
    return set_error(CC_ERR_UNSUPPORTED, "cc_eval_predict_cascade: feature type %d", e->type);
  const bool haar = e->type == CC_FEATURE_HAAR;
  if (haar && m.max_nodes_per_tree == 1) return predict_haar_stumps(e, t, m, d_idx, n_samples, out);
  // Queued copies read the host vectors and m until the synchronisation below. On an early return the device buffers,
  // declared last, go first, and hipFree waits for the device, so no copy outlives its source.
  const std::vector<HaarPredictNode> haar_nodes = haar ? haar_predict_nodes(m) : std::vector<HaarPredictNode>();
  const std::vector<LbpPredictNode> lbp_nodes = haar ? std::vector<LbpPredictNode>() : lbp_predict_nodes(m);
  WalkTablesDev walk;
  DevBuf<HaarPredictNode> d_haar_nodes;
  DevBuf<LbpPredictNode> d_lbp_nodes;
  CC_HIP(walk.upload(m, e->stream.s));
  CC_HIP(haar ? d_haar_nodes.upload(haar_nodes, e->stream.s) : d_lbp_nodes.upload(lbp_nodes, e->stream.s));
  CC_HIP(e->d_pred.ensure((size_t)n_samples));
  PredictArgs A;
  A.sum = t.sum.p;
  A.tilted = e->use_tilted ? t.tilted.p : nullptr;
  A.normfactor = t.nf.p;
  A.sample_idx = d_idx;
  A.n_samples = n_samples;
  A.cols = e->cols;
  A.walk = walk.tables();
  A.nodes = haar ? (const void*)d_haar_nodes.p : (const void*)d_lbp_nodes.p;
  A.out = e->d_pred.p;
  if (haar)
    hipLaunchKernelGGL(k_predict<true>, dim3((n_samples + 63) / 64), dim3(64), 0, e->stream.s, A);
  else
    hipLaunchKernelGGL(k_predict<false>, dim3((n_samples + 63) / 64), dim3(64), 0, e->stream.s, A);
  CC_HIP(hipGetLastError());
  if (out) CC_HIP(hipMemcpyAsync(out, e->d_pred.p, (size_t)n_samples, hipMemcpyDeviceToHost, e->stream.s));
  CC_HIP(hipStreamSynchronize(e->stream.s));  // the tables above are freed on return
  return CC_OK;
}

}  // namespace ccamd

using namespace ccamd;

extern "C" {

cc_status cc_eval_predict_cascade(cc_evaluator* e, const cc_cascade* c, const int32_t* sample_idx, int n_samples, uint8_t* out) {
  if (!e || !c || !out) return set_error(CC_ERR_INVALID_ARG, "cc_eval_predict_cascade: null argument");
  const Cascade& m = c->m;
  cc_status st = predict_check(e, m, "cc_eval_predict_cascade");
  if (st != CC_OK) return st;
  if (n_samples < 0) return set_error(CC_ERR_INVALID_ARG, "cc_eval_predict_cascade: negative sample count");
  st = eval_device(e);
  if (st != CC_OK) return st;
  if (n_samples == 0) return CC_OK;
  std::lock_guard<std::mutex> lk(e->mu);
  if (cc_status fst = flush_pending_images(e); fst != CC_OK) return fst;  // images set one at a time reach the device first
  const int32_t* d_idx = nullptr;
  st = upload_indices(e, sample_idx, n_samples, &d_idx);
  if (st != CC_OK) return st;
  return predict_stored(e, e->samples, m, d_idx, n_samples, out);
}

}  // extern "C"
