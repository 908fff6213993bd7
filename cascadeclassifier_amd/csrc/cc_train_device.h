// Training-side code shared by cc_eval_calc.hip (bulk operator()), cc_eval_predict.hip (predict), cc_eval_store.hip (host
// mirror), cc_negmine.hip (negative mining) and cc_hog.hip (HOG predict): the trainer's feature arithmetic and the walk over
// the stages of a trained cascade, each written once, and the host code that lays their tables out. Bit-exact against the
// reference: every translation unit that includes this is built with -ffp-contract=off. Not part of cc_eval_common.h, whose
// text goes to hiprtc and into the specialiser's cache key.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "cc_eval_internal.h"

namespace ccamd {

#include "cc_eval_common.h"  // wave_sum_f64

// ------------------------------------------------------------------------------------------------
// Feature values. `at` maps an offset stored in the record to the integral entry there: the call sites read the
// XOR-swizzled LDS tile, a row in global memory or a host vector.
// ------------------------------------------------------------------------------------------------
// CvLBPEvaluator::Feature::calc (lbpfeatures.h:70-83): the 3x3-cell code from the 4x4 lattice of corner values.
__host__ __device__ __forceinline__ int lbp_code(const int (&p)[16]) {
  const int c = p[5] - p[6] - p[9] + p[10];
  return (p[0] - p[1] - p[4] + p[5] >= c ? 128 : 0) | (p[1] - p[2] - p[5] + p[6] >= c ? 64 : 0) |
         (p[2] - p[3] - p[6] + p[7] >= c ? 32 : 0) | (p[6] - p[7] - p[10] + p[11] >= c ? 16 : 0) |
         (p[10] - p[11] - p[14] + p[15] >= c ? 8 : 0) | (p[9] - p[10] - p[13] + p[14] >= c ? 4 : 0) |
         (p[8] - p[9] - p[12] + p[13] >= c ? 2 : 0) | (p[4] - p[5] - p[8] + p[9] >= c ? 1 : 0);
}
// The code of feature F through a reader. The two batch kernels fill p[] themselves: with their LDS reader handed one
// level further down the compiler schedules k_eval_batch<false> differently (28 instead of 31 VGPRs, other read order).
template <class At>
__host__ __device__ __forceinline__ int lbp_code_at(const LbpFeatDev& F, At at) {
  int p[16];
#pragma unroll
  for (int j = 0; j < 16; j++) p[j] = at(F.p[j]);
  return lbp_code(p);
}
// CvHaarEvaluator::Feature::calc (haarfeatures.h:114-122): the third rectangle only where it has a weight.
template <class At>
__host__ __device__ __forceinline__ float haar_sum(const HaarFeatDev& F, At at) {
  float ret = F.w[0] * (float)(at(F.p[0][0]) - at(F.p[0][1]) - at(F.p[0][2]) + at(F.p[0][3])) +
              F.w[1] * (float)(at(F.p[1][0]) - at(F.p[1][1]) - at(F.p[1][2]) + at(F.p[1][3]));
  if (F.w[2] != 0.0f) ret += F.w[2] * (float)(at(F.p[2][0]) - at(F.p[2][1]) - at(F.p[2][2]) + at(F.p[2][3]));
  return ret;
}
// operator() (haarfeatures.h:108-112). The batch kernels divide by their hoisted div_by_refined instead (cc_eval_calc.hip).
__host__ __device__ __forceinline__ float haar_value(float ret, float nf) { return nf == 0.0f ? 0.0f : ret / nf; }

// ------------------------------------------------------------------------------------------------
// CvCascadeClassifier::predict (boost.cpp:461-477, o_cvcascadeboosttree.cpp:16-39) over the tables of a Cascade: stage st
// holds trees [stage_first[st], + stage_ntrees[st]); tree t has its root at node tree_root[t] and its leaves from
// leaves[tree_leaf0[t]] on; stage_thr already has CV_THRESHOLD_EPS subtracted. A stump is a tree of one node.
// `child(n)` is node n's decision: > 0 the index of a node inside the tree, <= 0 leaf -child.
// ------------------------------------------------------------------------------------------------
struct WalkTables {
  int nstages;
  const int* stage_first;
  const int* stage_ntrees;
  const float* stage_thr;
  const int* tree_root;
  const int* tree_leaf0;
  const float* leaves;
};

// One lane walks stage after stage, tree after tree: the stage sum is a double over float leaves in tree order.
template <class Child>
__device__ __forceinline__ bool walk_stages(const WalkTables& T, Child child) {
  for (int st = 0; st < T.nstages; st++) {
    double acc = 0;
    const int first = T.stage_first[st], nt = T.stage_ntrees[st];
    for (int t = first; t < first + nt; t++) {
      const int root = T.tree_root[t];
      int idx = 0;
      do idx = child(root + idx);
      while (idx > 0);
      acc += (double)T.leaves[T.tree_leaf0[t] - idx];
    }
    if (acc < (double)T.stage_thr[st]) return false;
  }
  return true;
}

// One wavefront walks a STUMP cascade: lane l takes stumps l, l + 64, ... of a stage and the votes meet in a DPP wave sum.
// The sum's order differs from the trainer's, so the host picks this form only where stage_sums_order_independent
// holds. Wave-uniform result.
template <class Child>
__device__ __forceinline__ bool walk_stages_wave(const WalkTables& T, int lane, Child child) {
  for (int st = 0; st < T.nstages; st++) {
    const int first = T.stage_first[st], nt = T.stage_ntrees[st];
    double part = 0;
    for (int t = first + lane; t < first + nt; t += 64) part += (double)T.leaves[T.tree_leaf0[t] - child(T.tree_root[t])];
    if (wave_sum_f64(part) < (double)T.stage_thr[st]) return false;
  }
  return true;
}

// The walk tables of a cascade on the device; the node records, which differ from kernel to kernel, go beside them.
struct WalkTablesDev {
  DevBuf<int> stage_first, stage_ntrees, tree_root, tree_leaf0;
  DevBuf<float> stage_thr, leaves;
  int nstages = 0;
  // Only queues the copies: `m` has to outlive a synchronisation of `st`, and so has this object.
  hipError_t upload(const Cascade& m, hipStream_t st) {
    nstages = (int)m.stage_ntrees.size();
    for (hipError_t e : {stage_first.upload(m.stage_first, st), stage_ntrees.upload(m.stage_ntrees, st), stage_thr.upload(m.stage_threshold, st),
                         tree_root.upload(m.tree_first_node, st), tree_leaf0.upload(m.tree_first_leaf, st), leaves.upload(m.leaves, st)})
      if (e != hipSuccess) return e;
    return hipSuccess;
  }
  WalkTables tables() const { return {nstages, stage_first.p, stage_ntrees.p, stage_thr.p, tree_root.p, tree_leaf0.p, leaves.p}; }
};

// ------------------------------------------------------------------------------------------------
// Feature records from geometry (host)
// ------------------------------------------------------------------------------------------------
// Byte offset of integral entry p in the batch kernel's swizzled LDS tile (see k_eval_batch), plus a base in bytes.
inline int batch_entry(int p, int S, int base_bytes) { return (p * S + (p & (std::min(S, 32) - 1))) * 4 + base_bytes; }

// batch_S > 0: offsets for k_eval_batch (swizzled tile of batch_S samples; a tilted feature reads the tilted tile
// `tilted_base` bytes behind the sum tile); batch_S == 0: plain entry offsets (fastRect, row stride `step`).
inline void haar_to_dev(const HaarFeature& f, int step, HaarFeatDev& d, int batch_S = 0, int tilted_base = 0) {
  std::memset(&d, 0, sizeof(d));
  d.tilted = f.tilted;
  for (int j = 0; j < 3; j++) d.w[j] = f.w[j];
  for (int j = 0; j < 3; j++) {
    if (f.w[j] == 0.0f) break;  // offsets stay 0 from the first zero weight on (haarfeatures.cpp:292-308)
    const int x = f.r[j][0], y = f.r[j][1], w = f.r[j][2], h = f.r[j][3];
    if (!f.tilted) {  // CV_SUM_OFFSETS, traincascade_features.h:40-50
      d.p[j][0] = x + step * y;
      d.p[j][1] = x + w + step * y;
      d.p[j][2] = x + step * (y + h);
      d.p[j][3] = x + w + step * (y + h);
    } else {  // CV_TILTED_OFFSETS, traincascade_features.h:54-63
      d.p[j][0] = x + step * y;
      d.p[j][1] = x - h + step * (y + h);
      d.p[j][2] = x + w + step * (y + w);
      d.p[j][3] = x + w - h + step * (y + w + h);
    }
    if (batch_S > 0)
      for (int k = 0; k < 4; k++) d.p[j][k] = batch_entry(d.p[j][k], batch_S, f.tilted ? tilted_base : 0);
  }
  if (batch_S > 0)  // unused rectangles read entry 0 of their tile (value times weight 0 upstream; never added here)
    for (int j = 0; j < 3; j++)
      if (f.w[j] == 0.0f)
        for (int k = 0; k < 4; k++) d.p[j][k] = batch_entry(0, batch_S, f.tilted ? tilted_base : 0);
}

inline void lbp_to_dev(const int32_t* r, int step, LbpFeatDev& d, int batch_S = 0) {  // lbpfeatures.cpp:53-63
  for (int rr = 0; rr < 4; rr++)
    for (int cc = 0; cc < 4; cc++) {
      const int p = (r[0] + cc * r[2]) + step * (r[1] + rr * r[3]);
      d.p[4 * rr + cc] = batch_S > 0 ? batch_entry(p, batch_S, 0) : p;
    }
}

// A whole catalog (haar_catalog / lbp_catalog, cc_host.cpp) of a W-wide window; batch_S and tilted_base as above.
inline std::vector<HaarFeatDev> haar_catalog_dev(const std::vector<HaarFeature>& cat, int W, int batch_S = 0, int tilted_base = 0) {
  std::vector<HaarFeatDev> dev(cat.size());
  for (size_t i = 0; i < dev.size(); i++) haar_to_dev(cat[i], W + 1, dev[i], batch_S, tilted_base);
  return dev;
}
inline std::vector<LbpFeatDev> lbp_catalog_dev(const std::vector<int32_t>& rects, int W, int batch_S = 0) {
  std::vector<LbpFeatDev> dev(rects.size() / 4);
  for (size_t i = 0; i < dev.size(); i++) lbp_to_dev(&rects[i * 4], W + 1, dev[i], batch_S);
  return dev;
}

// Tree nodes of k_predict: the feature with plain offsets into a stored sample's row, and the node's decision.
struct HaarPredictNode {
  HaarFeatDev f;
  float thr;
  int left, right;  // child > 0: node index inside the tree; child <= 0: leaf index -child
  int pad;
};
struct LbpPredictNode {
  LbpFeatDev f;
  int left, right;
  int subset[8];
  int pad[2];
};
inline void haar_feature_to_dev(const Cascade& m, int fi, HaarFeatDev& d) {  // feature fi with plain offsets
  HaarFeature f;
  std::memcpy(f.r, &m.haar_rects[(size_t)fi * 12], sizeof(f.r));
  std::memcpy(f.w, &m.haar_weights[(size_t)fi * 3], sizeof(f.w));
  f.tilted = m.haar_tilted[fi];
  haar_to_dev(f, m.win_w + 1, d);
}
inline std::vector<HaarPredictNode> haar_predict_nodes(const Cascade& m) {
  std::vector<HaarPredictNode> nodes(m.node_feature.size());
  for (size_t i = 0; i < nodes.size(); i++) {
    haar_feature_to_dev(m, m.node_feature[i], nodes[i].f);
    nodes[i].thr = m.node_threshold[i];
    nodes[i].left = m.node_left[i];
    nodes[i].right = m.node_right[i];
    nodes[i].pad = 0;
  }
  return nodes;
}
inline std::vector<LbpPredictNode> lbp_predict_nodes(const Cascade& m) {
  std::vector<LbpPredictNode> nodes(m.node_feature.size());
  for (size_t i = 0; i < nodes.size(); i++) {
    std::memset(&nodes[i], 0, sizeof(nodes[i]));
    lbp_to_dev(&m.lbp_rects[(size_t)m.node_feature[i] * 4], m.win_w + 1, nodes[i].f);
    nodes[i].left = m.node_left[i];
    nodes[i].right = m.node_right[i];
    for (int j = 0; j < 8; j++) nodes[i].subset[j] = m.node_subset[i * 8 + j];
  }
  return nodes;
}

}  // namespace ccamd
