// One boosted stage of weak trees on gfx950 (section 6b of the C ABI). Replaces the loop of CvCascadeBoost::train
// (traincascade/lib/src/boost.cpp:409-459) with update_weights (:160-407) and isErrDesired (:479-518),
// CvBoost::trim_weights (o_cvboost.cpp:101-139), CvDTree::try_split_node (o_cvdtree.cpp:122-187), CvBoostTree::calc_node_value
// (o_cvboostree.cpp:657-732), calc_node_dir (:87-149) and CvCascadeBoostTree::predict (o_cvcascadeboosttree.cpp:16-39).
// A stump is the tree of depth 1: one round function grows both.
//
// All per-sample state (y, weights, subsample mask, weak_eval, stage sums, the node a sample stands at) stays in HBM for the
// booster's life; a round sends the host a few small records (root sums, per searched node the chosen split with the
// children's sums, trimming and stage status).
//
// Every sum the reference forms in a loop is formed here in the same order by ONE lane (block_serial_sums): the other
// wavefronts of the block compute the terms and stage them in LDS a chunk ahead, so the adding lane never waits on HBM,
// and the independent sums of one pass (rcw0 / sum / sum2, the two children's sums, sumW / err) sit in neighbouring lanes of
// the same wavefront and cost one sum's time. A term of a sample that does not take part is +0.0, which leaves a sum
// that started at +0.0 unchanged.
#include <hipcub/hipcub.hpp>

#include <cfloat>
#include <cmath>
#include <cstring>
#include <memory>

#include "cc_eval_internal.h"

namespace ccamd {

constexpr int BOOST_CHUNK = 512;                 // samples staged per step of a serial sum
constexpr int BOOST_THREADS = 64 + BOOST_CHUNK;  // wavefront 0 adds, the others stage the next chunk
constexpr int BOOST_MAX_SUMS = 6;

struct BoostLds {
  double term[2][BOOST_MAX_SUMS][BOOST_CHUNK];
};

// out[k] = term(0, k) + term(1, k) + ... + term(n - 1, k), added in that order, for k < K. term(i, .) is called exactly
// once per i (it may write per-sample results) and fills t[0..K). All threads of the block call this.
template <int K, class Term>
__device__ void block_serial_sums(int n, BoostLds& lds, double* out, Term term) {
  static_assert(K <= BOOST_MAX_SUMS, "LDS holds six sums' terms");
  const int t = threadIdx.x;
  auto fill = [&](int c) {
    if (t < 64) return;
    const int j = t - 64, i = c * BOOST_CHUNK + j;
    double v[K];
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = 0.0;
    if (i < n) term(i, v);
#pragma unroll
    for (int k = 0; k < K; k++) lds.term[c & 1][k][j] = v[k];
  };
  const int chunks = (n + BOOST_CHUNK - 1) / BOOST_CHUNK;
  double a = 0.0;
  if (chunks > 0) fill(0);
  __syncthreads();
  for (int c = 0; c < chunks; c++) {
    if (c + 1 < chunks) fill(c + 1);
    if (t < K) {
      const int m = min(BOOST_CHUNK, n - c * BOOST_CHUNK);
      const double* src = lds.term[c & 1][t];
#pragma unroll 8
      for (int j = 0; j < m; j++) a += src[j];
    }
    __syncthreads();
  }
  if (t < K) out[t] = a;
}

// ---- records that cross to the host ----------------------------------------------------------------
struct NodeRec {  // the sums of calc_node_value (o_cvboostree.cpp:676-683, :710-718) over one node's samples in increasing order
  double s[3];    // regression: rcw0, sum, sum2; classifier: rcw[0], rcw[1]
  int n, n_cls0, n_cls1, pad;
};
struct SplitRec {  // the ordered winner (arg-max kernel) and the two children's calc_node_value sums
  int var;         // index into the presorted range; -1: no split with quality > 0
  float quality;
  int split_point;
  float ord_c;
  NodeRec child[2];  // left, right
};
struct TailRec {
  double sums[2];  // Discrete: sumW, err of boost.cpp:295-300
  double trim_threshold;
  int nz, pos_true, n_false, pad;
  float threshold, pad2;
};

// A categorical split: the subset bit of a sample's code sends it left (CV_DTREE_CAT_DIR).
struct Subset {
  int w[8];
  __device__ bool left(int c) const { return (w[c >> 5] >> (c & 31)) & 1; }
};

// ---- a tree on the device -------------------------------------------------------------------------------
// Nodes are numbered as the round creates them: the root is 0, the children of a split are consecutive (left, right).
// Two node numbers per sample say where the tree has sent it so far: node_dir by direction (calc_node_dir; -1 for a
// sample outside the subsample), which is the node whose sums and searches the sample takes part in, and node_pred by
// the predict rule (o_cvcascadeboosttree.cpp:16-39), for every sample. Applying node k's split moves the samples that
// stand at k to its children; a sample's number ends at its leaf. A stump is the tree that stops after the root's split.
// At the root the numbers are implied (every sample of the subsample stands there by direction, every sample by predict),
// so the root's split reads the mask and writes both arrays without reading them: they need no initial pass.

// A sample's terms of calc_node_value: 2 sums for a classifier, 3 for regression. sum2 only feeds the node's risk, which
// only the regression-accuracy rule reads: RISK = false leaves it out (2 sums) for nodes that the depth limit makes leaves.
template <bool CLASSIFIER, bool RISK>
__device__ __forceinline__ void node_terms(double wi, int yi, double* v) {
  if (CLASSIFIER)
    v[yi > 0 ? 1 : 0] = wi;
  else {
    const double t = (double)(float)yi;
    v[0] = wi;
    v[1] = t * wi;
    if (RISK) v[2] = t * t * wi;
  }
}
// A sample's entry of the dense node table cc_split.hip's kernels read (upload_node_table's forms and "absent" entries).
template <bool CLASSIFIER>
__device__ __forceinline__ void table_entry(double* __restrict__ tab, int form8, const AbsentEntry& absent, int i, bool in_node, double wi, int yi) {
  const bool c1 = yi > 0;
  const double t = (double)(float)yi;
  if (form8)
    tab[i] = !in_node ? absent.e8 : CLASSIFIER ? (c1 ? -wi : wi) : t * wi;
  else {
    tab[2 * i] = in_node ? wi : absent.e16.w;
    tab[2 * i + 1] = !in_node ? absent.e16.t : CLASSIFIER ? (c1 ? 1.0 : 0.0) : t * wi;
  }
}

// The root: its table is written and its calc_node_value sums are formed over the active samples in increasing order.
template <bool CLASSIFIER>
__global__ __launch_bounds__(BOOST_THREADS) void k_boost_root(int n, const double* __restrict__ w, const uint8_t* __restrict__ mask,
                                                              const int8_t* __restrict__ y, int form8, AbsentEntry absent, double* __restrict__ tab,
                                                              NodeRec* __restrict__ rec) {
  __shared__ BoostLds lds;
  __shared__ int cnt[2];
  if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
  __syncthreads();
  block_serial_sums<CLASSIFIER ? 2 : 3>(n, lds, rec->s, [&](int i, double* v) {
    const double wi = w[i];
    const bool act = mask[i] != 0;
    const int yi = y[i];
    table_entry<CLASSIFIER>(tab, form8, absent, i, act, wi, yi);
    if (!act) return;
    node_terms<CLASSIFIER, true>(wi, yi, v);
    atomicAdd(&cnt[yi > 0 ? 1 : 0], 1);
  });
  __syncthreads();
  if (threadIdx.x == 0) {
    rec->n = cnt[0] + cnt[1];
    rec->n_cls0 = cnt[0];
    rec->n_cls1 = cnt[1];
  }
}

// The table of node k > 0: the samples direction sent there. Its sums came with its parent's split (k_boost_children).
template <bool CLASSIFIER>
__global__ __launch_bounds__(256) void k_boost_table(int n, const double* __restrict__ w, const int8_t* __restrict__ y, const int* __restrict__ node_dir,
                                                     int k, int form8, AbsentEntry absent, double* __restrict__ tab) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) table_entry<CLASSIFIER>(tab, form8, absent, i, node_dir[i] == k, w[i], y[i]);
}

// ---- winner over the ordered variables ----------------------------------------------------------------------
// pick_winner's rule (o_cvdtree.cpp:320-351): the first variable, in variable order, with the largest (float)quality among
// those that found a split, and only if that is > 0. Arg-max with (value descending, index ascending).
__global__ __launch_bounds__(1024) void k_boost_argmax(const double* __restrict__ best_val, const int* __restrict__ best_i,
                                                       const float* __restrict__ best_vl, const float* __restrict__ best_vr, int F,
                                                       SplitRec* __restrict__ rec) {
  __shared__ float s_q[1024];
  __shared__ int s_f[1024];
  float q = 0.f;  // only qualities > 0 can win
  int f = -1;
  for (int i = threadIdx.x; i < F; i += blockDim.x) {  // increasing i: a later equal value does not replace
    if (best_i[i] < 0) continue;
    const float v = (float)best_val[i];
    if (v > q) {
      q = v;
      f = i;
    }
  }
  s_q[threadIdx.x] = q;
  s_f[threadIdx.x] = f;
  __syncthreads();
  for (int step = 512; step > 0; step >>= 1) {
    if ((int)threadIdx.x < step) {
      const float q2 = s_q[threadIdx.x + step];
      const int f2 = s_f[threadIdx.x + step];
      const float q1 = s_q[threadIdx.x];
      const int f1 = s_f[threadIdx.x];
      if (f2 >= 0 && (f1 < 0 || q2 > q1 || (q2 == q1 && f2 < f1))) {
        s_q[threadIdx.x] = q2;
        s_f[threadIdx.x] = f2;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int win = s_f[0];
    rec->var = win;
    rec->quality = win >= 0 ? s_q[0] : -1.f;
    rec->split_point = win >= 0 ? best_i[win] : -1;
    rec->ord_c = win >= 0 ? (best_vl[win] + best_vr[win]) * 0.5f : 0.f;
  }
}

// ---- apply the split of node k: its samples move to children `left_id` and `left_id + 1` -------------------------
// Ordered: one pass over the winner's presorted row ([group][rank][64]), which meets every sample once. A sample that
// direction holds at k has as its rank in the node's sorted order the running count of such entries before it (ballot
// within a wavefront, carried across wavefronts and chunks): left iff rank <= split_point (calc_node_dir,
// o_cvboostree.cpp:130-144). A sample that predict holds at k goes left iff value <= ord_c.
// After a split presort only the variables below `resident` have a row in the tables; a streamed winner's row is the
// winner row its chunk left behind (k_stream_winner, cc_split.hip): one entry per rank. Which of the two is read is
// decided here, from rec->var.
template <class TI>
__global__ __launch_bounds__(1024) void k_boost_apply_ord(const float* __restrict__ sv, const TI* __restrict__ si, int n, int resident,
                                                          const float* __restrict__ win_val, const TI* __restrict__ win_idx,
                                                          const uint8_t* __restrict__ mask, const SplitRec* __restrict__ rec, int k, int left_id,
                                                          int* __restrict__ node_dir, int* __restrict__ node_pred) {
  __shared__ int wave_cnt[16];
  __shared__ int carried;
  const int f = rec->var, split_point = rec->split_point;
  if (f < 0) return;
  const float ord_c = rec->ord_c;
  const bool streamed = f >= resident;
  const size_t base = streamed ? 0 : (size_t)(f >> 6) * n * 64 + (f & 63), stride = streamed ? 1 : 64;
  if (streamed) {
    sv = win_val;
    si = win_idx;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carried = 0;
  __syncthreads();
  for (int r0 = 0; r0 < n; r0 += 1024) {
    const int r = r0 + threadIdx.x;
    unsigned idx = 0;
    float v = 0.f;
    bool act = false, pred = false, ok = false;
    if (r < n) {
      idx = (unsigned)si[base + (size_t)r * stride];
      v = sv[base + (size_t)r * stride];
      ok = idx < (unsigned)n;  // always, with presort's tables; never touch anything outside the arrays
      if (ok) {
        act = k == 0 ? mask[idx] != 0 : node_dir[idx] == k;
        pred = k == 0 || node_pred[idx] == k;
      }
    }
    const unsigned long long b = __ballot(act);
    const int before = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[wave] = __popcll(b);
    __syncthreads();
    int rank = carried + before;
    for (int j = 0; j < wave; j++) rank += wave_cnt[j];
    if (act)
      node_dir[idx] = left_id + (rank <= split_point ? 0 : 1);
    else if (ok && k == 0)
      node_dir[idx] = -1;
    if (pred) node_pred[idx] = left_id + (v <= ord_c ? 0 : 1);
    __syncthreads();
    if (threadIdx.x == 0) {
      int s = carried;
      for (int j = 0; j < 16; j++) s += wave_cnt[j];
      carried = s;
    }
    __syncthreads();
  }
}

// Categorical: both rules read the subset bit of the sample's code (o_cvboostree.cpp:102-110).
__global__ __launch_bounds__(256) void k_boost_apply_cat(const uint8_t* __restrict__ codes_row, int n, const uint8_t* __restrict__ mask, Subset subset,
                                                         int k, int left_id, int* __restrict__ node_dir, int* __restrict__ node_pred) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int child = left_id + (subset.left(codes_row[i]) ? 0 : 1);
  if (k == 0) {
    node_dir[i] = mask[i] ? child : -1;
    node_pred[i] = child;
    return;
  }
  if (node_dir[i] == k) node_dir[i] = child;
  if (node_pred[i] == k) node_pred[i] = child;
}

// ---- calc_node_value of the two children of a split, each over its samples in increasing order ------------------
template <bool CLASSIFIER, bool RISK>
__global__ __launch_bounds__(BOOST_THREADS) void k_boost_children(int n, const double* __restrict__ w, const int8_t* __restrict__ y,
                                                                  const int* __restrict__ node_dir, int left_id, int check_rec,
                                                                  SplitRec* __restrict__ rec) {
  constexpr int K = CLASSIFIER || !RISK ? 2 : 3;
  __shared__ BoostLds lds;
  __shared__ double sums[2 * K];
  __shared__ int cnt[4];
  if (check_rec && rec->var < 0) return;
  if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
  __syncthreads();
  block_serial_sums<2 * K>(n, lds, sums, [&](int i, double* v) {
    const int side = node_dir[i] - left_id;
    if (side != 0 && side != 1) return;
    const int yi = y[i];
    node_terms<CLASSIFIER, RISK>(w[i], yi, v + side * K);
    atomicAdd(&cnt[side * 2 + (yi > 0 ? 1 : 0)], 1);
  });
  __syncthreads();
  if (threadIdx.x < 2) {
    NodeRec& c = rec->child[threadIdx.x];
    for (int j = 0; j < 3; j++) c.s[j] = j < K ? sums[threadIdx.x * K + j] : 0.0;
    c.n_cls0 = cnt[threadIdx.x * 2];
    c.n_cls1 = cnt[threadIdx.x * 2 + 1];
    c.n = c.n_cls0 + c.n_cls1;
  }
}

// ---- update_weights, stage sums ------------------------------------------------------------------------
struct UpdateArgs {
  int n;
  double* w;
  double* weak_eval;
  double* stage_sum;
  const int8_t* y;
  const int* node_dir;   // the leaf direction sent the sample to; -1: the sample was not in the tree's subsample
  const int* node_pred;  // the leaf predict sends it to
  const double* value;   // node->value by node number (Discrete: before tree->scale)
  double scale_c;        // Discrete: C, and exp(C) in scale1
  double scale1;
  TailRec* tail;
};
// weak_eval of sample i: its leaf's value if it was in the tree's subsample (o_cvboostree.cpp:74-84), else predict (boost.cpp:270-281)
__device__ inline double weak_response(const UpdateArgs& A, int i) {
  const int d = A.node_dir[i];
  return A.value[d >= 0 ? d : A.node_pred[i]];
}
__device__ inline void renormalize(const UpdateArgs& A, const double* sumw_shared) {
  __syncthreads();
  double sumW = *sumw_shared;
  if (sumW > FLT_EPSILON) {  // boost.cpp:401-406
    sumW = 1. / sumW;
    for (int i = threadIdx.x; i < A.n; i += blockDim.x) A.w[i] *= sumW;
  }
}

// Gentle / Real (boost.cpp:318-335, :379-397): weak_eval *= -y; exp; w *= weak_eval; sumW; renormalise; stage sums.
__global__ __launch_bounds__(BOOST_THREADS) void k_boost_update_exp(UpdateArgs A) {
  __shared__ BoostLds lds;
  __shared__ double sums[1];
  block_serial_sums<1>(A.n, lds, sums, [&](int i, double* v) {
    double we = weak_response(A, i);
    A.stage_sum[i] += A.value[A.node_pred[i]];
    we *= (double)(-(int)A.y[i]);
    we = exp(we);
    A.weak_eval[i] = we;
    const double wi = A.w[i] * we;
    A.w[i] = wi;
    v[0] = wi;
  });
  renormalize(A, sums);
}

// Discrete, first loop (boost.cpp:295-300): sumW and err.
__global__ __launch_bounds__(BOOST_THREADS) void k_boost_discrete_err(UpdateArgs A) {
  __shared__ BoostLds lds;
  block_serial_sums<2>(A.n, lds, A.tail->sums, [&](int i, double* v) {
    const double we = weak_response(A, i);
    A.weak_eval[i] = we;
    const double wi = A.w[i];
    v[0] = wi;
    v[1] = wi * (we != (double)A.y[i] ? 1.0 : 0.0);
  });
}
// Discrete, second loop (:307-316): w *= scale[weak_eval != y]; sumW; renormalise; stage sums with the scaled leaves.
__global__ __launch_bounds__(BOOST_THREADS) void k_boost_discrete_update(UpdateArgs A) {
  __shared__ BoostLds lds;
  __shared__ double sums[1];
  block_serial_sums<1>(A.n, lds, sums, [&](int i, double* v) {
    A.stage_sum[i] += A.value[A.node_pred[i]] * A.scale_c;
    const double wi = A.w[i] * (A.weak_eval[i] != (double)A.y[i] ? A.scale1 : 1.);
    A.w[i] = wi;
    v[0] = wi;
  });
  renormalize(A, sums);
}

// ---- trim_weights (o_cvboost.cpp:119-134) over the ascending copy of the weights ------------------------------
__global__ __launch_bounds__(BOOST_THREADS) void k_boost_trim(int n, const double* __restrict__ sorted, const double* __restrict__ w, double rate,
                                                              uint8_t* __restrict__ mask, TailRec* __restrict__ tail) {
  __shared__ double chunk[2][BOOST_CHUNK];
  __shared__ int stop_at;  // the index the walk broke at; n when it ran to the end
  __shared__ int nz;
  const int t = threadIdx.x;
  if (t == 0) stop_at = -1, nz = 0;
  auto fill = [&](int c) {
    if (t < 64) return;
    const int i = c * BOOST_CHUNK + t - 64;
    chunk[c & 1][t - 64] = i < n ? sorted[i] : 0.0;
  };
  const int chunks = (n + BOOST_CHUNK - 1) / BOOST_CHUNK;
  double sum = 1. - rate;
  fill(0);
  __syncthreads();
  for (int c = 0; c < chunks && stop_at < 0; c++) {
    if (c + 1 < chunks) fill(c + 1);
    if (t == 0) {
      const int m = min(BOOST_CHUNK, n - c * BOOST_CHUNK);
      for (int j = 0; j < m; j++) {
        if (sum <= 0) {
          stop_at = c * BOOST_CHUNK + j;
          break;
        }
        sum -= chunk[c & 1][j];
      }
    }
    __syncthreads();
  }
  const int at = stop_at < 0 ? n : stop_at;
  const double threshold = at < n ? sorted[at] : DBL_MAX;
  int mine = 0;
  for (int i = t; i < n; i += blockDim.x) {
    const int f = w[i] >= threshold;
    mask[i] = (uint8_t)f;
    mine += f;
  }
  atomicAdd(&nz, mine);
  __syncthreads();
  if (t == 0) {
    tail->trim_threshold = threshold;
    tail->nz = nz;
  }
}

// ---- isErrDesired (boost.cpp:479-518) ---------------------------------------------------------------------------
__global__ void k_boost_gather_pos(const int* __restrict__ pos_idx, int n_pos, const double* __restrict__ stage_sum, float* __restrict__ eval) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n_pos) eval[j] = (float)stage_sum[pos_idx[j]] + 0.0f;  // + 0: one zero for the sort (-0 == +0 to std::sort)
}
__global__ __launch_bounds__(1024) void k_boost_status(const float* __restrict__ eval, int n_pos, int threshold_idx, int n, const int8_t* __restrict__ y,
                                                       const double* __restrict__ stage_sum, TailRec* __restrict__ tail) {
  __shared__ int ties, n_false;
  if (threadIdx.x == 0) ties = 0, n_false = 0;
  __syncthreads();
  const float threshold = eval[threshold_idx];
  int a = 0, b = 0;
  for (int i = threadIdx.x; i < threshold_idx; i += blockDim.x) a += fabsf(eval[i] - threshold) < FLT_EPSILON;
  const float bound = threshold - 0.00001F;  // CV_THRESHOLD_EPS
  for (int i = threadIdx.x; i < n; i += blockDim.x)
    if (y[i] < 0) b += !(stage_sum[i] < (double)bound);
  atomicAdd(&ties, a);
  atomicAdd(&n_false, b);
  __syncthreads();
  if (threadIdx.x == 0) {
    tail->threshold = threshold;
    tail->pos_true = n_pos - threshold_idx + ties;
    tail->n_false = n_false;
  }
}

__global__ void k_boost_init(int n, double w0, double* __restrict__ w, double* __restrict__ weak_eval, double* __restrict__ stage_sum,
                             uint8_t* __restrict__ mask) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  w[i] = w0;
  weak_eval[i] = 0.0;
  stage_sum[i] = 0.0;
  mask[i] = 1;
}

__global__ void k_debug_exp64(const double* __restrict__ x, int n, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = exp(x[i]);
}

static inline double log_ratio(double val) {  // o_cvboostree.cpp:11-17, boost.cpp:28-36
  const double eps = 1e-5;
  val = std::max(val, eps);
  val = std::min(val, 1. - eps);
  return std::log(val / (1. - val));
}

}  // namespace ccamd

using namespace ccamd;

// A node of the round's tree on the host, at its node number (creation order).
struct TreeNode {
  int left = -1, right = -1;  // node numbers of the children; -1: a leaf
  int depth = 0;
  NodeRec rec{};
  double value = 0.0;  // node->value
  int var_idx = -1, split_point = -1;
  float quality = -1.f, ord_c = 0.f;
  int32_t subset[8] = {};
};

struct cc_boost {
  cc_evaluator* e = nullptr;
  int n = 0, max_depth = 1;
  std::vector<TreeNode> tree;  // of the last trained round (Discrete: values after tree->scale)
  cc_boost_params p{};
  uint64_t generation = 0;
  bool classifier = false, gini = false, categorical = false;
  int n_pos = 0, n_neg = 0, n_weak = 0;
  bool have_subsample = false;
  float threshold = 0.f, hit_rate = 0.f, false_alarm = 0.f;
  DevBuf<double> w, weak_eval, stage_sum, sort_in, sort_out, value;  // value: node->value by node number
  DevBuf<int8_t> y;
  DevBuf<uint8_t> mask;
  DevBuf<float> eval_in, eval_out;
  DevBuf<int> pos_idx, node_dir, node_pred;
  DevBuf<char> cub_temp, recs;  // recs: the root's NodeRec, SplitRec, TailRec
  size_t cub_w_bytes = 0, cub_f_bytes = 0;
  PinnedBuf pin, pin_value;
  OwnEvent ev[10];  // marks between the parts of a round
  double last_ms[8] = {};  // device time of the last round's parts (cc_boost_last_round_ms)
  NodeRec* d_root() { return reinterpret_cast<NodeRec*>(recs.p); }
  SplitRec* d_split() { return reinterpret_cast<SplitRec*>(recs.p + 64); }
  TailRec* d_tail() { return reinterpret_cast<TailRec*>(recs.p + 192); }
  size_t max_nodes() const { return 2 * (size_t)n + 1; }  // every leaf holds a sample: at most 2 n - 1 nodes
};
static_assert(sizeof(NodeRec) <= 64 &&sizeof(SplitRec) <= 128 && sizeof(TailRec) <= 64, "record slots");

static cc_status boost_round_locked(cc_boost* b, cc_weak* out) {
  cc_evaluator* e = b->e;
  const int n = b->n;
  hipStream_t st = e->stream.s;
  if (b->generation != e->generation || e->presort_n != n)
    return set_error(CC_ERR_INVALID_ARG, "cc_boost_round: the evaluator's samples or presorted tables changed after cc_boost_create; create a new booster");
  std::memset(out, 0, sizeof(*out));
  out->var_idx = -1;
  out->split_point = -1;
  out->quality = -1.f;
  out->stage_threshold = b->threshold;
  out->hit_rate = b->hit_rate;
  out->false_alarm = b->false_alarm;
  for (double& x : b->last_ms) x = 0;
  auto not_trained = [&]() {
    out->trained = 0;
    out->stop = 4;
    return CC_OK;
  };
  char* pin = static_cast<char*>(b->pin.p);

  // calc_node_value's result (o_cvboostree.cpp:684-732) from a node's sums
  auto node_value = [&](const NodeRec& r) {
    if (!b->classifier) return r.s[1] * (1. / r.s[0]);
    if (b->p.boost_type == 0) return (double)((r.s[1] > r.s[0]) * 2 - 1);
    return 0.5 * log_ratio(r.s[1] / (r.s[0] + r.s[1]));
  };
  // CvDTree::try_split_node's reasons not to search a node (o_cvdtree.cpp:130-145)
  auto is_leaf = [&](const TreeNode& nd) {
    const NodeRec& r = nd.rec;
    if (r.n <= 10 || nd.depth >= b->max_depth) return true;  // min_sample_count, o_cvdtreeparams.cpp:8
    if (b->classifier) return (r.n_cls0 != 0) + (r.n_cls1 != 0) == 1;
    const double rcw0 = r.s[0], sum = r.s[1], sum2 = r.s[2];
    const double iw = 1. / rcw0;
    double risk = sum2 - (sum * iw) * sum;
    risk *= r.n * iw * r.n * iw;  // o_cvboostree.cpp:724
    return std::sqrt(risk) / r.n < 0.01f;  // regression_accuracy
  };
  auto span = [&](int a, int c) {
    float ms = 0;
    return hipEventElapsedTime(&ms, b->ev[a].e, b->ev[c].e) == hipSuccess ? (double)ms : 0.0;
  };

  // 1. the root: node numbers, node table and calc_node_value
  const TableForm form = split_table_form_unit(n);
  const int form8 = form == TABLE_LDS8 ? 1 : 0;
  CC_HIP(e->d_split_tab.ensure((size_t)n * 2));
  const AbsentEntry absent = b->categorical ? ABSENT_CATEGORICAL : ABSENT_ORDERED;
  (void)hipEventRecord(b->ev[0].e, st);
  hipLaunchKernelGGL(b->classifier ? k_boost_root<true> : k_boost_root<false>, dim3(1), dim3(BOOST_THREADS), 0, st, n, b->w.p, b->mask.p, b->y.p, form8,
                     absent, e->d_split_tab.p, b->d_root());
  CC_HIP(hipGetLastError());
  (void)hipEventRecord(b->ev[1].e, st);
  CC_HIP(hipMemcpyAsync(pin, b->d_root(), sizeof(NodeRec), hipMemcpyDeviceToHost, st));
  CC_HIP(hipStreamSynchronize(st));
  std::vector<TreeNode> tree(1);
  std::memcpy(&tree[0].rec, pin, sizeof(NodeRec));
  out->n_active = tree[0].rec.n;
  tree[0].value = node_value(tree[0].rec);
  b->last_ms[0] = span(0, 1);
  // 2. no tree (boost.cpp:436-440)
  if (is_leaf(tree[0])) return not_trained();

  // 3. - 5. CvDTree::try_split_node for every node that is not a leaf; siblings are independent, left first as the reference
  const int mode = !b->classifier ? 0 : (b->gini ? 1 : 2);
  const int F = e->presort_f1 - e->presort_f0;
  std::vector<int> todo(1, 0);
  while (!todo.empty()) {
    const int k = todo.back();
    todo.pop_back();
    if (k != 0) {
      if (is_leaf(tree[(size_t)k])) continue;
      (void)hipEventRecord(b->ev[0].e, st);
      hipLaunchKernelGGL(b->classifier ? k_boost_table<true> : k_boost_table<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, b->w.p, b->y.p,
                         b->node_dir.p, k, form8, absent, e->d_split_tab.p);
      CC_HIP(hipGetLastError());
      (void)hipEventRecord(b->ev[1].e, st);
    }
    const int left_id = (int)tree.size();
    if ((size_t)left_id + 2 > b->max_nodes()) return set_error(CC_ERR_HIP, "cc_boost_round: the tree outgrew its %d samples", n);
    // 3. best split of node k
    if (!b->categorical) {
      const NodeRec& r = tree[(size_t)k].rec;
      const double w0 = r.s[0], w1 = b->classifier ? r.s[1] : 0.0;
      // after a split presort: the head, then the streamed chunks, the leader so far and its sorted row kept on the device
      if (cc_status s = split_launch_ordered(e, mode, form, w0, w1, tree[(size_t)k].value * w0, true); s != CC_OK) return s;
      const size_t fpad = ((size_t)F + 63) / 64 * 64;
      const OrdResult dev(e->d_split_out.p, fpad);
      (void)hipEventRecord(b->ev[2].e, st);
      hipLaunchKernelGGL(k_boost_argmax, dim3(1), dim3(1024), 0, st, dev.best_val, dev.best_i, dev.best_vl, dev.best_vr, F, b->d_split());
      (void)hipEventRecord(b->ev[3].e, st);
      // 4. directions and the predict rule
      with_index_type(wide_index((size_t)n), [&](auto ti) {
        using TI = decltype(ti);
        hipLaunchKernelGGL(k_boost_apply_ord<TI>, dim3(1), dim3(1024), 0, st, e->head.val.p, static_cast<const TI*>(e->head.idx()), n, e->presort_resident,
                           e->d_win_val.p, reinterpret_cast<const TI*>(e->d_win_idx.p), b->mask.p, b->d_split(), k, left_id, b->node_dir.p, b->node_pred.p);
      });
      CC_HIP(hipGetLastError());
    } else {
      cc_split sp;
      if (cc_status s = split_categorical_from_table(e, b->classifier, b->gini, form, &sp); s != CC_OK) return s;
      if (k != 0) b->last_ms[0] += span(0, 1);
      if (!sp.found) {  // find_best_split returned NULL
        if (k == 0) return not_trained();
        b->last_ms[1] += e->last_ms;
        continue;
      }
      TreeNode& nd = tree[(size_t)k];
      nd.var_idx = sp.var_idx;
      nd.quality = sp.quality;
      std::memcpy(nd.subset, sp.subset, sizeof(sp.subset));
      Subset subset;
      std::memcpy(subset.w, sp.subset, sizeof(sp.subset));
      (void)hipEventRecord(b->ev[3].e, st);
      hipLaunchKernelGGL(k_boost_apply_cat, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, e->d_codes.p + (size_t)(sp.var_idx - e->presort_f0) * n, n,
                         b->mask.p, subset, k, left_id, b->node_dir.p, b->node_pred.p);
      CC_HIP(hipGetLastError());
    }
    (void)hipEventRecord(b->ev[4].e, st);
    // 5. calc_node_value of the children
    // children at the depth limit are leaves whatever their risk
    const bool risk = !b->classifier && tree[(size_t)k].depth + 1 < b->max_depth;
    hipLaunchKernelGGL((b->classifier ? k_boost_children<true, false> : risk ? k_boost_children<false, true> : k_boost_children<false, false>), dim3(1),
                       dim3(BOOST_THREADS), 0, st, n, b->w.p, b->y.p, b->node_dir.p, left_id, b->categorical ? 0 : 1, b->d_split());
    CC_HIP(hipGetLastError());
    (void)hipEventRecord(b->ev[5].e, st);
    CC_HIP(hipMemcpyAsync(pin, b->d_split(), sizeof(SplitRec), hipMemcpyDeviceToHost, st));
    CC_HIP(hipStreamSynchronize(st));
    SplitRec sr;
    std::memcpy(&sr, pin, sizeof(sr));
    // the categorical search has noted its own time; the ordered one, head and streamed chunks, is read here
    b->last_ms[1] += b->categorical ? e->last_ms : split_search_ms(e);
    if (!b->categorical) {
      if (k != 0) b->last_ms[0] += span(0, 1);
      b->last_ms[2] += span(2, 3);
    }
    b->last_ms[3] += span(3, 4);
    b->last_ms[4] += span(4, 5);
    if (!b->categorical) {
      if (sr.var < 0) {  // find_best_split returned NULL
        if (k == 0) return not_trained();
        continue;
      }
      TreeNode& nd = tree[(size_t)k];
      nd.var_idx = e->presort_f0 + sr.var;
      nd.quality = sr.quality;
      nd.ord_c = sr.ord_c;
      nd.split_point = sr.split_point;
    }
    tree[(size_t)k].left = left_id;
    tree[(size_t)k].right = left_id + 1;
    for (int side = 0; side < 2; side++) {
      TreeNode c;
      c.depth = tree[(size_t)k].depth + 1;
      c.rec = sr.child[side];
      c.value = node_value(c.rec);
      tree.push_back(c);
    }
    todo.push_back(left_id + 1);
    todo.push_back(left_id);
  }
  const TreeNode& root = tree[0];
  out->var_idx = root.var_idx;
  out->quality = root.quality;
  out->ord_c = root.ord_c;
  out->split_point = root.split_point;
  std::memcpy(out->subset, root.subset, sizeof(root.subset));

  // 6. update_weights, 7. stage sums: a sample's leaf value through its node number
  double* values = static_cast<double*>(b->pin_value.p);
  for (size_t k = 0; k < tree.size(); k++) values[k] = tree[k].value;
  CC_HIP(hipMemcpyAsync(b->value.p, values, tree.size() * 8, hipMemcpyHostToDevice, st));
  UpdateArgs U{};
  U.n = n;
  U.w = b->w.p;
  U.weak_eval = b->weak_eval.p;
  U.stage_sum = b->stage_sum.p;
  U.y = b->y.p;
  U.node_dir = b->node_dir.p;
  U.node_pred = b->node_pred.p;
  U.value = b->value.p;
  U.scale_c = 1.0;
  U.scale1 = 1.0;
  U.tail = b->d_tail();
  (void)hipEventRecord(b->ev[6].e, st);
  if (b->p.boost_type != 0) {
    hipLaunchKernelGGL(k_boost_update_exp, dim3(1), dim3(BOOST_THREADS), 0, st, U);
    CC_HIP(hipGetLastError());
  } else {
    hipLaunchKernelGGL(k_boost_discrete_err, dim3(1), dim3(BOOST_THREADS), 0, st, U);
    CC_HIP(hipGetLastError());
    CC_HIP(hipMemcpyAsync(pin, b->d_tail(), sizeof(TailRec), hipMemcpyDeviceToHost, st));
    CC_HIP(hipStreamSynchronize(st));
    TailRec tr;
    std::memcpy(&tr, pin, sizeof(tr));
    double sumW = tr.sums[0], err = tr.sums[1];
    if (sumW != 0) err /= sumW;
    const double Cc = err = -log_ratio(err);
    U.scale_c = Cc;
    U.scale1 = std::exp(err);
    hipLaunchKernelGGL(k_boost_discrete_update, dim3(1), dim3(BOOST_THREADS), 0, st, U);
    CC_HIP(hipGetLastError());
    for (TreeNode& nd : tree) nd.value *= Cc;  // tree->scale(C)
  }
  (void)hipEventRecord(b->ev[7].e, st);
  b->n_weak++;
  out->trained = 1;
  out->left_value = tree[(size_t)root.left].value;
  out->right_value = tree[(size_t)root.right].value;
  b->tree = std::move(tree);

  // 8. trim_weights
  const bool trimming = b->p.weight_trim_rate > 0. && b->p.weight_trim_rate < 1.;
  if (trimming) {
    CC_HIP(hipMemcpyAsync(b->sort_in.p, b->w.p, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
    // non-negative doubles: the bit pattern orders them
    CC_HIP(hipcub::DeviceRadixSort::SortKeys(b->cub_temp.p, b->cub_w_bytes, reinterpret_cast<const unsigned long long*>(b->sort_in.p),
                                             reinterpret_cast<unsigned long long*>(b->sort_out.p), n, 0, 64, st));
    hipLaunchKernelGGL(k_boost_trim, dim3(1), dim3(BOOST_THREADS), 0, st, n, b->sort_out.p, b->w.p, b->p.weight_trim_rate, b->mask.p, b->d_tail());
    CC_HIP(hipGetLastError());
  }
  (void)hipEventRecord(b->ev[8].e, st);
  // 9. isErrDesired
  const int threshold_idx = (int)((1.0F - b->p.min_hit_rate) * b->n_pos);
  if (b->n_pos > 0) {
    hipLaunchKernelGGL(k_boost_gather_pos, dim3((unsigned)((b->n_pos + 255) / 256)), dim3(256), 0, st, b->pos_idx.p, b->n_pos, b->stage_sum.p, b->eval_in.p);
    CC_HIP(hipcub::DeviceRadixSort::SortKeys(b->cub_temp.p, b->cub_f_bytes, b->eval_in.p, b->eval_out.p, b->n_pos, 0, 32, st));
    hipLaunchKernelGGL(k_boost_status, dim3(1), dim3(1024), 0, st, b->eval_out.p, b->n_pos, std::min(std::max(threshold_idx, 0), b->n_pos - 1), n, b->y.p,
                       b->stage_sum.p, b->d_tail());
    CC_HIP(hipGetLastError());
  }
  (void)hipEventRecord(b->ev[9].e, st);
  CC_HIP(hipMemcpyAsync(pin, b->d_tail(), sizeof(TailRec), hipMemcpyDeviceToHost, st));
  CC_HIP(hipStreamSynchronize(st));
  TailRec tr;
  std::memcpy(&tr, pin, sizeof(tr));
  b->last_ms[5] = span(6, 7);
  b->last_ms[6] = span(7, 8);
  b->last_ms[7] = span(8, 9);
  const int nz = trimming ? tr.nz : n;
  if (trimming) b->have_subsample = nz < n;
  if (nz == 0) {  // boost.cpp:444
    out->stop = 3;
    return CC_OK;
  }
  if (b->n_pos > 0) {
    b->threshold = tr.threshold;
    b->hit_rate = ((float)tr.pos_true) / ((float)b->n_pos);
    b->false_alarm = ((float)tr.n_false) / ((float)b->n_neg);
  }
  out->stage_threshold = b->threshold;
  out->hit_rate = b->hit_rate;
  out->false_alarm = b->false_alarm;
  out->stop = b->false_alarm <= b->p.max_false_alarm ? 1 : (b->n_weak >= b->p.max_weak_count ? 2 : 0);
  return CC_OK;
}

extern "C" {

cc_status cc_boost_create(cc_evaluator* e, int n_samples, const cc_boost_params* p, cc_boost** out) {
  return cc_boost_create_depth(e, n_samples, p, 1, out);
}

cc_status cc_boost_create_depth(cc_evaluator* e, int n_samples, const cc_boost_params* p, int max_depth, cc_boost** out) {
  if (!p || !out) return set_error(CC_ERR_INVALID_ARG, "cc_boost_create: null argument");
  *out = nullptr;
  if (!e)  // no evaluator exists without a device: say which of the two is missing
    return cc_device_count() > 0 ? set_error(CC_ERR_INVALID_ARG, "cc_boost_create: null evaluator")
                                 : set_error(CC_ERR_NO_DEVICE, "cc_boost_create: no usable HIP device; this library has no CPU fallback");
  if (max_depth < 1) return set_error(CC_ERR_INVALID_ARG, "cc_boost_create: max_depth %d", max_depth);
  if (p->boost_type == 2)
    return set_error(CC_ERR_UNSUPPORTED, "cc_boost_create: LOGIT boost is not supported (its responses change every round)");
  if (p->boost_type != 0 && p->boost_type != 1 && p->boost_type != 3)
    return set_error(CC_ERR_INVALID_ARG, "cc_boost_create: unknown boost type %d", p->boost_type);
  if (!(p->min_hit_rate > 0 && p->min_hit_rate < 1 && p->max_false_alarm > 0 && p->max_false_alarm < 1))  // boost.cpp:534-541
    return set_error(CC_ERR_INVALID_ARG, "cc_boost_create: min_hit_rate and max_false_alarm must lie in (0, 1)");
  if (p->max_weak_count < 1) return set_error(CC_ERR_INVALID_ARG, "cc_boost_create: max_weak_count %d", p->max_weak_count);
  if (e->presort_n <= 0 || e->presort_n != n_samples)
    return set_error(CC_ERR_INVALID_ARG, "cc_boost_create: call cc_eval_presort over exactly n_samples = %d first (presorted: %d)", n_samples, e->presort_n);
  if (cc_status st = eval_device(e); st != CC_OK) return st;
  std::lock_guard<std::mutex> lk(e->mu);
  const int n = n_samples;
  std::unique_ptr<cc_boost> b(new cc_boost());
  b->e = e;
  b->n = n;
  b->max_depth = std::min(max_depth, 25);  // o_cvdtreetraindata.cpp:105
  b->p = *p;
  b->generation = e->generation;
  b->classifier = p->boost_type == 0 || p->boost_type == 1;
  int criteria = p->split_criteria;
  if (criteria != 1 && criteria != 3) criteria = p->boost_type == 0 ? 3 : 1;  // o_cvboostree.cpp:188-190
  b->gini = criteria == 1;
  b->categorical = e->type == CC_FEATURE_LBP;
  if (b->categorical && e->cat_sorted_n != n)
    return set_error(CC_ERR_UNSUPPORTED, "cc_boost_create: the categorical search needs the (code, sample)-sorted table of cc_eval_presort");
  std::vector<int8_t> y((size_t)n);
  std::vector<int> pos;
  for (int i = 0; i < n; i++) {
    const float c = e->cls[(size_t)i];
    if (c == 1.0f)
      pos.push_back(i);
    else if (c != 0.0f)
      return set_error(CC_ERR_INVALID_ARG, "cc_boost_create: label %g of sample %d is neither 0 nor 1", (double)c, i);
    y[(size_t)i] = c == 1.0f ? 1 : -1;
  }
  b->n_pos = (int)pos.size();
  b->n_neg = n - b->n_pos;
  hipStream_t st = e->stream.s;
  CC_HIP(b->w.ensure((size_t)n));
  CC_HIP(b->weak_eval.ensure((size_t)n));
  CC_HIP(b->stage_sum.ensure((size_t)n));
  CC_HIP(b->sort_in.ensure((size_t)n));
  CC_HIP(b->sort_out.ensure((size_t)n));
  CC_HIP(b->y.ensure((size_t)n));
  CC_HIP(b->node_dir.ensure((size_t)n));
  CC_HIP(b->node_pred.ensure((size_t)n));
  CC_HIP(b->mask.ensure((size_t)n));
  CC_HIP(b->value.ensure(b->max_nodes()));
  CC_HIP(b->pin_value.ensure(b->max_nodes() * 8));
  CC_HIP(b->eval_in.ensure((size_t)std::max(1, b->n_pos)));
  CC_HIP(b->eval_out.ensure((size_t)std::max(1, b->n_pos)));
  CC_HIP(b->pos_idx.ensure((size_t)std::max(1, b->n_pos)));
  CC_HIP(b->recs.ensure(256));
  CC_HIP(b->pin.ensure(256));
  CC_HIP(hipMemsetAsync(b->recs.p, 0, 256, st));
  for (OwnEvent& x : b->ev) CC_HIP(x.create());
  CC_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, b->cub_w_bytes, static_cast<const unsigned long long*>(nullptr), static_cast<unsigned long long*>(nullptr), n,
                                           0, 64, st));
  CC_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, b->cub_f_bytes, static_cast<const float*>(nullptr), static_cast<float*>(nullptr), std::max(1, b->n_pos), 0,
                                           32, st));
  CC_HIP(b->cub_temp.ensure(std::max<size_t>({b->cub_w_bytes, b->cub_f_bytes, 1})));
  CC_HIP(hipMemcpyAsync(b->y.p, y.data(), (size_t)n, hipMemcpyHostToDevice, st));
  if (b->n_pos > 0) CC_HIP(hipMemcpyAsync(b->pos_idx.p, pos.data(), pos.size() * 4, hipMemcpyHostToDevice, st));
  // boost.cpp:190-265: weights 1./n, every sample active, no renormalisation (sumW is 0 there)
  hipLaunchKernelGGL(k_boost_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, 1. / n, b->w.p, b->weak_eval.p, b->stage_sum.p, b->mask.p);
  CC_HIP(hipGetLastError());
  CC_HIP(hipStreamSynchronize(st));  // y and pos are pageable and about to go out of scope
  *out = b.release();
  return CC_OK;
}

void cc_boost_destroy(cc_boost* b) { delete b; }

cc_status cc_boost_round(cc_boost* b, cc_weak* out) {
  if (!b || !out) return set_error(CC_ERR_INVALID_ARG, "cc_boost_round: null argument");
  if (cc_status st = eval_device(b->e); st != CC_OK) return st;
  std::lock_guard<std::mutex> lk(b->e->mu);
  return boost_round_locked(b, out);
}

cc_status cc_boost_train_stage(cc_boost* b, cc_weak* out, int cap, int* n_weak) {
  if (!b || !out || !n_weak || cap < 1) return set_error(CC_ERR_INVALID_ARG, "cc_boost_train_stage: bad argument");
  *n_weak = 0;
  for (int k = 0; k < cap; k++) {
    if (cc_status st = cc_boost_round(b, &out[k]); st != CC_OK) return st;
    *n_weak = k + 1;
    if (out[k].stop != 0) break;
  }
  return CC_OK;
}

cc_status cc_boost_get_state(cc_boost* b, double* weights, double* weak_eval, uint8_t* mask, double* stage_sum) {
  if (!b) return set_error(CC_ERR_INVALID_ARG, "cc_boost_get_state: null booster");
  if (cc_status st = eval_device(b->e); st != CC_OK) return st;
  std::lock_guard<std::mutex> lk(b->e->mu);
  hipStream_t st = b->e->stream.s;
  const size_t n = (size_t)b->n;
  if (weights) CC_HIP(hipMemcpyAsync(weights, b->w.p, n * 8, hipMemcpyDeviceToHost, st));
  if (weak_eval) CC_HIP(hipMemcpyAsync(weak_eval, b->weak_eval.p, n * 8, hipMemcpyDeviceToHost, st));
  if (mask) CC_HIP(hipMemcpyAsync(mask, b->mask.p, n, hipMemcpyDeviceToHost, st));
  if (stage_sum) CC_HIP(hipMemcpyAsync(stage_sum, b->stage_sum.p, n * 8, hipMemcpyDeviceToHost, st));
  CC_HIP(hipStreamSynchronize(st));
  return CC_OK;
}

cc_status cc_boost_last_tree(cc_boost* b, cc_tree_node* nodes, int node_cap, double* leaves, int leaf_cap, int* n_nodes) {
  if (!b || !n_nodes) return set_error(CC_ERR_INVALID_ARG, "cc_boost_last_tree: null argument");
  std::lock_guard<std::mutex> lk(b->e->mu);
  const std::vector<TreeNode>& tree = b->tree;
  if (tree.empty()) return set_error(CC_ERR_INVALID_ARG, "cc_boost_last_tree: no round has trained a tree yet");
  // CvCascadeBoostTree::write (o_cvcascadeboosttree.cpp:41-93): internal nodes breadth-first from the root; a child that
  // splits gets the next internal number when its parent is written, a leaf the next leaf number
  std::vector<int> queue(1, 0);
  for (size_t q = 0; q < queue.size(); q++)
    for (int c : {tree[(size_t)queue[q]].left, tree[(size_t)queue[q]].right})
      if (tree[(size_t)c].left >= 0) queue.push_back(c);
  *n_nodes = (int)queue.size();
  if (node_cap < *n_nodes || leaf_cap < *n_nodes + 1 || !nodes || !leaves)
    return set_error(CC_ERR_BUFFER_TOO_SMALL, "cc_boost_last_tree: the tree has %d nodes and %d leaves", *n_nodes, *n_nodes + 1);
  int next_node = 1, next_leaf = 0;
  for (size_t q = 0; q < queue.size(); q++) {
    const TreeNode& nd = tree[(size_t)queue[q]];
    cc_tree_node& o = nodes[q];
    auto ref = [&](int c) {
      if (tree[(size_t)c].left >= 0) return next_node++;
      leaves[next_leaf] = tree[(size_t)c].value;
      return -(next_leaf++);
    };
    o.left = ref(nd.left);
    o.right = ref(nd.right);
    o.depth = nd.depth;
    o.n_samples = nd.rec.n;
    o.var_idx = nd.var_idx;
    o.split_point = nd.split_point;
    o.quality = nd.quality;
    o.ord_c = nd.ord_c;
    std::memcpy(o.subset, nd.subset, sizeof(o.subset));
    o.value = nd.value;
  }
  return CC_OK;
}

cc_status cc_boost_last_round_ms(cc_boost* b, double* ms, int cap, int* n_parts) {
  if (!b || !ms || !n_parts) return set_error(CC_ERR_INVALID_ARG, "cc_boost_last_round_ms: null argument");
  *n_parts = 8;
  for (int i = 0; i < 8 && i < cap; i++) ms[i] = b->last_ms[i];
  return CC_OK;
}

cc_status cc_debug_exp64(int device, const double* x, int n, double* out) {
  if (n < 0 || (n > 0 && (!x || !out))) return set_error(CC_ERR_INVALID_ARG, "cc_debug_exp64: bad argument");
  if (n == 0) return CC_OK;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return set_error(CC_ERR_NO_DEVICE, "cc_debug_exp64: no HIP device");
  if (device < 0 || device >= count) return set_error(CC_ERR_OUT_OF_RANGE, "cc_debug_exp64: device %d out of range (%d)", device, count);
  CC_HIP(hipSetDevice(device));
  OwnStream s;
  CC_HIP(s.create());
  DevBuf<double> d_in, d_out;
  CC_HIP(d_in.ensure((size_t)n));
  CC_HIP(d_out.ensure((size_t)n));
  CC_HIP(copy_sync(d_in.p, x, (size_t)n * 8, hipMemcpyHostToDevice, s.s));
  hipLaunchKernelGGL(k_debug_exp64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s.s, d_in.p, n, d_out.p);
  CC_HIP(hipGetLastError());
  CC_HIP(copy_sync(out, d_out.p, (size_t)n * 8, hipMemcpyDeviceToHost, s.s));
  return CC_OK;
}

}  // extern "C"
