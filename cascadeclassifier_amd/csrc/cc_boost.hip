// One boosted stage of stumps on gfx950 (section 6b of the C ABI). Replaces the loop of CvCascadeBoost::train
// (traincascade/lib/src/boost.cpp:409-459) with update_weights (:160-407) and isErrDesired (:479-518),
// CvBoost::trim_weights (o_cvboost.cpp:101-139) and, for trees of one split, CvBoostTree::calc_node_value
// (o_cvboostree.cpp:657-732), calc_node_dir (:87-149) and CvCascadeBoostTree::predict (o_cvcascadeboosttree.cpp:16-39).
//
// All per-sample state (y, weights, subsample mask, weak_eval, stage sums) stays in HBM for the booster's life; a round
// sends the host a few small records (root sums, the chosen split with the leaves' sums, trimming and stage status).
//
// Every sum the reference forms in a loop is formed here in the same order by ONE lane (block_serial_sums): the other
// wavefronts of the block compute the terms and stage them in LDS a chunk ahead, so the adding lane never waits on HBM,
// and the independent sums of one pass (rcw0 / sum / sum2, the four leaf sums, sumW / err) sit in neighbouring lanes of
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
constexpr int BOOST_MAX_SUMS = 4;

struct BoostLds {
  double term[2][BOOST_MAX_SUMS][BOOST_CHUNK];
};

// out[k] = term(0, k) + term(1, k) + ... + term(n - 1, k), added in that order, for k < K. term(i, .) is called exactly
// once per i (it may write per-sample results) and fills t[0..K). All threads of the block call this.
template <int K, class Term>
__device__ void block_serial_sums(int n, BoostLds& lds, double* out, Term term) {
  static_assert(K <= BOOST_MAX_SUMS, "LDS holds four sums' terms");
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
struct RootRec {
  double s[4];  // regression: rcw0, sum, sum2; classifier: rcw[0], rcw[1]
  int n_active, n_cls0, n_cls1, pad;
};
struct SplitRec {  // the ordered winner (arg-max kernel) and the leaves' sums
  int var;         // index into the presorted range; -1: no split with quality > 0
  float quality;
  int split_point;
  float ord_c;
  double leaf[4];  // regression: L rcw0, L sum, R rcw0, R sum; classifier: L rcw[0], L rcw[1], R rcw[0], R rcw[1]
};
struct TailRec {
  double sums[2];  // Discrete: sumW, err of boost.cpp:295-300
  double trim_threshold;
  int nz, pos_true, n_false, pad;
  float threshold, pad2;
};

// How a trained stump sends a sample: ordered `value <= ord_c`, categorical the subset bit of its code.
struct Stump {
  int categorical;
  float ord_c;
  int subset[8];
  __device__ bool left(float v) const {
    if (!categorical) return v <= ord_c;
    const int c = (int)v;
    return (subset[c >> 5] >> (c & 31)) & 1;
  }
};

// ---- node table and root value ------------------------------------------------------------------------
// The dense per-sample table cc_split.hip's kernels read (upload_node_table's forms and "absent" entries) and the root's
// calc_node_value sums (o_cvboostree.cpp:676-683, :710-718) over the active samples in increasing order.
template <bool CLASSIFIER>
__global__ __launch_bounds__(BOOST_THREADS) void k_boost_root(int n, const double* __restrict__ w, const uint8_t* __restrict__ mask,
                                                              const int8_t* __restrict__ y, int form8, AbsentEntry absent, double* __restrict__ tab,
                                                              RootRec* __restrict__ rec) {
  __shared__ BoostLds lds;
  __shared__ int cnt[3];
  if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
  __syncthreads();
  block_serial_sums<CLASSIFIER ? 2 : 3>(n, lds, rec->s, [&](int i, double* v) {
    const double wi = w[i];
    const bool act = mask[i] != 0, c1 = y[i] > 0;
    const double t = (double)(float)y[i];
    if (form8)
      tab[i] = !act ? absent.e8 : CLASSIFIER ? (c1 ? -wi : wi) : t * wi;
    else {
      tab[2 * i] = act ? wi : absent.e16.w;
      tab[2 * i + 1] = !act ? absent.e16.t : CLASSIFIER ? (c1 ? 1.0 : 0.0) : t * wi;
    }
    if (!act) return;
    atomicAdd(&cnt[0], 1);
    if (CLASSIFIER) {
      v[c1 ? 1 : 0] = wi;
      atomicAdd(&cnt[c1 ? 2 : 1], 1);
    } else {
      v[0] = wi;
      v[1] = t * wi;
      v[2] = t * t * wi;
    }
  });
  __syncthreads();
  if (threadIdx.x == 0) {
    rec->n_active = cnt[0];
    rec->n_cls0 = cnt[1];
    rec->n_cls1 = cnt[2];
  }
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

// ---- apply the split -----------------------------------------------------------------------------------
// Ordered: one pass over the winner's presorted row ([group][rank][64]). Every sample's value goes to val[sample]; an
// active sample's rank in the node's sorted order is the running count of active entries before it (ballot within a
// wavefront, carried across wavefronts and chunks); left iff rank <= split_point (calc_node_dir, o_cvboostree.cpp:130-144).
template <class TI>
__global__ __launch_bounds__(1024) void k_boost_apply_ord(const float* __restrict__ sv, const TI* __restrict__ si, int n,
                                                          const uint8_t* __restrict__ mask, const SplitRec* __restrict__ rec,
                                                          float* __restrict__ val, int8_t* __restrict__ dir) {
  __shared__ int wave_cnt[16];
  __shared__ int carried;
  const int f = rec->var, split_point = rec->split_point;
  if (f < 0) return;
  const size_t base = (size_t)(f >> 6) * n * 64 + (f & 63);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carried = 0;
  __syncthreads();
  for (int r0 = 0; r0 < n; r0 += 1024) {
    const int r = r0 + threadIdx.x;
    unsigned idx = 0;
    float v = 0.f;
    bool act = false, ok = false;
    if (r < n) {
      idx = (unsigned)si[base + (size_t)r * 64];
      v = sv[base + (size_t)r * 64];
      ok = idx < (unsigned)n;  // always, with presort's tables; never write outside the arrays
      act = ok && mask[idx] != 0;
    }
    const unsigned long long b = __ballot(act);
    const int before = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[wave] = __popcll(b);
    __syncthreads();
    int rank = carried + before;
    for (int k = 0; k < wave; k++) rank += wave_cnt[k];
    if (ok) {
      val[idx] = v;
      dir[idx] = act ? (rank <= split_point ? -1 : 1) : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int s = carried;
      for (int k = 0; k < 16; k++) s += wave_cnt[k];
      carried = s;
    }
    __syncthreads();
  }
}

// Categorical: the direction is the subset bit of the sample's code (o_cvboostree.cpp:102-110).
__global__ __launch_bounds__(256) void k_boost_apply_cat(const uint8_t* __restrict__ codes_row, int n, const uint8_t* __restrict__ mask,
                                                         Stump st, float* __restrict__ val, int8_t* __restrict__ dir) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = (float)codes_row[i];
  val[i] = v;
  dir[i] = mask[i] ? (st.left(v) ? -1 : 1) : 0;
}

// ---- leaves: calc_node_value of the two children, each over its samples in increasing order ---------------
template <bool CLASSIFIER>
__global__ __launch_bounds__(BOOST_THREADS) void k_boost_leaves(int n, const double* __restrict__ w, const int8_t* __restrict__ y,
                                                                const int8_t* __restrict__ dir, int check_rec, SplitRec* __restrict__ rec) {
  __shared__ BoostLds lds;
  if (check_rec && rec->var < 0) return;
  block_serial_sums<4>(n, lds, rec->leaf, [&](int i, double* v) {
    const int d = dir[i];
    if (d == 0) return;
    const double wi = w[i];
    const int side = d < 0 ? 0 : 2;
    if (CLASSIFIER)
      v[side + (y[i] > 0 ? 1 : 0)] = wi;
    else {
      v[side] = wi;
      v[side + 1] = (double)(float)y[i] * wi;
    }
  });
}

// ---- update_weights, stage sums ------------------------------------------------------------------------
struct UpdateArgs {
  int n;
  double* w;
  double* weak_eval;
  double* stage_sum;
  const int8_t* y;
  const int8_t* dir;  // -1 left, 1 right, 0: the sample was not in the node
  const float* val;   // the split variable's value, by sample
  Stump st;
  double left_value, right_value;  // node->value of the leaves (Discrete: before tree->scale)
  double scale_c;                  // Discrete: C, and exp(C) in scale1
  double scale1;
  TailRec* tail;
};
// weak_eval of sample i: its leaf's value if it was in the node (o_cvboostree.cpp:74-84), else predict (boost.cpp:270-281)
__device__ inline double weak_response(const UpdateArgs& A, const Stump& st, int i, bool& pred_left) {
  pred_left = st.left(A.val[i]);
  const int d = A.dir[i];
  const bool left = d != 0 ? d < 0 : pred_left;
  return left ? A.left_value : A.right_value;
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
  const Stump& st = A.st;
  block_serial_sums<1>(A.n, lds, sums, [&](int i, double* v) {
    bool pred_left;
    double we = weak_response(A, st, i, pred_left);
    A.stage_sum[i] += pred_left ? A.left_value : A.right_value;
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
  const Stump& st = A.st;
  block_serial_sums<2>(A.n, lds, A.tail->sums, [&](int i, double* v) {
    bool pred_left;
    const double we = weak_response(A, st, i, pred_left);
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
  const Stump& st = A.st;
  block_serial_sums<1>(A.n, lds, sums, [&](int i, double* v) {
    const bool pred_left = st.left(A.val[i]);
    A.stage_sum[i] += (pred_left ? A.left_value : A.right_value) * A.scale_c;
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
                             uint8_t* __restrict__ mask, int8_t* __restrict__ dir, float* __restrict__ val) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  w[i] = w0;
  weak_eval[i] = 0.0;
  stage_sum[i] = 0.0;
  mask[i] = 1;
  dir[i] = 0;
  val[i] = 0.f;
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

struct cc_boost {
  cc_evaluator* e = nullptr;
  int n = 0;
  cc_boost_params p{};
  uint64_t generation = 0;
  bool classifier = false, gini = false, categorical = false;
  int n_pos = 0, n_neg = 0, n_weak = 0;
  bool have_subsample = false;
  float threshold = 0.f, hit_rate = 0.f, false_alarm = 0.f;
  DevBuf<double> w, weak_eval, stage_sum, sort_in, sort_out;
  DevBuf<int8_t> y, dir;
  DevBuf<uint8_t> mask;
  DevBuf<float> val, eval_in, eval_out;
  DevBuf<int> pos_idx;
  DevBuf<char> cub_temp, recs;  // recs: RootRec, SplitRec, TailRec
  size_t cub_w_bytes = 0, cub_f_bytes = 0;
  PinnedBuf pin;
  hipEvent_t ev[12] = {};
  double last_ms[8] = {};  // device time of the last round's parts (cc_boost_last_round_ms)
  RootRec* d_root() { return reinterpret_cast<RootRec*>(recs.p); }
  SplitRec* d_split() { return reinterpret_cast<SplitRec*>(recs.p + 64); }
  TailRec* d_tail() { return reinterpret_cast<TailRec*>(recs.p + 192); }
  ~cc_boost() {
    for (hipEvent_t& x : ev)
      if (x) (void)hipEventDestroy(x);
  }
};
static_assert(sizeof(RootRec) <= 64 && sizeof(SplitRec) <= 128 && sizeof(TailRec) <= 64, "record slots");

static cc_status boost_round_locked(cc_boost* b, cc_weak* out) {
  cc_evaluator* e = b->e;
  const int n = b->n;
  hipStream_t st = e->stream;
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

  // 1. node table and root calc_node_value
  const TableForm form = split_table_form_unit(n);
  CC_HIP(e->d_split_tab.ensure((size_t)n * 2));
  const AbsentEntry absent = b->categorical ? ABSENT_CATEGORICAL : ABSENT_ORDERED;
  (void)hipEventRecord(b->ev[0], st);
  hipLaunchKernelGGL(b->classifier ? k_boost_root<true> : k_boost_root<false>, dim3(1), dim3(BOOST_THREADS), 0, st, n, b->w.p, b->mask.p, b->y.p,
                     form == TABLE_LDS8 ? 1 : 0, absent, e->d_split_tab.p, b->d_root());
  CC_HIP(hipGetLastError());
  (void)hipEventRecord(b->ev[1], st);
  CC_HIP(hipMemcpyAsync(pin, b->d_root(), sizeof(RootRec), hipMemcpyDeviceToHost, st));
  CC_HIP(hipStreamSynchronize(st));
  RootRec root;
  std::memcpy(&root, pin, sizeof(root));
  out->n_active = root.n_active;
  const int na = root.n_active;
  double node_value = 0.0;
  // 2. no tree (o_cvdtree.cpp:130-145)
  if (na <= 10) return not_trained();  // min_sample_count, o_cvdtreeparams.cpp:8
  if (b->classifier) {
    if ((root.n_cls0 != 0) + (root.n_cls1 != 0) == 1) return not_trained();
  } else {
    const double rcw0 = root.s[0], sum = root.s[1], sum2 = root.s[2];
    const double iw = 1. / rcw0;
    node_value = sum * iw;
    double risk = sum2 - (sum * iw) * sum;
    risk *= na * iw * na * iw;
    if (std::sqrt(risk) / na < 0.01f) return not_trained();  // regression_accuracy
  }

  // 3. best split
  Stump stump{};
  stump.categorical = b->categorical ? 1 : 0;
  const int mode = !b->classifier ? 0 : (b->gini ? 1 : 2);
  const int F = e->presort_f1 - e->presort_f0;
  const bool idx16 = n <= 65536;
  if (!b->categorical) {
    const double w0 = root.s[0], w1 = b->classifier ? root.s[1] : 0.0;
    if (cc_status s = split_launch_ordered(e, mode, form, w0, w1, node_value * w0); s != CC_OK) return s;
    const size_t fpad = ((size_t)F + 63) / 64 * 64;
    const OrdResult dev(e->d_split_out.p, fpad);
    (void)hipEventRecord(b->ev[2], st);
    hipLaunchKernelGGL(k_boost_argmax, dim3(1), dim3(1024), 0, st, dev.best_val, dev.best_i, dev.best_vl, dev.best_vr, F, b->d_split());
    (void)hipEventRecord(b->ev[3], st);
    // 4. directions
    if (idx16)
      hipLaunchKernelGGL(k_boost_apply_ord<uint16_t>, dim3(1), dim3(1024), 0, st, e->d_sorted_val.p, e->d_sorted_idx16.p, n, b->mask.p, b->d_split(),
                         b->val.p, b->dir.p);
    else
      hipLaunchKernelGGL(k_boost_apply_ord<int32_t>, dim3(1), dim3(1024), 0, st, e->d_sorted_val.p, e->d_sorted_idx32.p, n, b->mask.p, b->d_split(),
                         b->val.p, b->dir.p);
    CC_HIP(hipGetLastError());
  } else {
    cc_split sp;
    if (cc_status s = split_categorical_from_table(e, b->classifier, b->gini, form, &sp); s != CC_OK) return s;
    if (!sp.found) return not_trained();
    out->var_idx = sp.var_idx;
    out->quality = sp.quality;
    std::memcpy(out->subset, sp.subset, sizeof(sp.subset));
    std::memcpy(stump.subset, sp.subset, sizeof(sp.subset));
    (void)hipEventRecord(b->ev[3], st);
    hipLaunchKernelGGL(k_boost_apply_cat, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, e->d_codes.p + (size_t)(sp.var_idx - e->presort_f0) * n, n,
                       b->mask.p, stump, b->val.p, b->dir.p);
    CC_HIP(hipGetLastError());
  }
  (void)hipEventRecord(b->ev[4], st);
  // 5. leaves
  hipLaunchKernelGGL(b->classifier ? k_boost_leaves<true> : k_boost_leaves<false>, dim3(1), dim3(BOOST_THREADS), 0, st, n, b->w.p, b->y.p, b->dir.p,
                     b->categorical ? 0 : 1, b->d_split());
  CC_HIP(hipGetLastError());
  (void)hipEventRecord(b->ev[5], st);
  CC_HIP(hipMemcpyAsync(pin, b->d_split(), sizeof(SplitRec), hipMemcpyDeviceToHost, st));
  CC_HIP(hipStreamSynchronize(st));
  SplitRec sr;
  std::memcpy(&sr, pin, sizeof(sr));
  {
    float ms = 0;
    if (hipEventElapsedTime(&ms, e->ev_a, e->ev_b) == hipSuccess) e->last_ms = ms;
    b->last_ms[1] = e->last_ms;
  }
  if (!b->categorical) {
    if (sr.var < 0) return not_trained();
    out->var_idx = e->presort_f0 + sr.var;
    out->quality = sr.quality;
    out->ord_c = sr.ord_c;
    out->split_point = sr.split_point;
    stump.ord_c = sr.ord_c;
  }
  double lv, rv;
  if (!b->classifier) {
    lv = sr.leaf[1] * (1. / sr.leaf[0]);
    rv = sr.leaf[3] * (1. / sr.leaf[2]);
  } else if (b->p.boost_type == 0) {
    lv = (sr.leaf[1] > sr.leaf[0]) * 2 - 1;
    rv = (sr.leaf[3] > sr.leaf[2]) * 2 - 1;
  } else {
    lv = 0.5 * log_ratio(sr.leaf[1] / (sr.leaf[0] + sr.leaf[1]));
    rv = 0.5 * log_ratio(sr.leaf[3] / (sr.leaf[2] + sr.leaf[3]));
  }

  // 6. update_weights, 7. stage sums
  UpdateArgs U{};
  U.n = n;
  U.w = b->w.p;
  U.weak_eval = b->weak_eval.p;
  U.stage_sum = b->stage_sum.p;
  U.y = b->y.p;
  U.dir = b->dir.p;
  U.val = b->val.p;
  U.st = stump;
  U.left_value = lv;
  U.right_value = rv;
  U.scale_c = 1.0;
  U.scale1 = 1.0;
  U.tail = b->d_tail();
  (void)hipEventRecord(b->ev[6], st);
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
    lv *= Cc;  // tree->scale(C)
    rv *= Cc;
  }
  (void)hipEventRecord(b->ev[7], st);
  b->n_weak++;
  out->trained = 1;
  out->left_value = lv;
  out->right_value = rv;

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
  (void)hipEventRecord(b->ev[8], st);
  // 9. isErrDesired
  const int threshold_idx = (int)((1.0F - b->p.min_hit_rate) * b->n_pos);
  if (b->n_pos > 0) {
    hipLaunchKernelGGL(k_boost_gather_pos, dim3((unsigned)((b->n_pos + 255) / 256)), dim3(256), 0, st, b->pos_idx.p, b->n_pos, b->stage_sum.p, b->eval_in.p);
    CC_HIP(hipcub::DeviceRadixSort::SortKeys(b->cub_temp.p, b->cub_f_bytes, b->eval_in.p, b->eval_out.p, b->n_pos, 0, 32, st));
    hipLaunchKernelGGL(k_boost_status, dim3(1), dim3(1024), 0, st, b->eval_out.p, b->n_pos, std::min(std::max(threshold_idx, 0), b->n_pos - 1), n, b->y.p,
                       b->stage_sum.p, b->d_tail());
    CC_HIP(hipGetLastError());
  }
  (void)hipEventRecord(b->ev[9], st);
  CC_HIP(hipMemcpyAsync(pin, b->d_tail(), sizeof(TailRec), hipMemcpyDeviceToHost, st));
  CC_HIP(hipStreamSynchronize(st));
  TailRec tr;
  std::memcpy(&tr, pin, sizeof(tr));
  auto span = [&](int a, int c) {
    float ms = 0;
    return hipEventElapsedTime(&ms, b->ev[a], b->ev[c]) == hipSuccess ? (double)ms : 0.0;
  };
  b->last_ms[0] = span(0, 1);
  if (!b->categorical) b->last_ms[2] = span(2, 3);
  b->last_ms[3] = span(3, 4);
  b->last_ms[4] = span(4, 5);
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
  if (!e || !p || !out) return set_error(CC_ERR_INVALID_ARG, "cc_boost_create: null argument");
  *out = nullptr;
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
  hipStream_t st = e->stream;
  CC_HIP(b->w.ensure((size_t)n));
  CC_HIP(b->weak_eval.ensure((size_t)n));
  CC_HIP(b->stage_sum.ensure((size_t)n));
  CC_HIP(b->sort_in.ensure((size_t)n));
  CC_HIP(b->sort_out.ensure((size_t)n));
  CC_HIP(b->y.ensure((size_t)n));
  CC_HIP(b->dir.ensure((size_t)n));
  CC_HIP(b->mask.ensure((size_t)n));
  CC_HIP(b->val.ensure((size_t)n));
  CC_HIP(b->eval_in.ensure((size_t)std::max(1, b->n_pos)));
  CC_HIP(b->eval_out.ensure((size_t)std::max(1, b->n_pos)));
  CC_HIP(b->pos_idx.ensure((size_t)std::max(1, b->n_pos)));
  CC_HIP(b->recs.ensure(256));
  CC_HIP(b->pin.ensure(256));
  CC_HIP(hipMemsetAsync(b->recs.p, 0, 256, st));
  for (hipEvent_t& x : b->ev) CC_HIP(hipEventCreate(&x));
  CC_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, b->cub_w_bytes, static_cast<const unsigned long long*>(nullptr), static_cast<unsigned long long*>(nullptr), n,
                                           0, 64, st));
  CC_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, b->cub_f_bytes, static_cast<const float*>(nullptr), static_cast<float*>(nullptr), std::max(1, b->n_pos), 0,
                                           32, st));
  CC_HIP(b->cub_temp.ensure(std::max<size_t>({b->cub_w_bytes, b->cub_f_bytes, 1})));
  CC_HIP(hipMemcpyAsync(b->y.p, y.data(), (size_t)n, hipMemcpyHostToDevice, st));
  if (b->n_pos > 0) CC_HIP(hipMemcpyAsync(b->pos_idx.p, pos.data(), pos.size() * 4, hipMemcpyHostToDevice, st));
  // boost.cpp:190-265: weights 1./n, every sample active, no renormalisation (sumW is 0 there)
  hipLaunchKernelGGL(k_boost_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, 1. / n, b->w.p, b->weak_eval.p, b->stage_sum.p, b->mask.p,
                     b->dir.p, b->val.p);
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
  hipStream_t st = b->e->stream;
  const size_t n = (size_t)b->n;
  if (weights) CC_HIP(hipMemcpyAsync(weights, b->w.p, n * 8, hipMemcpyDeviceToHost, st));
  if (weak_eval) CC_HIP(hipMemcpyAsync(weak_eval, b->weak_eval.p, n * 8, hipMemcpyDeviceToHost, st));
  if (mask) CC_HIP(hipMemcpyAsync(mask, b->mask.p, n, hipMemcpyDeviceToHost, st));
  if (stage_sum) CC_HIP(hipMemcpyAsync(stage_sum, b->stage_sum.p, n * 8, hipMemcpyDeviceToHost, st));
  CC_HIP(hipStreamSynchronize(st));
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
