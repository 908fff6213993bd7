// Best-split search of a boosted-tree node on gfx950 (section 6 of the C ABI).
// Replaces CvDTree::find_best_split (traincascade/lib/src/o_cvdtree.cpp:313-357) with the per-variable searches of
// CvBoostTree (o_cvboostree.cpp:151-516) over the variable data of CvCascadeBoostTrainData
// (o_cvcascadeboosttraindata.cpp:403-482).
//
// MI355X-first shape: the reference keeps a budgeted slice of sorted indices in host memory and re-evaluates + re-sorts
// every other variable for every node; here the sorted order of EVERY variable stays resident in HBM for the whole
// stage (6 B per (variable, sample): 19.5 GB for 162 336 x 20 000), and one node search is a single streaming pass.
// Where the tables of all variables do not fit, cc_eval_presort_split keeps a head of them resident and does for the rest
// what the reference does beyond its caches (get_ord_var_data's uncached branch, o_cvcascadeboosttraindata.cpp:437-458):
// evaluate, sort and search them again at every node, chunk by chunk through the same kernels.
//
// The tables, their layout in HBM ([group][rank][64 lanes]: SortedTable) and their memory are cc_presort.hip's; the kernels
// and the searches over them are here.
//
// The running sums of the reference are sequential double additions in sorted order; they are reproduced bit for bit by
// giving each variable to one thread. Parallelism comes from the 10^5 variables, not from the scan.
#include <algorithm>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <thread>

#include "cc_eval_internal.h"

namespace ccamd {

// ------------------------------------------------------------------------------------------------
// Ordered variables: one thread per variable walks its sorted samples.
//   MODE 0: find_split_ord_reg   (o_cvboostree.cpp:361-426)
//   MODE 1: find_split_ord_class, GINI      (o_cvboostree.cpp:192-221)
//   MODE 2: find_split_ord_class, MISCLASS  (o_cvboostree.cpp:222-238)
// The reference tests the boundary between sorted positions i and i+1 after adding sample i; here the test happens when
// the NEXT node member arrives (samples outside the node are skipped), which is the same sequence of operations.
// ------------------------------------------------------------------------------------------------
struct SplitOrdArgs {
  const float* sv;
  const void* si;
  const SplitEntry* tab;
  int n_pre;       // samples per variable in the tables
  int n_vars;
  double w_total0, w_total1;  // weights[n], weights[n + 1]
  double rsum0;               // node_value * weights[n]
  double* best_val;
  int* best_i;
  float* best_vl;
  float* best_vr;
  int n_groups;
  int dbg_nogather;  // timing experiment (CCAMD_DEBUG_SPLIT_NOGATHER): every lane reads table entry `lane`
};

// TAB selects where the per-sample table lives: 0 = global memory (16-B entries; any size), 1 = LDS, 16-B entries,
// 2 = LDS, 8-B entries (regression with responses +-1: entry = response * w, w = |entry|; classification: entry = w with
// the class in the sign bit; NaN = not in the node). A wavefront's 64 lanes gather 64 unrelated entries per rank, which
// costs ~64 L2 requests from global memory but a few LDS cycles from a block-resident copy.
#ifndef CC_SPLIT_UNROLL
#define CC_SPLIT_UNROLL 16  // ranks whose loads are in flight per thread before the sequential part consumes them
#endif
template <int MODE, class TI, int TAB>
__global__ __launch_bounds__(1024) void k_split_ord(SplitOrdArgs A) {
  extern __shared__ double l_tab[];
  const int lane = threadIdx.x & 63;
  const int group = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (TAB != 0) {
    const int words = A.n_pre * (TAB == 1 ? 2 : 1);
    const double* src = reinterpret_cast<const double*>(A.tab);
    for (int i = threadIdx.x; i < words; i += blockDim.x) l_tab[i] = src[i];
    __syncthreads();
  }
  if (group >= A.n_groups) return;
  const int f = group * 64 + lane;
  const size_t base = (size_t)group * A.n_pre * 64 + lane;
  const float* sv = A.sv + base;
  const TI* si = reinterpret_cast<const TI*>(A.si) + base;
  const float epsilon = FLT_EPSILON * 2;
  double L = 0, R, lsum = 0, rsum = 0, lcw0 = 0, lcw1 = 0, rcw0 = A.w_total0, rcw1 = A.w_total1;
  if (MODE == 0) {
    R = A.w_total0;
    rsum = A.rsum0;
  } else {
    R = rcw0 + rcw1;
    rsum = rcw0 * rcw0 + rcw1 * rcw1;  // rsum2; lsum plays lsum2
  }
  double best_val = -1.0;
  int best_i = -1, count = 0;
  float prev = 0.f, vl = 0.f, vr = 0.f;
  constexpr int U = CC_SPLIT_UNROLL;
  for (int r0 = 0; r0 < A.n_pre; r0 += U) {
    float v[U];
    SplitEntry e[U];
    unsigned s[U];
#pragma unroll
    for (int k = 0; k < U; k++) {
      const bool in = r0 + k < A.n_pre;
      v[k] = in ? sv[(size_t)(r0 + k) * 64] : 0.f;
      s[k] = in ? (unsigned)si[(size_t)(r0 + k) * 64] : 0u;
    }
#pragma unroll
    for (int k = 0; k < U; k++) {
      const unsigned g = A.dbg_nogather ? (unsigned)lane : s[k];
      if (TAB == 0)
        e[k] = A.tab[g];
      else if (TAB == 1)
        e[k] = reinterpret_cast<const SplitEntry*>(l_tab)[g];
      else {
        const double x = l_tab[g];
        e[k].w = fabs(x);  // NaN stays NaN: fails the membership test below
        e[k].t = MODE == 0 ? x : (__double_as_longlong(x) < 0 ? 1.0 : 0.0);
      }
      if (r0 + k >= A.n_pre) e[k].w = -1.0;
    }
#pragma unroll
    for (int k = 0; k < U; k++) {
      const double w = e[k].w;
      if (!(w >= 0.0)) continue;
      if (count > 0 && prev + epsilon < v[k]) {
        double val;
        bool candidate = true;
        if (MODE == 2) {
          const double a = lcw0 + rcw1, b = lcw1 + rcw0;
          val = a > b ? a : b;
        } else {
          const double num = MODE == 0 ? lsum * lsum * R + rsum * rsum * L : lsum * R + rsum * L;
          const double den = L * R;
          // The quotient can only matter if it exceeds best_val. num < best_val * den * (1 - 2^-50) (two roundings,
          // each within 2^-53) implies num / den < best_val exactly, hence fl(num / den) <= best_val: the division
          // is skipped without changing any result. Anything else (incl. den <= 0, NaN) takes the division.
          candidate = !(den > 0.0 && num < best_val * den * (1.0 - 0x1p-50));
          val = candidate ? num / den : 0.0;
        }
        if (candidate && best_val < val) {
          best_val = val;
          best_i = count - 1;
          vl = prev;
          vr = v[k];
        }
      }
      if (MODE == 0) {
        const double t = e[k].t;
        L += w;
        R -= w;
        lsum += t;
        rsum -= t;
      } else {
        const bool c1 = e[k].t != 0.0;
        if (MODE == 1) {
          const double w2 = w * w;
          L += w;
          R -= w;
          const double lv = c1 ? lcw1 : lcw0, rv = c1 ? rcw1 : rcw0;
          lsum += 2 * lv * w + w2;
          rsum -= 2 * rv * w - w2;
          if (c1) {
            lcw1 = lv + w;
            rcw1 = rv - w;
          } else {
            lcw0 = lv + w;
            rcw0 = rv - w;
          }
        } else {
          if (c1) {
            lcw1 += w;
            rcw1 -= w;
          } else {
            lcw0 += w;
            rcw0 -= w;
          }
        }
      }
      prev = v[k];
      count++;
    }
  }
  if (f < A.n_vars) {
    A.best_val[f] = best_val;
    A.best_i[f] = best_i;
    A.best_vl[f] = vl;
    A.best_vr[f] = vr;
  }
}

// ------------------------------------------------------------------------------------------------
// The same search, re-shaped in round 4 for the case the LDS table of 8-byte entries covers (TAB 2 above: +-1 responses or
// class labels, <= 20 480 samples -- every node of a cascade stage): straight-line code with ONE rare branch per rank.
// Counters of k_split_ord at configs[4] (profiles/r04_training_kernels.txt): the block-per-CU launch gives a SIMD 2.5
// wavefronts, each of which walks 20 000 ranks through four divergent branches per rank (membership, value change,
// candidate, record) -- 6 s_cbranch per rank, 45 vector instructions, one issued every ~6.5 cycles: neither memory (34 %
// of HBM) nor the LDS (10 % busy) limits it, the branch bubbles and the instruction count of a lone wavefront do.
// Here
//  * a sample outside the node adds +0.0 to every running sum (exact: the sums start at +0 / are only ever decreased by
//    +0) and is kept out of `count`, `prev` and the value-change test by its mask bit: no membership branch;
//  * the quality's numerator / denominator and the "cannot beat the record" test are computed for every rank; only a
//    lane that may set a record enters the one branch, which holds the division and the record update;
//  * the record's threshold best * (1 - 2^-50) is kept beside the record instead of being recomputed per rank (one
//    multiplication less; the test stays a sufficient condition: num < fl(bt * den), bt = fl(best (1 - 2^-50)), den > 0,
//    best > 0 imply num / den < best, hence fl(num / den) <= best);
//  * the loads of the next 16 ranks are issued before the current 16 are consumed.
// Operation order of every sum and of the quality expression is the reference's (o_cvboostree.cpp:361-426, :192-238).
// ------------------------------------------------------------------------------------------------
constexpr int SPLIT_LEAN_WAVES = 12;  // wavefronts per block at most: 3 per SIMD, i.e. 168 VGPRs for the two chunks of table reads in flight
template <int MODE, class TI>
__global__ __launch_bounds__(64 * SPLIT_LEAN_WAVES) void k_split_ord_lean(SplitOrdArgs A) {
  extern __shared__ double l_tab[];
  const int lane = threadIdx.x & 63;
  const int group = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  {
    const double* src = reinterpret_cast<const double*>(A.tab);
    for (int i = threadIdx.x; i < A.n_pre; i += blockDim.x) l_tab[i] = src[i];
    __syncthreads();
  }
  if (group >= A.n_groups) return;
  const int f = group * 64 + lane;
  const size_t base = (size_t)group * A.n_pre * 64 + lane;
  const float* sv = A.sv + base;
  const TI* si = reinterpret_cast<const TI*>(A.si) + base;
  const float epsilon = FLT_EPSILON * 2;
  constexpr unsigned NOT_IN_NODE_HI = 0x7ff80000u;  // high word of the quiet NaN the host writes for samples outside the node (low word 0)
  double L = 0, R, lsum = 0, rsum = 0, lcw0 = 0, lcw1 = 0, rcw0 = A.w_total0, rcw1 = A.w_total1;
  if (MODE == 0) {
    R = A.w_total0;
    rsum = A.rsum0;
  } else {
    R = rcw0 + rcw1;
    rsum = rcw0 * rcw0 + rcw1 * rcw1;  // rsum2; lsum plays lsum2
  }
  double best_val = -1.0;
  double bt = -HUGE_VAL;  // best_val * (1 - 2^-50) once best_val > 0; -inf before: every value change is a candidate
  int best_i = -1, count = 0;
  float prev = 0.f, vl = 0.f, vr = 0.f;
  constexpr int U = CC_SPLIT_UNROLL;
  static_assert(3 * U <= SPLIT_TABLE_PAD_RANKS, "table padding covers the read-ahead");
  float va[U], vb[U];
  unsigned sa[U], sb[U];
  auto load = [&](int r0, float (&vv)[U], unsigned (&ss)[U]) {  // no bounds checks: see SPLIT_TABLE_PAD_RANKS
#pragma unroll
    for (int k = 0; k < U; k++) {
      vv[k] = sv[(size_t)(r0 + k) * 64];
      ss[k] = (unsigned)si[(size_t)(r0 + k) * 64];
    }
  };
  // A chunk is consumed in blocks of B ranks: the running sums, the quality's numerator / denominator and the "cannot beat
  // the record" test of the B ranks are straight-line code (the B evaluations are independent chains the scheduler can
  // interleave -- a branch per rank, as in k_split_ord, serialises them: the 4-deep dependent double chain plus the branch
  // of one rank then sits in front of the next rank's), and ONE branch per block asks whether any lane has a candidate
  // in any of the B ranks. Inside it the candidates are taken in rank order against the up-to-date record, exactly as the
  // sequential loop does. The test in the straight-line part uses the record as of the block's start: an older (smaller)
  // record only makes the test more conservative (more candidates), never wrong.
  constexpr int B = 4;
  static_assert(U % B == 0, "chunks are whole blocks");
  auto process = [&](int r0, const float (&vv)[U], const unsigned (&ss)[U]) {
    double x[U];
#pragma unroll
    for (int k = 0; k < U; k++) {
      unsigned g = A.dbg_nogather ? (unsigned)lane : ss[k];
      g = g < (unsigned)A.n_pre ? g : 0u;  // ranks behind the last group's end carry padding
      x[k] = l_tab[g];
    }
#pragma unroll
    for (int k0 = 0; k0 < U; k0 += B) {
      double num[B], den[B];  // MODE 2: num = the quality itself
      bool cand[B];
      int cnt[B];
      float pv[B];
#pragma unroll
      for (int j = 0; j < B; j++) {
        const int k = k0 + j;
        const unsigned long long xb = (unsigned long long)__double_as_longlong(x[k]);
        const unsigned lo = (unsigned)xb, hi = (unsigned)(xb >> 32);
        const bool member = (hi != NOT_IN_NODE_HI) & (r0 + k < A.n_pre);
        const unsigned thi = member ? hi : 0u;  // outside the node: +0.0 (the marker's low word is 0)
        const unsigned tlo = member ? lo : 0u;  // (read-ahead ranks may carry any entry)
        const double w = __hiloint2double((int)(thi & 0x7fffffffu), (int)tlo);
        const float val_k = vv[k];
        const bool changed = member & (count > 0) & (prev + epsilon < val_k);
        cnt[j] = count;
        pv[j] = prev;
        if (MODE == 2) {
          const double a = lcw0 + rcw1, b = lcw1 + rcw0;
          num[j] = a > b ? a : b;
          den[j] = 1.0;
          cand[j] = changed & (best_val < num[j]);
        } else {
          num[j] = MODE == 0 ? lsum * lsum * R + rsum * rsum * L : lsum * R + rsum * L;
          den[j] = L * R;
          // anything but "den > 0 and provably below the record" takes the division (incl. den <= 0, NaN), as k_split_ord does
          cand[j] = changed & !((den[j] > 0.0) & (num[j] < bt * den[j]));
        }
        if (MODE == 0) {
          const double t = __hiloint2double((int)thi, (int)tlo);  // response * w, sign included
          L += w;
          R -= w;
          lsum += t;
          rsum -= t;
        } else {
          const bool c1 = (int)thi < 0;  // class 1 carries the sign bit
          if (MODE == 1) {
            const double w2 = w * w;
            L += w;
            R -= w;
            const double lv = c1 ? lcw1 : lcw0, rv = c1 ? rcw1 : rcw0;
            lsum += 2 * lv * w + w2;
            rsum -= 2 * rv * w - w2;
            const double nl = lv + w, nr = rv - w;
            lcw1 = c1 ? nl : lcw1;
            rcw1 = c1 ? nr : rcw1;
            lcw0 = c1 ? lcw0 : nl;
            rcw0 = c1 ? rcw0 : nr;
          } else {
            const double w1 = c1 ? w : 0.0, w0 = c1 ? 0.0 : w;
            lcw1 += w1;
            rcw1 -= w1;
            lcw0 += w0;
            rcw0 -= w0;
          }
        }
        prev = member ? val_k : prev;
        count += member ? 1 : 0;
      }
      bool any = cand[0];
#pragma unroll
      for (int j = 1; j < B; j++) any |= cand[j];
      if (__builtin_expect(any, 0)) {
#pragma unroll
        for (int j = 0; j < B; j++) {
          if (cand[j]) {
            const double val = MODE == 2 ? num[j] : num[j] / den[j];
            if (best_val < val) {
              best_val = val;
              if (MODE != 2) bt = val > 0.0 ? val * (1.0 - 0x1p-50) : -HUGE_VAL;
              best_i = cnt[j] - 1;
              vl = pv[j];
              vr = vv[k0 + j];
            }
          }
        }
      }
    }
  };
  load(0, va, sa);
  for (int r0 = 0; r0 < A.n_pre; r0 += 2 * U) {  // two chunks per trip: the next chunk's table reads fly while one is consumed
    load(r0 + U, vb, sb);
    process(r0, va, sa);
    load(r0 + 2 * U, va, sa);
    process(r0 + U, vb, sb);
  }
  if (f < A.n_vars) {
    A.best_val[f] = best_val;
    A.best_i[f] = best_i;
    A.best_vl[f] = vl;
    A.best_vr[f] = vr;
  }
}

// ------------------------------------------------------------------------------------------------
// Categorical variables (LBP, 256 categories): one block per variable, one thread per category; the node's samples are
// streamed through LDS in node order and every thread adds the samples of its own category, i.e. each category's sums
// are accumulated in the reference's order (o_cvboostree.cpp:456-464 regression, :283-288 classification).
// hist[var][category] = {sum of response*w, sum of w} or {w of class 0, w of class 1}.
// ------------------------------------------------------------------------------------------------
template <bool CLASSIFIER>
__global__ __launch_bounds__(256) void k_split_cat(const uint8_t* __restrict__ codes, int n_pre, const int32_t* __restrict__ node_idx,
                                                   const SplitEntry* __restrict__ node_tab, int n, double* __restrict__ hist) {
  __shared__ int l_code[256];
  __shared__ double l_w[256], l_t[256];
  const int f = blockIdx.x, cat = threadIdx.x;
  double a0 = 0, a1 = 0;
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + threadIdx.x;
    int code = -1;
    double w = 0, t = 0;
    if (i < n) {
      const int g = node_idx ? node_idx[i] : i;
      code = codes[(size_t)f * n_pre + g];
      const SplitEntry e = node_tab[i];
      w = e.w;
      t = e.t;
    }
    l_code[threadIdx.x] = code;
    l_w[threadIdx.x] = w;
    l_t[threadIdx.x] = t;
    __syncthreads();
    const int m = min(256, n - i0);
    for (int j = 0; j < m; j++) {
      if (l_code[j] == cat) {
        if (CLASSIFIER) {
          if (l_t[j] != 0.0)
            a1 += l_w[j];
          else
            a0 += l_w[j];
        } else {
          a0 += l_t[j];
          a1 += l_w[j];
        }
      }
    }
    __syncthreads();
  }
  hist[((size_t)f * 256 + cat) * 2] = a0;
  hist[((size_t)f * 256 + cat) * 2 + 1] = a1;
}

// ------------------------------------------------------------------------------------------------
// Categorical variables, round 4: the same per-category sums from a table sorted once per stage.
// cc_eval_presort sorts every LBP variable's samples by (code, sample) -- the stable row sort the ordered variables use --
// and stores (sample << 8 | code) as [group][rank][64]. A category's samples are then one contiguous run in increasing
// sample order, so ONE thread per variable (lane = variable: coalesced 256-B reads per rank, as k_split_ord) adds each
// category up in the reference's order (o_cvboostree.cpp:456-464, :283-288) PROVIDED the node lists its samples in increasing
// order, which is what a trainer's nodes do (the root is 0..n-1 or the kept samples in order, children are stable
// partitions of their parent); any other node order takes k_split_cat above. Samples outside the node add +0.0 (exact:
// the sums start at +0 and x + 0.0 == x). Work per node: n_pre table entries per variable instead of n * 256 compares.
// ------------------------------------------------------------------------------------------------
struct SplitCatArgs {
  const uint32_t* packed;
  const SplitEntry* tab;
  int n_pre, n_vars, n_groups;
  int waves;     // wavefronts of a block that own a (group, part) (the others only help to copy the table)
  int parts;     // a variable's ranks are cut into this many parts ...
  int part_len;  // ... of this many ranks (a multiple of SPLIT_CAT_DEPTH * SPLIT_CAT_UNROLL)
  double* hist;
};
// Table layout: [group][rank / 4][64 lanes][4 ranks] -- a lane reads four consecutive ranks of its variable with one 16-byte
// load, a wavefront 1 KB per load instruction. Per-sample table: a sample outside the node is stored as +0.0 (8-byte form:
// response * w, or w with the class in the sign bit) or {0, 0} (16-byte form), so it takes no test at all.
// Parts: 8 464 LBP variables are 133 groups -- one wavefront on every eighth SIMD. A variable's ranks can be cut into parts,
// each walked by its own wavefront, without splitting a sum: the part in which a category's run STARTS owns it, walks on past
// its nominal end until that run is over, and skips a run it found already under way at its first rank. (Helps when runs
// are short; aligned positives give a variable one code for half the samples, and the walk past the end then costs what
// the cut saved.)
template <bool CLASSIFIER, int TAB>
__global__ __launch_bounds__(256) void k_split_cat_sorted(SplitCatArgs A) {
  extern __shared__ double l_tab[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // scalar: rank tests below are wave-uniform
  if (TAB != 0) {
    const int words = A.n_pre * (TAB == 1 ? 2 : 1);
    const double* src = reinterpret_cast<const double*>(A.tab);
    for (int i = threadIdx.x; i < words; i += blockDim.x) l_tab[i] = src[i];
    __syncthreads();
  }
  const int unit = blockIdx.x * A.waves + wave;
  const int group = unit / A.parts, part = unit - group * A.parts;
  if (wave >= A.waves || group >= A.n_groups) return;
  const int f = group * 64 + lane;
  const bool live = f < A.n_vars;
  const int n4 = (A.n_pre + 3) >> 2;
  const uint4* p = reinterpret_cast<const uint4*>(A.packed) + (size_t)group * n4 * 64 + lane;
  double* h = A.hist + (size_t)(live ? f : 0) * 512;
  const int begin = part * A.part_len, end = min(A.n_pre, begin + A.part_len);
  if (begin >= A.n_pre) return;
  // cur: the code of the run the walk is in; own: this part sums that run
  int cur = -1;
  if (begin > 0) cur = (int)(A.packed[(((size_t)group * n4 + ((begin - 1) >> 2)) * 64 + lane) * 4 + ((begin - 1) & 3)] & 255u);
  bool own = false;
  double a0 = 0, a1 = 0;
  constexpr int U = SPLIT_CAT_UNROLL, D = SPLIT_CAT_DEPTH;
  static_assert(2 * D * U <= SPLIT_CAT_PAD_RANKS && U % 4 == 0, "table padding covers the read-ahead");
  uint4 buf[D][U / 4];
  auto load = [&](int r0, uint4(&x)[U / 4]) {
#pragma unroll
    for (int k = 0; k < U / 4; k++) x[k] = p[(size_t)((r0 >> 2) + k) * 64];
  };
  auto process = [&](int r0, const uint4(&x4)[U / 4]) {
    uint32_t x[U];
#pragma unroll
    for (int k = 0; k < U / 4; k++) {
      x[4 * k] = x4[k].x;
      x[4 * k + 1] = x4[k].y;
      x[4 * k + 2] = x4[k].z;
      x[4 * k + 3] = x4[k].w;
    }
    double w[U], t[U];
#pragma unroll
    for (int k = 0; k < U; k++) {
      const unsigned g = x[k] >> 8;
      if (TAB == 2) {
        t[k] = l_tab[g];
        w[k] = 0;
      } else {
        const SplitEntry e = TAB == 1 ? reinterpret_cast<const SplitEntry*>(l_tab)[g] : A.tab[g];
        w[k] = e.w;
        t[k] = e.t;
      }
    }
#pragma unroll
    for (int k = 0; k < U; k++) {
      if (r0 + k >= A.n_pre) break;  // wave-uniform
      const int code = (int)(x[k] & 255u);
      if (code != cur) {
        if (own && live) {
          h[2 * cur] = a0;
          h[2 * cur + 1] = a1;
        }
        a0 = 0;
        a1 = 0;
        cur = code;
        own = r0 + k < end;  // a run that starts behind the nominal end is the next part's
      }
      if (TAB == 2) {
        if (CLASSIFIER) {  // entry = w, class 1 in the sign bit: max(x, +0) is w for class 0 and 0 for class 1
          a0 += fmax(t[k], 0.0);
          a1 += fmax(-t[k], 0.0);
        } else {  // entry = response * w with response +-1
          a0 += t[k];
          a1 += fabs(t[k]);
        }
      } else if (CLASSIFIER) {
        const bool c1 = t[k] != 0.0;
        a0 += c1 ? 0.0 : w[k];
        a1 += c1 ? w[k] : 0.0;
      } else {
        a0 += t[k];
        a1 += w[k];
      }
    }
  };
#pragma unroll
  for (int d = 0; d < D; d++) load(begin + d * U, buf[d]);
  int r0 = begin;
  while (r0 < end || (r0 < A.n_pre && __any(own))) {  // ... || runs that straddle the nominal end
#pragma unroll
    for (int d = 0; d < D; d++) {
      process(r0 + d * U, buf[d]);
      load(r0 + (D + d) * U, buf[d]);
    }
    r0 += D * U;
  }
  if (own && live) {
    h[2 * cur] = a0;
    h[2 * cur + 1] = a1;
  }
}

// ------------------------------------------------------------------------------------------------
// Streamed tail (cc_eval_presort_split): the best variable so far, kept on the device while the chunks of a node's search
// go by. One block reduces the variables [v0, v1) just searched by k_boost_argmax's rule (cc_boost.hip; pick_winner's,
// o_cvdtree.cpp:320-351): the first variable, in variable order, with the largest (float)quality among those that found
// a split, and only if that is > 0. The rule is associative -- rounding to float is monotone, so the largest float of a
// union is the larger of the parts' largest floats, and on a tie the earlier part holds the lower variable -- hence
// folding the parts in variable order (head, then chunk after chunk, a later part replacing only with a strictly
// larger float) ends at the variable k_boost_argmax finds over all of them. A part that takes the lead and has a
// table (a chunk: its table is overwritten by the next one) leaves the leader's sorted row, values and sample numbers,
// in the winner row, where k_boost_apply_ord finds it after the last chunk.
// ------------------------------------------------------------------------------------------------
template <class TI>
__global__ __launch_bounds__(1024) void k_stream_winner(const double* __restrict__ best_val, const int* __restrict__ best_i, int v0, int v1, int reset,
                                                        const float* __restrict__ tab_val, const TI* __restrict__ tab_idx, int n,
                                                        StreamBest* __restrict__ state, float* __restrict__ win_val, TI* __restrict__ win_idx) {
  __shared__ float s_q[1024];
  __shared__ int s_f[1024];
  __shared__ int s_take;
  float q = 0.f;  // only qualities > 0 can win
  int f = -1;
  for (int i = v0 + (int)threadIdx.x; i < v1; i += (int)blockDim.x) {  // increasing i: a later equal value does not replace
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
      const float q2 = s_q[threadIdx.x + step], q1 = s_q[threadIdx.x];
      const int f2 = s_f[threadIdx.x + step], f1 = s_f[threadIdx.x];
      if (f2 >= 0 && (f1 < 0 || q2 > q1 || (q2 == q1 && f2 < f1))) {
        s_q[threadIdx.x] = q2;
        s_f[threadIdx.x] = f2;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    StreamBest cur = *state;
    if (reset) cur = StreamBest{-1, 0.f};
    const bool take = s_f[0] >= 0 && s_q[0] > cur.quality;  // strictly: the leader so far has the lower variable number
    if (take) cur = StreamBest{s_f[0], s_q[0]};
    *state = cur;
    s_take = take && tab_val ? s_f[0] - v0 : -1;
  }
  __syncthreads();
  const int fl = s_take;  // the new leader's place in the chunk table
  if (fl < 0) return;
  const size_t base = (size_t)(fl >> 6) * n * 64 + (fl & 63);
  for (int r = threadIdx.x; r < n; r += blockDim.x) {
    win_val[r] = tab_val[base + (size_t)r * 64];
    win_idx[r] = tab_idx[base + (size_t)r * 64];
  }
}

}  // namespace ccamd

using namespace ccamd;

// compute units of a device (hipGetDeviceProperties fills a 1.5 KB struct and takes ~1 ms: asked once per device)
static int device_cus(int device) {
  static std::mutex mu;
  static int cached[64] = {0};
  std::lock_guard<std::mutex> lk(mu);
  if (device >= 0 && device < 64 && cached[device] > 0) return cached[device];
  int v = 0;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || v < 1) v = 256;
  if (device >= 0 && device < 64) cached[device] = v;
  return v;
}

// The LDS opt-in is per device and cheap: set on every launch that needs it.
template <class Args>
static cc_status launch(void (*kernel)(Args), unsigned blocks, unsigned threads, size_t lds, hipStream_t stream, const Args& args) {
  if (lds > 64 * 1024) CC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), lds, stream, args);
  CC_HIP(hipGetLastError());
  return CC_OK;
}

// One call, arguments checked: the node and what the three searches share.
struct SplitQuery {
  cc_evaluator* e;
  const int32_t* sample_idx;  // NULL: samples 0 .. n-1
  int n;
  const double* weights;
  const float* responses;
  const int32_t* class_labels;
  double node_value;
  bool is_classifier, gini;
  int N, F, var0;  // presorted samples and variables; per-variable outputs are indexed from presort's fi_begin = var0
  cc_split* out;
  double* per_var_quality;
  int32_t* per_var_point;

  int sample(int i) const { return sample_idx ? sample_idx[i] : i; }
  // 8-byte entry: response * w (w = |entry|), or w with the class in the sign bit
  double entry8(int i) const { return is_classifier ? (class_labels[i] ? -weights[i] : weights[i]) : responses[i] * weights[i]; }
  SplitEntry entry16(int i) const { return SplitEntry{weights[i], is_classifier ? (double)class_labels[i] : responses[i] * weights[i]}; }
};

constexpr size_t SPLIT_LDS_CAP = 160 * 1024;
// A table in LDS implies 16-bit sample numbers in the sorted tables: no kernel pairs int32_t with an LDS form.
static_assert(SPLIT_LDS_CAP / 8 <= 65536, "an LDS table holds at most 65 536 samples");

static size_t table_bytes(TableForm form, size_t entries) { return entries * (form == TABLE_LDS8 ? 8 : 16); }
static size_t table_lds(TableForm form, int N) { return form == TABLE_GLOBAL16 ? 0 : table_bytes(form, (size_t)N); }

// 8-byte entries need a class or a response of +-1, and whenever 16-byte entries would fit LDS so do 8-byte ones:
// TABLE_LDS16 is what regression with other responses (LOGIT) gets, and nothing else does.
static TableForm table_form(int N, bool unit_entries) {
  if (std::getenv("CCAMD_SPLIT_GLOBAL_TABLE")) return TABLE_GLOBAL16;
  if (unit_entries && (size_t)N * 8 <= SPLIT_LDS_CAP) return TABLE_LDS8;
  return (size_t)N * 16 <= SPLIT_LDS_CAP ? TABLE_LDS16 : TABLE_GLOBAL16;
}
static TableForm table_form(const SplitQuery& q) {
  bool unit_responses = !q.is_classifier;
  for (int i = 0; i < q.n && unit_responses; i++) unit_responses = q.responses[i] == 1.0f || q.responses[i] == -1.0f;
  return table_form(q.N, q.is_classifier || unit_responses);
}
namespace ccamd {
TableForm split_table_form_unit(int N) { return table_form(N, true); }
}

// What a table holds for a stored sample that is not in the node. The ordered kernels test for it: w = -1, or the quiet
// NaN whose high word k_split_ord_lean compares (0x7ff80000, low word 0). k_split_cat_sorted adds every entry up: +0.0.
const AbsentEntry ccamd::ABSENT_ORDERED = {std::numeric_limits<double>::quiet_NaN(), {-1.0, 0.0}};
const AbsentEntry ccamd::ABSENT_CATEGORICAL = {0.0, {0.0, 0.0}};

// Builds the node's table in pin_in and sends it to d_split_tab. With `absent`: dense, one entry per stored sample and
// `absent` for those outside the node. Without: the compact list of k_split_cat, the node's entries in node order
// (16-byte: TABLE_GLOBAL16) and their stored-sample numbers, which go to d_split_idx.
static cc_status upload_node_table(const SplitQuery& q, TableForm form, const AbsentEntry* absent) {
  cc_evaluator* e = q.e;
  const size_t m = absent ? (size_t)q.N : (size_t)q.n, bytes = table_bytes(form, m);
  CC_HIP(e->pin_in.ensure(bytes + (absent ? 0 : m * 4)));
  double* tab8 = static_cast<double*>(e->pin_in.p);
  SplitEntry* tab16 = static_cast<SplitEntry*>(e->pin_in.p);
  int32_t* idx_host = reinterpret_cast<int32_t*>(static_cast<char*>(e->pin_in.p) + bytes);
  if (absent && form == TABLE_LDS8) std::fill_n(tab8, m, absent->e8);
  if (absent && form != TABLE_LDS8) std::fill_n(tab16, m, absent->e16);
  std::vector<uint8_t> seen((size_t)q.N, 0);
  for (int i = 0; i < q.n; i++) {
    const int g = q.sample(i), slot = absent ? g : i;
    if (g < 0 || g >= q.N) return set_error(CC_ERR_OUT_OF_RANGE, "cc_eval_find_best_split: sample index %d outside the %d presorted samples", g, q.N);
    if (seen[(size_t)g]) return set_error(CC_ERR_INVALID_ARG, "cc_eval_find_best_split: sample %d occurs twice in the node", g);
    seen[(size_t)g] = 1;
    if (!absent) idx_host[i] = g;
    if (form == TABLE_LDS8)
      tab8[slot] = q.entry8(i);
    else
      tab16[slot] = q.entry16(i);
  }
  CC_HIP(e->d_split_tab.ensure(m * 2));
  CC_HIP(hipMemcpyAsync(e->d_split_tab.p, e->pin_in.p, bytes, hipMemcpyHostToDevice, e->stream.s));
  if (absent) return CC_OK;
  CC_HIP(e->d_split_idx.ensure(m));
  CC_HIP(hipMemcpyAsync(e->d_split_idx.p, idx_host, m * 4, hipMemcpyHostToDevice, e->stream.s));
  return CC_OK;
}

// The kernels that can be launched, and no others: what is not named here is not in the code object. With the table in
// global memory the index type follows N; with it in LDS the indices are 16-bit (SPLIT_LDS_CAP) and TABLE_LDS16 is
// regression only (table_form). k_split_ord_lean for the regression / GINI searches (Gentle 6.77 against 7.01 ms, GINI
// 8.91 against 9.31 at configs[4]); the MISCLASS search has no division and nothing to hoist: the round-1 kernel stays
// (4.46 against 4.76 ms). A combination that cannot occur gets no kernel, and its launch fails.
static void (*ordered_kernel(int mode, TableForm form, bool idx16))(SplitOrdArgs) {
  if (form == TABLE_GLOBAL16 && !idx16) return mode == 0 ? k_split_ord<0, int32_t, 0> : mode == 1 ? k_split_ord<1, int32_t, 0> : k_split_ord<2, int32_t, 0>;
  if (form == TABLE_GLOBAL16) return mode == 0 ? k_split_ord<0, uint16_t, 0> : mode == 1 ? k_split_ord<1, uint16_t, 0> : k_split_ord<2, uint16_t, 0>;
  if (!idx16) return nullptr;
  if (form == TABLE_LDS16) return mode == 0 ? k_split_ord<0, uint16_t, 1> : nullptr;
  return mode == 0 ? k_split_ord_lean<0, uint16_t> : mode == 1 ? k_split_ord_lean<1, uint16_t> : k_split_ord<2, uint16_t, 2>;
}
static void (*categorical_sorted_kernel(bool is_classifier, TableForm form))(SplitCatArgs) {
  if (form == TABLE_GLOBAL16) return is_classifier ? k_split_cat_sorted<true, 0> : k_split_cat_sorted<false, 0>;
  if (form == TABLE_LDS16) return is_classifier ? nullptr : k_split_cat_sorted<false, 1>;
  return is_classifier ? k_split_cat_sorted<true, 2> : k_split_cat_sorted<false, 2>;
}

// ev_a .. ev_b for cc_eval_last_kernel_ms; the stream has been synchronised
static void note_kernel_ms(cc_evaluator* e) {
  float ms = 0;
  if (hipEventElapsedTime(&ms, e->ev_a.e, e->ev_b.e) == hipSuccess) e->last_ms = ms;
}

// The winner, variable by variable as DTreeBestSplitFinder::operator() does (o_cvdtree.cpp:320-342): a variable reports
// a split only if it beats the best quality so far (a float), and replaces it only if its own quality, rounded to
// float, is larger. Fills the per-variable outputs and the winner's part of q.out; returns the winner, or -1 for no split.
template <class Found, class Quality, class Point>
static int pick_winner(const SplitQuery& q, Found found, Quality quality, Point point) {
  float best_q = -1.f;
  int winner = -1;
  for (int f = 0; f < q.F; f++) {
    if (q.per_var_quality) q.per_var_quality[f] = found(f) ? quality(f) : -1.0;
    if (q.per_var_point) q.per_var_point[f] = point(f);
    if (!found(f) || !((double)best_q < quality(f))) continue;
    const float v = (float)quality(f);
    if (best_q < v) {
      best_q = v;
      winner = f;
    }
  }
  if (winner < 0 || !(best_q > 0)) return -1;  // o_cvdtree.cpp:351
  q.out->found = 1;
  q.out->var_idx = q.var0 + winner;
  q.out->quality = best_q;
  return winner;
}

// The ordered search of the presorted variables over the node table in d_split_tab (`form`; built by upload_node_table
// or, on the device, by the booster): the per-variable results stay in d_split_out as OrdResult lays them out, between
// ev_a and ev_b on the evaluator's stream. One table of n_vars sorted variables (the resident table or a chunk's) whose
// first variable is number var_offset (a multiple of 64) of the presorted range: results at that offset of OrdResult.
static cc_status launch_ordered_table(cc_evaluator* e, int mode, TableForm form, double w_total0, double w_total1, double rsum0, const SortedTable& t,
                                      int n_vars, int var_offset) {
  const int N = e->presort_n, F = e->presort_f1 - e->presort_f0;
  const size_t groups = ((size_t)n_vars + 63) / 64, fpad = ((size_t)F + 63) / 64 * 64;
  const OrdResult dev(e->d_split_out.p, fpad);
  // in the struct's order: sv, si, tab, n_pre, n_vars, w_total0, w_total1, rsum0, best_val, best_i, best_vl, best_vr, n_groups, dbg_nogather
  const SplitOrdArgs A{t.val.p, t.idx(), reinterpret_cast<const SplitEntry*>(e->d_split_tab.p), N, n_vars, w_total0, w_total1, rsum0,
                       dev.best_val + var_offset, dev.best_i + var_offset, dev.best_vl + var_offset, dev.best_vr + var_offset, (int)groups,
                       std::getenv("CCAMD_DEBUG_SPLIT_NOGATHER") ? 1 : 0};
  // wavefronts per block: with the table in LDS one block owns a CU, so spread the groups evenly over the CUs
  // (162 336 variables = 2 537 groups -> 254 blocks of 10 wavefronts on 256 CUs); from global memory, one wavefront
  // per block.
  int wpb = 1;
  if (form != TABLE_GLOBAL16) {
    const int cus = device_cus(e->device);
    wpb = (int)std::min<size_t>(16, std::max<size_t>(1, (groups + cus - 1) / cus));
    if (form == TABLE_LDS8 && mode != 2) wpb = std::min(wpb, SPLIT_LEAN_WAVES);  // k_split_ord_lean
  }
  const unsigned blocks = (unsigned)((groups + wpb - 1) / wpb);
  (void)hipEventRecord(e->ev_a.e, e->stream.s);
  if (cc_status st = launch(ordered_kernel(mode, form, !t.wide), blocks, 64u * wpb, table_lds(form, N), e->stream.s, A); st != CC_OK) return st;
  (void)hipEventRecord(e->ev_b.e, e->stream.s);
  return CC_OK;
}

// The leader after the variables [v0, v1) of OrdResult (k_stream_winner); tab: the chunk table they were searched in, or
// NULL for the head, whose rows stay where they are.
static cc_status launch_stream_winner(cc_evaluator* e, int v0, int v1, bool reset, const SortedTable* tab) {
  const OrdResult dev(e->d_split_out.p, ((size_t)(e->presort_f1 - e->presort_f0) + 63) / 64 * 64);
  with_index_type(wide_index((size_t)e->presort_n), [&](auto ti) {
    using TI = decltype(ti);
    hipLaunchKernelGGL((k_stream_winner<TI>), dim3(1), dim3(1024), 0, e->stream.s, dev.best_val, dev.best_i, v0, v1, reset ? 1 : 0,
                       tab ? tab->val.p : nullptr, tab ? static_cast<const TI*>(tab->idx()) : nullptr, e->presort_n, e->d_win_state.p, e->d_win_val.p,
                       reinterpret_cast<TI*>(e->d_win_idx.p));
  });
  CC_HIP(hipGetLastError());
  return CC_OK;
}

// cc_eval_stream_profile: one more event in the stream, no host wait
static cc_status stream_mark(cc_evaluator* e) {
  if (!e->stream_profile) return CC_OK;
  if (e->stream_ev_used == e->stream_ev.size()) {
    e->stream_ev.emplace_back();
    CC_HIP(e->stream_ev.back().create());
  }
  CC_HIP(hipEventRecord(e->stream_ev[e->stream_ev_used++].e, e->stream.s));
  return CC_OK;
}

// The streamed tail of a node's search: per chunk, in variable order, what cc_eval_presort does once per stage for a
// resident variable -- evaluate, stable row sort, k_interleave into the chunk table (fill_sorted_table) -- then the
// ordered kernel over that table. The reference does the same for a variable outside its caches at every node
// (CvCascadeBoostTrainData::get_ord_var_data, o_cvcascadeboosttraindata.cpp:437-458). Nothing waits on the host.
static cc_status stream_ordered_tail(cc_evaluator* e, int mode, TableForm form, double w_total0, double w_total1, double rsum0, bool track_winner) {
  const int N = e->presort_n, F = e->presort_f1 - e->presort_f0, R = e->presort_resident, C = e->presort_chunk;
  if (track_winner && R > 0)
    if (cc_status st = launch_stream_winner(e, 0, R, true, nullptr); st != CC_OK) return st;
  e->stream_ev_used = 0;
  for (int c0 = R; c0 < F; c0 += C) {
    const int nf = std::min(C, F - c0);
    if (cc_status st = fill_sorted_table(e, *e->stream_rows, e->presort_f0 + c0, nf, e->chunk, 0, stream_mark); st != CC_OK) return st;
    // a short last chunk: the zeroed read-ahead padding stands behind ITS last group (a full chunk's was zeroed by the presort)
    if (nf < C)
      if (cc_status st = e->chunk.zero_padding(((size_t)nf + 63) / 64 * 64 * (size_t)N, e->stream.s); st != CC_OK) return st;
    if (cc_status st = stream_mark(e); st != CC_OK) return st;
    if (cc_status st = launch_ordered_table(e, mode, form, w_total0, w_total1, rsum0, e->chunk, nf, c0); st != CC_OK) return st;
    if (cc_status st = stream_mark(e); st != CC_OK) return st;
    if (track_winner)
      if (cc_status st = launch_stream_winner(e, c0, c0 + nf, c0 == 0, &e->chunk); st != CC_OK) return st;
    if (cc_status st = stream_mark(e); st != CC_OK) return st;
  }
  return CC_OK;
}

cc_status ccamd::split_launch_ordered(cc_evaluator* e, int mode, TableForm form, double w_total0, double w_total1, double rsum0, bool track_winner) {
  const int F = e->presort_f1 - e->presort_f0, R = e->presort_resident;
  CC_HIP(e->d_split_out.ensure(((size_t)F + 63) / 64 * 64 * 3));  // OrdResult::bytes + slack
  if (R >= F) return launch_ordered_table(e, mode, form, w_total0, w_total1, rsum0, e->head, F, 0);
  (void)hipEventRecord(e->ev_stream_a.e, e->stream.s);
  if (R > 0)
    if (cc_status st = launch_ordered_table(e, mode, form, w_total0, w_total1, rsum0, e->head, R, 0); st != CC_OK) return st;
  const cc_status st = stream_ordered_tail(e, mode, form, w_total0, w_total1, rsum0, track_winner);
  (void)hipEventRecord(e->ev_b.e, e->stream.s);
  return st;
}

double ccamd::split_search_ms(cc_evaluator* e) {
  const bool streamed = e->presort_n > 0 && e->presort_resident < e->presort_f1 - e->presort_f0;
  float ms = 0;
  if (hipEventElapsedTime(&ms, streamed ? e->ev_stream_a.e : e->ev_a.e, e->ev_b.e) == hipSuccess) e->last_ms = ms;
  if (streamed && e->stream_profile) {
    for (double& x : e->stream_phase_ms) x = 0;
    for (size_t i = 0; i + 5 < e->stream_ev_used; i += 6)
      for (int k = 0; k < 5; k++)
        if (hipEventElapsedTime(&ms, e->stream_ev[i + k].e, e->stream_ev[i + k + 1].e) == hipSuccess) e->stream_phase_ms[k] += ms;
  }
  return e->last_ms;
}

static cc_status search_ordered(const SplitQuery& q) {
  cc_evaluator* e = q.e;
  const int mode = !q.is_classifier ? 0 : (q.gini ? 1 : 2);
  const TableForm form = table_form(q);
  if (cc_status st = upload_node_table(q, form, &ABSENT_ORDERED); st != CC_OK) return st;
  if (cc_status st = split_launch_ordered(e, mode, form, q.weights[q.n], q.weights[q.n + 1], q.node_value * q.weights[q.n]); st != CC_OK) return st;
  const size_t fpad = ((size_t)q.F + 63) / 64 * 64;
  CC_HIP(e->pin_out.ensure(fpad * 24));
  CC_HIP(hipMemcpyAsync(e->pin_out.p, e->d_split_out.p, OrdResult::bytes(fpad), hipMemcpyDeviceToHost, e->stream.s));
  CC_HIP(hipStreamSynchronize(e->stream.s));
  (void)split_search_ms(e);
  const OrdResult got(e->pin_out.p, fpad);
  const int winner = pick_winner(q, [&](int f) { return got.best_i[f] >= 0; }, [&](int f) { return got.best_val[f]; }, [&](int f) { return got.best_i[f]; });
  if (winner >= 0) {
    q.out->ord_c = (got.best_vl[winner] + got.best_vr[winner]) * 0.5f;
    q.out->split_point = got.best_i[winner];
  }
  return CC_OK;
}

// Per-category sums of a node that lists its samples in increasing order, from the (code, sample)-sorted table.
static cc_status search_categorical_sorted(const SplitQuery& q, size_t hist_n, TableForm form) {
  cc_evaluator* e = q.e;
  const int N = q.N;
  (void)hipEventRecord(e->ev_a.e, e->stream.s);
  CC_HIP(hipMemsetAsync(e->d_split_out.p, 0, hist_n * 8, e->stream.s));  // categories without a sample
  const size_t groups = ((size_t)q.F + 63) / 64;
  SplitCatArgs A;
  A.packed = e->d_cat_sorted.p;
  A.tab = reinterpret_cast<const SplitEntry*>(e->d_split_tab.p);
  A.n_pre = N;
  A.n_vars = q.F;
  A.n_groups = (int)groups;
  A.hist = e->d_split_out.p;
  // One wavefront per (group, part); with the table in LDS a block owns a CU (<= 4 wavefronts of it): as many parts as
  // give every CU a full block, no part shorter than 1 024 ranks. CCAMD_SPLIT_CAT_PARTS overrides (1 = round-4 first form).
  const int cus = device_cus(e->device);
  int parts = (int)std::max<size_t>(1, (size_t)cus * 4 / groups);
  parts = std::max(1, std::min(parts, N / 1024));
  if (const char* v = std::getenv("CCAMD_SPLIT_CAT_PARTS")) parts = std::max(1, std::min(64, std::atoi(v)));
  const int chunk = SPLIT_CAT_DEPTH * SPLIT_CAT_UNROLL;
  A.parts = parts;
  A.part_len = ((N + parts - 1) / parts + chunk - 1) / chunk * chunk;
  const size_t units = groups * (size_t)parts;
  A.waves = form == TABLE_GLOBAL16 ? 4 : (int)std::min<size_t>(4, std::max<size_t>(1, (units + cus - 1) / cus));
  const unsigned blocks = (unsigned)((units + A.waves - 1) / A.waves);
  const cc_status st = launch(categorical_sorted_kernel(q.is_classifier, form), blocks, 256, table_lds(form, N), e->stream.s, A);
  (void)hipEventRecord(e->ev_b.e, e->stream.s);
  return st;
}

// The same sums for a node in any order: its samples streamed through k_split_cat.
static cc_status search_categorical_stream(const SplitQuery& q) {
  cc_evaluator* e = q.e;
  if (cc_status st = upload_node_table(q, TABLE_GLOBAL16, nullptr); st != CC_OK) return st;
  (void)hipEventRecord(e->ev_a.e, e->stream.s);
  hipLaunchKernelGGL(q.is_classifier ? k_split_cat<true> : k_split_cat<false>, dim3((unsigned)q.F), dim3(256), 0, e->stream.s, e->d_codes.p, q.N,
                     q.sample_idx ? e->d_split_idx.p : nullptr, reinterpret_cast<const SplitEntry*>(e->d_split_tab.p), q.n, e->d_split_out.p);
  (void)hipEventRecord(e->ev_b.e, e->stream.s);
  CC_HIP(hipGetLastError());
  return CC_OK;
}

// The 34.7 MB of sums (8 464 variables) come back in pieces; the host's part -- ordering each variable's categories and
// scanning them (split_categories) -- starts on a piece as soon as it has landed, on up to 16 threads.
static cc_status reduce_category_sums(const SplitQuery& q, size_t hist_n, std::vector<CatSplit>& res) {
  cc_evaluator* e = q.e;
  const int F = q.F;
  CC_HIP(e->pin_out.ensure(hist_n * 8));
  constexpr int kPieces = 8;
  for (int c = 0; c < kPieces; c++)
    if (!e->ev_piece[c].e) CC_HIP(e->ev_piece[c].create(hipEventDisableTiming));
  const int per_piece = (F + kPieces - 1) / kPieces;
  double* hist = static_cast<double*>(e->pin_out.p);
  for (int c = 0; c < kPieces; c++) {
    const int f0 = std::min(F, c * per_piece), f1 = std::min(F, f0 + per_piece);
    if (f1 > f0)
      CC_HIP(hipMemcpyAsync(hist + (size_t)f0 * 512, e->d_split_out.p + (size_t)f0 * 512, (size_t)(f1 - f0) * 512 * 8, hipMemcpyDeviceToHost, e->stream.s));
    CC_HIP(hipEventRecord(e->ev_piece[c].e, e->stream.s));
  }
  std::atomic<int> copy_failed{0};
  const bool trace = std::getenv("CCAMD_TRACE_SPLIT") != nullptr;  // host-side timeline of the call's tail (stderr)
  const auto t_enq = std::chrono::steady_clock::now();
  double landed_ms[kPieces] = {};
  {
    const int nt = std::max(1, std::min<int>({(int)std::thread::hardware_concurrency(), 16, F / 64 + 1}));
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++)
      th.emplace_back([&, t]() {
        for (int c = 0; c < kPieces; c++) {
          if (hipEventSynchronize(e->ev_piece[c].e) != hipSuccess) {
            copy_failed = 1;
            return;
          }
          if (trace && t == 0) landed_ms[c] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_enq).count();
          const int f0 = std::min(F, c * per_piece), f1 = std::min(F, f0 + per_piece);
          for (int f = f0 + t; f < f1; f += nt) split_categories(hist + (size_t)f * 512, 256, q.is_classifier, q.gini, res[(size_t)f]);
        }
      });
    for (auto& x : th) x.join();
  }
  if (trace) {
    std::fprintf(stderr, "[ccamd split] after the last enqueue: pieces landed (as seen by worker 0) at");
    for (int c = 0; c < kPieces; c++) std::fprintf(stderr, " %.2f", landed_ms[c]);
    std::fprintf(stderr, " ms; workers done at %.2f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_enq).count());
  }
  CC_HIP(hipStreamSynchronize(e->stream.s));
  if (copy_failed) return set_error(CC_ERR_HIP, "cc_eval_find_best_split: copying the category sums back failed");
  note_kernel_ms(e);
  return CC_OK;
}

static cc_status finish_categorical(const SplitQuery& q, size_t hist_n);
static cc_status search_categorical(const SplitQuery& q) {
  const size_t hist_n = (size_t)q.F * 256 * 2;
  CC_HIP(q.e->d_split_out.ensure(hist_n));
  bool ascending = true;  // the node lists its samples in increasing order: what k_split_cat_sorted's exactness needs
  for (int i = 1; i < q.n && ascending && q.sample_idx; i++) ascending = q.sample_idx[i - 1] < q.sample_idx[i];
  const bool sorted = ascending && q.e->cat_sorted_n == q.N && cat_sorted_table_enabled();
  if (sorted) {
    const TableForm form = table_form(q);
    if (cc_status st = upload_node_table(q, form, &ABSENT_CATEGORICAL); st != CC_OK) return st;
    if (cc_status st = search_categorical_sorted(q, hist_n, form); st != CC_OK) return st;
  } else if (cc_status st = search_categorical_stream(q); st != CC_OK)
    return st;
  return finish_categorical(q, hist_n);
}

// The categorical search over the node table the booster built in d_split_tab (`form`, absent samples as
// ABSENT_CATEGORICAL, node = stored samples in increasing order): the sorted-table kernel, then the host's category
// ordering exactly as cc_eval_find_best_split does it.
cc_status ccamd::split_categorical_from_table(cc_evaluator* e, bool is_classifier, bool gini, TableForm form, cc_split* out) {
  if (e->cat_sorted_n != e->presort_n)
    return set_error(CC_ERR_UNSUPPORTED, "cc_boost: the categorical search needs the (code, sample)-sorted table of cc_eval_presort");
  std::memset(out, 0, sizeof(*out));
  out->quality = -1.f;
  const int F = e->presort_f1 - e->presort_f0;
  const SplitQuery q{e, nullptr, e->presort_n, nullptr, nullptr, nullptr, 0.0, is_classifier, gini, e->presort_n, F, e->presort_f0, out, nullptr, nullptr};
  const size_t hist_n = (size_t)F * 256 * 2;
  CC_HIP(e->d_split_out.ensure(hist_n));
  if (cc_status st = search_categorical_sorted(q, hist_n, form); st != CC_OK) return st;
  return finish_categorical(q, hist_n);
}

static cc_status finish_categorical(const SplitQuery& q, size_t hist_n) {
  std::vector<CatSplit> res((size_t)q.F);
  if (cc_status st = reduce_category_sums(q, hist_n, res); st != CC_OK) return st;
  const int winner = pick_winner(q, [&](int f) { return res[(size_t)f].found; }, [&](int f) { return res[(size_t)f].quality; },
                                 [&](int f) { return res[(size_t)f].found ? res[(size_t)f].n_left - 1 : -1; });
  if (winner >= 0) std::memcpy(q.out->subset, res[(size_t)winner].subset, sizeof(q.out->subset));
  return CC_OK;
}

extern "C" {

cc_status cc_eval_stream_profile(cc_evaluator* e, int enable) {
  if (!e) return set_error(CC_ERR_INVALID_ARG, "cc_eval_stream_profile: null evaluator");
  std::lock_guard<std::mutex> lk(e->mu);
  e->stream_profile = enable != 0;
  return CC_OK;
}

cc_status cc_eval_stream_phase_ms(cc_evaluator* e, double* ms, int cap, int* n_parts) {
  if (!e || !ms || !n_parts) return set_error(CC_ERR_INVALID_ARG, "cc_eval_stream_phase_ms: null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  *n_parts = 5;
  for (int i = 0; i < 5 && i < cap; i++) ms[i] = e->stream_phase_ms[i];
  return CC_OK;
}

cc_status cc_eval_find_best_split(cc_evaluator* e, const int32_t* sample_idx, int n, const double* weights, const float* responses,
                                  const int32_t* class_labels, double node_value, int boost_type, int split_criteria, cc_split* out,
                                  double* per_var_quality, int32_t* per_var_point) {
  if (!e || !weights || !out) return set_error(CC_ERR_INVALID_ARG, "cc_eval_find_best_split: null argument");
  if (boost_type < 0 || boost_type > 3) return set_error(CC_ERR_INVALID_ARG, "cc_eval_find_best_split: unknown boost type %d", boost_type);
  const bool is_classifier = boost_type == 0 || boost_type == 1;
  if (is_classifier ? !class_labels : !responses)
    return set_error(CC_ERR_INVALID_ARG, "cc_eval_find_best_split: %s", is_classifier ? "class_labels required for DISCRETE / REAL boost"
                                                                                        : "responses required for LOGIT / GENTLE boost");
  if (e->presort_n <= 0) return set_error(CC_ERR_INVALID_ARG, "cc_eval_find_best_split: call cc_eval_presort first");
  const int N = e->presort_n;
  if (n < 0 || n > N) return set_error(CC_ERR_OUT_OF_RANGE, "cc_eval_find_best_split: n %d exceeds the %d presorted samples", n, N);
  int criteria = split_criteria;
  if (criteria != 1 && criteria != 3) criteria = boost_type == 0 ? 3 : 1;  // o_cvboostree.cpp:188-190
  if (cc_status st = eval_device(e); st != CC_OK) return st;
  std::memset(out, 0, sizeof(*out));
  out->quality = -1.f;
  const int F = e->presort_f1 - e->presort_f0;
  if (per_var_quality)
    for (int f = 0; f < F; f++) per_var_quality[f] = -1.0;
  if (per_var_point)
    for (int f = 0; f < F; f++) per_var_point[f] = -1;
  if (n <= 1) return CC_OK;  // get_num_valid(vi) <= 1: no variable is searched
  for (int i = 0; i < n; i++) {
    if (is_classifier && (class_labels[i] < 0 || class_labels[i] > 1))
      return set_error(CC_ERR_INVALID_ARG, "cc_eval_find_best_split: class label %d of sample %d is not 0 / 1", class_labels[i], i);
    if (!(weights[i] >= 0.0)) return set_error(CC_ERR_INVALID_ARG, "cc_eval_find_best_split: weight of sample %d is negative or NaN", i);
  }
  std::lock_guard<std::mutex> lk(e->mu);
  const SplitQuery q{e, sample_idx, n, weights, responses, class_labels, node_value, is_classifier, criteria == 1, N, F, e->presort_f0, out,
                     per_var_quality, per_var_point};
  return e->type != CC_FEATURE_LBP ? search_ordered(q) : search_categorical(q);  // ordered variables: Haar, HOG
}

}  // extern "C"
