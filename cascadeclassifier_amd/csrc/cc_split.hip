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
// Data layout in HBM (cc_eval_presort): variables in groups of 64; per group the sorted values (f32) and sample indices
// (u16 when n_samples <= 65 536, else i32) are interleaved [group][rank][64 lanes], so that lane = variable reads of
// one rank are one coalesced 256-B / 128-B segment. LBP: category codes u8 [variable][sample].
//
// The running sums of the reference are sequential double additions in sorted order; they are reproduced bit for bit by
// giving each variable to one thread. Parallelism comes from the 10^5 variables, not from the scan.
#include <hipcub/hipcub.hpp>

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
// [rows][n] row-major (one sorted variable per row) -> [group][rank][64]
// ------------------------------------------------------------------------------------------------
template <class TI>
__global__ __launch_bounds__(256) void k_interleave(const float* __restrict__ vals, const int* __restrict__ idx, int rows, int n,
                                                    float* __restrict__ out_val, TI* __restrict__ out_idx, size_t group0) {
  __shared__ float tv[64][65];
  __shared__ int ti[64][65];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = blockIdx.x * 64, g = blockIdx.y;
  for (int j = wave; j < 64; j += 4) {
    const int row = g * 64 + j;
    float v = 0.f;
    int s = 0;
    if (row < rows && r0 + lane < n) {
      v = vals[(size_t)row * n + r0 + lane];
      s = idx[(size_t)row * n + r0 + lane];
    }
    tv[j][lane] = v;
    ti[j][lane] = s;
  }
  __syncthreads();
  for (int rr = wave; rr < 64; rr += 4) {
    if (r0 + rr >= n) break;
    const size_t o = ((group0 + g) * (size_t)n + r0 + rr) * 64 + lane;
    out_val[o] = tv[lane][rr];
    out_idx[o] = (TI)ti[lane][rr];
  }
}

// ------------------------------------------------------------------------------------------------
// Stable sort of every row of [rows][n] (one variable per row) with the sample position as the value: one block of 1024
// threads per row, the whole row in registers + LDS (hipcub::BlockRadixSort: LSD radix, stable -- equal values keep
// increasing sample order, what std::stable_sort over (value, index) gives the reference,
// o_cvcascadeboosttraindata.cpp:582-596). A row of a boosting stage (<= 24 576 samples) fits a CU's LDS, so it is read
// once and written once: 8 B + 8 B per element instead of the ~70 B of a device-wide segmented radix sort's four passes.
// ------------------------------------------------------------------------------------------------
constexpr int SORT_THREADS = 1024;
template <int ITEMS>
struct RowSort {
  using Sort = hipcub::BlockRadixSort<float, SORT_THREADS, ITEMS, unsigned short>;
  static constexpr size_t lds_bytes = sizeof(typename Sort::TempStorage);
};
template <int ITEMS>
__global__ __launch_bounds__(SORT_THREADS) void k_sort_rows_block(const float* __restrict__ vals, int rows, int n, float* __restrict__ keys_out,
                                                                  int* __restrict__ idx_out) {
  extern __shared__ __attribute__((aligned(16))) char sort_lds[];
  using Sort = typename RowSort<ITEMS>::Sort;
  typename Sort::TempStorage& temp = *reinterpret_cast<typename Sort::TempStorage*>(sort_lds);
  const int row = blockIdx.x;
  if (row >= rows) return;
  const float* src = vals + (size_t)row * n;
  float key[ITEMS];
  unsigned short val[ITEMS];
#pragma unroll
  for (int i = 0; i < ITEMS; i++) {  // blocked arrangement: thread t owns positions t * ITEMS ..
    const int pos = (int)threadIdx.x * ITEMS + i;
    // padding = +inf: sorts behind every finite value. Precondition: no NaN among the values (a NaN's radix key sorts behind
    // +inf and would push padding into the first n ranks). The evaluators cannot produce one: Haar values are finite sums
    // divided by a positive norm factor or 0 when it is 0 (haarfeatures.h:108-112), LBP codes are 0..255.
    key[i] = pos < n ? src[pos] : __int_as_float(0x7f800000);
    val[i] = (unsigned short)pos;
  }
  Sort(temp).SortBlockedToStriped(key, val);
#pragma unroll
  for (int i = 0; i < ITEMS; i++) {  // striped: rank = i * 1024 + t, consecutive lanes write consecutive ranks
    const int rank = i * SORT_THREADS + (int)threadIdx.x;
    if (rank < n) {
      keys_out[(size_t)row * n + rank] = key[i];
      idx_out[(size_t)row * n + rank] = (int)val[i];
    }
  }
}
template <int ITEMS>
static hipError_t launch_sort_rows_block(const float* vals, int rows, int n, float* keys_out, int* idx_out, hipStream_t st) {
  constexpr size_t lds = RowSort<ITEMS>::lds_bytes;
  if (lds > 64 * 1024) {
    // The opt-in is per device and cheap: set it on every launch (a process-wide "done" flag, as round 3 kept, leaves the
    // second device of a process without it, and is not thread-safe).
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sort_rows_block<ITEMS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((k_sort_rows_block<ITEMS>), dim3((unsigned)rows), dim3(SORT_THREADS), lds, st, vals, rows, n, keys_out, idx_out);
  return hipGetLastError();
}

int sort_rows_block_limit() { return SORT_THREADS * 24; }
hipError_t sort_rows_block(const float* vals, int rows, int n, float* keys_out, int* idx_out, hipStream_t st) {
  if (n <= SORT_THREADS * 4) return launch_sort_rows_block<4>(vals, rows, n, keys_out, idx_out, st);
  if (n <= SORT_THREADS * 8) return launch_sort_rows_block<8>(vals, rows, n, keys_out, idx_out, st);
  if (n <= SORT_THREADS * 12) return launch_sort_rows_block<12>(vals, rows, n, keys_out, idx_out, st);
  if (n <= SORT_THREADS * 16) return launch_sort_rows_block<16>(vals, rows, n, keys_out, idx_out, st);
  if (n <= SORT_THREADS * 20) return launch_sort_rows_block<20>(vals, rows, n, keys_out, idx_out, st);
  return launch_sort_rows_block<24>(vals, rows, n, keys_out, idx_out, st);
}

__global__ void k_codes_u8(const float* __restrict__ in, uint8_t* __restrict__ out, size_t total) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) out[i] = (uint8_t)(int)in[i];
}

__global__ void k_iota_rows2(int* __restrict__ v, size_t total, int n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) v[i] = (int)(i % (size_t)n);
}

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
constexpr int SPLIT_TABLE_PAD_RANKS = 64;  // the sorted tables are allocated (and zeroed) this many ranks beyond the last group's end:
                                           // the lean kernel reads up to 3 chunks ahead without bounds checks
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
constexpr int SPLIT_CAT_UNROLL = 16;  // ranks per chunk: four 16-byte loads per lane
constexpr int SPLIT_CAT_DEPTH = 6;    // chunks whose loads are in flight (one wavefront per SIMD: latency is hidden by distance, not by occupancy)
// zeroed ranks behind the table: read-ahead without bounds checks. A trip that starts at rank r0 < n_pre consumes DEPTH chunks and
// requests the DEPTH after them: ranks up to r0 + 2 * DEPTH * UNROLL - 1.
constexpr int SPLIT_CAT_PAD_RANKS = (2 * SPLIT_CAT_DEPTH + 1) * SPLIT_CAT_UNROLL;
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

// [rows][n] sorted codes (as floats) and sample positions -> (sample << 8 | code) as [group][rank / 4][64][4]
__global__ __launch_bounds__(256) void k_interleave_cat(const float* __restrict__ vals, const int* __restrict__ idx, int rows, int n,
                                                        uint32_t* __restrict__ out, size_t group0) {
  __shared__ uint32_t tv[64][65];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = blockIdx.x * 64, g = blockIdx.y;
  for (int j = wave; j < 64; j += 4) {
    const int row = g * 64 + j;
    uint32_t v = 0;
    if (row < rows && r0 + lane < n) v = ((uint32_t)idx[(size_t)row * n + r0 + lane] << 8) | ((uint32_t)(int)vals[(size_t)row * n + r0 + lane] & 255u);
    tv[j][lane] = v;
  }
  __syncthreads();
  const size_t n4 = ((size_t)n + 3) >> 2;
  for (int rr = wave; rr < 64; rr += 4) {  // [group][rank / 4][lane][rank % 4]; r0 is a multiple of 64
    if (r0 + rr >= n) break;
    out[(((group0 + g) * n4 + ((r0 + rr) >> 2)) * 64 + lane) * 4 + (rr & 3)] = tv[lane][rr];
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

// RowSorter (cc_eval_internal.h): the scratch of one pass and its two sorts.
cc_status RowSorter::init() {
  CC_HIP(e->d_out.ensure((size_t)FB * N));
  CC_HIP(keys_out.ensure((size_t)FB * N));
  CC_HIP(sorted.ensure((size_t)FB * N));
  return CC_OK;
}
cc_status RowSorter::prepare_segmented() {
  if (segmented_ready) return CC_OK;
  const size_t cap = (size_t)FB * N;
  CC_HIP(iota.ensure(cap));
  CC_HIP(offsets.ensure((size_t)FB + 1));
  std::vector<int> off((size_t)FB + 1);
  for (int i = 0; i <= FB; i++) off[(size_t)i] = (int)((size_t)i * N);
  CC_HIP(hipMemcpyAsync(offsets.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, e->stream.s));
  CC_HIP(hipStreamSynchronize(e->stream.s));  // `off` is pageable and about to go out of scope
  hipLaunchKernelGGL(k_iota_rows2, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, e->stream.s, iota.p, cap, N);
  segmented_ready = true;
  return CC_OK;
}
cc_status RowSorter::sort(int nf) {
  if (N <= sort_rows_block_limit()) {  // a row fits one block: sorted in LDS, read once and written once
    // a part that refuses the ~100 KB LDS request (or the launch) takes the device-wide sort below instead of failing
    if (sort_rows_block(e->d_out.p, nf, N, keys_out.p, sorted.p, e->stream.s) == hipSuccess) return CC_OK;
    (void)hipGetLastError();
  }
  if (cc_status st = prepare_segmented(); st != CC_OK) return st;
  const size_t total = (size_t)nf * N;
  size_t temp_bytes = 0;
  CC_HIP(hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, temp_bytes, e->d_out.p, keys_out.p, iota.p, sorted.p, (int)total, nf, offsets.p,
                                                     offsets.p + 1, 0, 32, e->stream.s));
  CC_HIP(temp.ensure(std::max<size_t>(temp_bytes, 1)));
  // stable: equal values keep increasing sample order
  CC_HIP(hipcub::DeviceSegmentedRadixSort::SortPairs(temp.p, temp_bytes, e->d_out.p, keys_out.p, iota.p, sorted.p, (int)total, nf, offsets.p,
                                                     offsets.p + 1, 0, 32, e->stream.s));
  return CC_OK;
}

// ---- what a presort costs in device memory ---------------------------------------------------
// variables per pass: whole groups of 64, at most 2^28 values per scratch array (cc_eval_presort_range's FB before its min with F)
static size_t pass_vars_rule(size_t N) { return std::max<size_t>(64, (((size_t)1 << 28) / N) / 64 * 64); }
struct PresortCosts {
  using u128 = unsigned __int128;
  u128 N, per;  // samples; bytes of a table entry: a float and a 16- or 32-bit sample number
  explicit PresortCosts(size_t n) : N(n), per(4 + (n <= 65536 ? 2 : 4)) {}
  // all tables resident plus one pass's scratch: presort_memory_check's sum for ordered variables
  u128 resident(size_t F) const { return (u128)((F + 63) / 64 * 64) * N * per + (u128)std::min(F, pass_vars_rule((size_t)N)) * N * 16; }
  // a head of R variables (a multiple of 64) with its read-ahead padding; nothing for no head
  u128 head(size_t R) const { return R ? ((u128)R * N + (u128)SPLIT_TABLE_PAD_RANKS * 64) * per : 0; }
  // one chunk of C variables: values, sorted keys, sorted indices and iota (16 B per value, as RowSorter), and the chunk
  // table with its read-ahead padding
  u128 chunk(size_t C) const { return (u128)C * N * 16 + ((u128)C * N + (u128)SPLIT_TABLE_PAD_RANKS * 64) * per; }
  u128 winner() const { return N * 8; }  // the winner row: a float and up to 4 bytes of sample number per sample
  u128 split(size_t R, size_t C) const { return head(R) + chunk(C) + winner(); }
};
// What the evaluator holds for sorted tables and, while a split presort lasts, for streaming.
static size_t held_table_bytes(const cc_evaluator* e) {
  size_t b = e->d_sorted_val.n * 4 + e->d_sorted_idx16.n * 2 + e->d_sorted_idx32.n * 4 + e->d_codes.n + e->d_cat_sorted.n * 4;
  if (e->stream_rows)
    b += e->d_out.n * 4 + e->stream_rows->bytes() + e->d_chunk_val.n * 4 + e->d_chunk_idx16.n * 2 + e->d_chunk_idx32.n * 4 + e->d_win_val.n * 4 +
         e->d_win_idx.n * 4 + e->d_win_state.n * sizeof(StreamBest);
  return b;
}
// A presort with every table resident streams nothing: the chunk scratch of an earlier split presort goes back.
static void release_stream_scratch(cc_evaluator* e) {
  e->stream_rows.reset();
  e->d_chunk_val.release();
  e->d_chunk_idx16.release();
  e->d_chunk_idx32.release();
  e->d_win_val.release();
  e->d_win_idx.release();
  e->presort_chunk = 0;
}

// The resident tables plus one pass's scratch have to fit what is free plus what the evaluator already holds for them
// (the chunk scratch of an earlier split presort is given back first: this presort streams nothing).
static cc_status presort_memory_check(cc_evaluator* e, bool haar, bool cat_table, int F, int N, int FB) {
  release_stream_scratch(e);
  const size_t groups = ((size_t)F + 63) / 64;
  size_t free_b = 0, total_b = 0;
  CC_HIP(hipMemGetInfo(&free_b, &total_b));
  const size_t resident = haar ? groups * 64 * (size_t)N * (4 + (N <= 65536 ? 2 : 4)) : (size_t)F * N + (cat_table ? groups * 64 * ((size_t)N + 3 + SPLIT_CAT_PAD_RANKS) * 4 : 0);
  const size_t have = e->d_sorted_val.n * 4 + e->d_sorted_idx16.n * 2 + e->d_sorted_idx32.n * 4 + e->d_codes.n + e->d_cat_sorted.n * 4 + e->d_out.n * 4;
  const size_t scratch = (size_t)FB * N * (haar || cat_table ? 16 : 4);
  if (resident + scratch > free_b + have)
    return set_error(CC_ERR_UNSUPPORTED, "cc_eval_presort: needs %.1f GB of device memory (%.1f GB free)",
                     (double)(resident + scratch) / 1e9, (double)(free_b + have) / 1e9);
  return CC_OK;
}

// Sorted values and sample numbers (TI: 16-bit while they fit) of the F ordered variables from fi_begin, [group][rank][64].
template <class TI>
static cc_status build_ordered_tables(cc_evaluator* e, RowSorter& rows, const void* feats, int fi_begin, int F, DevBuf<TI>& d_sorted_idx) {
  const int N = rows.N, FB = rows.FB;
  // tables + SPLIT_TABLE_PAD_RANKS ranks of zeroed padding behind the last group (read-ahead of k_split_ord_lean)
  const size_t used = ((size_t)F + 63) / 64 * 64 * (size_t)N, pad = (size_t)SPLIT_TABLE_PAD_RANKS * 64;
  CC_HIP(e->d_sorted_val.ensure(used + pad));
  CC_HIP(hipMemsetAsync(e->d_sorted_val.p + used, 0, pad * sizeof(float), e->stream.s));
  CC_HIP(d_sorted_idx.ensure(used + pad));
  CC_HIP(hipMemsetAsync(d_sorted_idx.p + used, 0, pad * sizeof(TI), e->stream.s));
  for (int f0 = 0; f0 < F; f0 += FB) {
    const int f1 = std::min(F, f0 + FB), nf = f1 - f0;
    if (cc_status st = launch_batch(e, true, feats, fi_begin + f0, fi_begin + f1, nullptr, N, e->d_out.p, 1, 0); st != CC_OK) return st;
    if (cc_status st = rows.sort(nf); st != CC_OK) return st;
    hipLaunchKernelGGL((k_interleave<TI>), dim3((unsigned)((N + 63) / 64), (unsigned)((nf + 63) / 64)), dim3(256), 0, e->stream.s, rows.keys_out.p,
                       rows.sorted.p, nf, N, e->d_sorted_val.p, d_sorted_idx.p, (size_t)f0 / 64);
    CC_HIP(hipGetLastError());
  }
  return CC_OK;
}

// Ordered variables (Haar, HOG), every table resident.
template <class TI>
static cc_status presort_ordered(cc_evaluator* e, RowSorter& rows, const void* feats, int fi_begin, int F, DevBuf<TI>& d_sorted_idx) {
  e->presort_resident = F;
  return build_ordered_tables(e, rows, feats, fi_begin, F, d_sorted_idx);
}

// Categorical variables (LBP): the codes [variable][sample] and, with cat_table, the (code, sample)-sorted table beside them.
static cc_status presort_categorical(cc_evaluator* e, RowSorter& rows, const void* feats, int fi_begin, int F, bool cat_table) {
  const int N = rows.N, FB = rows.FB;
  e->presort_resident = F;
  CC_HIP(e->d_codes.ensure((size_t)F * N));
  if (cat_table) {
    // ranks padded to a multiple of 4 per group (the tail of a group's last quad is never summed: r >= n_pre); zeroed
    // padding behind the last group for the read-ahead
    const size_t used = ((size_t)F + 63) / 64 * 64 * ((((size_t)N + 3) >> 2) << 2), pad = (size_t)SPLIT_CAT_PAD_RANKS * 64;
    CC_HIP(e->d_cat_sorted.ensure(used + pad));
    CC_HIP(hipMemsetAsync(e->d_cat_sorted.p, 0, (used + pad) * sizeof(uint32_t), e->stream.s));
  }
  for (int f0 = 0; f0 < F; f0 += FB) {
    const int f1 = std::min(F, f0 + FB), nf = f1 - f0;
    const size_t total = (size_t)nf * N;
    CC_HIP(e->d_out.ensure(total));
    if (cc_status st = launch_batch(e, false, feats, fi_begin + f0, fi_begin + f1, nullptr, N, e->d_out.p, 1, 0); st != CC_OK) return st;
    hipLaunchKernelGGL(k_codes_u8, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, e->stream.s, e->d_out.p,
                       e->d_codes.p + (size_t)f0 * N, total);
    if (!cat_table) continue;
    if (cc_status st = rows.sort(nf); st != CC_OK) return st;
    hipLaunchKernelGGL(k_interleave_cat, dim3((unsigned)((N + 63) / 64), (unsigned)((nf + 63) / 64)), dim3(256), 0, e->stream.s, rows.keys_out.p,
                       rows.sorted.p, nf, N, e->d_cat_sorted.p, (size_t)f0 / 64);
  }
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
// ev_a and ev_b on the evaluator's stream.
// One table of n_vars sorted variables ([group][rank][64] with its read-ahead padding: the resident table or a chunk's)
// whose first variable is number var_offset (a multiple of 64) of the presorted range: results at that offset of OrdResult.
static cc_status launch_ordered_table(cc_evaluator* e, int mode, TableForm form, double w_total0, double w_total1, double rsum0, const float* sv,
                                      const void* si, int n_vars, int var_offset) {
  const int N = e->presort_n, F = e->presort_f1 - e->presort_f0;
  const bool idx16 = N <= 65536;
  const size_t groups = ((size_t)n_vars + 63) / 64, fpad = ((size_t)F + 63) / 64 * 64;
  const OrdResult dev(e->d_split_out.p, fpad);
  // in the struct's order: sv, si, tab, n_pre, n_vars, w_total0, w_total1, rsum0, best_val, best_i, best_vl, best_vr, n_groups, dbg_nogather
  const SplitOrdArgs A{sv, si, reinterpret_cast<const SplitEntry*>(e->d_split_tab.p), N, n_vars, w_total0, w_total1, rsum0,
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
  if (cc_status st = launch(ordered_kernel(mode, form, idx16), blocks, 64u * wpb, table_lds(form, N), e->stream.s, A); st != CC_OK) return st;
  (void)hipEventRecord(e->ev_b.e, e->stream.s);
  return CC_OK;
}

// The leader after the variables [v0, v1) of OrdResult (k_stream_winner); tab_val / tab_idx: the chunk table they were
// searched in, or NULL for the head, whose rows stay where they are.
template <class TI>
static cc_status launch_stream_winner(cc_evaluator* e, int v0, int v1, bool reset, const float* tab_val, const TI* tab_idx) {
  const size_t fpad = ((size_t)(e->presort_f1 - e->presort_f0) + 63) / 64 * 64;
  const OrdResult dev(e->d_split_out.p, fpad);
  hipLaunchKernelGGL((k_stream_winner<TI>), dim3(1), dim3(1024), 0, e->stream.s, dev.best_val, dev.best_i, v0, v1, reset ? 1 : 0, tab_val, tab_idx,
                     e->presort_n, e->d_win_state.p, e->d_win_val.p, reinterpret_cast<TI*>(e->d_win_idx.p));
  CC_HIP(hipGetLastError());
  return CC_OK;
}

// The streamed tail of a node's search: per chunk, in variable order, what cc_eval_presort does once per stage for a
// resident variable -- evaluate (launch_batch), stable row sort (RowSorter), k_interleave into the chunk table -- then the
// ordered kernel over that table. The reference does the same for a variable outside its caches at every node
// (CvCascadeBoostTrainData::get_ord_var_data, o_cvcascadeboosttraindata.cpp:437-458). Nothing waits on the host.
template <class TI>
static cc_status stream_ordered_tail(cc_evaluator* e, int mode, TableForm form, double w_total0, double w_total1, double rsum0, bool track_winner,
                                     DevBuf<TI>& d_chunk_idx) {
  const int N = e->presort_n, F = e->presort_f1 - e->presort_f0, R = e->presort_resident, C = e->presort_chunk;
  RowSorter& rows = *e->stream_rows;
  const size_t pad = (size_t)SPLIT_TABLE_PAD_RANKS * 64;
  if (track_winner && R > 0)
    if (cc_status st = launch_stream_winner<TI>(e, 0, R, true, nullptr, nullptr); st != CC_OK) return st;
  e->stream_ev_used = 0;
  auto mark = [&]() -> cc_status {  // profiling only: one more event in the stream, no host wait
    if (!e->stream_profile) return CC_OK;
    if (e->stream_ev_used == e->stream_ev.size()) {
      e->stream_ev.emplace_back();
      CC_HIP(e->stream_ev.back().create());
    }
    CC_HIP(hipEventRecord(e->stream_ev[e->stream_ev_used++].e, e->stream.s));
    return CC_OK;
  };
  for (int c0 = R; c0 < F; c0 += C) {
    const int nf = std::min(C, F - c0);
    if (cc_status st = mark(); st != CC_OK) return st;
    if (cc_status st = launch_batch(e, true, e->d_haar.p, e->presort_f0 + c0, e->presort_f0 + c0 + nf, nullptr, N, e->d_out.p, 1, 0); st != CC_OK) return st;
    if (cc_status st = mark(); st != CC_OK) return st;
    if (cc_status st = rows.sort(nf); st != CC_OK) return st;
    if (cc_status st = mark(); st != CC_OK) return st;
    const size_t groups = ((size_t)nf + 63) / 64, used = groups * 64 * (size_t)N;
    hipLaunchKernelGGL((k_interleave<TI>), dim3((unsigned)((N + 63) / 64), (unsigned)groups), dim3(256), 0, e->stream.s, rows.keys_out.p, rows.sorted.p, nf, N,
                       e->d_chunk_val.p, d_chunk_idx.p, (size_t)0);
    CC_HIP(hipGetLastError());
    if (nf < C) {  // a short last chunk: the zeroed read-ahead padding stands behind ITS last group (a full chunk's was zeroed by the presort)
      CC_HIP(hipMemsetAsync(e->d_chunk_val.p + used, 0, pad * sizeof(float), e->stream.s));
      CC_HIP(hipMemsetAsync(d_chunk_idx.p + used, 0, pad * sizeof(TI), e->stream.s));
    }
    if (cc_status st = mark(); st != CC_OK) return st;
    if (cc_status st = launch_ordered_table(e, mode, form, w_total0, w_total1, rsum0, e->d_chunk_val.p, d_chunk_idx.p, nf, c0); st != CC_OK) return st;
    if (cc_status st = mark(); st != CC_OK) return st;
    if (track_winner)
      if (cc_status st = launch_stream_winner<TI>(e, c0, c0 + nf, c0 == 0, e->d_chunk_val.p, d_chunk_idx.p); st != CC_OK) return st;
    if (cc_status st = mark(); st != CC_OK) return st;
  }
  return CC_OK;
}

cc_status ccamd::split_launch_ordered(cc_evaluator* e, int mode, TableForm form, double w_total0, double w_total1, double rsum0, bool track_winner) {
  const int N = e->presort_n, F = e->presort_f1 - e->presort_f0, R = e->presort_resident;
  const bool idx16 = N <= 65536;
  CC_HIP(e->d_split_out.ensure(((size_t)F + 63) / 64 * 64 * 3));  // OrdResult::bytes + slack
  const void* head_idx = idx16 ? (const void*)e->d_sorted_idx16.p : (const void*)e->d_sorted_idx32.p;
  if (R >= F) return launch_ordered_table(e, mode, form, w_total0, w_total1, rsum0, e->d_sorted_val.p, head_idx, F, 0);
  (void)hipEventRecord(e->ev_stream_a.e, e->stream.s);
  if (R > 0)
    if (cc_status st = launch_ordered_table(e, mode, form, w_total0, w_total1, rsum0, e->d_sorted_val.p, head_idx, R, 0); st != CC_OK) return st;
  const cc_status st = idx16 ? stream_ordered_tail(e, mode, form, w_total0, w_total1, rsum0, track_winner, e->d_chunk_idx16)
                             : stream_ordered_tail(e, mode, form, w_total0, w_total1, rsum0, track_winner, e->d_chunk_idx32);
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
  const bool stream_only = std::getenv("CCAMD_SPLIT_CAT_STREAM") != nullptr;  // read per call: tests compare the two paths
  const bool sorted = ascending && q.e->cat_sorted_n == q.N && !stream_only;
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

// The split presort of ordered variables with 16- or 32-bit sample numbers: head tables, chunk table, winner row.
template <class TI>
static cc_status presort_split_ordered(cc_evaluator* e, int fi_begin, int R, int C, DevBuf<TI>& d_sorted_idx, DevBuf<TI>& d_chunk_idx) {
  RowSorter& rows = *e->stream_rows;
  const size_t N = (size_t)rows.N, pad = (size_t)SPLIT_TABLE_PAD_RANKS * 64;
  if (R > 0)
    if (cc_status st = build_ordered_tables(e, rows, e->d_haar.p, fi_begin, R, d_sorted_idx); st != CC_OK) return st;
  // the whole chunk table zeroed once: a full chunk's read-ahead padding is never written again
  CC_HIP(e->d_chunk_val.ensure((size_t)C * N + pad));
  CC_HIP(hipMemsetAsync(e->d_chunk_val.p, 0, ((size_t)C * N + pad) * sizeof(float), e->stream.s));
  CC_HIP(d_chunk_idx.ensure((size_t)C * N + pad));
  CC_HIP(hipMemsetAsync(d_chunk_idx.p, 0, ((size_t)C * N + pad) * sizeof(TI), e->stream.s));
  CC_HIP(e->d_win_val.ensure(N));
  CC_HIP(e->d_win_idx.ensure(N));
  CC_HIP(e->d_win_state.ensure(1));
  CC_HIP(hipMemsetAsync(e->d_win_val.p, 0, N * 4, e->stream.s));
  CC_HIP(hipMemsetAsync(e->d_win_idx.p, 0, N * 4, e->stream.s));
  CC_HIP(hipMemsetAsync(e->d_win_state.p, 0, sizeof(StreamBest), e->stream.s));
  return CC_OK;
}

extern "C" {

cc_status cc_eval_presort_range(cc_evaluator* e, int fi_begin, int fi_end, int n_samples) {
  if (!e) return set_error(CC_ERR_INVALID_ARG, "cc_eval_presort: null evaluator");
  if (n_samples < 1 || n_samples > e->max_samples)
    return set_error(CC_ERR_OUT_OF_RANGE, "cc_eval_presort: n_samples %d out of range (max_samples %d)", n_samples, e->max_samples);
  if (fi_begin < 0 || fi_end > e->nfeat || fi_begin >= fi_end)
    return set_error(CC_ERR_OUT_OF_RANGE, "cc_eval_presort: features [%d, %d) out of range (%d)", fi_begin, fi_end, e->nfeat);
  if (cc_status st = eval_device(e); st != CC_OK) return st;
  std::lock_guard<std::mutex> lk(e->mu);
  if (cc_status st = flush_pending_images(e); st != CC_OK) return st;
  e->presort_n = 0;  // until the epilogue: a failure below leaves no tables to search
  e->generation++;   // a booster created over the earlier tables refuses its next round
  const bool haar = e->type != CC_FEATURE_LBP;  // HOG variables are ordered: the Haar tables (launch_batch dispatches HOG)
  const int F = fi_end - fi_begin, N = n_samples;
  const void* feats = haar ? (const void*)e->d_haar.p : (const void*)e->d_lbp.p;
  // variables per pass: whole groups of 64, at most 2^28 values per scratch array
  const int FB = (int)std::min<size_t>((size_t)F, std::max<size_t>(64, (((size_t)1 << 28) / (size_t)N) / 64 * 64));
  // LBP keeps the (code, sample)-sorted table of k_split_cat_sorted beside the codes while sample numbers fit 24 bits
  const bool no_cat_table = std::getenv("CCAMD_SPLIT_CAT_STREAM") != nullptr;  // A/B: round-1 categorical search only
  const bool cat_table = !haar && N < (1 << 24) && !no_cat_table;
  if (cc_status st = presort_memory_check(e, haar, cat_table, F, N, FB); st != CC_OK) return st;
  RowSorter rows(e, N, FB);
  if (haar || cat_table)
    if (cc_status st = rows.init(); st != CC_OK) return st;
  const cc_status st = !haar        ? presort_categorical(e, rows, feats, fi_begin, F, cat_table)
                       : N <= 65536 ? presort_ordered(e, rows, feats, fi_begin, F, e->d_sorted_idx16)
                                    : presort_ordered(e, rows, feats, fi_begin, F, e->d_sorted_idx32);
  if (st != CC_OK) return st;
  CC_HIP(hipStreamSynchronize(e->stream.s));
  // epilogue: the tables are valid
  e->presort_n = N;
  e->presort_f0 = fi_begin;
  e->presort_f1 = fi_end;
  e->cat_sorted_n = cat_table ? N : 0;
  return CC_OK;
}

cc_status cc_eval_presort(cc_evaluator* e, int n_samples) {
  if (!e) return set_error(CC_ERR_INVALID_ARG, "cc_eval_presort: null evaluator");
  return cc_eval_presort_range(e, 0, e->nfeat, n_samples);
}

cc_status cc_presort_plan(int feature_type, int n_vars, int n_samples, uint64_t budget_bytes, int* resident_vars, int* chunk_vars,
                          uint64_t* bytes_needed) {
  if (!resident_vars || !chunk_vars || !bytes_needed) return set_error(CC_ERR_INVALID_ARG, "cc_presort_plan: null argument");
  if (feature_type != CC_FEATURE_HAAR && feature_type != CC_FEATURE_LBP && feature_type != CC_FEATURE_HOG)
    return set_error(CC_ERR_INVALID_ARG, "cc_presort_plan: unknown feature type %d", feature_type);
  if (n_vars < 1 || n_samples < 1) return set_error(CC_ERR_OUT_OF_RANGE, "cc_presort_plan: %d variables, %d samples", n_vars, n_samples);
  *resident_vars = *chunk_vars = 0;
  *bytes_needed = 0;
  if (budget_bytes == 0) {  // what the device has free now
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
      (void)hipGetLastError();
      return set_error(CC_ERR_NO_DEVICE, "cc_presort_plan: budget_bytes = 0 asks the device for its free memory, and there is no usable HIP device");
    }
    budget_bytes = free_b;
  }
  using u128 = PresortCosts::u128;
  const size_t F = (size_t)n_vars, N = (size_t)n_samples;
  const u128 budget = budget_bytes, top = ~(uint64_t)0;
  if (feature_type == CC_FEATURE_LBP) {  // presort_memory_check's sum for categorical variables
    const bool cat_table = N < ((size_t)1 << 24) && !std::getenv("CCAMD_SPLIT_CAT_STREAM");
    const u128 need = (u128)F * N + (cat_table ? (u128)((F + 63) / 64 * 64) * (N + 3 + SPLIT_CAT_PAD_RANKS) * 4 : 0) +
                      (u128)std::min(F, pass_vars_rule(N)) * N * (cat_table ? 16 : 4);
    if (need > budget)
      return set_error(CC_ERR_UNSUPPORTED, "cc_presort_plan: categorical variables are not streamed, and their tables need %.0f bytes (budget %.0f)",
                       (double)need, (double)budget);
    *resident_vars = n_vars;
    *bytes_needed = (uint64_t)need;
    return CC_OK;
  }
  const PresortCosts cost(N);
  if (cost.resident(F) <= budget) {
    *resident_vars = n_vars;
    *bytes_needed = (uint64_t)cost.resident(F);
    return CC_OK;
  }
  if (cost.split(0, 64) > budget)
    return set_error(CC_ERR_UNSUPPORTED, "cc_presort_plan: a budget of %llu bytes holds neither every table nor one chunk of 64 variables x %d samples; the smallest budget that works is %llu",
                     (unsigned long long)budget_bytes, n_samples, (unsigned long long)std::min({cost.split(0, 64), cost.resident(F), top}));
  // Everything but the last group resident needs a chunk of 64 only (a chunk is never larger than the tail).
  const size_t r_max = (F - 1) / 64 * 64;
  if (cost.split(r_max, 64) <= budget) {
    *resident_vars = (int)r_max;
    *chunk_vars = 64;
    *bytes_needed = (uint64_t)cost.split(r_max, 64);
    return CC_OK;
  }
  // Otherwise the chunk first, up to the pass rule, and a head only beside a chunk of that size: a head that shrank
  // whenever the chunk grew by a group would not be monotone in the budget. u128 sums: nothing below can wrap.
  const size_t c_rule = std::min((F + 63) / 64 * 64, pass_vars_rule(N));
  const u128 per_chunk_group = cost.chunk(128) - cost.chunk(64);  // 64 variables more
  const size_t C = (size_t)std::min<u128>(c_rule, 64 + (budget - cost.split(0, 64)) / per_chunk_group * 64);
  const u128 left = budget - cost.split(0, C), pad_bytes = cost.head(64) - (u128)64 * N * cost.per;
  const size_t R = C == c_rule && left > pad_bytes ? (size_t)std::min<u128>((left - pad_bytes) / ((u128)64 * N * cost.per) * 64, (F - 1) / 64 * 64) : 0;
  *resident_vars = (int)R;
  *chunk_vars = (int)C;
  *bytes_needed = (uint64_t)cost.split(R, C);
  return CC_OK;
}

cc_status cc_eval_table_bytes(cc_evaluator* e, uint64_t* bytes) {
  if (!e || !bytes) return set_error(CC_ERR_INVALID_ARG, "cc_eval_table_bytes: null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  *bytes = held_table_bytes(e);
  return CC_OK;
}

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

cc_status cc_eval_presort_budget(cc_evaluator* e, uint64_t* bytes) {
  if (!e || !bytes) return set_error(CC_ERR_INVALID_ARG, "cc_eval_presort_budget: null argument");
  if (cc_status st = eval_device(e); st != CC_OK) return st;
  std::lock_guard<std::mutex> lk(e->mu);
  size_t free_b = 0, total_b = 0;
  CC_HIP(hipMemGetInfo(&free_b, &total_b));
  *bytes = (uint64_t)free_b + held_table_bytes(e);
  return CC_OK;
}

cc_status cc_eval_presort_split(cc_evaluator* e, int fi_begin, int fi_end, int n_samples, int resident_vars, int chunk_vars) {
  if (!e) return set_error(CC_ERR_INVALID_ARG, "cc_eval_presort_split: null evaluator");
  if (n_samples < 1 || n_samples > e->max_samples)
    return set_error(CC_ERR_OUT_OF_RANGE, "cc_eval_presort_split: n_samples %d out of range (max_samples %d)", n_samples, e->max_samples);
  if (fi_begin < 0 || fi_end > e->nfeat || fi_begin >= fi_end)
    return set_error(CC_ERR_OUT_OF_RANGE, "cc_eval_presort_split: features [%d, %d) out of range (%d)", fi_begin, fi_end, e->nfeat);
  const int F = fi_end - fi_begin, N = n_samples, R = resident_vars;
  if (R == F) return cc_eval_presort_range(e, fi_begin, fi_end, n_samples);  // nothing is streamed: today's presort
  if (R < 0 || R > F || R % 64 != 0)
    return set_error(CC_ERR_INVALID_ARG, "cc_eval_presort_split: resident_vars %d is neither a multiple of 64 in [0, %d] nor %d", R, F, F);
  if (chunk_vars < 64 || chunk_vars % 64 != 0)
    return set_error(CC_ERR_INVALID_ARG, "cc_eval_presort_split: chunk_vars %d is not a multiple of 64 of at least 64", chunk_vars);
  if (e->type == CC_FEATURE_LBP)
    return set_error(CC_ERR_UNSUPPORTED, "cc_eval_presort_split: categorical variables are not streamed (LBP takes resident_vars = %d only)", F);
  if (cc_status st = eval_device(e); st != CC_OK) return st;
  std::lock_guard<std::mutex> lk(e->mu);
  if (cc_status st = flush_pending_images(e); st != CC_OK) return st;
  e->presort_n = 0;  // until the epilogue: a failure below leaves no tables to search
  e->generation++;   // a booster created over the earlier tables refuses its next round
  // no chunk larger than the tail or than a pass of the full presort (at most 2^28 values per scratch array)
  const int C = (int)std::min<size_t>({(size_t)chunk_vars, ((size_t)(F - R) + 63) / 64 * 64, pass_vars_rule((size_t)N)});
  // Exactly what the plan counts is held afterwards: larger buffers of an earlier presort go back first.
  const PresortCosts cost((size_t)N);
  const size_t pad = (size_t)SPLIT_TABLE_PAD_RANKS * 64, head_n = R ? (size_t)R * N + pad : 0, chunk_n = (size_t)C * N;
  const bool idx16 = N <= 65536;
  release_stream_scratch(e);
  if (e->d_sorted_val.n > head_n) e->d_sorted_val.release();
  if (e->d_sorted_idx16.n > (idx16 ? head_n : 0)) e->d_sorted_idx16.release();
  if (e->d_sorted_idx32.n > (idx16 ? 0 : head_n)) e->d_sorted_idx32.release();
  if (e->d_out.n > chunk_n) e->d_out.release();
  size_t free_b = 0, total_b = 0;
  CC_HIP(hipMemGetInfo(&free_b, &total_b));
  const size_t have = e->d_sorted_val.n * 4 + e->d_sorted_idx16.n * 2 + e->d_sorted_idx32.n * 4 + e->d_out.n * 4;
  if (cost.split((size_t)R, (size_t)C) > (PresortCosts::u128)free_b + have)
    return set_error(CC_ERR_UNSUPPORTED, "cc_eval_presort_split: needs %.1f GB of device memory (%.1f GB free)",
                     (double)cost.split((size_t)R, (size_t)C) / 1e9, (double)(free_b + have) / 1e9);
  if (!e->ev_stream_a.e) CC_HIP(e->ev_stream_a.create());
  e->stream_rows.reset(new RowSorter(e, N, C));
  if (cc_status st = e->stream_rows->init(); st != CC_OK) return st;
  if (N > sort_rows_block_limit())  // the segmented sort's offsets and iota now, not inside the first node's search
    if (cc_status st = e->stream_rows->prepare_segmented(); st != CC_OK) return st;
  const cc_status st = idx16 ? presort_split_ordered(e, fi_begin, R, C, e->d_sorted_idx16, e->d_chunk_idx16)
                             : presort_split_ordered(e, fi_begin, R, C, e->d_sorted_idx32, e->d_chunk_idx32);
  if (st != CC_OK) return st;
  CC_HIP(hipStreamSynchronize(e->stream.s));
  // epilogue: the head's tables are valid
  e->presort_n = N;
  e->presort_f0 = fi_begin;
  e->presort_f1 = fi_end;
  e->cat_sorted_n = 0;
  e->presort_resident = R;
  e->presort_chunk = C;
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
