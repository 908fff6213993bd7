// Filling a stage's training set on gfx950 (section 6c of the C ABI): the loop of CvCascadeClassifier::fillPassedSamples
// (cascadeclassifier.cpp:329-357) over pass flags that are already on the device. The loop takes candidates in order, keeps
// the ones that pass, and stops when it has `want` of them, when the acceptance ratio has fallen to its bound, or when the
// candidates run out. Here: a count of the flags before every position (reduce per block, scan of the block totals, apply),
// the first position at which one of the three stop conditions holds, and the list of the positions kept before it.
// No block waits for another one: the three steps are separate launches. cc_negminer_fill (cc_negmine.hip) runs this over the
// mined window stream; cc_eval_fill_passed below runs it over packed candidates (the positives).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>

#include "cc_eval_internal.h"

namespace ccamd {

constexpr int FILL_THREADS = 256;
constexpr int FILL_PER_THREAD = 4;
constexpr int FILL_TILE = FILL_THREADS * FILL_PER_THREAD;  // positions per block
constexpr unsigned long long FILL_NO_STOP = ~0ull;

// The flags of the tile's positions base + r * 256 + thread (r < 4; beyond n: not set) and, in rank[r], how many flags
// of the tile are set before that position. Returns the tile's total. A wavefront's 64 flags are one ballot; the 16
// wavefront totals (4 per r) are summed in position order. One call per kernel (the LDS array is not fenced behind it).
__device__ __forceinline__ int fill_tile_ranks(const uint8_t* __restrict__ flags, long long n, long long base, bool (&flag)[FILL_PER_THREAD],
                                               int (&rank)[FILL_PER_THREAD]) {
  __shared__ int wave_total[FILL_PER_THREAD * (FILL_THREADS / 64)];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < FILL_PER_THREAD; r++) {
    const long long pos = base + r * FILL_THREADS + threadIdx.x;
    flag[r] = pos < n && flags[pos] != 0;
    const unsigned long long b = __ballot(flag[r]);
    rank[r] = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[r * (FILL_THREADS / 64) + wave] = __popcll(b);
  }
  __syncthreads();
  int acc = 0;
#pragma unroll
  for (int k = 0; k < FILL_PER_THREAD * (FILL_THREADS / 64); k++) {
#pragma unroll
    for (int r = 0; r < FILL_PER_THREAD; r++)
      if (k == r * (FILL_THREADS / 64) + wave) rank[r] += acc;
    acc += wave_total[k];
  }
  return acc;
}

// (a) reduce: flags set in block b's tile of [start, n]
__global__ __launch_bounds__(FILL_THREADS) void k_fill_reduce(const uint8_t* __restrict__ flags, long long n, long long start,
                                                              long long* __restrict__ block) {
  bool flag[FILL_PER_THREAD];
  int rank[FILL_PER_THREAD];
  const int total = fill_tile_ranks(flags, n, start + (long long)blockIdx.x * FILL_TILE, flag, rank);
  if (threadIdx.x == 0) block[blockIdx.x] = total;
}

// (a) scan of the block totals, in place, exclusive: one wavefront, 64 totals per step with the carry of the steps before
__global__ __launch_bounds__(64) void k_fill_scan_blocks(long long* __restrict__ block, int nb) {
  const int lane = threadIdx.x;
  long long carry = 0;
  for (int i0 = 0; i0 < nb; i0 += 64) {
    const int i = i0 + lane;
    const long long v = i < nb ? block[i] : 0;
    long long incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (i < nb) block[i] = carry + incl - v;
    carry += __shfl(incl, 63);
  }
}

// The reason the loop stops at stream position pos with P flags set in [start, pos), or -1 if it goes on: in the order of
// the reference's checks (cascadeclassifier.cpp:333, :337, :342).
__device__ __forceinline__ int fill_stop_reason(long long pos, long long P, long long n, long long start, int want, long long g0, long long c0,
                                                double ratio) {
  if (P >= want) return CC_FILL_FILLED;
  const long long c = c0 + (pos - start), g = g0 + P;
  if (c != 0 && (double)(g + 1) / (double)c <= ratio) return CC_FILL_RATIO;
  return pos == n ? CC_FILL_EXHAUSTED : -1;
}

// (b) apply + the first stop: every position of [start, n] (n itself: one past the end, where the stream is exhausted)
__global__ __launch_bounds__(FILL_THREADS) void k_fill_first_stop(const uint8_t* __restrict__ flags, long long n, long long start, int want,
                                                                  long long g0, long long c0, double ratio,
                                                                  const long long* __restrict__ block, FillRecord* __restrict__ rec) {
  bool flag[FILL_PER_THREAD];
  int rank[FILL_PER_THREAD];
  const long long base = start + (long long)blockIdx.x * FILL_TILE;
  fill_tile_ranks(flags, n, base, flag, rank);
  const long long before = block[blockIdx.x];
  unsigned long long first = FILL_NO_STOP;
#pragma unroll
  for (int r = 0; r < FILL_PER_THREAD; r++) {
    const long long pos = base + r * FILL_THREADS + threadIdx.x;
    if (pos > n) continue;
    const int why = fill_stop_reason(pos, before + rank[r], n, start, want, g0, c0, ratio);
    if (why >= 0) first = min(first, (unsigned long long)pos * 4ull + (unsigned)why);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) first = min(first, (unsigned long long)__shfl_xor((long long)first, d));
  if ((threadIdx.x & 63) == 0 && first != FILL_NO_STOP) atomicMin(&rec->stop, first);
}

// (c) the keep list: the set flags before the stop, by rank; the count at the stop is n_filled
__global__ __launch_bounds__(FILL_THREADS) void k_fill_keep(const uint8_t* __restrict__ flags, long long n, long long start,
                                                            int want, const long long* __restrict__ block, FillRecord* rec,
                                                            long long* __restrict__ keep) {
  const long long stop = (long long)(rec->stop >> 2);
  const long long base = start + (long long)blockIdx.x * FILL_TILE;
  if (base > stop) return;  // the whole block
  bool flag[FILL_PER_THREAD];
  int rank[FILL_PER_THREAD];
  fill_tile_ranks(flags, n, base, flag, rank);
  const long long before = block[blockIdx.x];
#pragma unroll
  for (int r = 0; r < FILL_PER_THREAD; r++) {
    const long long pos = base + r * FILL_THREADS + threadIdx.x;
    // before the stop fewer than `want` flags are set (the loop would have stopped): the bound only restates it
    if (pos < stop && flag[r] && before + rank[r] < want) keep[before + rank[r]] = pos;
    if (pos == stop) rec->n_filled = (int)(before + rank[r]);
  }
}

// rows of the scratch tables -> their slots: one block per kept row
struct CopyRowsArgs {
  const long long* keep;  // scratch row of kept candidate r
  int first_slot, cols;
  const int32_t *sum_src, *tilted_src;
  int32_t *sum_dst, *tilted_dst;
  const float *nf_src, *hog_src;
  float *nf_dst, *hog_dst;
};
__global__ __launch_bounds__(256) void k_fill_copy_rows(CopyRowsArgs A) {
  const size_t src = (size_t)A.keep[blockIdx.x], dst = (size_t)A.first_slot + blockIdx.x;
  if (A.hog_src) {
    const size_t len = (size_t)A.cols * 10;
    for (size_t i = threadIdx.x; i < len; i += 256) A.hog_dst[dst * len + i] = A.hog_src[src * len + i];
    return;
  }
  for (int i = threadIdx.x; i < A.cols; i += 256) {
    A.sum_dst[dst * A.cols + i] = A.sum_src[src * A.cols + i];
    if (A.tilted_src) A.tilted_dst[dst * A.cols + i] = A.tilted_src[src * A.cols + i];
  }
  if (A.nf_src && threadIdx.x == 0) A.nf_dst[dst] = A.nf_src[src];
}

cc_status fill_select(FillWork& w, const uint8_t* d_flags, long long n, long long start, int want, long long got_before,
                      long long consumed_before, double ratio, hipStream_t st, FillResult* out) {
  const long long nb64 = (n - start + 1 + FILL_TILE - 1) / FILL_TILE;
  if (nb64 > 0x7fffffffLL) return set_error(CC_ERR_OUT_OF_RANGE, "fill: %lld stream positions are more than one launch covers", n - start);
  const int nb = (int)nb64;
  CC_HIP(w.d_block.ensure((size_t)nb));
  CC_HIP(w.d_keep.ensure((size_t)std::max(want, 1)));
  CC_HIP(w.d_rec.ensure(1));
  CC_HIP(w.h_rec.ensure(sizeof(FillRecord)));
  CC_HIP(hipMemsetAsync(w.d_rec.p, 0xff, sizeof(FillRecord), st));
  hipLaunchKernelGGL(k_fill_reduce, dim3(nb), dim3(FILL_THREADS), 0, st, d_flags, n, start, w.d_block.p);
  hipLaunchKernelGGL(k_fill_scan_blocks, dim3(1), dim3(64), 0, st, w.d_block.p, nb);
  hipLaunchKernelGGL(k_fill_first_stop, dim3(nb), dim3(FILL_THREADS), 0, st, d_flags, n, start, want, got_before, consumed_before, ratio,
                     w.d_block.p, w.d_rec.p);
  hipLaunchKernelGGL(k_fill_keep, dim3(nb), dim3(FILL_THREADS), 0, st, d_flags, n, start, want, w.d_block.p, w.d_rec.p, w.d_keep.p);
  CC_HIP(hipGetLastError());
  CC_HIP(copy_sync(w.h_rec.p, w.d_rec.p, sizeof(FillRecord), hipMemcpyDeviceToHost, st));
  const FillRecord rec = *static_cast<const FillRecord*>(w.h_rec.p);
  if (rec.stop == FILL_NO_STOP || rec.n_filled < 0 || rec.n_filled > want)
    return set_error(CC_ERR_HIP, "fill: the selection kernels left no stop record");
  out->n_filled = rec.n_filled;
  out->stop = (int)(rec.stop & 3);
  out->n_consumed = (long long)(rec.stop >> 2) - start;
  return CC_OK;
}

namespace {

constexpr int FILL_CHUNK = 2048;  // candidates set, predicted and selected per step of cc_eval_fill_passed

}  // namespace

}  // namespace ccamd

using namespace ccamd;

extern "C" {

int cc_debug_fill_scan_tile(void) { return FILL_TILE; }

cc_status cc_debug_fill_select(int device, const uint8_t* flags, int64_t n, int64_t start, int want, int64_t got_before,
                               int64_t consumed_before, double ratio, int* n_filled, int64_t* n_consumed, int* stop, int64_t* keep_index) {
  if ((!flags && n > 0) || !n_filled || !n_consumed || !stop) return set_error(CC_ERR_INVALID_ARG, "cc_debug_fill_select: null argument");
  if (n < 0 || start < 0 || start > n || want < 0) return set_error(CC_ERR_INVALID_ARG, "cc_debug_fill_select: bad range");
  cc_status st = ensure_device(device);
  if (st != CC_OK) return st;
  OwnStream s;
  CC_HIP(s.create());
  DevBuf<uint8_t> d_flags;
  FillWork w;
  CC_HIP(d_flags.ensure((size_t)std::max<int64_t>(n, 1)));
  if (n > 0) CC_HIP(hipMemcpyAsync(d_flags.p, flags, (size_t)n, hipMemcpyHostToDevice, s.s));
  FillResult r;
  st = fill_select(w, d_flags.p, n, start, want, got_before, consumed_before, ratio, s.s, &r);
  if (st != CC_OK) return st;
  if (keep_index && r.n_filled > 0)
    CC_HIP(copy_sync(keep_index, w.d_keep.p, (size_t)r.n_filled * sizeof(int64_t), hipMemcpyDeviceToHost, s.s));
  *n_filled = r.n_filled;
  *n_consumed = r.n_consumed;
  *stop = r.stop;
  return CC_OK;
}

cc_status cc_eval_fill_passed(cc_evaluator* e, const cc_cascade* stages, const uint8_t* imgs, int n_imgs, int first_idx, int want,
                              uint8_t label, int* n_filled, int64_t* n_consumed) {
  if (!e || (!imgs && n_imgs > 0) || !n_filled || !n_consumed) return set_error(CC_ERR_INVALID_ARG, "cc_eval_fill_passed: null argument");
  if (n_imgs < 0) return set_error(CC_ERR_INVALID_ARG, "cc_eval_fill_passed: negative candidate count");
  if (first_idx < 0 || want < 0 || (long long)first_idx + want > e->max_samples)
    return set_error(CC_ERR_OUT_OF_RANGE, "cc_eval_fill_passed: samples [%d, %lld) exceed max_samples %d", first_idx, (long long)first_idx + want,
                     e->max_samples);
  cc_status st = stages ? predict_check(e, stages->m, "cc_eval_fill_passed") : CC_OK;
  if (st != CC_OK) return st;
  st = eval_device(e);
  if (st != CC_OK) return st;
  *n_filled = 0;
  *n_consumed = 0;
  if (want == 0 || n_imgs == 0) return CC_OK;
  std::lock_guard<std::mutex> lk(e->mu);
  st = flush_pending_images(e);
  if (st != CC_OK) return st;
  const bool hog = e->type == CC_FEATURE_HOG, haar = e->type == CC_FEATURE_HAAR;
  const size_t px = (size_t)e->W * e->H, cols = (size_t)e->cols;
  const int chunk = std::min(n_imgs, FILL_CHUNK);
  SampleTables& rows = e->fill_rows;  // rows 0 .. chunk: the candidates are set and predicted here
  if (hog)
    CC_HIP(rows.hog.ensure((size_t)chunk * cols * 10));
  else {
    CC_HIP(rows.sum.ensure((size_t)chunk * cols));
    if (e->use_tilted) CC_HIP(rows.tilted.ensure((size_t)chunk * cols));
    if (haar) CC_HIP(rows.nf.ensure((size_t)chunk));
  }
  CC_HIP(e->d_imgs.ensure((size_t)chunk * px));
  CC_HIP(e->d_pred.ensure((size_t)chunk));
  int got = 0;
  long long consumed = 0;
  for (int c0 = 0; c0 < n_imgs && got < want; c0 += chunk) {
    const int n = std::min(chunk, n_imgs - c0);
    CC_HIP(hipMemcpyAsync(e->d_imgs.p, imgs + (size_t)c0 * px, (size_t)n * px, hipMemcpyHostToDevice, e->stream.s));
    st = launch_set_images(e, rows, e->d_imgs.p, n, 0);
    if (st == CC_OK && stages) st = predict_stored(e, rows, stages->m, nullptr, n, nullptr);
    if (st != CC_OK) return st;
    if (!stages) CC_HIP(hipMemsetAsync(e->d_pred.p, 1, (size_t)n, e->stream.s));
    FillResult r;
    st = fill_select(e->fill, e->d_pred.p, n, 0, want - got, 0, 0, 0.0, e->stream.s, &r);
    if (st != CC_OK) return st;
    if (r.n_filled > 0) {
      e->generation++;
      CopyRowsArgs A{};
      A.keep = e->fill.d_keep.p;
      A.first_slot = first_idx + got;
      A.cols = (int)cols;
      if (hog) {
        A.hog_src = rows.hog.p;
        A.hog_dst = e->samples.hog.p;
      } else {
        A.sum_src = rows.sum.p;
        A.sum_dst = e->samples.sum.p;
        if (e->use_tilted) {
          A.tilted_src = rows.tilted.p;
          A.tilted_dst = e->samples.tilted.p;
        }
        if (haar) {
          A.nf_src = rows.nf.p;
          A.nf_dst = e->samples.nf.p;
        }
      }
      hipLaunchKernelGGL(k_fill_copy_rows, dim3(r.n_filled), dim3(256), 0, e->stream.s, A);
      CC_HIP(hipGetLastError());
      CC_HIP(hipStreamSynchronize(e->stream.s));  // the scratch rows are rewritten by the next chunk
      for (int i = 0; i < r.n_filled; i++) e->cls[(size_t)first_idx + got + i] = (float)label;
      if (e->mirror_idx >= first_idx + got && e->mirror_idx < first_idx + got + r.n_filled) e->mirror_idx = -1;
    }
    got += r.n_filled;
    consumed = c0 + r.n_consumed;
  }
  *n_filled = got;
  *n_consumed = consumed;
  return CC_OK;
}

}  // extern "C"
