// Detection on gfx950, the device code: sliding-window cascade evaluation with early exit (the kernels of cc_eval_kernel.inc),
// the stage-0 skip-rule filter, two instrumentation kernels, and the launchers of all of them: no other file launches these
// kernels. The detector that drives them is in cc_detector.h, cc_tables.hip, cc_pass.hip and cc_detect_api.hip; the pyramid and
// integral images come from cc_front.hip, the specialised kernels' source and code objects from cc_spec.hip. Replaces
// cv::CascadeClassifier::detectMultiScale as called by the reference's detection tool (tools/detection/Cpp/main.cpp:42-45);
// behaviour follows SURVEY.md Appendix A.
//
// Data layout in HBM (per frame slot f of a pass; all slabs are sized for the largest pass, at most max_batch frames):
//   pyramid  u8   : scale s at pyr + f*pyr_frame_bytes + img_ofs[s], row pitch pitch8[s] (multiple of 4)
//   integral i32  : sum   at integ + (f*nchan + 0)*int_frame_elems + int_ofs[s], (h+1) rows x pitchI[s] (multiple of 4)
//                   sqsum at integ + (f*nchan + 1)*int_frame_elems + int_ofs[s]   (Haar only; u32 wrap-around). With an even
//                   window size, scales scanned with step 2 keep only what the variance test reads: odd rows, and
//                   of those the odd columns packed (column 2c+1 at c)
//   rej0 mask u64 : bit gx&63 of word mask_ofs[s] + gy*nxw[s] + (gx>>6) = window (gx,gy) was rejected AT STAGE 0
//   candidates    : one global list {frame, scale, gx, gy} + counter; the filtered list adds the output rectangle.
//
// Arithmetic is compiled with -ffp-contract=off: Haar feature values and stage sums follow the CPU operation order
// exactly (float multiply/add without fusion, double stage accumulator), which makes decisions bit-identical.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cc_detector.h"

namespace ccamd {

#include "cc_eval_kernel.inc"

// Calibration stream for the FETCH_SIZE counter: same load shape as stage_tile (dword per lane, coalesced).
__global__ __launch_bounds__(256) void k_stream_dwords(const uint32_t* __restrict__ p, size_t n_words, uint32_t* __restrict__ out) {
  uint32_t acc = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (size_t)gridDim.x * blockDim.x) acc += p[i];
  if (acc == 0x9e3779b9u) atomicAdd(out, acc);  // keeps the loads alive; practically never taken
  atomicAdd(out + 1 + (threadIdx.x & 15), acc);
}

// ------------------------------------------------------------------------------------------------
// K5: stage-0 skip rule. OpenCV's scan loop skips the next grid position of a row after a window rejected at stage 0
// (SURVEY.md A.5): window i is visited iff the run of consecutive stage-0 rejections immediately before it has even
// length. Walk the rej0 bit mask backwards, a 64-bit word at a time.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool visited_by_scan(const unsigned long long* __restrict__ row_mask, int gx) {
  int run = 0;
  int pos = gx - 1;
  while (pos >= 0) {
    const int b = pos & 63;
    const unsigned long long w = row_mask[pos >> 6] << (63 - b);  // bit `pos` now at bit 63
    const int ones = min(__clzll((long long)~w), b + 1);          // leading ones (clz(0) = 64)
    run += ones;
    if (ones < b + 1) break;
    pos -= b + 1;
  }
  return (run & 1) == 0;
}

__global__ __launch_bounds__(256) void k_filter_candidates(const CandRaw* __restrict__ cands, const int* __restrict__ cand_count,
                                                           int cand_cap, const ScaleDev* __restrict__ sd,
                                                           const unsigned long long* __restrict__ masks,
                                                           size_t mask_frame_words, CandOut* __restrict__ out,
                                                           int* __restrict__ out_count) {
  const int n = min(*cand_count, cand_cap);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const CandRaw c = cands[i];
    const ScaleDev S = sd[c.scale];
    const unsigned long long* row = masks + (size_t)c.frame * mask_frame_words + S.mask_ofs + (size_t)c.gy * S.nxw;
    if (!visited_by_scan(row, c.gx)) continue;
    const int slot = atomicAdd(out_count, 1);
    CandOut o;
    o.frame = c.frame;
    o.scale = c.scale;
    o.gx = c.gx;
    o.gy = c.gy;
    o.x = __float2int_rn((float)(c.gx * S.ystep) * S.scale);
    o.y = __float2int_rn((float)(c.gy * S.ystep) * S.scale);
    o.w = S.win_w;
    o.h = S.win_h;
    o.sum = c.sum;
    out[slot] = o;  // out has cand_cap entries; slot < n <= cand_cap
  }
}

__global__ void k_debug_visited(const ScaleDev* __restrict__ sd, int nscales, const int* __restrict__ rowblk_first,
                                const unsigned long long* __restrict__ masks, uint8_t* __restrict__ visited) {
  // one block per grid row of frame 0
  const int s = find_segment(rowblk_first, nscales, blockIdx.x);
  const ScaleDev S = sd[s];
  const int gy = blockIdx.x - rowblk_first[s];
  const unsigned long long* row = masks + S.mask_ofs + (size_t)gy * S.nxw;
  for (int gx = threadIdx.x; gx < S.nx; gx += blockDim.x)
    visited[(size_t)S.win_ofs + (size_t)gy * S.nx + gx] = visited_by_scan(row, gx) ? 1 : 0;
}

// Parity instrumentation of inv_sqrt_as_float (cc_eval_kernel.inc): counts values nf for which it differs from
// (float)(1.0 / sqrt(nf)). nf is drawn as the kernels form it -- area * valsqsum - valsum^2 for a random window size, pixel
// sum and squared sum (an integer-valued double) -- and, every fourth draw, as an arbitrary integer below 2^52.
__global__ void k_vnf_check(unsigned long long seed, int per_thread, unsigned long long* mismatches) {
  unsigned long long x = seed + (unsigned long long)(blockIdx.x * blockDim.x + threadIdx.x) * 0x9E3779B97F4A7C15ull;
  auto next = [&]() {
    x ^= x << 13;
    x ^= x >> 7;
    x ^= x << 17;
    return x;
  };
  unsigned long long bad = 0;
  for (int i = 0; i < per_thread; i++) {
    const unsigned long long r = next();
    double nf;
    if ((i & 3) == 3) {
      nf = (double)(1ull + (next() >> 12));
    } else {
      const unsigned w = 1u + (unsigned)(r & 0xffu), h = 1u + (unsigned)((r >> 8) & 0xffu);
      const double area = (double)(w * h);
      const unsigned long long n = (unsigned long long)w * h;
      const unsigned long long sm = (r >> 16) % (255ull * n + 1ull);
      // any squared sum a window with that pixel sum can have: between sm^2 / n and 255 * sm
      const unsigned long long lo_sq = (sm * sm + n - 1) / n, hi_sq = 255ull * sm;
      const unsigned long long sq = lo_sq + (hi_sq > lo_sq ? next() % (hi_sq - lo_sq + 1ull) : 0ull);
      nf = area * (double)(unsigned)sq - (double)(int)sm * (double)(int)sm;  // the kernels' expression (valsqsum wraps at 2^32 like theirs)
    }
    if (!(nf > 0.)) continue;
    if (__float_as_uint(inv_sqrt_as_float(nf)) != __float_as_uint((float)(1. / sqrt(nf)))) bad++;
  }
  if (bad) atomicAdd(mismatches, bad);
}

// Arguments of the cascade kernel for a pass in `slot`, all but `tiles` and `stamps` (per launch).
static EvalArgs eval_args(const cc_detector* d, const Plan* P, int slot, int nchan, bool tilt, int sq_compact, bool debug) {
  const bool haar = d->m.feature_type == CC_FEATURE_HAAR;
  EvalArgs A;
  A.integ = d->d_integ[slot].p;
  A.int_frame_elems = P->front.L.int_frame_elems;
  A.nchan = nchan;
  A.tilt_chan = tilt ? 2 : -1;
  A.sd = P->front.d_sd.p;
  A.W0 = d->m.win_w;
  A.H0 = d->m.win_h;
  A.nstages = (int)d->m.stage_ntrees.size();
  A.stage_first = d->d_stage_first.p;
  A.stage_ntrees = d->d_stage_ntrees.p;
  A.group_first = d->d_group_first.p;
  A.ngroups = d->n_groups;
  A.dense_from = d->dense_from;
  A.wave_below = d->wave_below;
  A.stop_after = d->stop_after;
  A.split_stumps = d->split_stumps;
  A.early_skip = d->early_skip;
  A.sq_compact = sq_compact;
  A.stage_thr = d->d_stage_thr.p;
  A.masks = d->d_masks[slot].p;
  A.mask_frame_words = P->mask_frame_words;
  A.cands = d->d_cands[slot].p;
  A.cand_count = d->d_counts[slot].p;
  A.cand_cap = d->cand_cap;
  A.stamps = nullptr;
  A.dbg_codes = debug ? d->d_dbg_codes.p : nullptr;
  A.dbg_sums = debug ? d->d_dbg_sums.p : nullptr;
  A.stumps1 = haar ? (const void*)d->d_haar1.p : (const void*)d->d_lbp1.p;
  A.stumps2 = haar ? (const void*)d->d_haar2.p : (const void*)d->d_lbp2.p;
  A.wstumps1 = d->d_haar1w.p ? (const void*)d->d_haar1w.p : A.stumps1;
  A.wstumps2 = d->d_haar2w.p ? (const void*)d->d_haar2w.p : A.stumps2;
  A.wave_q = d->d_wave_q.p;
  A.wave_thr_q = d->d_wave_thr_q.p;
  A.gstumps = haar ? (const void*)d->d_haar_g.p : (const void*)d->d_lbp_g.p;
  A.lbp16_all = d->lbp16_all;
  if (!haar && d->d_lbp16.p) A.wstumps2 = d->d_lbp16.p;  // LBP wave phase of kernels with 16-bit tiles
  A.trees = d->m.max_nodes_per_tree > 1 ? 1 : 0;
  A.nodes1 = haar ? (const void*)d->d_hnode1.p : (const void*)d->d_lnode1.p;
  A.nodes2 = haar ? (const void*)d->d_hnode2.p : (const void*)d->d_lnode2.p;
  A.tree_root = d->d_tree_root.p;
  A.tree_leaf0 = d->d_tree_leaf0.p;
  A.leaves = d->d_leaves.p;
  return A;
}

int eval_stamp_slots() { return STAMP_SLOTS; }

cc_status launch_eval(cc_detector* d, const Plan* P, int slot, int nchan, bool tilt, int sq_compact, bool debug, unsigned long long* stamps,
                      const EvalLaunch* launches, int n_launches, int nf, hipStream_t st) {
  const bool haar = d->m.feature_type == CC_FEATURE_HAAR;
  EvalArgs A = eval_args(d, P, slot, nchan, tilt, sq_compact, debug);
  A.stamps = stamps;
  for (int i = 0; i < n_launches; i++) {
    const EvalLaunch& L = launches[i];
    if (L.n_tiles == 0) continue;
    A.tiles = L.tiles;
    A.wave_below = L.wave_below >= 0 ? L.wave_below : d->wave_below;
    if (L.fn) {
      void* params[] = {&A};
      // (the pass's EV_EVAL pair spans all cascade-kernel launches; the STEP-1 module's launch is also timed on its own)
      EvScope ev1(d, i == 1 ? EV_EVAL_STEP1 : -1, st);
      CC_HIP(hipModuleLaunchKernel(L.fn, (unsigned)L.n_tiles, (unsigned)nf, 1, EVAL_THREADS, 1, 1, (unsigned)L.lds, st, params, nullptr));
    } else if (haar)
      hipLaunchKernelGGL(k_eval_haar, dim3(L.n_tiles, nf), dim3(EVAL_THREADS), L.lds, st, A);
    else
      hipLaunchKernelGGL(k_eval_lbp, dim3(L.n_tiles, nf), dim3(EVAL_THREADS), L.lds, st, A);
    if (A.stamps) A.stamps += (size_t)L.n_tiles * (size_t)nf * STAMP_SLOTS;
  }
  return CC_OK;
}

void launch_filter_candidates(cc_detector* d, const Plan* P, int slot, hipStream_t st) {
  hipLaunchKernelGGL(k_filter_candidates, dim3(64), dim3(256), 0, st, d->d_cands[slot].p, d->d_counts[slot].p, d->cand_cap, P->front.d_sd.p,
                     d->d_masks[slot].p, P->mask_frame_words, d->d_out[slot].p, d->d_counts[slot].p + 1);
}

void launch_debug_visited(cc_detector* d, const Plan* P, int slot, hipStream_t st) {
  hipLaunchKernelGGL(k_debug_visited, dim3(P->n_grid_rows), dim3(256), 0, st, P->front.d_sd.p, (int)P->front.L.sd.size(), P->d_gridrow_first.p,
                     d->d_masks[slot].p, d->d_dbg_visited.p);
}

cc_status allow_large_lds(const cc_detector* d) {
  if (d->lds <= 64 * 1024) return CC_OK;
  if (d->m.feature_type == CC_FEATURE_HAAR)
    CC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_eval_haar), hipFuncAttributeMaxDynamicSharedMemorySize, (int)d->lds));
  else
    CC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_eval_lbp), hipFuncAttributeMaxDynamicSharedMemorySize, (int)d->lds));
  return CC_OK;
}

}  // namespace ccamd

using namespace ccamd;

extern "C" {

// ---- building blocks -------------------------------------------------------------------------------------------
cc_status cc_debug_vnf_check(int device, uint64_t n_values, uint64_t seed, uint64_t* mismatches) {
  if (!mismatches) return set_error(CC_ERR_INVALID_ARG, "cc_debug_vnf_check: null output");
  cc_status st = ensure_device(device);
  if (st != CC_OK) return st;
  unsigned long long* d = nullptr;
  CC_HIP(hipMalloc(reinterpret_cast<void**>(&d), sizeof(unsigned long long)));
  CC_HIP(hipMemset(d, 0, sizeof(unsigned long long)));
  const int threads = 256, blocks = 4096;
  const int per_thread = (int)std::max<uint64_t>(1, std::min<uint64_t>((n_values + (uint64_t)threads * blocks - 1) / ((uint64_t)threads * blocks), 1u << 20));
  hipLaunchKernelGGL(k_vnf_check, dim3(blocks), dim3(threads), 0, 0, (unsigned long long)seed, per_thread, d);
  unsigned long long h = 0;
  const hipError_t e2 = hipMemcpy(&h, d, sizeof(h), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e2 != hipSuccess) return set_error(CC_ERR_HIP, "cc_debug_vnf_check: %s", hipGetErrorString(e2));
  *mismatches = h;
  return CC_OK;
}

cc_status cc_debug_stream_dwords(int device, size_t n_bytes, int repeats, uint32_t* checksum) {
  if (n_bytes < 4 || repeats < 1) return set_error(CC_ERR_INVALID_ARG, "cc_debug_stream_dwords: bad argument");
  cc_status st = ensure_device(device);
  if (st != CC_OK) return st;
  DevBuf<uint32_t> buf, out;
  const size_t n_words = n_bytes / 4;
  CC_HIP(buf.ensure(n_words));
  CC_HIP(out.ensure(32));
  CC_HIP(hipMemset(buf.p, 1, n_words * 4));
  CC_HIP(hipMemset(out.p, 0, 32 * 4));
  for (int r = 0; r < repeats; r++)
    hipLaunchKernelGGL(k_stream_dwords, dim3(256 * 8), dim3(256), 0, nullptr, buf.p, n_words, out.p);
  CC_HIP(hipGetLastError());
  uint32_t h[32];
  CC_HIP(hipMemcpy(h, out.p, sizeof(h), hipMemcpyDeviceToHost));
  uint32_t c = 0;
  for (int i = 1; i < 17; i++) c += h[i];
  if (checksum) *checksum = c;
  return CC_OK;
}

}  // extern "C"
