// Training-side feature evaluator on gfx950, bulk operator() over (feature range x samples) of the stored samples
// (cc_eval_store.hip): the batch kernels, the sorted precalc, feature lists for one sample, custom Haar features and
// Feature::calc on caller-held integrals (haarfeatures.h:108-122, lbpfeatures.h:70-83).
//
// The batch kernel stages a tile of samples TRANSPOSED into LDS ([integral entry][sample]) so that a wavefront's lanes
// (samples) hit distinct banks, and writes out[(fi - fi_begin) * n_samples + s] with the sample index fastest (coalesced
// row segments).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "cc_train_device.h"

namespace ccamd {

// ------------------------------------------------------------------------------------------------
// Bulk operator(): block = BATCH_THREADS threads, a tile of S samples staged transposed into LDS, loops over a feature chunk.
// lane -> (feature sub-index, sample): s = lane % S.
// ------------------------------------------------------------------------------------------------
struct BatchArgs {
  const int32_t* sum;
  const int32_t* tilted;
  const float* normfactor;
  const int32_t* sample_idx;  // optional
  int n_samples;
  int cols;
  int S;                      // samples per tile (power of two, <= 64)
  int feat_begin, feat_end;   // indices into the feature table
  int feats_per_block;
  const void* feats;
  float* out;                 // [feat_end - feat_begin][out_pitch], the first n_samples of a row are written
  size_t out_pitch;           // elements between the rows of two features (>= n_samples)
  int n_tiles, xcd_tiles;     // wide kernel: sample tiles, and whether the grid is laid out XCD by XCD
  int debug_nostore;          // timing experiment: skip the output stores
  int normalized;             // Haar: divide by normfactor (operator()) or not (Feature::calc)
  int use_tilted;
};

constexpr int BATCH_THREADS = 1024;  // 16 wavefronts per block: the LDS tile allows two blocks per CU = full occupancy

// LDS tile [entry p][S samples], XOR-swizzled: sample s of entry p sits at word p * S + (s ^ (p & (S - 1))).
// Staging writes walk consecutive entries of one sample (coalesced global reads): without the swizzle all 64 lanes of a
// store would hit one bank (stride S words); with it they spread over S banks. The evaluation reads one entry for S
// consecutive samples: the swizzle permutes them within the same S words, still conflict-free. The feature tables hold
// byte offsets of the swizzled entry, (p * S + (p & (S - 1))) * 4 (tilted features: plus the tilted tile's base), so that a
// corner read is ONE xor with the lane's sample byte index: address = entry ^ (s * 4).
__device__ __forceinline__ int batch_tile_word(int p, int s, int S) { return p * S + (s ^ (p & (min(S, 32) - 1))); }

// a / b, correctly rounded, with the part that depends on b alone hoisted: operator() divides every feature value of a
// sample by the same norm factor (haarfeatures.h:108-112). The compiler's expansion of an IEEE float division is
//   y0 = rcp(b); y1 = fma(fma(-b, y0, 1), y0, y0); q0 = a * y1; q1 = fma(fma(-b, q0, a), y1, q0); q = fma(fma(-b, q1, a), y1, q1)
// wrapped in v_div_scale / v_div_fmas / v_div_fixup, which rescale operands whose exponents would push an intermediate
// into the denormal or overflow range and patch zero / infinity / NaN results; for finite normal operands far from both
// ends (norm factors are >= 1 and < 2^21, feature sums are 0 or of magnitude >= 2^-8 and < 2^27) those three are the
// identity, so the same five operations give the same bits. A zero dividend keeps its sign. Checked against the division
// operator on the device over 2^32 operand pairs plus the edge values (cc_debug_division_check, tests/test_gpu_eval.py).
__device__ __forceinline__ float refined_rcp(float b) {
  const float y0 = __builtin_amdgcn_rcpf(b);
  return __builtin_fmaf(__builtin_fmaf(-b, y0, 1.0f), y0, y0);
}
__device__ __forceinline__ float div_by_refined(float a, float b, float y1) {
  const float q0 = a * y1;
  const float q1 = __builtin_fmaf(__builtin_fmaf(-b, q0, a), y1, q0);
  const float q = __builtin_fmaf(__builtin_fmaf(-b, q1, a), y1, q1);
  return a == 0.0f ? a : q;
}

// Counts operand pairs for which div_by_refined differs from the division operator (parity instrumentation).
__global__ void k_division_check(unsigned long long seed, int per_thread, unsigned long long* mismatches) {
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
    // b: norm factors, any float in [1, 2^21); a: any float with magnitude in [2^-8, 2^27), either sign
    const float b = __uint_as_float(0x3F800000u + (unsigned)(r % (21u << 23)));
    const unsigned am = 0x3B800000u + (unsigned)((r >> 32) % (35u << 23));
    const float a = __uint_as_float(am | ((unsigned)(r >> 63) << 31));
    const float y1 = refined_rcp(b);
    if (__float_as_uint(div_by_refined(a, b, y1)) != __float_as_uint(a / b)) bad++;
    // integer-valued dividends (what the catalog's integer weights produce) against integer-valued and sqrt-like divisors
    const float ai = (float)(int)((r >> 8) % 33554432u) - 16777216.0f;
    const float bi = sqrtf((float)(1u + (unsigned)(r >> 40) % 16777215u) * (float)(1u + (unsigned)(r >> 16) % 65535u));
    if (bi >= 1.0f && bi < 2097152.0f && __float_as_uint(div_by_refined(ai, bi, refined_rcp(bi))) != __float_as_uint(ai / bi)) bad++;
  }
  if (bad) atomicAdd(mismatches, bad);
}

template <bool HAAR>
__global__ __launch_bounds__(BATCH_THREADS) void k_eval_batch(BatchArgs A) {
  extern __shared__ int32_t lds[];  // [cols][S] (+ [cols][S] tilted)
  const int S = A.S;
  const int s0 = blockIdx.x * S;
  int32_t* lsum = lds;
  int32_t* ltil = lds + (size_t)A.cols * S;
  // stage: consecutive threads read consecutive entries of one sample (coalesced), write transposed
  for (int e = threadIdx.x; e < A.cols * S; e += BATCH_THREADS) {
    const int s = e / A.cols, p = e - s * A.cols;
    int v = 0, t = 0;
    if (s0 + s < A.n_samples) {
      const int si = A.sample_idx ? A.sample_idx[s0 + s] : s0 + s;
      v = A.sum[(size_t)si * A.cols + p];
      if (HAAR && A.use_tilted) t = A.tilted[(size_t)si * A.cols + p];
    }
    lsum[batch_tile_word(p, s, S)] = v;
    if (HAAR && A.use_tilted) ltil[batch_tile_word(p, s, S)] = t;
  }
  __syncthreads();
  const int s = threadIdx.x % S;
  const int fsub = threadIdx.x / S, fpar = BATCH_THREADS / S;
  const bool valid = s0 + s < A.n_samples;
  float nf = 1.f;
  if (HAAR && A.normalized && valid) nf = A.normfactor[A.sample_idx ? A.sample_idx[s0 + s] : s0 + s];
  const int f0 = A.feat_begin + blockIdx.y * A.feats_per_block;
  const int f1 = min(f0 + A.feats_per_block, A.feat_end);
  const char* tile = reinterpret_cast<const char*>(lds);
  const int s4 = s * 4;
  auto at = [&](int entry) { return *reinterpret_cast<const int32_t*>(tile + (entry ^ s4)); };
  if (HAAR) {
    // software pipeline: the next feature's record (a 64-byte per-lane global load) is in flight while this one is evaluated
    const HaarFeatDev* feats = reinterpret_cast<const HaarFeatDev*>(A.feats);
    const float y1 = refined_rcp(nf);  // the sample's norm factor does not change from feature to feature
    HaarFeatDev F = feats[min(f0 + fsub, f1 - 1)];
#pragma unroll 2
    for (int f = f0 + fsub; f < f1; f += fpar) {
      const HaarFeatDev N = feats[min(f + fpar, f1 - 1)];
      const float ret = haar_sum(F, at);
      const float val = A.normalized ? (nf == 0.0f ? 0.0f : div_by_refined(ret, nf, y1)) : ret;
      if (valid && (!A.debug_nostore || val == 12345.678f)) A.out[(size_t)(f - A.feat_begin) * A.out_pitch + s0 + s] = val;
      F = N;
    }
  } else {
    const LbpFeatDev* feats = reinterpret_cast<const LbpFeatDev*>(A.feats);
    for (int f = f0 + fsub; f < f1; f += fpar) {
      const LbpFeatDev F = feats[f];
      int p[16];
#pragma unroll
      for (int j = 0; j < 16; j++) p[j] = at(F.p[j]);
      const float val = (float)lbp_code(p);
      if (valid && (!A.debug_nostore || val == 12345.678f)) A.out[(size_t)(f - A.feat_begin) * A.out_pitch + s0 + s] = val;
    }
  }
}

// Wide variant (S == 64, no tilted tile; the 24x24 BASIC / CORE / LBP shapes): a block owns a tile of 64 samples (one
// block per CU, 160 KB of LDS) and a WAVEFRONT evaluates one feature for the 64 samples, so the feature record is
// wave-uniform and travels through scalar loads. In the narrow kernel above every lane fetches its half-wavefront's
// 64-byte record with vector loads: 64 lanes x 52 bytes through the texture-address path cost ~64 cycles per
// iteration and CU, more than the arithmetic (~25) and the LDS reads (~18) together.
__device__ __forceinline__ HaarFeatDev load_feat(const HaarFeatDev __attribute__((address_space(4)))* p) {
  HaarFeatDev o;
  const int __attribute__((address_space(4)))* w = (const int __attribute__((address_space(4)))*)p;
  int* d = reinterpret_cast<int*>(&o);
#pragma unroll
  for (int i = 0; i < 16; i++) d[i] = w[i];
  return o;
}
__device__ __forceinline__ LbpFeatDev load_feat(const LbpFeatDev __attribute__((address_space(4)))* p) {
  LbpFeatDev o;
  const int __attribute__((address_space(4)))* w = (const int __attribute__((address_space(4)))*)p;
#pragma unroll
  for (int i = 0; i < 16; i++) o.p[i] = w[i];
  return o;
}

template <bool HAAR>
__global__ __launch_bounds__(BATCH_THREADS) void k_eval_batch_wide(BatchArgs A) {
  extern __shared__ int32_t lds[];  // [cols][64], swizzled like the narrow tile (S = 64: word p * 64 + (s ^ (p & 31)))
  constexpr int S = 64;
  // Blocks b and b + 8 run on the same XCD (round-robin dispatch): give each XCD a contiguous run of sample tiles, so that
  // the 256-byte pieces its CUs write into a feature row are neighbours in that XCD's L2 (placement affects speed only).
  const int tiles_per_xcd = (A.n_tiles + 7) >> 3;
  const int tile = A.xcd_tiles ? (int)(blockIdx.x & 7) * tiles_per_xcd + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  if (tile >= A.n_tiles) return;
  const int s0 = tile * S;
  {
    // Staging: wavefront w copies samples w, w + 16, ... (4 of the 64); its lanes walk the sample's entries, 8 loads in
    // flight per lane before the first LDS store (the tile is the first thing the block touches: nothing else hides
    // the latency of these loads, and one CU runs one block).
    const int lane = threadIdx.x & 63, w0 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int UNROLL = 8;
    for (int s = w0; s < S; s += BATCH_THREADS / 64) {
      const bool in = s0 + s < A.n_samples;  // wave-uniform
      const int si = in ? (A.sample_idx ? A.sample_idx[s0 + s] : s0 + s) : 0;
      const int32_t* src = A.sum + (size_t)si * A.cols;
      for (int p0 = 0; p0 < A.cols; p0 += 64 * UNROLL) {
        int v[UNROLL];
#pragma unroll
        for (int k = 0; k < UNROLL; k++) {
          const int p = p0 + k * 64 + lane;
          v[k] = 0;
          if (in && p < A.cols) v[k] = src[p];
        }
#pragma unroll
        for (int k = 0; k < UNROLL; k++) {
          const int p = p0 + k * 64 + lane;
          if (p < A.cols) lds[p * S + (s ^ (p & 31))] = v[k];
        }
      }
    }
  }
  __syncthreads();
  const int s = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool valid = s0 + s < A.n_samples;
  float nf = 1.f;
  if (HAAR && A.normalized && valid) nf = A.normfactor[A.sample_idx ? A.sample_idx[s0 + s] : s0 + s];
  const int f0 = A.feat_begin + blockIdx.y * A.feats_per_block;
  const int f1 = min(f0 + A.feats_per_block, A.feat_end);
  // A corner read is ONE xor: LDS address = (tile base + s * 4) ^ entry. That equals base + ((s * 4) ^ entry) because the
  // tile starts at LDS address 0 (this kernel has no static shared memory in front of its dynamic tile; checked below:
  // any base with its low 18 bits clear would do, the tile spans less than 2^18 bytes).
  const unsigned tile_base = (unsigned)(unsigned long long)(const __attribute__((address_space(3))) char*)lds;
  if (tile_base & 0x3FFFFu) __builtin_trap();
  const unsigned s4 = tile_base + (unsigned)s * 4u;
  auto at = [&](int entry) { return *(const __attribute__((address_space(3))) int32_t*)(unsigned long long)(s4 ^ (unsigned)entry); };
  constexpr int WAVES = BATCH_THREADS / 64;
  float* out = A.out + s0 + s;
  if (HAAR) {
    const HaarFeatDev __attribute__((address_space(4)))* feats = (const HaarFeatDev __attribute__((address_space(4)))*)A.feats;
    const float y1 = refined_rcp(nf);
    auto eval = [&](const HaarFeatDev& F, int f) {
      if (A.debug_nostore == 2) {  // timing experiment: the store stream alone
        if (valid) out[(size_t)(f - A.feat_begin) * A.out_pitch] = F.w[0];
        return;
      }
      if (A.debug_nostore == 3) {  // timing experiment: the store stream alone in 512-byte pieces (every second tile writes two)
        if (!(tile & 1)) {
          if (valid) out[(size_t)(f - A.feat_begin) * A.out_pitch] = F.w[0];
          if (s0 + 64 + s < A.n_samples) out[(size_t)(f - A.feat_begin) * A.out_pitch + 64] = F.w[0];
        }
        return;
      }
      const float ret = haar_sum(F, at);
      const float val = A.normalized ? (nf == 0.0f ? 0.0f : div_by_refined(ret, nf, y1)) : ret;
      if (valid && (A.debug_nostore != 1 || val == 12345.678f)) out[(size_t)(f - A.feat_begin) * A.out_pitch] = val;
    };
    // Two features per trip: their records (scalar loads, wave-uniform) are requested together. Scalar loads and LDS reads
    // share one completion counter and scalar data may return out of order, so a wavefront cannot wait for an LDS read
    // while a scalar load is in flight without waiting for that load too: a record fetch cannot be overlapped with the
    // evaluation of the previous feature, only amortised over more features.
    // (Round 3 tried requesting the NEXT trip's records before this trip's LDS reads, so that their latency runs under the
    // LDS round trip: the arithmetic alone got 10 % faster (5.9 -> 5.3 ms without the stores), the kernel did not
    // (6.57 vs 6.43 ms): the store stream alone takes 5.8 ms and is what bounds it. Not kept.)
    for (int f = f0 + wave; f < f1; f += 2 * WAVES) {
      const bool two = f + WAVES < f1;
      const HaarFeatDev Fa = load_feat(feats + f), Fb = load_feat(feats + (two ? f + WAVES : f));
      eval(Fa, f);
      if (two) eval(Fb, f + WAVES);
    }
  } else {
    const LbpFeatDev __attribute__((address_space(4)))* feats = (const LbpFeatDev __attribute__((address_space(4)))*)A.feats;
    auto eval = [&](const LbpFeatDev& F, int f) {
      int p[16];
#pragma unroll
      for (int j = 0; j < 16; j++) p[j] = at(F.p[j]);
      const float val = (float)lbp_code(p);
      if (valid && (!A.debug_nostore || val == 12345.678f)) out[(size_t)(f - A.feat_begin) * A.out_pitch] = val;
    };
    for (int f = f0 + wave; f < f1; f += 2 * WAVES) {
      const bool two = f + WAVES < f1;
      const LbpFeatDev Fa = load_feat(feats + f), Fb = load_feat(feats + (two ? f + WAVES : f));
      eval(Fa, f);
      if (two) eval(Fb, f + WAVES);
    }
  }
}

// operator()(feature_idx[k], si) for a list of catalog features and one stored sample: one thread per list entry, the
// sample's integral row read straight from global memory (2.5 KB, cache resident after the first touch).
template <bool HAAR>
__global__ __launch_bounds__(256) void k_eval_list(const void* __restrict__ feats, const int32_t* __restrict__ list, int n,
                                                   const int32_t* __restrict__ sum_row, const int32_t* __restrict__ tilted_row,
                                                   const float* __restrict__ nf_of_sample, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (HAAR) {
    const float nf = *nf_of_sample;
    const HaarFeatDev F = reinterpret_cast<const HaarFeatDev*>(feats)[list[i]];
    const int32_t* b = F.tilted ? tilted_row : sum_row;
    out[i] = haar_value(haar_sum(F, [&](int o) { return b[o]; }), nf);
  } else {
    const LbpFeatDev F = reinterpret_cast<const LbpFeatDev*>(feats)[list[i]];
    out[i] = (float)lbp_code_at(F, [&](int o) { return sum_row[o]; });
  }
}

// Feature::calc on caller-held integral rows: one thread per (feature, row).
__global__ void k_feature_calc_rows(const HaarFeatDev* __restrict__ feats, int n_feats, const int32_t* __restrict__ sum,
                                    const int32_t* __restrict__ tilted, int n_rows, int row_len, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_feats * n_rows) return;
  const int f = i / n_rows, r = i - f * n_rows;
  const HaarFeatDev F = feats[f];
  const int32_t* b = (F.tilted ? tilted : sum) + (size_t)r * row_len;
  out[i] = haar_sum(F, [&](int o) { return b[o]; });
}

__global__ void k_iota_rows(int* __restrict__ v, size_t total, int n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) v[i] = (int)(i % (size_t)n);
}
__global__ void k_narrow_u16(const int* __restrict__ in, unsigned short* __restrict__ out, size_t total) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) out[i] = (unsigned short)in[i];
}

cc_status batch_kernels_allow_lds(int bytes) {
  CC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_eval_batch<true>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  CC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_eval_batch<false>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  CC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_eval_batch_wide<true>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  CC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_eval_batch_wide<false>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  return CC_OK;
}

cc_status launch_batch(cc_evaluator* e, bool haar, const void* feats, int fb, int fe, const int32_t* d_idx, int ns,
                       float* d_out_ptr, int normalized, size_t out_pitch) {
  if (e->type == CC_FEATURE_HOG) return hog_launch_batch(e, fb, fe, d_idx, ns, d_out_ptr, out_pitch);  // fb, fe: variables
  BatchArgs A;
  A.sum = e->samples.sum.p;
  A.tilted = e->use_tilted ? e->samples.tilted.p : nullptr;
  A.normfactor = e->samples.nf.p;
  A.sample_idx = d_idx;
  A.n_samples = ns;
  A.cols = e->cols;
  A.S = e->S;
  A.feat_begin = fb;
  A.feat_end = fe;
  A.feats = feats;
  A.out = d_out_ptr;
  A.out_pitch = out_pitch ? out_pitch : (size_t)ns;
  A.normalized = normalized;
  A.debug_nostore = std::getenv("CCAMD_DEBUG_EVAL_NOSTORE") ? std::max(1, std::atoi(std::getenv("CCAMD_DEBUG_EVAL_NOSTORE"))) : 0;
  A.use_tilted = e->use_tilted ? 1 : 0;
  const int nfe = fe - fb;
  const int tiles = (ns + e->S - 1) / e->S;
  // Feature chunks: a block stages its sample tile once per chunk and then walks the chunk's features. Enough chunks for
  // about `rounds` rounds of blocks over the chip (balance), each amortising its tile load over >= 2048 features.
  // Measured at 162 336 x 20 000 (ms for the whole matrix): 2 chunks per launch 7.9, 5: 7.2, 16: 6.6, 32: 7.0, 64: 8.0.
  const int per_cu = e->S == 64 ? 1 : 2, rounds = 20;
  int chunks = (256 * per_cu * rounds + tiles - 1) / std::max(tiles, 1);
  chunks = std::max(1, std::min(chunks, (nfe + 2047) / 2048));
  A.feats_per_block = (nfe + chunks - 1) / chunks;
  chunks = (nfe + A.feats_per_block - 1) / A.feats_per_block;
  const size_t lds = (size_t)e->cols * e->S * 4 * (haar && e->use_tilted ? 2 : 1);
  (void)hipEventRecord(e->ev_a.e, e->stream.s);
  A.n_tiles = tiles;
  A.xcd_tiles = std::getenv("CCAMD_EVAL_NO_XCD_TILES") ? 0 : 1;
  if (e->S == 64) {  // wide tile (cc_eval_create chose it): one feature per wavefront, scalar record loads
    const int gx = A.xcd_tiles ? ((tiles + 7) / 8) * 8 : tiles;
    if (haar)
      hipLaunchKernelGGL(k_eval_batch_wide<true>, dim3(gx, chunks), dim3(BATCH_THREADS), lds, e->stream.s, A);
    else
      hipLaunchKernelGGL(k_eval_batch_wide<false>, dim3(gx, chunks), dim3(BATCH_THREADS), lds, e->stream.s, A);
  } else if (haar)
    hipLaunchKernelGGL(k_eval_batch<true>, dim3(tiles, chunks), dim3(BATCH_THREADS), lds, e->stream.s, A);
  else
    hipLaunchKernelGGL(k_eval_batch<false>, dim3(tiles, chunks), dim3(BATCH_THREADS), lds, e->stream.s, A);
  (void)hipEventRecord(e->ev_b.e, e->stream.s);
  CC_HIP(hipGetLastError());
  return CC_OK;
}

cc_status upload_indices(cc_evaluator* e, const int32_t* sample_idx, int ns, const int32_t** d_idx) {
  *d_idx = nullptr;
  if (!sample_idx) {
    if (ns > e->max_samples) return set_error(CC_ERR_OUT_OF_RANGE, "n_samples %d exceeds max_samples %d", ns, e->max_samples);
    return CC_OK;
  }
  for (int i = 0; i < ns; i++)
    if (sample_idx[i] < 0 || sample_idx[i] >= e->max_samples)
      return set_error(CC_ERR_OUT_OF_RANGE, "sample index %d out of range (max_samples %d)", sample_idx[i], e->max_samples);
  CC_HIP(e->d_idx.ensure((size_t)ns));
  CC_HIP(hipMemcpyAsync(e->d_idx.p, sample_idx, (size_t)ns * 4, hipMemcpyHostToDevice, e->stream.s));
  *d_idx = e->d_idx.p;
  return CC_OK;
}

static cc_status check_feature_range(const cc_evaluator* e, int fb, int fe, const char* who) {
  if (fb < 0 || fe > e->nfeat || fb > fe) return set_error(CC_ERR_OUT_OF_RANGE, "%s: features [%d, %d) out of range (%d)", who, fb, fe, e->nfeat);
  return CC_OK;
}

static HaarFeature haar_feature_of(const cc_haar_feature& in) {
  HaarFeature f;
  std::memcpy(f.r, in.r, sizeof(f.r));
  std::memcpy(f.w, in.w, sizeof(f.w));
  f.tilted = in.tilted != 0;
  return f;
}

// The catalog with plain fastRect offsets (row stride W + 1, the host mirror's builder) on the device, uploaded once.
template <class T, class Build>
static cc_status plain_catalog(cc_evaluator* e, DevBuf<T>& buf, Build build) {
  if (buf.p) return CC_OK;
  const std::vector<T> dev = build();
  CC_HIP(buf.ensure(std::max<size_t>(dev.size(), 1)));
  CC_HIP(copy_sync(buf.p, dev.data(), dev.size() * sizeof(T), hipMemcpyHostToDevice, e->stream.s));
  return CC_OK;
}

// operator() of features [fi_begin, fi_end) on n_samples stored samples, rows `pitch` apart (0 = n_samples): into d_out on
// the device, or (host_out set) through e->d_out into host memory. `who`: the entry point, for the messages.
static cc_status calc_batch(cc_evaluator* e, int fi_begin, int fi_end, const int32_t* sample_idx, int n_samples, float* d_out, size_t pitch,
                            float* host_out, const char* who) {
  if (!e || !(host_out ? host_out : d_out)) return set_error(CC_ERR_INVALID_ARG, "%s: null argument", who);
  if (cc_status rst = check_feature_range(e, fi_begin, fi_end, who); rst != CC_OK) return rst;
  if (n_samples < 0) return set_error(CC_ERR_INVALID_ARG, "%s: negative sample count", who);
  if (pitch != 0 && pitch < (size_t)n_samples)
    return set_error(CC_ERR_INVALID_ARG, "%s: pitch %zu is smaller than the %d samples of a row", who, pitch, n_samples);
  cc_status st = eval_device(e);
  if (st != CC_OK) return st;
  if (fi_begin == fi_end || n_samples == 0) return CC_OK;
  std::lock_guard<std::mutex> lk(e->mu);
  if (cc_status fst = flush_pending_images(e); fst != CC_OK) return fst;  // images set one at a time reach the device first
  const int32_t* d_idx = nullptr;
  st = upload_indices(e, sample_idx, n_samples, &d_idx);
  if (st != CC_OK) return st;
  const bool haar = e->type == CC_FEATURE_HAAR;
  const size_t total = (size_t)(fi_end - fi_begin) * n_samples;
  if (host_out) {
    CC_HIP(e->d_out.ensure(total));
    d_out = e->d_out.p;
  }
  st = launch_batch(e, haar, haar ? (const void*)e->d_haar.p : (const void*)e->d_lbp.p, fi_begin, fi_end, d_idx, n_samples, d_out, 1, pitch);
  if (st != CC_OK) return st;
  if (host_out) CC_HIP(hipMemcpyAsync(host_out, d_out, total * 4, hipMemcpyDeviceToHost, e->stream.s));
  CC_HIP(hipStreamSynchronize(e->stream.s));
  float ms = 0;
  if (hipEventElapsedTime(&ms, e->ev_a.e, e->ev_b.e) == hipSuccess) e->last_ms = ms;
  return CC_OK;
}

}  // namespace ccamd

using namespace ccamd;

extern "C" {

cc_status cc_debug_division_check(int device, uint64_t n_pairs, uint64_t seed, uint64_t* mismatches) {
  if (!mismatches) return set_error(CC_ERR_INVALID_ARG, "cc_debug_division_check: null output");
  if (cc_status st = ensure_device(device); st != CC_OK) return st;
  DevBuf<unsigned long long> d;
  CC_HIP(d.ensure(1));
  OwnStream own;  // not the legacy stream: see copy_sync
  if (hipError_t es = own.create(); es != hipSuccess) return set_error(CC_ERR_HIP, "cc_debug_division_check: %s", hipGetErrorString(es));
  (void)hipMemsetAsync(d.p, 0, sizeof(unsigned long long), own.s);
  const int threads = 256, blocks = 4096;
  const int per_thread = (int)std::max<uint64_t>(1, std::min<uint64_t>((n_pairs + (uint64_t)threads * blocks - 1) / ((uint64_t)threads * blocks), 1u << 20));
  hipLaunchKernelGGL(k_division_check, dim3(blocks), dim3(threads), 0, own.s, (unsigned long long)seed, per_thread, d.p);
  unsigned long long h = 0;
  const hipError_t e2 = copy_sync(&h, d.p, sizeof(h), hipMemcpyDeviceToHost, own.s);
  if (e2 != hipSuccess) return set_error(CC_ERR_HIP, "cc_debug_division_check: %s", hipGetErrorString(e2));
  *mismatches = h;
  return CC_OK;
}

cc_status cc_eval_calc_batch(cc_evaluator* e, int fi_begin, int fi_end, const int32_t* sample_idx, int n_samples, float* out,
                             int out_on_device) {
  return calc_batch(e, fi_begin, fi_end, sample_idx, n_samples, out_on_device ? out : nullptr, 0, out_on_device ? nullptr : out,
                    "cc_eval_calc_batch");
}

cc_status cc_eval_calc_batch_device(cc_evaluator* e, int fi_begin, int fi_end, const int32_t* sample_idx, int n_samples,
                                    float* d_out, size_t pitch) {
  return calc_batch(e, fi_begin, fi_end, sample_idx, n_samples, d_out, pitch, nullptr, "cc_eval_calc_batch_device");
}

cc_status cc_eval_calc_batch_sorted(cc_evaluator* e, int fi_begin, int fi_end, int n_samples, float* vals, void* idx, int idx_bytes) {
  if (!e || !idx) return set_error(CC_ERR_INVALID_ARG, "cc_eval_calc_batch_sorted: null argument");
  if (cc_status rst = check_feature_range(e, fi_begin, fi_end, "cc_eval_calc_batch_sorted"); rst != CC_OK) return rst;
  if (n_samples < 0 || n_samples > e->max_samples) return set_error(CC_ERR_OUT_OF_RANGE, "cc_eval_calc_batch_sorted: n_samples %d out of range", n_samples);
  if (idx_bytes != 2 && idx_bytes != 4) return set_error(CC_ERR_INVALID_ARG, "cc_eval_calc_batch_sorted: idx_bytes must be 2 or 4");
  if (idx_bytes == 2 && n_samples > 65536) return set_error(CC_ERR_INVALID_ARG, "cc_eval_calc_batch_sorted: 16-bit indices need n_samples <= 65536");
  cc_status st = eval_device(e);
  if (st != CC_OK) return st;
  const int nf = fi_end - fi_begin;
  if (nf == 0 || n_samples == 0) return CC_OK;
  std::lock_guard<std::mutex> lk(e->mu);
  if (cc_status fst = flush_pending_images(e); fst != CC_OK) return fst;  // images set one at a time reach the device first
  const bool haar = e->type == CC_FEATURE_HAAR;
  const size_t total = (size_t)nf * n_samples;
  if (total > (size_t)INT32_MAX) return set_error(CC_ERR_INVALID_ARG, "cc_eval_calc_batch_sorted: block too large (%zu values); use smaller feature ranges", total);
  DevBuf<float> keys_out;
  DevBuf<int> iota, sorted, offsets;
  DevBuf<unsigned short> narrow;
  DevBuf<char> temp;
  CC_HIP(e->d_out.ensure(total));
  CC_HIP(keys_out.ensure(total));
  CC_HIP(iota.ensure(total));
  CC_HIP(sorted.ensure(total));
  CC_HIP(offsets.ensure((size_t)nf + 1));
  st = launch_batch(e, haar, haar ? (const void*)e->d_haar.p : (const void*)e->d_lbp.p, fi_begin, fi_end, nullptr, n_samples, e->d_out.p, 1, 0);
  if (st != CC_OK) return st;
  bool sorted_in_blocks = false;
  if (n_samples <= sort_rows_block_limit()) {  // one block per row, the row in registers + LDS (cc_presort.hip)
    if (sort_rows_block(e->d_out.p, nf, n_samples, keys_out.p, sorted.p, e->stream.s) == hipSuccess)
      sorted_in_blocks = true;
    else
      (void)hipGetLastError();  // refused LDS request / launch: the device-wide segmented sort below
  }
  if (!sorted_in_blocks) {
    std::vector<int> off((size_t)nf + 1);
    for (int i = 0; i <= nf; i++) off[(size_t)i] = i * n_samples;
    CC_HIP(hipMemcpyAsync(offsets.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, e->stream.s));
    hipLaunchKernelGGL(k_iota_rows, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, e->stream.s, iota.p, total, n_samples);
    size_t temp_bytes = 0;
    CC_HIP(hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, temp_bytes, e->d_out.p, keys_out.p, iota.p, sorted.p, (int)total, nf,
                                                       offsets.p, offsets.p + 1, 0, 32, e->stream.s));
    CC_HIP(temp.ensure(std::max<size_t>(temp_bytes, 1)));
    // radix sort is stable: equal values keep increasing sample order
    CC_HIP(hipcub::DeviceSegmentedRadixSort::SortPairs(temp.p, temp_bytes, e->d_out.p, keys_out.p, iota.p, sorted.p, (int)total, nf,
                                                       offsets.p, offsets.p + 1, 0, 32, e->stream.s));
  }
  if (idx_bytes == 2) {
    CC_HIP(narrow.ensure(total));
    hipLaunchKernelGGL(k_narrow_u16, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, e->stream.s, sorted.p, narrow.p, total);
    CC_HIP(hipMemcpyAsync(idx, narrow.p, total * 2, hipMemcpyDeviceToHost, e->stream.s));
  } else
    CC_HIP(hipMemcpyAsync(idx, sorted.p, total * 4, hipMemcpyDeviceToHost, e->stream.s));
  if (vals) CC_HIP(hipMemcpyAsync(vals, e->d_out.p, total * 4, hipMemcpyDeviceToHost, e->stream.s));
  CC_HIP(hipGetLastError());
  CC_HIP(hipStreamSynchronize(e->stream.s));
  return CC_OK;
}

cc_status cc_eval_calc(cc_evaluator* e, int fi, int si, float* out) {
  if (!e || !out) return set_error(CC_ERR_INVALID_ARG, "cc_eval_calc: null argument");
  if (si < 0 || si >= e->max_samples) return set_error(CC_ERR_OUT_OF_RANGE, "cc_eval_calc: sample %d out of range (%d)", si, e->max_samples);
  // the window set last by cc_eval_set_image is answered from its host mirror, no launch; any other Haar / LBP sample leaves
  // the range check to cc_eval_calc_batch
  const bool hog = e->type == CC_FEATURE_HOG;
  if ((hog || si == e->mirror_idx) && (fi < 0 || fi >= e->nfeat))
    return set_error(CC_ERR_OUT_OF_RANGE, "cc_eval_calc: %s %d out of range (%d)", hog ? "variable" : "feature", fi, e->nfeat);
  const int32_t idx = si, feat = fi;
  if (mirror_answer(e, si, &feat, 1, out)) return CC_OK;
  return cc_eval_calc_batch(e, fi, fi + 1, &idx, 1, out, 0);
}

cc_status cc_eval_calc_list(cc_evaluator* e, const int32_t* feature_idx, int n_feats, int si, float* out) {
  if (!e || (n_feats > 0 && (!feature_idx || !out))) return set_error(CC_ERR_INVALID_ARG, "cc_eval_calc_list: null argument");
  if (n_feats < 0) return set_error(CC_ERR_INVALID_ARG, "cc_eval_calc_list: negative count");
  if (si < 0 || si >= e->max_samples) return set_error(CC_ERR_OUT_OF_RANGE, "cc_eval_calc_list: sample %d out of range (%d)", si, e->max_samples);
  for (int i = 0; i < n_feats; i++)
    if (feature_idx[i] < 0 || feature_idx[i] >= e->nfeat)
      return set_error(CC_ERR_OUT_OF_RANGE, "cc_eval_calc_list: feature %d out of range (%d)", feature_idx[i], e->nfeat);
  if (mirror_answer(e, si, feature_idx, n_feats, out)) return CC_OK;  // see cc_eval_calc
  cc_status st = eval_device(e);
  if (st != CC_OK) return st;
  if (n_feats == 0) return CC_OK;
  const bool haar = e->type == CC_FEATURE_HAAR;
  std::lock_guard<std::mutex> lk(e->mu);
  st = flush_pending_images(e);
  if (st != CC_OK) return st;
  CC_HIP(e->d_idx.ensure((size_t)n_feats));
  CC_HIP(e->d_out.ensure((size_t)n_feats));
  CC_HIP(hipMemcpyAsync(e->d_idx.p, feature_idx, (size_t)n_feats * 4, hipMemcpyHostToDevice, e->stream.s));
  if (e->type == CC_FEATURE_HOG)
    st = hog_launch_list(e, e->d_idx.p, n_feats, si, e->d_out.p);
  else {
    st = haar ? plain_catalog(e, e->d_haar_plain, [&]() { return haar_catalog_dev(e->haar, e->W); })
              : plain_catalog(e, e->d_lbp_plain, [&]() { return lbp_catalog_dev(e->lbp, e->W); });
    if (st != CC_OK) return st;
    const int32_t* row = e->samples.sum.p + (size_t)si * e->cols;
    const int32_t* trow = e->use_tilted ? e->samples.tilted.p + (size_t)si * e->cols : row;
    if (haar)
      hipLaunchKernelGGL(k_eval_list<true>, dim3((n_feats + 255) / 256), dim3(256), 0, e->stream.s, (const void*)e->d_haar_plain.p, e->d_idx.p,
                         n_feats, row, trow, e->samples.nf.p + si, e->d_out.p);
    else
      hipLaunchKernelGGL(k_eval_list<false>, dim3((n_feats + 255) / 256), dim3(256), 0, e->stream.s, (const void*)e->d_lbp_plain.p, e->d_idx.p,
                         n_feats, row, trow, e->samples.nf.p + si, e->d_out.p);
    CC_HIP(hipGetLastError());
  }
  if (st != CC_OK) return st;
  CC_HIP(hipMemcpyAsync(out, e->d_out.p, (size_t)n_feats * sizeof(float), hipMemcpyDeviceToHost, e->stream.s));
  CC_HIP(hipStreamSynchronize(e->stream.s));
  return CC_OK;
}

cc_status cc_eval_calc_custom_haar(cc_evaluator* e, const cc_haar_feature* feats, int n_feats, int normalized,
                                   const int32_t* sample_idx, int n_samples, float* out) {
  if (!e || !feats || !out) return set_error(CC_ERR_INVALID_ARG, "cc_eval_calc_custom_haar: null argument");
  if (e->type != CC_FEATURE_HAAR) return set_error(CC_ERR_INVALID_ARG, "cc_eval_calc_custom_haar: evaluator is not HAAR");
  if (n_feats < 0 || n_samples < 0) return set_error(CC_ERR_INVALID_ARG, "cc_eval_calc_custom_haar: negative count");
  cc_status st = eval_device(e);
  if (st != CC_OK) return st;
  if (n_feats == 0 || n_samples == 0) return CC_OK;
  std::vector<HaarFeatDev> dev((size_t)n_feats);
  for (int i = 0; i < n_feats; i++) {
    const HaarFeature f = haar_feature_of(feats[i]);
    if (f.tilted && !e->use_tilted) return set_error(CC_ERR_INVALID_ARG, "cc_eval_calc_custom_haar: tilted feature on an evaluator without tilted integrals (mode != ALL)");
    for (int j = 0; j < 3; j++) {  // every touched integral entry must lie inside the (W+1)x(H+1) window integral
      if (f.w[j] == 0.0f) break;
      const int x = f.r[j][0], y = f.r[j][1], w = f.r[j][2], h = f.r[j][3];
      bool ok = x >= 0 && y >= 0 && w >= 0 && h >= 0;
      ok = ok && (f.tilted ? (x - h >= 0 && x + w <= e->W && y + w + h <= e->H) : (x + w <= e->W && y + h <= e->H));
      if (!ok) return set_error(CC_ERR_OUT_OF_RANGE, "cc_eval_calc_custom_haar: rect %d of feature %d leaves the window", j, i);
    }
    haar_to_dev(f, e->W + 1, dev[i], e->S, e->use_tilted ? e->cols * e->S * 4 : 0);
  }
  std::lock_guard<std::mutex> lk(e->mu);
  if (cc_status fst = flush_pending_images(e); fst != CC_OK) return fst;  // images set one at a time reach the device first
  const int32_t* d_idx = nullptr;
  st = upload_indices(e, sample_idx, n_samples, &d_idx);
  if (st != CC_OK) return st;
  CC_HIP(e->d_custom.ensure((size_t)n_feats));
  CC_HIP(hipMemcpyAsync(e->d_custom.p, dev.data(), dev.size() * sizeof(HaarFeatDev), hipMemcpyHostToDevice, e->stream.s));
  const size_t total = (size_t)n_feats * n_samples;
  CC_HIP(e->d_out.ensure(total));
  st = launch_batch(e, true, e->d_custom.p, 0, n_feats, d_idx, n_samples, e->d_out.p, normalized ? 1 : 0, 0);
  if (st != CC_OK) return st;
  CC_HIP(hipMemcpyAsync(out, e->d_out.p, total * 4, hipMemcpyDeviceToHost, e->stream.s));
  CC_HIP(hipStreamSynchronize(e->stream.s));
  return CC_OK;
}

cc_status cc_haar_feature_calc(int device, const cc_haar_feature* feats, int n_feats, int step, const int32_t* sum,
                               const int32_t* tilted, int n_rows, int row_len, float* out) {
  if (!feats || !out || n_feats < 0 || n_rows < 0 || row_len < 1 || step < 1) return set_error(CC_ERR_INVALID_ARG, "cc_haar_feature_calc: bad argument");
  if (cc_status st = ensure_device(device); st != CC_OK) return st;
  if (n_feats == 0 || n_rows == 0) return CC_OK;
  std::vector<HaarFeatDev> dev((size_t)n_feats);
  bool need_sum = false, need_tilted = false;
  for (int i = 0; i < n_feats; i++) {
    const HaarFeature f = haar_feature_of(feats[i]);
    haar_to_dev(f, step, dev[i]);
    (f.tilted ? need_tilted : need_sum) = true;
    for (int j = 0; j < 3; j++)
      for (int k = 0; k < 4; k++)
        if (dev[i].p[j][k] < 0 || dev[i].p[j][k] >= row_len)
          return set_error(CC_ERR_OUT_OF_RANGE, "cc_haar_feature_calc: feature %d reads offset %d outside the %d-entry integral", i, dev[i].p[j][k], row_len);
  }
  if ((need_sum && !sum) || (need_tilted && !tilted)) return set_error(CC_ERR_INVALID_ARG, "cc_haar_feature_calc: a needed integral image is NULL");
  DevBuf<HaarFeatDev> d_f;
  DevBuf<int32_t> d_s, d_t;
  DevBuf<float> d_o;
  const size_t nint = (size_t)n_rows * row_len, nout = (size_t)n_feats * n_rows;
  OwnStream own;  // not the legacy stream: see copy_sync
  CC_HIP(own.create());
  CC_HIP(d_f.ensure((size_t)n_feats));
  CC_HIP(copy_sync(d_f.p, dev.data(), dev.size() * sizeof(HaarFeatDev), hipMemcpyHostToDevice, own.s));
  if (sum) {
    CC_HIP(d_s.ensure(nint));
    CC_HIP(copy_sync(d_s.p, sum, nint * 4, hipMemcpyHostToDevice, own.s));
  }
  if (tilted) {
    CC_HIP(d_t.ensure(nint));
    CC_HIP(copy_sync(d_t.p, tilted, nint * 4, hipMemcpyHostToDevice, own.s));
  }
  CC_HIP(d_o.ensure(nout));
  hipLaunchKernelGGL(k_feature_calc_rows, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, own.s, d_f.p, n_feats, d_s.p, d_t.p,
                     n_rows, row_len, d_o.p);
  CC_HIP(hipGetLastError());
  CC_HIP(copy_sync(out, d_o.p, nout * 4, hipMemcpyDeviceToHost, own.s));
  return CC_OK;
}

cc_status cc_eval_last_kernel_ms(cc_evaluator* e, double* ms) {
  if (!e || !ms) return set_error(CC_ERR_INVALID_ARG, "cc_eval_last_kernel_ms: null argument");
  *ms = e->last_ms;
  return CC_OK;
}

}  // extern "C"
