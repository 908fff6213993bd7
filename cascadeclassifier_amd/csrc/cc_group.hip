// Device side of what follows k_filter_candidates: the candidates of a pass put into OpenCV's single-threaded order
// (frame, scale, gy, gx) and cv::groupRectangles per frame, so that a detector's result can stay in device memory
// (cc_detect_batch_to_device), plus the building block cc_group_rectangles_device. The host twins are sort_candidates /
// group_pass (cc_detect_api.hip) and group_rectangles (cc_host.cpp); every step below restates theirs in the same integer,
// float and double operations, and nothing here depends on the order in which threads run ("Results that
// stay on the device").
//
// The scored forms (k_cand_rank<true>, k_group_frames_scored, k_group_compact<true>) carry what cv::groupRectangles(rects,
// rejectLevels, levelWeights, ...) carries: a level and a weight per rectangle, and per class the highest level and the largest
// weight among the members at that level (group_rectangles with both vectors, cc_host.cpp). The unscored kernels are the
// instantiations they were before.
//
// Every kernel finds its element counts in device memory (the filtered-candidate count, the segment offsets): the host
// launches fixed grids and never waits for a count before the next launch.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "cc_detect_internal.h"

namespace ccamd {

// A pass whose raw candidate list overflowed holds an arbitrary subset: its host redoes it with longer lists (the detector's
// grow-and-rerun). Until then nothing of it, and nothing of a pass launched behind it, may reach the caller's buffers:
// every kernel of such a pass returns at once, and the last one leaves `abort` set for the passes behind.
__device__ __forceinline__ bool pass_dead(const GroupGuard g) { return (g.counts && g.counts[0] > g.cand_cap) || (g.abort && *g.abort); }

// Workspace words are written with atomics by some steps and read by other threads after a barrier: reads go to the
// coherent level (in LDS this is a plain ds_read), and ws_sync orders plain stores to the global workspace as well.
__device__ __forceinline__ int ws_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long ws_ld(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void ws_sync() {
  __threadfence();
  __syncthreads();
}

// Exclusive scan of one value per thread over the block, continued from `carry` (the same in every thread; advanced by
// the block's total). Every thread of the block must call it. s_wave: THREADS / 64 ints of LDS.
template <int THREADS>
__device__ __forceinline__ int block_excl_scan(int v, int* s_wave, int& carry) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(inc, d, 64);
    if (lane >= d) inc += t;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  int before = 0, total = 0;
  for (int w = 0; w < THREADS / 64; w++) {
    const int t = s_wave[w];
    if (w < wave) before += t;
    total += t;
  }
  __syncthreads();  // s_wave is free for the next call
  const int pos = carry + before + inc - v;
  carry += total;
  return pos;
}

// ------------------------------------------------------------------------------------------------
// Ordering. The key (frame, scale, gy, gx) is unique per candidate, so a candidate's place in its frame is the number of
// the frame's keys below its own: a rank, the same whatever order the filter kernel's atomics left the list in.
//   k_cand_count    candidates per frame
//   k_cand_segments exclusive scan -> seg[nf + 1], cursors cleared
//   k_cand_bucket   key + list index of every candidate into its frame's segment (any order inside it)
//   k_cand_rank     rank inside the segment -> the rectangle at seg[f] + rank (SCORED: and the candidate's stage sum beside it)
// ------------------------------------------------------------------------------------------------
constexpr int ORDER_THREADS = 256;
constexpr int RANK_CHUNKS = 8;  // blocks that share one frame's ranks

__device__ __forceinline__ unsigned long long cand_key(const CandOut& c) {  // gx, gy <= 32768 (frame side limit), scale and frame < 2^16
  return ((unsigned long long)(c.frame & 0xffff) << 48) | ((unsigned long long)(c.scale & 0xffff) << 32) |
         ((unsigned long long)(c.gy & 0xffff) << 16) | (unsigned long long)(c.gx & 0xffff);
}

__global__ __launch_bounds__(ORDER_THREADS) void k_cand_count(GroupGuard g, const CandOut* __restrict__ cands, int nf,
                                                              int* __restrict__ frame_cnt) {
  if (pass_dead(g)) return;
  const int n = min(g.counts[1], g.cand_cap);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int f = cands[i].frame;
    if ((unsigned)f < (unsigned)nf) atomicAdd(frame_cnt + f, 1);
  }
}

// One block. cnt[nf] -> seg[nf + 1]; cnt becomes the cursors of k_cand_bucket (zero).
__global__ __launch_bounds__(ORDER_THREADS) void k_cand_segments(GroupGuard g, int nf, int* __restrict__ cnt, int* __restrict__ seg) {
  __shared__ int s_wave[ORDER_THREADS / 64];
  const bool dead = pass_dead(g);  // a dead pass: empty segments, so that whatever reads seg stays inside its buffers
  int carry = 0;
  for (int f0 = 0; f0 < nf; f0 += ORDER_THREADS) {
    const int f = f0 + threadIdx.x;
    const int v = (f < nf && !dead) ? cnt[f] : 0;
    const int pos = block_excl_scan<ORDER_THREADS>(v, s_wave, carry);
    if (f < nf) {
      seg[f] = pos;
      cnt[f] = 0;
    }
  }
  if (threadIdx.x == 0) seg[nf] = carry;
}

__global__ __launch_bounds__(ORDER_THREADS) void k_cand_bucket(GroupGuard g, const CandOut* __restrict__ cands, int nf,
                                                               const int* __restrict__ seg, int* __restrict__ cursor,
                                                               unsigned long long* __restrict__ keys, int* __restrict__ src) {
  if (pass_dead(g)) return;
  const int n = min(g.counts[1], g.cand_cap);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const CandOut c = cands[i];
    if ((unsigned)c.frame >= (unsigned)nf) continue;
    const int at = seg[c.frame] + atomicAdd(cursor + c.frame, 1);  // < seg[frame + 1] <= n: k_cand_count counted the same list
    keys[at] = cand_key(c);
    src[at] = i;
  }
}

// grid (nf, RANK_CHUNKS): the blocks of a frame take its candidates in turns of ORDER_THREADS and count, for each, the
// frame's keys below it, a tile of keys at a time through LDS.
template <bool SCORED>
__global__ __launch_bounds__(ORDER_THREADS) void k_cand_rank(GroupGuard g, const CandOut* __restrict__ cands, const int* __restrict__ seg,
                                                             const unsigned long long* __restrict__ keys, const int* __restrict__ src,
                                                             cc_rect* __restrict__ rects, double* __restrict__ sums) {
  if (pass_dead(g)) return;
  __shared__ unsigned long long s_keys[ORDER_THREADS];
  const int base = seg[blockIdx.x], n = seg[blockIdx.x + 1] - base;
  for (int i0 = blockIdx.y * ORDER_THREADS; i0 < n; i0 += RANK_CHUNKS * ORDER_THREADS) {  // block-uniform
    const int i = i0 + threadIdx.x;
    const unsigned long long mine = i < n ? keys[base + i] : 0ull;
    int rank = 0;
    for (int t0 = 0; t0 < n; t0 += ORDER_THREADS) {
      __syncthreads();
      if (t0 + (int)threadIdx.x < n) s_keys[threadIdx.x] = keys[base + t0 + threadIdx.x];
      __syncthreads();
      const int tn = min(ORDER_THREADS, n - t0);
      for (int k = 0; k < tn; k++) rank += s_keys[k] < mine ? 1 : 0;  // same address in every lane: a broadcast
    }
    if (i < n) {
      const CandOut c = cands[src[base + i]];
      rects[base + rank] = cc_rect{c.x, c.y, c.w, c.h};  // rank < n: the keys are distinct
      if constexpr (SCORED) sums[base + rank] = c.sum;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Grouping: one work-group per frame, group_rectangles (cc_host.cpp) step by step.
//   classes   union-find over all similar pairs: a root only ever hooks itself (compare-and-swap) under a smaller index, so
//             links never form a cycle, none is ever undone, and when all pairs are in, every component's one root is its
//             smallest member -- whatever the order of the hooks. Class number = rank of that root among the roots =
//             order of first appearance (cv::partition).
//   averages  int32 sums by integer atomics (exact, order-free), s = 1.f / cnt correctly rounded, rint((float)sum * s)
//   filters   cnt <= threshold; inside a bigger class
//   output    survivors in class order, at the frame's INPUT offset of `grouped` (there are never more than went in);
//             k_group_offsets / k_group_compact pack the frames behind one another
// Workspace: GROUP_WS_INTS ints per rectangle -- parent, class of a root (later: nothing), and per class x y w h sums and the
// count. In LDS up to GROUP_LDS_RECTS rectangles, else the frame's slice of the caller's global workspace.
// Scored (group_rectangles with levels and weights, cc_host.cpp "outputRejectLevels variant"): per class also
//   level     max(0, highest member level): an integer atomicMax from 0, beside the sums
//   weight    the largest weight among the members at that level, from DBL_MIN when the level stayed 0: a 64-bit atomicMax
//             over weight_key, an unsigned image of the double in which the integers order as the values do. Both maxima
//             are the same whatever order the members arrive in. (+0.0 and -0.0 are equal values with different images: where
//             they tie for a class's best, the host keeps the one it met first and the device +0.0. NaN has no place in
//             the order on either side.)
// and the workspace is GROUP_WS_INTS_SCORED ints per rectangle: the seven, the level, and the two halves of the weight's
// image (8-byte aligned: it starts 8 n ints into a slice that starts at an even number of ints). In LDS up to
// GROUP_LDS_RECTS_SCORED rectangles.
// ------------------------------------------------------------------------------------------------
constexpr int GROUP_THREADS = 1024;
constexpr int GROUP_LDS_RECTS = 2048;  // 7 x 2048 x 4 B = 56 KiB of the 64 KiB a block may declare
constexpr int GROUP_LDS_RECTS_SCORED = 1536;  // 10 x 1536 x 4 B = 60 KiB
static_assert(GROUP_WS_INTS_SCORED % 2 == 0, "a frame's slice of the scored workspace starts 8-byte aligned");

// What the scored grouping reads and writes beside the rectangles; levels null: every rectangle has const_level.
struct ScoresIO {
  const int32_t* levels;
  int const_level;
  const double* weights;
  int32_t* out_levels;
  double* out_weights;
};

// a < b as doubles (neither NaN, and not a zero against the other zero) <=> weight_key(a) < weight_key(b) as integers
__device__ __forceinline__ unsigned long long weight_key(double w) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(w);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_weight(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

__device__ __forceinline__ bool similar_rects(const cc_rect a, const cc_rect b, double eps) {
  const double delta = eps * (min(a.width, b.width) + min(a.height, b.height)) * 0.5;
  return abs(a.x - b.x) <= delta && abs(a.y - b.y) <= delta && abs(a.x + a.width - b.x - b.width) <= delta &&
         abs(a.y + a.height - b.y - b.height) <= delta;
}

__device__ __forceinline__ int find_root(const int* parent, int i) {
  for (int p; (p = ws_ld(parent + i)) != i;) i = p;
  return i;
}

__device__ __forceinline__ void unite(int* parent, int i, int j) {
  int a = find_root(parent, i), b = find_root(parent, j);
  while (a != b) {
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicCAS(parent + a, a, b);  // a > b
    if (old == a) break;
    a = find_root(parent, old);  // a got a parent meanwhile: go on from there
    b = find_root(parent, b);
  }
}

// sc: the frame's own levels / weights and where its survivors' go (SCORED only; offsets as for rects / out).
template <bool SCORED>
__device__ __forceinline__ void group_frame(int* ws, int* s_wave, const cc_rect* __restrict__ rects, int n, int group_threshold,
                                            double eps, cc_rect* __restrict__ out, int* __restrict__ out_count, const ScoresIO sc) {
  int* parent = ws;
  int* cls = ws + n;
  int* sx = ws + 2 * (size_t)n;
  int* sy = ws + 3 * (size_t)n;
  int* sw = ws + 4 * (size_t)n;
  int* sh = ws + 5 * (size_t)n;
  int* cnt = ws + 6 * (size_t)n;
  int* lvl = ws + 7 * (size_t)n;                                                                  // SCORED
  unsigned long long* wkey = reinterpret_cast<unsigned long long*>(ws + 8 * (size_t)n);  // SCORED
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += GROUP_THREADS) parent[i] = i;
  ws_sync();
  for (int i = tid; i < n; i += GROUP_THREADS) {
    const cc_rect a = rects[i];
    for (int j = i + 1; j < n; j++)
      if (similar_rects(a, rects[j], eps)) unite(parent, i, j);
  }
  ws_sync();
  // every rectangle straight under its root (a reader meets the old parent or the root: both lead to the root)
  for (int i = tid; i < n; i += GROUP_THREADS) {
    const int r = find_root(parent, i);
    if (r != i) __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  ws_sync();
  int nclasses = 0;
  for (int i0 = 0; i0 < n; i0 += GROUP_THREADS) {
    const int i = i0 + tid;
    const bool root = i < n && ws_ld(parent + i) == i;
    const int c = block_excl_scan<GROUP_THREADS>(root ? 1 : 0, s_wave, nclasses);
    if (root) cls[i] = c;
  }
  for (int c = tid; c < nclasses; c += GROUP_THREADS) {
    sx[c] = sy[c] = sw[c] = sh[c] = cnt[c] = 0;
    if constexpr (SCORED) {
      lvl[c] = 0;
      wkey[c] = 0;  // below every weight's image
    }
  }
  ws_sync();
  for (int i = tid; i < n; i += GROUP_THREADS) {
    const cc_rect r = rects[i];
    const int c = ws_ld(cls + ws_ld(parent + i));
    atomicAdd(sx + c, r.x);
    atomicAdd(sy + c, r.y);
    atomicAdd(sw + c, r.width);
    atomicAdd(sh + c, r.height);
    atomicAdd(cnt + c, 1);
    if constexpr (SCORED) atomicMax(lvl + c, sc.levels ? sc.levels[i] : sc.const_level);
  }
  ws_sync();
  if constexpr (SCORED)  // the class levels are final: the members at their class's level offer their weights
    for (int i = tid; i < n; i += GROUP_THREADS) {
      const int c = ws_ld(cls + ws_ld(parent + i));
      if ((sc.levels ? sc.levels[i] : sc.const_level) == ws_ld(lvl + c)) atomicMax(wkey + c, weight_key(sc.weights[i]));
    }
  for (int c = tid; c < nclasses; c += GROUP_THREADS) {
    const float s = __fdiv_rn(1.f, (float)ws_ld(cnt + c));
    const int x = __float2int_rn((float)ws_ld(sx + c) * s), y = __float2int_rn((float)ws_ld(sy + c) * s);
    const int w = __float2int_rn((float)ws_ld(sw + c) * s), h = __float2int_rn((float)ws_ld(sh + c) * s);
    sx[c] = x;
    sy[c] = y;
    sw[c] = w;
    sh[c] = h;
  }
  ws_sync();
  int n_out = 0;
  for (int c0 = 0; c0 < nclasses; c0 += GROUP_THREADS) {
    const int c = c0 + tid;
    bool keep = false;
    cc_rect r1{0, 0, 0, 0};
    if (c < nclasses) {
      const int n1 = ws_ld(cnt + c);
      r1 = cc_rect{ws_ld(sx + c), ws_ld(sy + c), ws_ld(sw + c), ws_ld(sh + c)};
      keep = n1 > group_threshold;
      for (int j = 0; keep && j < nclasses; j++) {
        const int n2 = ws_ld(cnt + j);
        if (j == c || n2 <= group_threshold) continue;
        const cc_rect r2{ws_ld(sx + j), ws_ld(sy + j), ws_ld(sw + j), ws_ld(sh + j)};
        const int dx = __double2int_rn(r2.width * eps), dy = __double2int_rn(r2.height * eps);
        if (r1.x >= r2.x - dx && r1.y >= r2.y - dy && r1.x + r1.width <= r2.x + r2.width + dx &&
            r1.y + r1.height <= r2.y + r2.height + dy && (n2 > max(3, n1) || n1 < 3))
          keep = false;
      }
    }
    const int at = block_excl_scan<GROUP_THREADS>(keep ? 1 : 0, s_wave, n_out);
    if (keep) out[at] = r1;  // at < nclasses <= n
    if constexpr (SCORED)
      if (keep) {
        // a class of level 0 starts from DBL_MIN, one of a higher level has a member at that level (its image is not 0)
        const int l = ws_ld(lvl + c);
        sc.out_levels[at] = l;
        sc.out_weights[at] = key_weight(max(ws_ld(wkey + c), l == 0 ? weight_key(DBL_MIN) : 0ull));
      }
  }
  if (tid == 0) *out_count = n_out;
}

__global__ __launch_bounds__(GROUP_THREADS) void k_group_frames(GroupGuard g, const cc_rect* __restrict__ rects,
                                                                const int* __restrict__ offsets, int group_threshold, double eps,
                                                                int* __restrict__ ws, cc_rect* __restrict__ grouped,
                                                                int* __restrict__ out_count) {
  if (pass_dead(g)) return;
  __shared__ int s_ws[GROUP_WS_INTS * GROUP_LDS_RECTS];
  __shared__ int s_wave[GROUP_THREADS / 64];
  const int f = blockIdx.x;
  const int base = offsets[f], n = offsets[f + 1] - base;
  if (group_threshold <= 0 || n <= 0) {  // the ordered candidates as they are
    for (int i = threadIdx.x; i < n; i += GROUP_THREADS) grouped[base + i] = rects[base + i];
    if (threadIdx.x == 0) out_count[f] = max(n, 0);
    return;
  }
  if (n <= GROUP_LDS_RECTS)
    group_frame<false>(s_ws, s_wave, rects + base, n, group_threshold, eps, grouped + base, out_count + f, ScoresIO{});
  else
    group_frame<false>(ws + (size_t)GROUP_WS_INTS * base, s_wave, rects + base, n, group_threshold, eps, grouped + base, out_count + f,
                       ScoresIO{});
}

// k_group_frames with levels and weights: sc.levels / sc.weights lie beside rects, sc.out_levels / sc.out_weights beside grouped.
__global__ __launch_bounds__(GROUP_THREADS) void k_group_frames_scored(GroupGuard g, const cc_rect* __restrict__ rects,
                                                                       const int* __restrict__ offsets, int group_threshold, double eps,
                                                                       int* __restrict__ ws, cc_rect* __restrict__ grouped,
                                                                       int* __restrict__ out_count, const ScoresIO sc) {
  if (pass_dead(g)) return;
  __shared__ __attribute__((aligned(8))) int s_ws[GROUP_WS_INTS_SCORED * GROUP_LDS_RECTS_SCORED];
  __shared__ int s_wave[GROUP_THREADS / 64];
  const int f = blockIdx.x;
  const int base = offsets[f], n = offsets[f + 1] - base;
  if (group_threshold <= 0 || n <= 0) {  // the ordered candidates as they are, with their levels and weights
    for (int i = threadIdx.x; i < n; i += GROUP_THREADS) {
      grouped[base + i] = rects[base + i];
      sc.out_levels[base + i] = sc.levels ? sc.levels[base + i] : sc.const_level;
      sc.out_weights[base + i] = sc.weights[base + i];
    }
    if (threadIdx.x == 0) out_count[f] = max(n, 0);
    return;
  }
  const ScoresIO fs{sc.levels ? sc.levels + base : nullptr, sc.const_level, sc.weights + base, sc.out_levels + base, sc.out_weights + base};
  if (n <= GROUP_LDS_RECTS_SCORED)
    group_frame<true>(s_ws, s_wave, rects + base, n, group_threshold, eps, grouped + base, out_count + f, fs);
  else
    group_frame<true>(ws + (size_t)GROUP_WS_INTS_SCORED * base, s_wave, rects + base, n, group_threshold, eps, grouped + base,
                      out_count + f, fs);
}

// One block. Frames f0 .. f0 + nf of the batch: out_offsets[f0 + i] = *total + (rectangles of the frames before i);
// *total moves on and also lands in out_offsets[f0 + nf], so the offsets are complete after the batch's last pass.
__global__ __launch_bounds__(ORDER_THREADS) void k_group_offsets(GroupGuard g, const int* __restrict__ out_count, int nf,
                                                                 int32_t* __restrict__ out_offsets, int* __restrict__ total) {
  __shared__ int s_wave[ORDER_THREADS / 64];
  if (pass_dead(g)) {
    if (threadIdx.x == 0 && g.abort) *g.abort = 1;
    return;
  }
  int carry = *total;
  __syncthreads();  // every thread has read the total before thread 0 moves it on
  for (int f0 = 0; f0 < nf; f0 += ORDER_THREADS) {
    const int f = f0 + threadIdx.x;
    const int pos = block_excl_scan<ORDER_THREADS>(f < nf ? out_count[f] : 0, s_wave, carry);
    if (f < nf) out_offsets[f] = pos;
  }
  if (threadIdx.x == 0) {
    out_offsets[nf] = carry;
    *total = carry;
  }
}

// grid nf: frame f's rectangles from its input offset of `grouped` to its place in `out`, what fits below cap. SCORED: their
// levels and weights move with them (sc.levels / sc.weights beside grouped, sc.out_levels / sc.out_weights beside out).
template <bool SCORED>
__global__ __launch_bounds__(ORDER_THREADS) void k_group_compact(GroupGuard g, const cc_rect* __restrict__ grouped,
                                                                 const int* __restrict__ offsets, const int32_t* __restrict__ out_offsets,
                                                                 cc_rect* __restrict__ out, int cap, const ScoresIO sc) {
  if (pass_dead(g)) return;
  const int f = blockIdx.x;
  const int from = offsets[f], to = out_offsets[f], n = out_offsets[f + 1] - to;
  for (int i = threadIdx.x; i < n; i += ORDER_THREADS)
    if (to + i < cap) {
      out[to + i] = grouped[from + i];
      if constexpr (SCORED) {
        sc.out_levels[to + i] = sc.levels[from + i];
        sc.out_weights[to + i] = sc.weights[from + i];
      }
    }
}

hipError_t GroupBufs::ensure(size_t rects, size_t frames, bool ordering, bool scored) {
  rects = std::max<size_t>(rects, 1);
  for (hipError_t e : {grouped.ensure(rects), ws.ensure(rects * (scored ? GROUP_WS_INTS_SCORED : GROUP_WS_INTS)),
                       out_count.ensure(std::max<size_t>(frames, 1)),
                       ordering ? ordered.ensure(rects) : hipSuccess, ordering ? keys.ensure(rects) : hipSuccess,
                       ordering ? src.ensure(rects) : hipSuccess, ordering ? seg.ensure(frames + 1) : hipSuccess,
                       ordering ? frame_cnt.ensure(std::max<size_t>(frames, 1)) : hipSuccess,
                       scored ? grouped_levels.ensure(rects) : hipSuccess, scored ? grouped_weights.ensure(rects) : hipSuccess,
                       scored && ordering ? ordered_weights.ensure(rects) : hipSuccess})
    if (e != hipSuccess) return e;
  return hipSuccess;
}

void launch_order_candidates(hipStream_t st, const GroupGuard g, const CandOut* cands, int nf, GroupBufs& B, bool scored) {
  if (nf <= 0) return;
  (void)hipMemsetAsync(B.frame_cnt.p, 0, (size_t)nf * sizeof(int), st);
  hipLaunchKernelGGL(k_cand_count, dim3(64), dim3(ORDER_THREADS), 0, st, g, cands, nf, B.frame_cnt.p);
  hipLaunchKernelGGL(k_cand_segments, dim3(1), dim3(ORDER_THREADS), 0, st, g, nf, B.frame_cnt.p, B.seg.p);
  hipLaunchKernelGGL(k_cand_bucket, dim3(64), dim3(ORDER_THREADS), 0, st, g, cands, nf, B.seg.p, B.frame_cnt.p, B.keys.p, B.src.p);
  if (scored)
    hipLaunchKernelGGL(k_cand_rank<true>, dim3(nf, RANK_CHUNKS), dim3(ORDER_THREADS), 0, st, g, cands, B.seg.p, B.keys.p, B.src.p,
                       B.ordered.p, B.ordered_weights.p);
  else
    hipLaunchKernelGGL(k_cand_rank<false>, dim3(nf, RANK_CHUNKS), dim3(ORDER_THREADS), 0, st, g, cands, B.seg.p, B.keys.p, B.src.p,
                       B.ordered.p, (double*)nullptr);
}

void launch_group_frames(hipStream_t st, const GroupGuard g, const cc_rect* rects, const int* offsets, int nf, int group_threshold,
                         double eps, GroupBufs& B, cc_rect* out, int cap, int32_t* out_offsets, int* total, const GroupScores& sc) {
  // scored: the frames' levels and weights are staged beside B.grouped and packed beside `out`
  const ScoresIO frames_io{sc.levels, sc.const_level, sc.weights, B.grouped_levels.p, B.grouped_weights.p};
  const ScoresIO compact_io{B.grouped_levels.p, 0, B.grouped_weights.p, sc.out_levels, sc.out_weights};
  if (nf > 0 && sc)
    hipLaunchKernelGGL(k_group_frames_scored, dim3(nf), dim3(GROUP_THREADS), 0, st, g, rects, offsets, group_threshold, eps, B.ws.p,
                       B.grouped.p, B.out_count.p, frames_io);
  else if (nf > 0)
    hipLaunchKernelGGL(k_group_frames, dim3(nf), dim3(GROUP_THREADS), 0, st, g, rects, offsets, group_threshold, eps, B.ws.p, B.grouped.p,
                       B.out_count.p);
  hipLaunchKernelGGL(k_group_offsets, dim3(1), dim3(ORDER_THREADS), 0, st, g, B.out_count.p, nf, out_offsets, total);
  if (nf > 0 && sc)
    hipLaunchKernelGGL(k_group_compact<true>, dim3(nf), dim3(ORDER_THREADS), 0, st, g, B.grouped.p, offsets, out_offsets, out, cap, compact_io);
  else if (nf > 0)
    hipLaunchKernelGGL(k_group_compact<false>, dim3(nf), dim3(ORDER_THREADS), 0, st, g, B.grouped.p, offsets, out_offsets, out, cap, ScoresIO{});
}

}  // namespace ccamd

using namespace ccamd;

// Both entry points below; sc empty: the unscored call.
static cc_status group_rectangles_device(int device, const cc_rect* rects, const int32_t* offsets, int n_frames, int group_threshold,
                                         double eps, cc_rect* out, int cap, int32_t* out_offsets, int* n_total, const GroupScores& sc) {
  if (!offsets || !out_offsets || !n_total || n_frames < 0 || cap < 0 || (cap > 0 && !out))
    return set_error(CC_ERR_INVALID_ARG, "cc_group_rectangles_device: bad argument");
  cc_status st = ensure_device(device);
  if (st != CC_OK) return st;
  OwnStream s;
  CC_HIP(s.create());
  // the offsets decide what the kernels index: look at them before anything is launched
  std::vector<int32_t> h_off((size_t)n_frames + 1);
  CC_HIP(copy_sync(h_off.data(), offsets, h_off.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s.s));
  if (h_off[0] < 0) return set_error(CC_ERR_INVALID_ARG, "cc_group_rectangles_device: negative offset");
  for (int f = 0; f < n_frames; f++)
    if (h_off[(size_t)f + 1] < h_off[(size_t)f]) return set_error(CC_ERR_INVALID_ARG, "cc_group_rectangles_device: offsets decrease at frame %d", f);
  const size_t n_rects = (size_t)h_off[(size_t)n_frames];
  if (n_rects > 0 && !rects) return set_error(CC_ERR_INVALID_ARG, "cc_group_rectangles_device: null rectangles");
  if (n_rects > 0 && sc && (!sc.levels || !sc.weights))
    return set_error(CC_ERR_INVALID_ARG, "cc_group_rectangles_device: null levels or weights");
  GroupBufs B;
  DevBuf<int> total;
  CC_HIP(B.ensure(n_rects, (size_t)n_frames, false, (bool)sc));
  CC_HIP(total.ensure(1));
  CC_HIP(hipMemsetAsync(total.p, 0, sizeof(int), s.s));
  launch_group_frames(s.s, GroupGuard{}, rects, offsets, n_frames, group_threshold, eps, B, out, cap, out_offsets, total.p, sc);
  CC_HIP(hipGetLastError());
  int h_total = 0;
  CC_HIP(copy_sync(&h_total, total.p, sizeof(int), hipMemcpyDeviceToHost, s.s));
  *n_total = h_total;
  if (h_total > cap) return set_error(CC_ERR_BUFFER_TOO_SMALL, "cc_group_rectangles_device: %d rectangles, capacity %d", h_total, cap);
  return CC_OK;
}

extern "C" cc_status cc_group_rectangles_device(int device, const cc_rect* rects, const int32_t* offsets, int n_frames,
                                                int group_threshold, double eps, cc_rect* out, int cap, int32_t* out_offsets,
                                                int* n_total) {
  return group_rectangles_device(device, rects, offsets, n_frames, group_threshold, eps, out, cap, out_offsets, n_total, GroupScores{});
}

extern "C" cc_status cc_group_rectangles_device_levels(int device, const cc_rect* rects, const int32_t* levels, const double* weights,
                                                       const int32_t* offsets, int n_frames, int group_threshold, double eps,
                                                       cc_rect* out, int32_t* out_levels, double* out_weights, int cap,
                                                       int32_t* out_offsets, int* n_total) {
  if (cap > 0 && (!out_levels || !out_weights)) return set_error(CC_ERR_INVALID_ARG, "cc_group_rectangles_device: bad argument");
  return group_rectangles_device(device, rects, offsets, n_frames, group_threshold, eps, out, cap, out_offsets, n_total,
                                 GroupScores{true, levels, 0, weights, out_levels, out_weights});
}
