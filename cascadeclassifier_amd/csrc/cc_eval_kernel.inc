// Device code of the cascade-evaluation kernel (K4), kept in its own file because it is compiled twice: ahead of time
// as part of cc_detect.hip, and at run time by hiprtc for ONE cascade with CC_SPEC_STAGES defined
// (cc_detector_specialize: the first stages become straight-line code with immediate LDS offsets and constants; the
// text of this file travels inside the library as a string, see the Makefile). Pure device code: no host includes.
// Lives inside namespace ccamd in both builds, after the declarations of cc_eval_common.h.

// Read-only tables (cascade, scale descriptors, tile list) are written by the host before the launch and never by a
// kernel: addressing them through the constant address space lets wave-uniform reads become scalar loads (s_load).
#define CC_CONST __attribute__((address_space(4)))
template <class T>
__device__ __forceinline__ const T CC_CONST* as_const_table(const T* p) {
  return (const T CC_CONST*)p;
}
// Copies one table record (a multiple of 4 bytes) out of the constant address space, dword by dword.
template <class T>
__device__ __forceinline__ T load_record(const T CC_CONST* p) {
  static_assert(sizeof(T) % 4 == 0, "table records are dword multiples");
  T out;
  const int CC_CONST* w = (const int CC_CONST*)p;
  int* o = reinterpret_cast<int*>(&out);
#pragma unroll
  for (unsigned i = 0; i < sizeof(T) / 4; i++) o[i] = w[i];
  return out;
}

// ------------------------------------------------------------------------------------------------
// K4: cascade evaluation. Block = 256 threads = 4 wavefronts = one tile of 64 x 8 window origins of one scale.
// The tile of the `sum` integral the windows touch is staged once into LDS (for STEP 2 with even and odd columns
// in separate planes, so that a wavefront's stride-2 corner reads are bank-conflict free); every rectangle corner
// is then an LDS read. The cascade's early exit is handled by COMPACTION instead of divergence:
//   phase D (dense)  : lane = window column, 2 window rows per thread: variance test + stage 0 for all 512 windows;
//                      wave ballots give the stage-0 rejection mask words; survivors are appended to an LDS queue;
//   phase T (thread) : stage by stage, one thread per queued window, survivors re-queued into the other LDS queue
//                      buffer. The queue is a table [row][bank class]: a window's class is the LDS bank of its tile
//                      base (win_class), lane l of a half-wavefront only ever takes windows of class l, so the 32 lanes
//                      that share an LDS access always hit 32 different banks: every corner gather of the compacted
//                      stages is conflict-free by construction (a dense queue of arbitrary survivors collides 2-2.6-way).
//                      The price is lanes without a window where a class has fewer survivors than the fullest one;
//   phase W (wave)   : once fewer than `wave_below` windows are left in the block, one wavefront per window: the 64
//                      lanes split the stage's stumps and reduce their votes. Only used when the stage sums of the
//                      cascade are provably order-independent (exact in double, checked on the host at load time),
//                      so the reduction is bit-identical to the sequential CPU accumulation.
// In the code: struct EvalTile holds what a block knows about its tile and the rules the phases share (deliver, enqueue,
// stage0_outcome, mask_column, never_visited, stage_sum, table_sum, deal_windows); its members stage_phase, dense_phase /
// dense_phase_rolled, thread_phase (+ split_stage) and wave_phase_haar / wave_phase_lbp are the phases, eval_tile is their
// sequence with the early exits between them, and eval_block picks the tile layout for the three kernels.
// ------------------------------------------------------------------------------------------------
// Stages the tile of the integral into LDS: one wavefront per tile row, lanes = groups of 4 consecutive entries
// (16-byte global loads; tile origins are multiples of 64 entries and row pitches multiples of 4, so they are aligned,
// and a group that holds at least one entry of the integral lies entirely inside the row pitch).
// STEP 2 splits each group into its even and odd columns (two 8-byte LDS stores into the two planes).
// The loads of up to STAGE_ROWS rows per wavefront are issued back to back before the first LDS store: one memory round
// trip per tile instead of one per row (the tile is the first thing a block touches, nothing else hides that latency).
constexpr int STAGE_ROWS = 12;
template <int STEP, class Geom>
__device__ __forceinline__ void stage_tile(int32_t* lds, const Geom& G, const int32_t* __restrict__ sum,
                                           const ScaleDev& S, int x0, int y0) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int quads = (G.cols + 3) >> 2;
  const bool right_edge = x0 + quads * 4 - 1 > S.w;  // block-uniform: some entries lie right of the integral's last column
  for (int q0 = 0; q0 < quads; q0 += 64) {
    const int qd = q0 + lane;
    const int c = qd * 4, gc = x0 + c;
    const bool in_tile = qd < quads;
    const bool col_ok = in_tile && gc <= S.w;
    for (int rb = wave; rb < G.rows; rb += EVAL_WAVES * STAGE_ROWS) {
      int4 v[STAGE_ROWS];
#pragma unroll
      for (int k = 0; k < STAGE_ROWS; k++) {
        const int r = rb + k * EVAL_WAVES, gr = y0 + r;
        v[k] = make_int4(0, 0, 0, 0);  // rows below the integral and entries right of it read as 0
        if (r < G.rows && gr <= S.h && col_ok) v[k] = *reinterpret_cast<const int4*>(sum + (size_t)gr * S.pitchI + gc);
      }
#pragma unroll
      for (int k = 0; k < STAGE_ROWS; k++) {
        const int r = rb + k * EVAL_WAVES;
        if (r < G.rows && in_tile) {
          int4 w = v[k];
          if (right_edge) {
            if (gc + 1 > S.w) w.y = 0;
            if (gc + 2 > S.w) w.z = 0;
            if (gc + 3 > S.w) w.w = 0;
          }
          if constexpr (Geom::k16) {  // four 16-bit entries = one 8-byte store
            *reinterpret_cast<int2*>(lds + r * G.row_stride + (c >> 1)) =
                make_int2((w.x & 0xffff) | (w.y << 16), (w.z & 0xffff) | (w.w << 16));
          } else if constexpr (STEP == 2) {  // c is a multiple of 4: even columns c, c+2 -> plane 0 at c/2; odd columns c+1, c+3 -> plane 1
            int32_t* row = lds + r * G.row_stride + (c >> 1);
            *reinterpret_cast<int2*>(row) = make_int2(w.x, w.z);
            *reinterpret_cast<int2*>(row + G.plane) = make_int2(w.y, w.w);
          } else {
            *reinterpret_cast<int4*>(lds + r * G.row_stride + c) = w;
          }
        }
      }
    }
  }
}

struct EvalArgs {
  const int32_t* integ;
  size_t int_frame_elems;
  int nchan;
  int tilt_chan;      // channel of the tilted integral, -1 if the cascade has no tilted feature
  const ScaleDev* sd;
  const int4* tiles;  // {scale, tx, ty, 0}
  int W0, H0;
  int nstages;
  const int* stage_first;  // first stump of each stage
  const int* stage_ntrees;
  const float* stage_thr;
  // Stage groups: group g covers stages group_first[g] .. group_first[g + 1] - 1 (ngroups + 1 entries, the last one =
  // nstages). The block compacts its surviving windows (queue rebuild + barrier) once per GROUP; inside a group a lane
  // keeps its window and leaves by predication. Group 0 is stage 0 alone (the dense phase; a dense group of several
  // stages was tried: a third inlined copy of the generated stages, more spills, slower). One stage per group = the old form.
  const int* group_first;
  int ngroups;
  // Queue form per group. The queue a group reads is a table [row][32]. Groups below `dense_from` keep one COLUMN per LDS
  // bank class (conflict-free corner gathers, but the table is as long as its fullest column); from group `dense_from`
  // on the table is a plain list filled row by row (wave-aggregated append): half as many rows at 50-100 windows per
  // tile, i.e. half the wavefront passes, for corner gathers that collide ~2.5-way. Worth it where the vector ALU, not the
  // LDS, is the busier pipe (LBP) and the tile is down to a few rows. INT_MAX = never.
  int dense_from;
  const void* stumps1;  // stump tables in STEP-1 / STEP-2 tile coordinates
  const void* stumps2;
  const void* wstumps1;  // Haar wave phase: per-stage reordered copies (NULL = use stumps1/2)
  const void* wstumps2;
  // Haar wave phase, per stage: wave_q[s] != 0 = the stage has an integer form. Its records in wstumps1/2 then carry the
  // leaves as int32 multiples of the quantum wave_q[s] (a power of two) in their leaf words, every stage sum is such a
  // multiple too (stage_quantum on the host), and `sum >= stage_thr[s]` is `multiple >= wave_thr_q[s]`. 0 = float leaves, sums in double.
  const double* wave_q;
  const int* wave_thr_q;
  const void* gstumps;  // the stump table with corners as (y << 16 | x) inside the window (GlobalReader; 16-bit tiles)
  int lbp16_all;         // LBP: every cell of the cascade sums below 2^16 and wstumps2 holds 16-bit-tile offsets (LBP wave phase)
  int trees;            // cascade has trees deeper than stumps: node tables below, no stump tables
  const void* nodes1;
  const void* nodes2;
  const int* tree_root;   // first node of each weak classifier
  const int* tree_leaf0;  // first leaf value of each weak classifier
  const float* leaves;
  int wave_below;       // switch to one wavefront per window when fewer windows than this are queued (0 = never)
  int early_skip;       // drop windows the scan loop provably never visits right after stage 0
  int sq_compact;       // squared sums of step-2 scales hold only what the variance test reads (odd rows, odd columns packed)
  int split_stumps;     // stage sums are exact (order-independent): wavefronts may split a stage's stumps
  int stop_after;       // timing experiments only: drop every window still alive after this stage (-1 = off)
  unsigned long long* masks;
  size_t mask_frame_words;
  CandRaw* cands;
  int* cand_count;
  int cand_cap;
  int32_t* dbg_codes;  // optional, frame 0 only
  double* dbg_sums;
  unsigned long long* stamps;  // timing experiments only (CCAMD_DEBUG_STAMPS): [block][STAMP_SLOTS] shader-clock stamps of wavefront 0
};
constexpr int STAMP_SLOTS = 40;  // 0 = block start, 1 = tile staged, 2 = dense phase done, 3 + st = stage st done, 39 = block end

// ---- one weak classifier on one window -------------------------------------------------------------------------
// Where a table-driven stump finds its corners. LdsReader: `b` = LDS address of the window's tile base, the record holds
// tile offsets. GlobalReader (16-bit tiles only): the record holds (y << 16 | x) inside the window and the corner is read
// from the 32-bit integral in global memory (L2-resident: the block staged the same rows a moment ago) -- the 16-bit tile
// cannot serve arbitrary rectangles, and the table-driven stages only see the few windows that are left by then.
struct LdsReader {
  const int32_t* b;
  __device__ __forceinline__ int operator()(int ofs) const { return b[ofs]; }
};
struct GlobalReader {
  const int32_t* g;  // the scale's sum integral (wave-uniform)
  unsigned org;      // element index of the window's origin
  int pitch;
  __device__ __forceinline__ int operator()(int p) const { return g[org + (unsigned)((p >> 16) * pitch + (p & 0xffff))]; }
};
template <class R>
__device__ __forceinline__ bool stump_goes_left(const R& rd, const HaarStumpDev& sp, float vnf) {
  const int r0 = rd(sp.ofs[0][0]) - rd(sp.ofs[0][1]) - rd(sp.ofs[0][2]) + rd(sp.ofs[0][3]);
  const int r1 = rd(sp.ofs[1][0]) - rd(sp.ofs[1][1]) - rd(sp.ofs[1][2]) + rd(sp.ofs[1][3]);
  float v = sp.w[0] * (float)r0 + sp.w[1] * (float)r1;
  if (sp.nrect == 3) {
    const int r2 = rd(sp.ofs[2][0]) - rd(sp.ofs[2][1]) - rd(sp.ofs[2][2]) + rd(sp.ofs[2][3]);
    v += sp.w[2] * (float)r2;
  }
  v *= vnf;
  return v < sp.thr;
}
template <class R>
__device__ __forceinline__ double stump_vote(const R& rd, const HaarStumpDev& sp, float vnf) {
  return (double)(stump_goes_left(rd, sp, vnf) ? sp.left : sp.right);
}
// The vote as the accumulator type of a wave-phase stage takes it. double: the leaf value. int: the record is one of the
// wave phase's own copies whose stage has an integer form, and its leaf words hold the leaves in units of the stage's
// quantum as int32 (EvalArgs::wave_q); they are picked as words, no float operation ever sees them.
template <class Acc, class R>
__device__ __forceinline__ Acc stump_vote_as(const R& rd, const HaarStumpDev& sp, float vnf) {
  if constexpr (sizeof(Acc) == sizeof(int))
    return stump_goes_left(rd, sp, vnf) ? __float_as_int(sp.left) : __float_as_int(sp.right);
  else
    return stump_vote(rd, sp, vnf);
}
template <class R>
__device__ __forceinline__ double stump_vote(const R& rd, const HaarStumpDev CC_CONST* spp, float vnf) {
  return stump_vote(rd, load_record(spp), vnf);
}

struct Lds16Reader {  // 16-bit tile: offsets count 16-bit entries from the window's tile base
  const unsigned short* h;
  __device__ __forceinline__ int operator()(int ofs) const { return (int)h[ofs]; }
};
// The vote of one LBP stump whose record sits in registers (LBP wave phase: a lane per stump). M16: the reader returns the
// low 16 bits of the integral, cell sums are taken modulo 2^16 (exact while 255 * cell area < 2^16). The subset word is
// picked from the record by the code's three top bits with selects -- no indexed access into the register copy.
template <bool M16, class R>
__device__ __forceinline__ float lbp_vote_f(const R& rd, const LbpStumpDev& sp) {
  int p[16];
#pragma unroll
  for (int j = 0; j < 16; j++) p[j] = rd(sp.ofs[j]);
  auto cell = [&](int a, int b, int c2, int d) {
    const int v = p[a] - p[b] - p[c2] + p[d];
    return M16 ? (v & 0xffff) : v;
  };
  const int c = cell(5, 6, 9, 10);
  const bool b7 = cell(0, 1, 4, 5) >= c, b6 = cell(1, 2, 5, 6) >= c, b5 = cell(2, 3, 6, 7) >= c;
  const int lo = (cell(6, 7, 10, 11) >= c ? 16 : 0) | (cell(10, 11, 14, 15) >= c ? 8 : 0) | (cell(9, 10, 13, 14) >= c ? 4 : 0) |
                 (cell(8, 9, 12, 13) >= c ? 2 : 0) | (cell(4, 5, 8, 9) >= c ? 1 : 0);
  const int l0 = b5 ? sp.subset[1] : sp.subset[0], l1 = b5 ? sp.subset[3] : sp.subset[2], l2 = b5 ? sp.subset[5] : sp.subset[4],
            l3 = b5 ? sp.subset[7] : sp.subset[6];
  const int m0 = b6 ? l1 : l0, m1 = b6 ? l3 : l2;
  const unsigned w = (unsigned)(b7 ? m1 : m0);
  return ((w >> lo) & 1u) ? sp.left : sp.right;
}

template <class R>
__device__ __forceinline__ double stump_vote(const R& rd, const LbpStumpDev CC_CONST* sp, float) {
  int p[16];
#pragma unroll
  for (int j = 0; j < 16; j++) p[j] = rd(sp->ofs[j]);
  const int c = p[5] - p[6] - p[9] + p[10];
  const int lbp = (p[0] - p[1] - p[4] + p[5] >= c ? 128 : 0) | (p[1] - p[2] - p[5] + p[6] >= c ? 64 : 0) |
                  (p[2] - p[3] - p[6] + p[7] >= c ? 32 : 0) | (p[6] - p[7] - p[10] + p[11] >= c ? 16 : 0) |
                  (p[10] - p[11] - p[14] + p[15] >= c ? 8 : 0) | (p[9] - p[10] - p[13] + p[14] >= c ? 4 : 0) |
                  (p[8] - p[9] - p[12] + p[13] >= c ? 2 : 0) | (p[4] - p[5] - p[8] + p[9] >= c ? 1 : 0);
  const int word = sp->subset[lbp >> 5];  // data-dependent word: read it from the table, not from a register copy
  return (double)((word & (1 << (lbp & 31))) ? sp->left : sp->right);
}

// One weak classifier that is a tree: walk from the root; each lane follows its own path (predictOrdered /
// predictCategorical). The loader guarantees child indices increase, so the walk ends.
__device__ __forceinline__ double tree_vote(const int32_t* b, const HaarNodeDev* __restrict__ nodes, int root, int leaf0,
                                            const float* __restrict__ leaves, float vnf) {
  int idx = 0;
  do {
    const HaarNodeDev* n = nodes + root + idx;
    const int r0 = b[n->ofs[0][0]] - b[n->ofs[0][1]] - b[n->ofs[0][2]] + b[n->ofs[0][3]];
    const int r1 = b[n->ofs[1][0]] - b[n->ofs[1][1]] - b[n->ofs[1][2]] + b[n->ofs[1][3]];
    float v = n->w[0] * (float)r0 + n->w[1] * (float)r1;
    if (n->nrect == 3) v += n->w[2] * (float)(b[n->ofs[2][0]] - b[n->ofs[2][1]] - b[n->ofs[2][2]] + b[n->ofs[2][3]]);
    v *= vnf;
    idx = v < n->thr ? n->left : n->right;
  } while (idx > 0);
  return (double)leaves[leaf0 - idx];
}
__device__ __forceinline__ double tree_vote(const int32_t* b, const LbpNodeDev* __restrict__ nodes, int root, int leaf0,
                                            const float* __restrict__ leaves, float) {
  int idx = 0;
  do {
    const LbpNodeDev* n = nodes + root + idx;
    int p[16];
#pragma unroll
    for (int j = 0; j < 16; j++) p[j] = b[n->ofs[j]];
    const int c = p[5] - p[6] - p[9] + p[10];
    const int lbp = (p[0] - p[1] - p[4] + p[5] >= c ? 128 : 0) | (p[1] - p[2] - p[5] + p[6] >= c ? 64 : 0) |
                    (p[2] - p[3] - p[6] + p[7] >= c ? 32 : 0) | (p[6] - p[7] - p[10] + p[11] >= c ? 16 : 0) |
                    (p[10] - p[11] - p[14] + p[15] >= c ? 8 : 0) | (p[9] - p[10] - p[13] + p[14] >= c ? 4 : 0) |
                    (p[8] - p[9] - p[12] + p[13] >= c ? 2 : 0) | (p[4] - p[5] - p[8] + p[9] >= c ? 1 : 0);
    idx = (n->subset[lbp >> 5] & (1 << (lbp & 31))) ? n->left : n->right;
  } while (idx > 0);
  return (double)leaves[leaf0 - idx];
}

// Maximum / sum of a non-negative int over the 64 lanes, wave-uniform; same DPP ladder as wave_sum_f64.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_i32(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xF, false);
}
__device__ __forceinline__ int wave_max_u32(int v) {
  v = max(v, dpp_i32<0xB1, 0xF>(v));
  v = max(v, dpp_i32<0x4E, 0xF>(v));
  v = max(v, dpp_i32<0x141, 0xF>(v));
  v = max(v, dpp_i32<0x140, 0xF>(v));
  v = max(v, dpp_i32<0x142, 0xA>(v));
  v = max(v, dpp_i32<0x143, 0xC>(v));
  return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ int wave_sum_u32(int v) {
  v += dpp_i32<0xB1, 0xF>(v);
  v += dpp_i32<0x4E, 0xF>(v);
  v += dpp_i32<0x141, 0xF>(v);
  v += dpp_i32<0x140, 0xF>(v);
  v += dpp_i32<0x142, 0xA>(v);
  v += dpp_i32<0x143, 0xC>(v);
  return __builtin_amdgcn_readlane(v, 63);
}
// The sum of a wave-phase stage's votes over the 64 lanes, by accumulator type. The int ladder is as good for signed
// terms (two's complement; the host guarantees no partial sum leaves int32): each step is ONE add that carries the DPP
// modifier, where a step of the double ladder is two DPP moves and a double add.
__device__ __forceinline__ int wave_total(int v) { return wave_sum_u32(v); }
__device__ __forceinline__ double wave_total(double v) { return wave_sum_f64(v); }

// (float)(1.0 / sqrt(nf)) -- setWindow's varianceNormFactor (SURVEY.md A.4) -- for nf > 0 (an integer-valued double: area *
// valsqsum - valsum^2), bit for bit, without the two correctly rounded double operations (~35 instructions: the dense
// phase spends 40 % of its vector ALU time on them). y = v_rsq_f64(nf) refined by two Newton steps is within 2^-50
// (relative) of 1 / sqrt(nf), the two-operation result within 2^-51; both therefore round to the same float unless y lies
// within a few double ulps of a float rounding boundary (the 29 bits below float precision equal to 2^28). Within 1024 ulps
// of one -- one window in 2^18 -- the two operations are done after all. Checked against them on the device over 2^32
// values of nf (cc_debug_vnf_check, tests/test_gpu_specialize.py). CC_EXACT_SLOW_VNF: always the two operations (A/B runs).
__device__ __forceinline__ float inv_sqrt_as_float(double nf) {
#ifndef CC_EXACT_SLOW_VNF
  double y = __builtin_amdgcn_rsq(nf);
#pragma unroll
  for (int it = 0; it < 2; it++) {
    const double e = __builtin_fma(-(nf * y), y, 1.0);  // 1 - nf y^2
    y = __builtin_fma(0.5 * y, e, y);
  }
  const unsigned below = (unsigned)(unsigned long long)__double_as_longlong(y) & 0x1fffffffu;
  if (__builtin_expect(below - 0x0ffffc00u > 0x800u, 1)) return (float)y;  // not within [2^28 - 1024, 2^28 + 1024]
#endif
  return (float)(1. / sqrt(nf));
}

#ifdef CC_SPEC_STAGES
// Run-time specialisation (cc_detector_specialize): stages 0 .. CC_SPEC_STAGES-1 of ONE stump cascade (Haar or LBP) as
// straight-line, software-pipelined code in which every LDS offset, weight, threshold and leaf value is an immediate.
// A stage is cut into SPEC_PARTS contiguous parts of stumps; spec_stage returns the sum over parts [p_lo, p_hi) for one
// window: (0, SPEC_PARTS) is the whole stage in stump order, a sub-range the share of one slice of the stump-split
// path. spec_stage0_x2 is stage 0 for the two windows a thread owns in the dense phase (their reads issued together).
// The host generates them for the two tile layouts and substitutes them for the marker line below.
template <int STEP>
__device__ __forceinline__ double spec_stage(int st, int p_lo, int p_hi, const int32_t* b, float vnf);
template <int STEP>
__device__ __forceinline__ void spec_stage0_x2(const int32_t* ba, const int32_t* bb, float vnfa, float vnfb, double& acc_a, double& acc_b);
//@@CC_SPEC_FUNCTIONS@@
#endif

template <bool C, class A, class B>
struct cc_select {
  using type = A;
};
template <class A, class B>
struct cc_select<false, A, B> {
  using type = B;
};

// What the thread phase hands to a wave phase: the group it stopped in front of and that group's queue.
struct QueueState {
  int qg = 1;  // current group = index of its queue table / counters
  int st = 1;  // first stage of the current group
  int n = 0, rows = 0, my_rows = 0;  // queued windows, rows of the table, rows that hold a window in this lane's column
};
// A wavefront's share of the queued windows in a wave phase: lane k < cnt holds the id of its k-th window.
struct WaveShare {
  int cnt, my_id;
  unsigned long long alive;  // bit k = the k-th window is still in the cascade
};

// One tile of one scale: what every phase of a block needs (all of it block- or lane-constant), the small rules the
// phases share, and the phases themselves. Everything is inlined into the kernel: eval_tile below is the whole sequence.
template <int STEP, bool HAAR, bool TREES>
struct EvalTile {
  using Stump = typename cc_select<HAAR, HaarStumpDev, LbpStumpDev>::type;
  using Node = typename cc_select<HAAR, HaarNodeDev, LbpNodeDev>::type;
  // 16-bit tile layout: run-time specialised builds the host compiled with CC_SPEC_TILE16, STEP-2 tiles only
#ifdef CC_SPEC_TILE16
  static constexpr bool G16 = STEP == 2 && !TREES;
#else
  static constexpr bool G16 = false;
#endif
  using Geom = typename cc_select<G16, TileGeom16, TileGeom<STEP>>::type;

  const EvalArgs& A;
  int32_t* const lds;
  const int4 T;
  const ScaleDev& S;
#ifdef CC_SPEC_W0  // run-time specialised build: the window size is a compile-time constant, and with it the tile geometry
  static constexpr int W0 = CC_SPEC_W0, H0 = CC_SPEC_H0;
#else
  const int W0 = A.W0, H0 = A.H0;
#endif
  const Geom G{W0, H0};
  // lean LDS layout (eval_lds_bytes): the run-time specialised Haar modules of one step each, compiled with CC_LEAN_LDS
#ifdef CC_LEAN_LDS
  static constexpr bool kLean = HAAR && !TREES;
#else
  static constexpr bool kLean = false;
#endif
  // (lean: no s_part area, see split_parts / wave_lists)
  double* const s_part = kLean ? nullptr : reinterpret_cast<double*>(lds + tile_words_padded(G.words()) * ((HAAR && A.tilt_chan >= 0) ? 2 : 1));
  // [TILE_Y][VNF_PITCH], lean [TILE_Y][TILE_X], see vnf_slot (Haar only)
  float* const s_vnf = kLean ? reinterpret_cast<float*>(lds + tile_words_padded(G.words())) : reinterpret_cast<float*>(s_part + PART_DOUBLES);
  unsigned short* const s_q = reinterpret_cast<unsigned short*>(s_vnf + (HAAR ? TILE_Y * (kLean ? TILE_X : VNF_PITCH) : 0));  // 2 tables [QUEUE_ROWS][32 classes]
  int* const s_cnt = reinterpret_cast<int*>(s_q + 2 * TILE_WINDOWS);  // [stage % 3][class] = queued windows
  const int frame = blockIdx.y;
  const int32_t* const sum = A.integ + ((size_t)frame * A.nchan + 0) * A.int_frame_elems + S.int_ofs;
  // the wave index is the same in all 64 lanes; say so, or every loop bounded by it is compiled as divergent
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int half = lane >> 5, cls = lane & 31;  // thread and wave phases: half-wavefront and queue column of the lane
  const int gx0 = T.y * TILE_X, gy0 = T.z * TILE_Y;
  const int skew = (STEP * G.row_stride) & 31;  // see win_class
  const Node* const nodes = reinterpret_cast<const Node*>(STEP == 2 ? A.nodes2 : A.nodes1);
  // table-driven stages: tile-offset records for the 32-bit tile of this layout; window-coordinate records (gstumps) when
  // the tile holds 16-bit entries and the corners come from global memory (GlobalReader)
  const Stump CC_CONST* const stumps = as_const_table(reinterpret_cast<const Stump*>(G16 ? A.gstumps : STEP == 2 ? A.stumps2 : A.stumps1));
  const int CC_CONST* const stage_first = as_const_table(A.stage_first);
  const int CC_CONST* const stage_ntrees = as_const_table(A.stage_ntrees);
  const float CC_CONST* const stage_thr = as_const_table(A.stage_thr);
  const int CC_CONST* const group_first = as_const_table(A.group_first);
  const double CC_CONST* const wave_q = as_const_table(A.wave_q);
  const int CC_CONST* const wave_thr_q = as_const_table(A.wave_thr_q);
  const bool dbg = A.dbg_codes != nullptr && frame == 0;

  __device__ __forceinline__ EvalTile(const EvalArgs& A_, int32_t* lds_, const int4 T_, const ScaleDev& S_) : A(A_), lds(lds_), T(T_), S(S_) {}

  // ---- the rules the phases share ---------------------------------------------------------------------------------
  // Tile row of this wavefront's k-th round of the staging and dense phases, and whether the tile has that row (wave-uniform;
  // only the last round of a height that is no multiple of the wavefronts can lie beyond the tile). See WIN_PER_THREAD.
  __device__ __forceinline__ int own_row(int k) const { return RAGGED_ROWS ? wave + k * EVAL_WAVES : wave * WIN_PER_THREAD + k; }
  __device__ __forceinline__ bool has_row(int k) const { return !RAGGED_ROWS || k < WIN_PER_THREAD - 1 || own_row(k) < TILE_Y; }
  __device__ __forceinline__ void stamp(int slot) const {  // wavefront 0 only; the buffer is read by nothing but the experiment's host code
    if (A.stamps && threadIdx.x == 0)
      A.stamps[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * STAMP_SLOTS + slot] = __builtin_amdgcn_s_memtime();
  }
  __device__ __forceinline__ int window_base(int id) const { return ((id >> 6) * STEP) * G.row_stride + (id & 63); }
  // where the table-driven stump records of window `id` find their corners (see LdsReader / GlobalReader)
  __device__ __forceinline__ auto table_reader(int id) const {
    if constexpr (G16)
      return GlobalReader{sum, (unsigned)((gy0 + (id >> 6)) * STEP) * (unsigned)S.pitchI + (unsigned)((gx0 + (id & 63)) * STEP), S.pitchI};
    else
      return LdsReader{lds + window_base(id)};
  }
  __device__ __forceinline__ void report(int id, int code, double last) const {  // parity instrumentation
    const size_t o = (size_t)S.win_ofs + (size_t)(gy0 + (id >> 6)) * S.nx + (gx0 + (id & 63));
    A.dbg_codes[o] = code;
    if (A.dbg_sums) A.dbg_sums[o] = last;
  }
  __device__ __forceinline__ void emit_candidate(int id, double last_sum) const {
    const int slot = atomicAdd(A.cand_count, 1);
    if (slot < A.cand_cap) A.cands[slot] = CandRaw{frame, T.x, gx0 + (id & 63), gy0 + (id >> 6), last_sum};
  }
  // Bank class of a window: its tile base mod 32 (every corner read of a stage adds the same constant for all windows).
  __device__ __forceinline__ int win_class(int id) const { return ((id & 63) + skew * (id >> 6)) & 31; }
  // s_vnf is laid out so that a window's entry sits on the bank of its class as well (up to the area's own bank offset,
  // the same for all windows): rows of pitch TILE_X + skew; lean layout: rows of pitch TILE_X, row r rotated by r * skew
  // columns -- slot = 64 r + ((x + r skew) mod 64), whose bank is (x + r skew) mod 32 = win_class, and the rotation maps a
  // row's 64 columns onto its 64 slots one to one.
  __device__ __forceinline__ int vnf_slot(int id) const {
    if constexpr (kLean)
      return (id & ~63) | (((id & 63) + skew * (id >> 6)) & 63);
    else
      return (id >> 6) * (TILE_X + skew) + (id & 63);
  }
  // Index into s_q of entry (row, c) of the queue table of group g. Lean layout: table 1 runs backwards from the end of the
  // area. queued: the entry itself, for a reader that holds `q` = where group g's table starts in the other layout.
  __device__ __forceinline__ int q_index(int g, int row, int c) const {
    if constexpr (kLean)
      return (g & 1) ? (2 * QUEUE_ROWS - 1 - row) * 32 + c : row * 32 + c;
    else
      return (g & 1) * TILE_WINDOWS + row * 32 + c;
  }
  __device__ __forceinline__ int queued(const unsigned short* q, int g, int row, int c) const {
    if constexpr (kLean)
      return s_q[q_index(g, row, c)];
    else
      return q[row * 32 + c];
  }
  // Lean layout, stump-split phase: the partial sums sit behind row `rows` of table 0, in the gap between the two tables
  // (neither holds more than `rows` rows in this group; the caller has checked lean_split_gap_bytes).
  __device__ __forceinline__ double* split_parts(int rows) const {
    if constexpr (kLean)
      return reinterpret_cast<double*>(s_q + rows * 32);
    else
      return s_part;
  }
  // Wave phases: a list of 64 window ids per wavefront. Lean layout: in the far end of the table that group h.qg does not
  // read -- a wave phase queues nothing, so that table is dead, and a table (TILE_WINDOWS >= 256 entries) holds the lists.
  __device__ __forceinline__ unsigned short* wave_lists(int qg) const {
    if constexpr (kLean)
      return s_q + ((qg & 1) ? 0 : 2 * TILE_WINDOWS - EVAL_WAVES * 64);
    else
      return reinterpret_cast<unsigned short*>(s_part);
  }
  // Appends the calling lanes with `pass` to the queue table of stage `st`: next free row of the window's class column.
  // The 32 lanes of a half-wavefront always hold windows of 32 different classes here (dense phase: 32 consecutive
  // columns of one row; thread phase: by construction of the table), so the atomics never meet on one counter.
  __device__ __forceinline__ void enqueue(bool pass, int id, int g) const {  // g = stage group whose queue receives the window
    if (g >= A.dense_from) {  // block-uniform. Every call site runs with all 64 lanes of the wavefront active.
      const unsigned long long m = __ballot(pass);
      int first = 0;
      if (lane == 0 && m) first = atomicAdd(&s_cnt[(g % 3) * 32], __builtin_popcountll(m));
      first = __builtin_amdgcn_readfirstlane(first);
      if constexpr (kLean) {
        const int i = first + lane_rank(m);
        if (pass) s_q[q_index(g, i >> 5, i & 31)] = (unsigned short)id;
      } else if (pass)
        s_q[(g & 1) * TILE_WINDOWS + first + lane_rank(m)] = (unsigned short)id;
    } else if (pass) {
      const int c = win_class(id);
      const int row = atomicAdd(&s_cnt[(g % 3) * 32 + c], 1);
      if constexpr (kLean)
        s_q[q_index(g, row, c)] = (unsigned short)id;
      else
        s_q[(g & 1) * TILE_WINDOWS + row * 32 + c] = (unsigned short)id;
    }
  }
  // A window that passed the last stage of its group: a candidate when that was the cascade's last group, otherwise it
  // queues for the next group. Called with all 64 lanes active (enqueue). The queue is marked as the straight path: without
  // the hint the compiler lays the candidate branch in front of it in the thread phase (table-driven kernels 0.4 % slower).
  __device__ __forceinline__ void deliver(bool pass, int id, double last_sum, bool last_group, int next_group) const {
    if (__builtin_expect(last_group, false)) {
      if (pass) {
        emit_candidate(id, last_sum);
        if (dbg) report(id, 1, last_sum);
      }
    } else
      enqueue(pass, id, next_group);
  }
  // Stage-0 skip rule, applied early: the scan loop never visits a window whose run of consecutive stage-0
  // rejections immediately to its left has odd length (k_filter_candidates), so such a window can stop here instead
  // of walking the later stages for nothing. The run is read off the row's ballot mask `m`; when it reaches the left edge
  // of this tile its length is only known for the first tile of a row, otherwise the window is kept (the final
  // filter decides). The parity instrumentation evaluates every window, so it is skipped there.
  __device__ __forceinline__ bool never_visited(unsigned long long m) const {
    bool never = false;
    if (!dbg && A.early_skip) {
      const unsigned long long lower = (1ull << lane) - 1ull;
      const unsigned long long zeros_below = ~m & lower;  // lower lanes that were NOT rejected at stage 0
      int run;
      bool known;
      if (zeros_below) {
        run = lane - 1 - (63 - __clzll((long long)zeros_below));
        known = true;
      } else {
        run = lane;
        known = T.y == 0;
      }
      if (known && (run & 1)) never = true;
    }
    return never;
  }
  // Stage-0 outcome of the wavefront's window row `ly` (lane = column): writes the row's rejection mask word and returns
  // whether the lane's window goes on. mask_col = mask_column(), worked out once per phase by the caller: formed here, the
  // compiler reloads the kernel arguments behind it, with a wait, for every row.
  __device__ __forceinline__ unsigned long long* mask_column() const {
    return A.masks + (size_t)frame * A.mask_frame_words + S.mask_ofs + T.y;
  }
  __device__ __forceinline__ bool stage0_outcome(int ly, bool alive, double acc, double thr, unsigned long long* mask_col) const {
    const int gy = gy0 + ly;
    bool pass = alive && !(acc < thr);
    const bool rej0 = alive && !pass;
    const unsigned long long m = __ballot(rej0);
    if (lane == 0 && gy < S.ny) mask_col[(size_t)gy * S.nxw] = m;
    if (dbg && rej0) report(ly * 64 + lane, 0, acc);
    if (never_visited(m)) pass = false;  // (every lane works it out: no branch on `pass`)
    return pass;
  }
  // Sum of one whole stage for one window, in stump order (the CPU's order). `want` only saves work for lanes whose
  // result is not used (tree walks); every lane addresses a window inside the tile either way.
  __device__ __forceinline__ double stage_sum(int s, int id, const int32_t* b, float vnf, bool want) const {
    double acc = 0.;
    const int first = stage_first[s], nt = stage_ntrees[s];
    if constexpr (TREES) {
      for (int j = 0; j < nt; j++) {
        const int root = as_const_table(A.tree_root)[first + j], leaf0 = as_const_table(A.tree_leaf0)[first + j];
        if (want) acc += tree_vote(b, nodes, root, leaf0, A.leaves, vnf);
      }
    } else {
#ifdef CC_SPEC_STAGES
      if (s < CC_SPEC_STAGES) return spec_stage<STEP>(s, 0, SPEC_PARTS, b, vnf);
#endif
      acc = table_sum(table_reader(id), first, nt, 0, 1, vnf);
    }
    return acc;
  }
  // Stumps lo, lo + step, ... of the `nt` >= 1 table-driven stumps from `first` on, for one window. Haar: software pipeline,
  // the next stump record is fetched (scalar loads) while this one is evaluated.
  template <class R>
  __device__ __forceinline__ double table_sum(const R& rd, int first, int nt, int lo, int step, float vnf) const {
    double acc = 0.;
    if constexpr (HAAR) {
      if (lo == 0 || lo < nt) {  // lo == 0 (a whole stage, a constant after inlining): the first load needs no test, nt >= 1
        Stump cur = load_record(stumps + first + lo);
        for (int j = lo; j < nt; j += step) {
          const Stump nxt = load_record(stumps + first + min(j + step, nt - 1));
          acc += stump_vote(rd, cur, vnf);
          cur = nxt;
        }
      }
    } else {
      for (int j = lo; j < nt; j += step) acc += stump_vote(rd, stumps + first + j, vnf);
    }
    return acc;
  }
  // Deals the queued windows of group h.qg to the wavefronts (both wave phases). Windows are numbered in table order (a
  // ballot per pair of rows) and dealt round-robin: wavefront w takes numbers w, w + EVAL_WAVES, ... and keeps its k-th
  // window's id in lane k. Every wavefront numbers the whole table itself and writes only its own share to a private list
  // (wave_lists: s_part is free here, its last readers finished before the barrier at the top of this stage; lean layout:
  // the other queue table, whose last readers finished before the same barrier); the host keeps wave_below <= 64, so a
  // share fits the 64 lanes.
  __device__ __forceinline__ WaveShare deal_windows(const QueueState& h) const {
    const unsigned short* q = s_q + (h.qg & 1) * TILE_WINDOWS;
    unsigned short* my_list = wave_lists(h.qg) + wave * 64;
    int numbered = 0;
    for (int r0 = 0; r0 < h.rows; r0 += 2) {
      const int row = r0 + half;
      const bool valid = row < h.my_rows;
      const int id = valid ? queued(q, h.qg, row, cls) : 0;
      const unsigned long long mask = __ballot(valid);
      const int number = numbered + lane_rank(mask);
      if (valid && number % EVAL_WAVES == wave) my_list[number / EVAL_WAVES] = (unsigned short)id;
      numbered += __builtin_popcountll(mask);
    }
    const int cnt = (numbered - wave + EVAL_WAVES - 1) / EVAL_WAVES;
    return WaveShare{cnt, lane < cnt ? my_list[lane] : 0, cnt >= 64 ? ~0ull : ((1ull << cnt) - 1ull)};
  }

  // ---- staging: the squared-sum corners of the variance test and the tile(s) of the integral --------------------------
  // The squared-sum integral is needed at 4 corners per window only: read them from global memory, and issue those
  // loads before the tile is staged so that their latency hides under the staging (they are combined afterwards).
  __device__ __forceinline__ void stage_phase(unsigned (&valsq_pre)[WIN_PER_THREAD]) const {
    unsigned sq_raw[WIN_PER_THREAD][4];
#pragma unroll
    for (int k = 0; k < WIN_PER_THREAD; k++) {
      sq_raw[k][0] = sq_raw[k][1] = sq_raw[k][2] = sq_raw[k][3] = 0;
      if (HAAR && has_row(k)) {
        // windows outside the grid read the last grid window's corners (unconditional loads: a branch here would make the
        // compiler wait for the data on the spot); they are never alive
        const int gx = min(gx0 + lane, S.nx - 1), gy = min(gy0 + own_row(k), S.ny - 1);
        const unsigned* sq = reinterpret_cast<const unsigned*>(A.integ + ((size_t)frame * A.nchan + 1) * A.int_frame_elems + S.int_ofs);
        const int nrx = W0 - 2, nry = H0 - 2;
        size_t q0;
        int dx;
        if (STEP == 2 && A.sq_compact) {  // odd rows only, odd columns packed: entry (row, 2c+1) sits at row*pitchI + c
          q0 = (size_t)(gy * 2 + 1) * S.pitchI + gx;
          dx = nrx >> 1;
        } else {
          q0 = (size_t)(gy * STEP + 1) * S.pitchI + (gx * STEP + 1);
          dx = nrx;
        }
        sq_raw[k][0] = sq[q0];
        sq_raw[k][1] = sq[q0 + dx];
        sq_raw[k][2] = sq[q0 + (size_t)nry * S.pitchI];
        sq_raw[k][3] = sq[q0 + (size_t)nry * S.pitchI + dx];
      }
    }
#ifdef CC_PRIO_STAGE  // tuning (hiprtc -D): issue priority of a block's wavefronts while they stage their tile
    __builtin_amdgcn_s_setprio(CC_PRIO_STAGE);
#endif
    stage_tile<STEP>(lds, G, sum, S, gx0 * STEP, gy0 * STEP);
    if (HAAR && A.tilt_chan >= 0)  // second tile right behind the first: tilted stumps simply carry offsets shifted by it (never with 16-bit tiles)
      stage_tile<STEP>(lds + tile_words_padded(G.words()), G,
                       A.integ + ((size_t)frame * A.nchan + A.tilt_chan) * A.int_frame_elems + S.int_ofs, S, gx0 * STEP, gy0 * STEP);
    if (threadIdx.x < 3 * 32) s_cnt[threadIdx.x] = 0;
#pragma unroll
    for (int k = 0; k < WIN_PER_THREAD; k++) valsq_pre[k] = sq_raw[k][0] - sq_raw[k][1] - sq_raw[k][2] + sq_raw[k][3];
    __syncthreads();
#ifdef CC_PRIO_STAGE
    __builtin_amdgcn_s_setprio(0);
#endif
  }

  // ---- phase D: variance test + stage 0, WIN_PER_THREAD window rows per thread ----------------------------------------
  // LBP stump kernels with more than two rows per thread (the 20-row tiles of the specialised LBP kernel: five) take the
  // rows one after the other in a rolled loop: there is no variance test to batch, and five unrolled copies of stage 0
  // kept 25 VGPRs in scratch (1.07 GB of spill stores per 32-frame launch in the counters). Same operations per window.
  static constexpr bool kRolledDense = !HAAR && !TREES && WIN_PER_THREAD > 2;
  __device__ __forceinline__ void dense_phase_rolled() const {
    const int gx = gx0 + lane;
    const double thr0 = (double)stage_thr[0];
    unsigned long long* const mask_col = mask_column();
    [[maybe_unused]] const int nt0 = stage_ntrees[0];
#pragma unroll 1
    for (int k = 0; k < WIN_PER_THREAD; k++) {
      if (!has_row(k)) continue;
      const int ly = own_row(k);
      const int32_t* b = lds + (ly * STEP) * G.row_stride + lane;
      const bool alive = gx < S.nx && gy0 + ly < S.ny;
      double acc = 0.;
      if (__any(alive)) {
#ifdef CC_SPEC_STAGES
        acc = spec_stage<STEP>(0, 0, SPEC_PARTS, b, 1.f);
#else
        for (int i = 0; i < nt0; i++) acc += stump_vote(LdsReader{b}, stumps + i, 1.f);
#endif
      }
      deliver(stage0_outcome(ly, alive, acc, thr0, mask_col), ly * 64 + lane, acc, A.nstages == 1, 1);
    }
  }
  // Returns false when the block ends here (stop_after == -3).
  __device__ __forceinline__ bool dense_phase(const unsigned (&valsq_pre)[WIN_PER_THREAD]) const {
    int base[WIN_PER_THREAD];
    float vnf[WIN_PER_THREAD];
    bool alive[WIN_PER_THREAD];
    const int gx = gx0 + lane;
#pragma unroll
    for (int k = 0; k < WIN_PER_THREAD; k++) {
      const int ly = own_row(k);
      const int gy = gy0 + ly;
      base[k] = (ly * STEP) * G.row_stride + lane;
      vnf[k] = 1.f;
      alive[k] = has_row(k) && gx < S.nx && gy < S.ny;
      if (HAAR) {
        const bool in_grid = alive[k];
        alive[k] = false;
        if (in_grid) {
          const int nrx = W0 - 2, nry = H0 - 2;
          const double area = (double)(nrx * nry);
          const int32_t* b = lds + base[k];
          int valsum;
          if constexpr (G16) {  // left and right half of the variance rectangle: each sum is exact modulo 2^16 (checked by the host)
            const unsigned short* h = reinterpret_cast<const unsigned short*>(b);
            const int hx = nrx >> 1;
            const unsigned a0 = h[G.at(1, 1)], a1 = h[G.at(1, 1 + hx)], a2 = h[G.at(1, 1 + nrx)];
            const unsigned c0 = h[G.at(1 + nry, 1)], c1 = h[G.at(1 + nry, 1 + hx)], c2 = h[G.at(1 + nry, 1 + nrx)];
            valsum = (int)(((a0 - a1 - c0 + c1) & 0xffffu) + ((a1 - a2 - c1 + c2) & 0xffffu));
          } else
            valsum = b[G.at(1, 1)] - b[G.at(1, 1 + nrx)] - b[G.at(1 + nry, 1)] + b[G.at(1 + nry, 1 + nrx)];
          const unsigned valsq = valsq_pre[k];
          double nf = area * (double)valsq - (double)valsum * (double)valsum;
          if (nf > 0.) {
            vnf[k] = inv_sqrt_as_float(nf);
            alive[k] = area * (double)vnf[k] < 1e-1;
          }
          if (dbg && !alive[k]) report(ly * 64 + lane, -1, 0.0);
        }
      }
    }
    if (A.stop_after == -3) {  // timing experiments: staging + variance test only
      float sink = 0;
#pragma unroll
      for (int k = 0; k < WIN_PER_THREAD; k++) sink += alive[k] ? vnf[k] : 0.f;
      if (HAAR && sink == 12345.f) s_vnf[0] = sink;
      return false;
    }
    bool any_mine = false;
    double acc[WIN_PER_THREAD];
#pragma unroll
    for (int k = 0; k < WIN_PER_THREAD; k++) {
      any_mine |= alive[k];
      acc[k] = 0.;
    }
    if (__any(any_mine)) {
      [[maybe_unused]] const int nt = stage_ntrees[0];
      if constexpr (TREES) {
        for (int i = 0; i < nt; i++) {
          const int root = as_const_table(A.tree_root)[i], leaf0 = as_const_table(A.tree_leaf0)[i];
#pragma unroll
          for (int k = 0; k < WIN_PER_THREAD; k++)
            if (alive[k]) acc[k] += tree_vote(lds + base[k], nodes, root, leaf0, A.leaves, vnf[k]);
        }
      } else {
#ifdef CC_SPEC_STAGES  // the generated stage 0: the two rows of a thread together where the tile gives it two
        if constexpr (WIN_PER_THREAD == 2 && !RAGGED_ROWS) {
          spec_stage0_x2<STEP>(lds + base[0], lds + base[1], vnf[0], vnf[1], acc[0], acc[1]);
        } else {
#pragma unroll
          for (int k = 0; k < WIN_PER_THREAD; k++)
            if (has_row(k)) acc[k] = spec_stage<STEP>(0, 0, SPEC_PARTS, lds + base[k], vnf[k]);
        }
#else
        if constexpr (HAAR) {
          // software pipeline: the next stump record is fetched (scalar loads) while this one is evaluated
          Stump cur = load_record(stumps);
          for (int i = 0; i < nt; i++) {
            const Stump nxt = load_record(stumps + min(i + 1, nt - 1));
#pragma unroll
            for (int k = 0; k < WIN_PER_THREAD; k++)
              if (has_row(k)) acc[k] += stump_vote(LdsReader{lds + base[k]}, cur, vnf[k]);
            cur = nxt;
          }
        } else {
          for (int i = 0; i < nt; i++) {
#pragma unroll
            for (int k = 0; k < WIN_PER_THREAD; k++)
              if (has_row(k)) acc[k] += stump_vote(LdsReader{lds + base[k]}, stumps + i, vnf[k]);
          }
        }
#endif
      }
    }
    const double thr = (double)stage_thr[0];
    unsigned long long* const mask_col = mask_column();
    bool pass_k[WIN_PER_THREAD];
#pragma unroll
    for (int k = 0; k < WIN_PER_THREAD; k++)  // (a row beyond the tile is another block's: no mask word, nothing delivered)
      pass_k[k] = has_row(k) && stage0_outcome(own_row(k), alive[k], acc[k], thr, mask_col);
    const bool last_group = A.nstages == 1;
#pragma unroll
    for (int k = 0; k < WIN_PER_THREAD; k++) {
      if (!has_row(k)) continue;
      const int id = own_row(k) * 64 + lane;
      if (HAAR && pass_k[k] && !last_group) s_vnf[vnf_slot(id)] = vnf[k];  // LBP blocks have no s_vnf area (eval_lds_bytes)
      deliver(pass_k[k], id, acc[k], last_group, 1);
    }
    return true;
  }

  // ---- phase T: one thread per queued window, stage by stage -----------------------------------------------------------
  // Half-wavefront h of wavefront g takes queue row 2g + h; its lane l the window of class l in that row (if the class
  // has that many). With few rows queued and order-independent (exact) stage sums, the block's wavefronts also SPLIT
  // THE STUMPS of the stage (slices j = slice, slice+ns, ...): the partial sums meet in LDS and slice 0 finishes the
  // window. This keeps all wavefronts busy through the long late stages instead of leaving one wave to walk them.
  // Returns false when the block ends here (stop_after); otherwise h says where the phase stopped.
  __device__ __forceinline__ bool thread_phase(QueueState& h) const {
    for (; h.qg < A.ngroups; h.qg++) {
      const int qg = h.qg;
      const int st = h.st = group_first[qg];
      const int st_end = group_first[qg + 1];
      if (A.stop_after >= 0 && st > A.stop_after) return false;
      __syncthreads();  // queue of group qg complete; previous readers of the buffers it overwrites are done
      // (the counts are clamped to what the tables can hold: a count that some bug corrupted must not become a loop bound
      // of 2^30 trips on a device where waves that never finish take the node down)
      if (qg >= A.dense_from) {  // plain list: entry i sits in row i / 32, column i % 32
        h.n = min(s_cnt[(qg % 3) * 32], TILE_WINDOWS);
        h.rows = (h.n + 31) >> 5;
        h.my_rows = max(0, (h.n - cls + 31) >> 5);  // rows that hold an entry in this lane's column
      } else {
        h.my_rows = min(s_cnt[(qg % 3) * 32 + cls], QUEUE_ROWS);  // windows queued in this lane's class
        h.rows = wave_max_u32(h.my_rows);                            // both halves hold the same 32 counts
        h.n = wave_sum_u32(h.my_rows) >> 1;
      }
      if (threadIdx.x < 32) s_cnt[((qg + 2) % 3) * 32 + threadIdx.x] = 0;  // counters of group qg+2 (last read in group qg-1)
      if (st + 2 < STAMP_SLOTS - 1) stamp(st + 2);  // the previous group (and the barrier behind it) done
      if (h.n == 0 || h.n < A.wave_below) break;
      const unsigned short* q = s_q + (qg & 1) * TILE_WINDOWS;
      const bool last_group = st_end >= A.nstages;
      const int groups = (h.rows + 1) >> 1;  // wavefronts needed to give every queue row a half-wavefront
      // Whole rounds of EVAL_WAVES row groups run one group per wavefront; the groups left over (all of them when there are
      // fewer groups than wavefronts) are split by stumps over the wavefronts, so that no wavefront walks a whole extra
      // pass alone while the others wait at the barrier. Only a group that is ONE stage can be split that way (the sum of
      // a stage must be known before the next one starts).
      const bool may_split = A.split_stumps && st_end - st == 1;
      const int g_split = may_split ? groups - groups % EVAL_WAVES : groups;  // first row group of the split part
      const int rem = groups - g_split;
      int ns = 1;                          // stump slices of the split part
      if (rem > 0)
        while (ns * 2 * rem <= EVAL_WAVES) ns *= 2;  // largest power of two with ns * rem <= wavefronts
      if constexpr (kLean)  // the partial sums travel between the queue tables (split_parts): as many slices as fit there
        while (ns > 1 && split_part_bytes(ns) > lean_split_gap_bytes(TILE_Y, h.rows)) ns >>= 1;
      // each lane walks the group's stages with its window; no barrier and no re-queueing between them, a window that
      // fails records its exit and only stops counting
      const int g_end = ns == 1 ? groups : g_split;
      for (int g = wave; g < g_end; g += EVAL_WAVES) {  // wave-uniform trip count
        const int row = g * 2 + half;
        const bool valid = row < h.my_rows;
        // a lane without a window evaluates the (in-tile) window `cls` of its own class, so it stays off the others' banks
        const int id = valid ? queued(q, qg, row, cls) : cls;
        const int32_t* b = lds + window_base(id);
        const float vnf = HAAR ? s_vnf[vnf_slot(id)] : 1.f;
        bool alive = valid;
        double acc = 0.;
        for (int s2 = st; s2 < st_end; s2++) {
          if (s2 > st && !__any(alive)) break;
          const double a = stage_sum(s2, id, b, vnf, alive);
          const bool pass = alive && !(a < (double)stage_thr[s2]);
          if (dbg && alive && !pass) report(id, -s2, a);
          if (alive) acc = a;
          alive = pass;
        }
        deliver(alive, id, acc, last_group, qg + 1);
      }
      if (ns > 1) split_stage(h, q, last_group, g_split, rem, ns);
    }
    return true;
  }
  // The stump-split part of a one-stage group: row groups g_split .. g_split + rem - 1, each cut into ns stump slices.
  __device__ __forceinline__ void split_stage(const QueueState& h, const unsigned short* q, bool last_group, int g_split, int rem, int ns) const {
    const int st = h.st;
    const int first = stage_first[st], nt = stage_ntrees[st];
    const int slice = wave % ns, grp = wave / ns;  // EVAL_WAVES / ns groups >= `rem`
    const int row = (g_split + grp) * 2 + half;
    const int i = grp * 64 + lane;
    const bool valid = row < h.my_rows;
    const int id = valid ? queued(q, h.qg, min(row, QUEUE_ROWS - 1), cls) : cls;  // (QUEUE_ROWS is not a power of two for every tile height)
    double acc = 0.;
    if (grp < rem) {
      [[maybe_unused]] const int32_t* b = lds + window_base(id);
      const float vnf = HAAR ? s_vnf[vnf_slot(id)] : 1.f;
#ifdef CC_SPEC_STAGES
      if (!TREES && st < CC_SPEC_STAGES)
        acc = spec_stage<STEP>(st, slice * (SPEC_PARTS / ns), (slice + 1) * (SPEC_PARTS / ns), b, vnf);
      else
#endif
        acc = table_sum(table_reader(id), first, nt, slice, ns, vnf);
      if (slice) split_parts(h.rows)[(slice - 1) * (EVAL_THREADS / ns) + i] = acc;  // <= (EVAL_WAVES - 1) * 64 entries for every ns
    }
    __syncthreads();  // partial sums visible
    if (grp < rem && slice == 0) {
      for (int k = 1; k < ns; k++) acc += split_parts(h.rows)[(k - 1) * (EVAL_THREADS / ns) + i];
      const bool pass = valid && !(acc < (double)stage_thr[st]);
      if (dbg && valid && !pass) report(id, -st, acc);
      deliver(pass, id, acc, last_group, h.qg + 1);
    }
  }

  // ---- phase W: one wavefront per window, lanes split the stumps -------------------------------------------------------
  // A wavefront takes its share of the queued windows (deal_windows) and walks them STAGE BY STAGE: lane j fetches stump
  // j's record once per stage (a per-lane 64-byte global load, the slow part) and keeps it in registers while the
  // wavefront's windows are evaluated against it one after the other. Lane k carries the stage sum of the wavefront's
  // k-th window.
  // A stage's sum is formed in one of two arithmetic forms, chosen per stage (wave-uniform) by the host's table wave_q: in
  // int32 multiples of the stage's quantum where the host has proved that every subset sum of the stage's votes is one
  // (stage_quantum) -- an integer vote is a select between two record words, and the 64 votes meet in six DPP adds -- and
  // in double otherwise. Either is the exact real sum of the votes, so (double)multiple * quantum IS the double sum.
  // wave_stage returns lane k's window's sum in the accumulator's units. The votes are reduced once per chunk of 64 stumps:
  // keeping a share's partial sums in registers over the chunks (one reduction per window and stage, the windows walked by an
  // unrolled loop) was measured slower, profiles/EXPERIMENTS.md 3.19.
  template <class Acc>
  __device__ __forceinline__ Acc wave_stage(const Stump* wstumps, int s2, unsigned long long alive, int my_id) const {
    const int first = stage_first[s2], nt = stage_ntrees[s2];
    Acc tot = 0;
    for (int c = 0; c < nt; c += 64) {
      const int j = c + lane;
      const Stump rec = wstumps[first + min(j, nt - 1)];
      for (unsigned long long m = alive; m; m &= m - 1ull) {
        const int k = __builtin_ctzll(m);
        const int id = __builtin_amdgcn_readlane(my_id, k);
        const float vnf = s_vnf[vnf_slot(id)];
        const Acc part = j < nt ? stump_vote_as<Acc>(table_reader(id), rec, vnf) : Acc(0);
        const Acc total = wave_total(part);
        if (lane == k) tot += total;
      }
    }
    return tot;
  }
  __device__ __forceinline__ void wave_phase_haar(const QueueState& h) const {
    const int st = h.st;
    const Stump* wstumps = reinterpret_cast<const Stump*>(G16 ? A.gstumps : STEP == 2 ? A.wstumps2 : A.wstumps1);
    const WaveShare w = deal_windows(h);
    const int cnt = w.cnt, my_id = w.my_id;
    unsigned long long alive = w.alive;
    const bool w_stamps = st + 2 < 30;  // stamp slots 30.. are free then: 30 = windows collected, 31 + i = i-th wave-phase stage done
    if (w_stamps) stamp(30);
    double last = 0.;
    int rej = 0;
    int s2 = st;
    for (; s2 < A.nstages && alive; s2++) {
      if (A.stop_after >= 0 && s2 > A.stop_after) break;
      const double q = G16 ? 0. : wave_q[s2];  // (kernels with 16-bit tiles read gstumps here, which other phases read too: float leaves)
      double tot;
      bool at_least_thr;
      if (q != 0.) {
        const int n = wave_stage<int>(wstumps, s2, alive, my_id);
        tot = (double)n * q;
        at_least_thr = n >= wave_thr_q[s2];
      } else {
        tot = wave_stage<double>(wstumps, s2, alive, my_id);
        at_least_thr = !(tot < (double)stage_thr[s2]);
      }
      const bool mine = (alive >> lane) & 1ull;
      const bool pass = mine && at_least_thr;
      if (mine) {
        last = tot;
        if (!pass) rej = s2;
      }
      alive = __ballot(pass);
      if (w_stamps && s2 - st < 8) stamp(31 + s2 - st);
    }
    const bool accepted = s2 == A.nstages && ((alive >> lane) & 1ull);
    if (lane < cnt) {
      if (accepted) emit_candidate(my_id, last);
      if (dbg && (accepted || !((alive >> lane) & 1ull))) report(my_id, accepted ? 1 : -rej, last);
    }
  }
  // ---- phase W for LBP stump cascades: one wavefront per window, lanes = the stumps of SEVERAL stages -------------------
  // LBP stages are short (3-10 stumps in the stock cascade) and a stump is a long dependent chain (16 corner reads, nine
  // cell sums, eight comparisons, the subset bit), so once a tile is down to a few windows every further stage costs a
  // barrier round plus its stumps' latencies one after the other -- 40 % of a block's life for a handful of windows
  // (profiles/r03_block_stamps.txt). Here a wavefront takes a window and its 64 lanes take the next <= 64 stumps of the
  // cascade at once, whole stages only: every lane evaluates one stump (its record sits in registers for all of the
  // wavefront's windows), the votes go to a small LDS scratch, and the first lanes add up one stage each IN STUMP ORDER --
  // the CPU's order, so no exactness condition is needed -- and test it; the first failing stage is the window's result.
  // Stages behind a failing one were evaluated for nothing, which costs no time: they ran in the same pass.
  __device__ __forceinline__ void wave_phase_lbp(const QueueState& h) const {
    float* votes = reinterpret_cast<float*>(reinterpret_cast<char*>(s_part) + EVAL_WAVES * 128) + wave * 64;  // behind the lists of deal_windows
    const WaveShare w = deal_windows(h);
    const int cnt = w.cnt, my_id = w.my_id;
    unsigned long long alive = w.alive;
    if (h.st + 2 < 30) stamp(30);
    // records: tile offsets of the layout this tile uses; with 16-bit tiles only when EVERY cell of the cascade fits 16 bits
    // (lbp16_all), otherwise window coordinates and the corners come from global memory
    const bool use16 = G16 && A.lbp16_all;
    const Stump* tab = reinterpret_cast<const Stump*>(G16 ? (use16 ? A.wstumps2 : A.gstumps) : STEP == 2 ? A.stumps2 : A.stumps1);
    double last = 0.;  // lane k: stage sum its window ended with
    int code = 1;      // lane k: result code of its window (1 = passed every stage so far)
    int s2 = h.st;
    while (s2 < A.nstages && alive) {
      if (A.stop_after >= 0 && s2 > A.stop_after) break;
      const int first = stage_first[s2];
      int e = s2 + 1;  // chunk = stages [s2, e): as many whole stages as fit 64 lanes (the host guarantees every stage does)
      while (e < A.nstages && stage_first[e] + stage_ntrees[e] - first <= 64) e++;
      const int n_st = e - s2, n_stumps = stage_first[e - 1] + stage_ntrees[e - 1] - first;
      const Stump rec = tab[first + min(lane, n_stumps - 1)];
      // lane t < n_st adds up stage s2 + t
      const int my_f0 = lane < n_st ? stage_first[s2 + lane] - first : 0, my_nt = lane < n_st ? stage_ntrees[s2 + lane] : 0;
      const double my_thr = lane < n_st ? (double)stage_thr[s2 + lane] : 0.;
      for (unsigned long long m = alive; m; m &= m - 1ull) {
        const int k = __builtin_ctzll(m);
        const int id = __builtin_amdgcn_readlane(my_id, k);
        float vote;
        if constexpr (G16) {
          if (use16)
            vote = lbp_vote_f<true>(Lds16Reader{reinterpret_cast<const unsigned short*>(lds + window_base(id))}, rec);
          else
            vote = lbp_vote_f<false>(table_reader(id), rec);
        } else
          vote = lbp_vote_f<false>(table_reader(id), rec);
        votes[lane] = vote;  // lanes beyond n_stumps hold a copy of the last stump's vote, never read
        double acc = 0.;
        for (int i = 0; i < my_nt; i++) acc += (double)votes[my_f0 + i];  // same wavefront: LDS operations stay in order
        const unsigned long long failed = __ballot(lane < n_st && acc < my_thr);
        const int t = failed ? __builtin_ctzll(failed) : n_st - 1;  // first failing stage of the chunk, else its last stage
        const double ended = readlane_f64(acc, t);
        if (lane == k) {
          last = ended;
          if (failed) code = -(s2 + t);
        }
        if (failed) alive &= ~(1ull << k);
      }
      s2 = e;
    }
    if (lane < cnt) {
      const bool accepted = code == 1 && s2 >= A.nstages;
      if (accepted) emit_candidate(my_id, last);
      if (dbg && (accepted || code != 1)) report(my_id, code, last);
    }
  }
};

template <int STEP, bool HAAR, bool TREES>
__device__ __forceinline__ void eval_tile(const EvalArgs& A, int32_t* lds, const int4 T, const ScaleDev& S) {
  using Tile = EvalTile<STEP, HAAR, TREES>;
  const Tile t(A, lds, T, S);
  t.stamp(0);
  unsigned valsq_pre[WIN_PER_THREAD];
  t.stage_phase(valsq_pre);
  t.stamp(1);
  if (A.stop_after == -2) return;  // timing experiments: tile staging only
  if constexpr (Tile::kRolledDense)
    t.dense_phase_rolled();
  else if (!t.dense_phase(valsq_pre))
    return;
  t.stamp(2);
#ifdef CC_PRIO_LATE  // tuning (hiprtc -D): issue priority once the dense phase is done
  __builtin_amdgcn_s_setprio(CC_PRIO_LATE);
#endif
  QueueState h;
  if (!t.thread_phase(h)) return;
  if (h.qg < A.ngroups && h.n != 0) {  // windows left for a wave phase (stump cascades; wave_below is 0 for the others)
    if constexpr (HAAR && !TREES) t.wave_phase_haar(h);
    if constexpr (!HAAR && !TREES && EVAL_WAVES >= 4) t.wave_phase_lbp(h);
  }
  t.stamp(STAMP_SLOTS - 1);
}

// Block entry: the block's tile and scale records, and the (block-uniform) choice of the tile layout by the scale's step.
// ONLY_STEP 1 / 2: only that layout is compiled in. ALLOW_TREES: cascades with trees deeper than stumps (rare; thread-
// per-window phases only) are served too.
template <bool HAAR, int ONLY_STEP, bool ALLOW_TREES>
__device__ __forceinline__ void eval_block(const EvalArgs& A) {
  extern __shared__ __attribute__((aligned(16))) int32_t lds[];
  const int4 T = load_record(as_const_table(A.tiles) + blockIdx.x);
  const ScaleDev S = load_record(as_const_table(A.sd) + T.x);
  constexpr bool kDo1 = ONLY_STEP != 2, kDo2 = ONLY_STEP != 1;
  if constexpr (ALLOW_TREES) {
    if (A.trees) {
      if (S.ystep == 2)
        eval_tile<2, HAAR, true>(A, lds, T, S);
      else
        eval_tile<1, HAAR, true>(A, lds, T, S);
      return;
    }
  }
  if (kDo2 && (!kDo1 || S.ystep == 2))
    eval_tile<2, HAAR, false>(A, lds, T, S);
  else if (kDo1)
    eval_tile<1, HAAR, false>(A, lds, T, S);
}

#ifndef CC_SPEC_STAGES
// One launch covers every scale: the tile's scale decides (block-uniformly) which layout it uses.
// keep the register budget of the LDS-bound occupancy (CC_EVAL_MIN_WAVES_PER_EU wavefronts per SIMD)
__global__ __launch_bounds__(EVAL_THREADS) __attribute__((amdgpu_waves_per_eu(CC_EVAL_MIN_WAVES_PER_EU, 8))) void k_eval_haar(EvalArgs A) {
  eval_block<true, 0, true>(A);
}

__global__ __launch_bounds__(EVAL_THREADS) void k_eval_lbp(EvalArgs A) {
  eval_block<false, 0, true>(A);
}
#endif

#ifdef CC_SPEC_STAGES
// Entry point of the run-time specialised module (stump cascades only; looked up by this unmangled name). The generated
// spec_stage functions are for one cascade, hence for one feature type: CC_SPEC_LBP selects which kernel is built.
// CC_ONLY_STEP (1 / 2): this module is launched over the tiles of STEP-1 / STEP-2 scales only (the host compiles one module
// per step when the two want different tile heights); the other path is not compiled in, and the entry point carries the
// step in its name so that a kernel trace lists the two launches of a pass separately.
#ifndef CC_ONLY_STEP
#define CC_ONLY_STEP 0
#endif
#if CC_ONLY_STEP == 1
#define CC_SPEC_ENTRY k_eval_spec_step1
#elif CC_ONLY_STEP == 2
#define CC_SPEC_ENTRY k_eval_spec_step2
#else
#define CC_SPEC_ENTRY k_eval_spec
#endif
#ifdef CC_SPEC_LBP
constexpr bool kSpecHaar = false;
#else
constexpr bool kSpecHaar = true;
#endif
extern "C" __global__ __launch_bounds__(EVAL_THREADS) __attribute__((amdgpu_waves_per_eu(CC_EVAL_MIN_WAVES_PER_EU, 8))) void CC_SPEC_ENTRY(EvalArgs A) {
  eval_block<kSpecHaar, CC_ONLY_STEP, false>(A);
}
#endif
