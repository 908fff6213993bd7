// Declarations shared by cc_eval_kernel.inc and the host and device code of the detection side: compile-time tile shape,
// device records of the cascade tables and scale descriptors, tile geometry and the 64-lane DPP reduction. Pure device
// code like the .inc, and like it included inside namespace ccamd; the hiprtc build gets the text of this file in front of
// the .inc (kEvalKernelSrc, see the Makefile), so the run-time modules see the same declarations.
#ifndef CC_EVAL_COMMON_H
#define CC_EVAL_COMMON_H

constexpr int TILE_X = 64;   // window origins per tile row = one wavefront = one rej0 mask word
// Tile shape: 8 window rows x 256 threads (4 wavefronts, 2 window rows per thread in the dense phase). A 24x24 cascade
// then needs ~30 KB of LDS per block: 5 blocks = 20 wavefronts per CU. Measured with the specialised kernel (tools/
// build_tile_variant.sh, G windows/s): 8x256 11.7, 12x256 11.2, 6x192 10.7, 16x512 10.4, 16x256 10.2, 4x256 10.1,
// 10x320 9.9, 12x384 9.7, 8x128 9.0, 4x128 8.8. Smaller blocks keep more wavefronts busy through the late stages (the
// barrier per stage spans 4 wavefronts instead of 8) at the price of more halo rows staged per window row.
#ifndef CC_TILE_Y
#define CC_TILE_Y 8
#endif
#ifndef CC_EVAL_THREADS
#define CC_EVAL_THREADS 256
#endif
#ifndef CC_EVAL_MIN_WAVES_PER_EU
// Register budget: the LDS-bound occupancy is 5 blocks = 5 wavefronts per SIMD, which leaves 96 VGPRs per lane. The
// specialised code is software-pipelined by explicit scheduling barriers (a few stumps' corner words in flight), so the
// scheduler has no freedom to hoist more reads than that.
#define CC_EVAL_MIN_WAVES_PER_EU 5
#endif
constexpr int TILE_Y = CC_TILE_Y;   // window origin rows per tile
constexpr int EVAL_THREADS = CC_EVAL_THREADS;  // wavefronts sharing one LDS tile (more waves per LDS byte = better latency hiding)
constexpr int EVAL_WAVES = EVAL_THREADS / 64;
// Window rows per thread in the dense phase. A tile height that is no multiple of the block's wavefronts (the run-time
// STEP-2 Haar module: 10 rows) deals tile row r to wavefront r % EVAL_WAVES -- wavefront w walks rows w, w + EVAL_WAVES, ... --
// and a wavefront skips, by a wave-uniform test, the round whose row lies beyond the tile (EvalTile::own_row / has_row).
// Heights that are multiples keep wavefront w on rows w * WIN_PER_THREAD ...: the code of those builds is unchanged.
constexpr int WIN_PER_THREAD = (TILE_Y + EVAL_WAVES - 1) / EVAL_WAVES;
constexpr bool RAGGED_ROWS = TILE_Y % EVAL_WAVES != 0;
// largest power of two <= EVAL_WAVES: the most slices the stump-split path cuts a stage into
constexpr int SPEC_PARTS = EVAL_WAVES >= 8 ? 8 : EVAL_WAVES >= 4 ? 4 : EVAL_WAVES >= 2 ? 2 : 1;

struct ScaleDev {
  int w, h;
  int pitch8, pitchI;
  long long img_ofs, int_ofs, mask_ofs, win_ofs, h_ofs;  // h_ofs: band-total rows of the integral builder
  int ystep, nx, ny, nxw, nbands;
  float scale;
  int win_w, win_h;
  int xtab_ofs, ytab_ofs;
};

// Haar stump in tile coordinates. ofs[j][k] = LDS offset of corner k of rect j relative to the window's tile base.
struct HaarStumpDev {
  int ofs[3][4];
  float w[3];
  float thr, left, right;
  int nrect;
  int pad;
};
struct LbpStumpDev {
  int ofs[16];
  float left, right;
  int subset[8];
  int pad[2];
};

// Internal tree nodes of cascades deeper than stumps (same corner-offset convention as the stump records);
// child > 0 = node index inside the tree, child <= 0 = leaf index -child.
struct HaarNodeDev {
  int ofs[3][4];
  float w[3];
  float thr;
  int left, right;
  int nrect;
  int pad;
};
struct LbpNodeDev {
  int ofs[16];
  int left, right;
  int subset[8];
  int pad[2];
};

struct CandRaw {
  int frame, scale, gx, gy;
  double sum;  // stage sum of the last stage (levelWeights of the outputRejectLevels overload)
};
struct CandOut {
  int frame, scale, gx, gy, x, y, w, h;
  double sum;
};

template <int STEP>
struct TileGeom {
  static constexpr bool k16 = false;
  int cols, rows, plane, row_stride;
  __host__ __device__ TileGeom(int W0, int H0, int tile_y = TILE_Y) {  // tile_y: host code sizing another build's tile
    cols = (TILE_X - 1) * STEP + W0 + 1;
    rows = (tile_y - 1) * STEP + H0 + 1;
    // padded so that the 8- / 16-byte LDS stores of stage_tile stay aligned and inside the row
    plane = STEP == 2 ? (((cols + 3) / 4 * 4) / 2 + 1) / 2 * 2 : 0;
    row_stride = STEP == 2 ? 2 * plane : (cols + 3) / 4 * 4;
    // Bank skew between consecutive window rows = STEP * row_stride mod 32. A skew of 0 or 16 makes the windows of one
    // bank class (see win_class) vertical neighbours / every second row, and neighbouring survivors pile up in the same
    // class; any other multiple of 4 spreads them (measured on the bench frames: 8-15 % fewer queue rows than skew 16).
    // STEP 2 (rows of 8-byte stores: any even stride) goes further and takes a skew of 4, 12, 20 or 28: for the windows
    // that survive on the bench frames those need 2 % fewer queue rows than 8 / 24 (tests/analysis/queue_rows_model.py).
    if (STEP == 2) {
      while (((2 * row_stride) & 31) % 8 == 0) row_stride += 2;
    } else if ((STEP * row_stride) % 16 == 0)
      row_stride += 4;
  }
  // LDS offset of integral entry (r, c) of the tile
  __host__ __device__ int at(int r, int c) const {
    return STEP == 2 ? r * row_stride + (c & 1) * plane + (c >> 1) : r * row_stride + c;
  }
  __host__ __device__ int words() const { return rows * row_stride; }
};

// STEP-2 tile with 16-BIT entries (run-time specialised kernels, CC_SPEC_TILE16): the low halves of the integral,
// row-major. A rectangle sum is a difference of four entries, so it is exact modulo 2^16 whenever the true sum is below
// 2^16 (255 * area < 65536); the host only selects this layout when it can generate every rectangle of the compiled
// stages that way (larger rectangles are cut into pieces that satisfy the bound). Half the LDS bytes of the 32-bit tile
// mean 8 instead of 5 resident blocks per CU. Window column l sits at 16-bit index 2l = dword l: a wavefront's corner
// reads hit 64 consecutive dwords whatever the (even or odd) column offset is, because every lane reads the SAME half
// of its dword -- no plane split is needed. STEP-1 tiles are small enough in 32 bits and keep them.
struct TileGeom16 {
  static constexpr bool k16 = true;
  int cols, rows, rs16, row_stride;  // rs16: 16-bit entries per tile row; row_stride: dwords per tile row
  __host__ __device__ TileGeom16(int W0, int H0, int tile_y = TILE_Y) {
    cols = (TILE_X - 1) * 2 + W0 + 1;
    rows = (tile_y - 1) * 2 + H0 + 1;
    rs16 = (cols + 3) / 4 * 4;  // 8-byte LDS stores of stage_tile stay aligned
    // window row ly starts ly * rs16 dwords into the tile (2 tile rows): keep that bank skew off 0 and 16 (see TileGeom)
    if (rs16 % 16 == 0) rs16 += 4;
    row_stride = rs16 / 2;
  }
  __host__ __device__ int at(int r, int c) const { return r * rs16 + c; }  // in 16-bit units
  __host__ __device__ int words() const { return rows * row_stride; }
};

constexpr int TILE_WINDOWS = TILE_X * TILE_Y;  // 512
constexpr int MAX_STAGES = 64;                 // stage index limit of the kernels (result codes, specialisation switch)
constexpr int PART_DOUBLES = (EVAL_WAVES - 1) * 64;  // partial stage sums of the stump-split phase: (slices-1) x windows
constexpr int QUEUE_ROWS = TILE_WINDOWS / 32;  // windows per bank class = deepest possible queue row count
constexpr int VNF_PITCH = TILE_X + 32;         // s_vnf row pitch TILE_X + skew (skew < 32): bank of a window's entry = its class
__host__ __device__ inline int tile_words_padded(int tile_words) { return (tile_words + 3) & ~3; }  // 16-byte multiple
// LDS bytes per block: integral tile(s) + partial sums + vnf (Haar only: LBP has no norm factor) + 2 queue tables of
// u16[QUEUE_ROWS][32] + 3 x 32 class counters. tile_y: window rows per tile of the build in question (the run-time
// specialised kernel may be compiled with another CC_TILE_Y than this translation unit).
//
// lean = the layout of the run-time specialised Haar modules of one step each (CC_LEAN_LDS; no tilted tile), whose tall
// tiles must not pay for side tables: integral tile + vnf [tile_y][TILE_X], every row rotated instead of padded (vnf_slot)
// + the 2 queue tables + the counters. The tables grow towards each other from the two ends of their area -- row r of
// table 0 is the area's r-th row of 32 entries, row r of table 1 its r-th row from the end -- and what the other layout
// keeps in s_part lives in the part of that area that is dead at the time: the stump-split phase's partial sums in the gap
// between the tables (lean_split_gap_bytes), the wave phases' window lists in the table that no longer receives windows.
// This is THE sum: what the launcher requests and what EvalTile's pointers divide up. Nothing is added to it: the module of
// STEP-2 tiles ends exactly on an allocation unit at 10 rows of a 24x24 window (lds_blocks_resident), and bytes put between
// its queue tables beyond that were measured to cost a resident block (profiles/EXPERIMENTS.md 3.24).
__host__ __device__ inline size_t eval_lds_bytes(int tile_words, bool tilted, bool haar = true, int tile_y = TILE_Y, bool lean = false) {
  if (lean) return (size_t)tile_words_padded(tile_words) * 4 + tile_y * TILE_X * 4 + 2 * (tile_y * TILE_X) * 2 + 3 * 32 * 4;
  return (size_t)tile_words_padded(tile_words) * 4 * (tilted ? 2 : 1) + PART_DOUBLES * 8 + (haar ? tile_y * VNF_PITCH * 4 : 0) +
         2 * (tile_y * TILE_X) * 2 + 3 * 32 * 4;
}
// Lean layout: bytes between the two queue tables while neither holds more than `rows` rows. A group's windows keep their
// bank class, so the table it fills never has more rows than the table it reads.
__host__ __device__ inline int lean_split_gap_bytes(int tile_y, int rows) { return 2 * (tile_y * TILE_X) * 2 - 2 * rows * 32 * 2; }
// Bytes of partial sums a stage cut into `ns` stump slices exchanges: slices 1 .. ns-1, one double per thread of a slice.
__host__ __device__ inline int split_part_bytes(int ns) { return (ns - 1) * (EVAL_THREADS / ns) * 8; }
// LDS of a CU (gfx950: 160 KiB) and the blocks of one kernel that fit it by their LDS request alone (a CU holds 32
// wavefronts: 8 blocks of 256 threads).
constexpr int CU_LDS_BYTES = 160 * 1024;
__host__ __device__ inline int lds_blocks_per_cu(size_t lds_bytes) {
  const int n = (int)((size_t)CU_LDS_BYTES / (lds_bytes ? lds_bytes : 1)), cap = 32 / EVAL_WAVES;
  return n > cap ? cap : n;
}
// The same with a block's request rounded up to units of 1 280 bytes (1 / 128 of the CU's LDS). Measured on the STEP-2 Haar
// module (profiles/EXPERIMENTS.md 3.24): requests of 31 072, 31 792 and 32 000 bytes (25 units) run five blocks to a CU,
// 32 256, 32 512 and 32 768 bytes (26 units) run four, although 5 x 32 768 is the CU's 160 KiB and the runtime's occupancy
// query answers 5 for all of them. The height of the STEP-2 module is chosen by this count.
constexpr int LDS_ALLOC_BYTES = 1280;
__host__ __device__ inline int lds_blocks_resident(size_t lds_bytes) {
  const size_t units = (lds_bytes + LDS_ALLOC_BYTES - 1) / LDS_ALLOC_BYTES;
  const int n = (int)((size_t)(CU_LDS_BYTES / LDS_ALLOC_BYTES) / (units ? units : 1)), cap = 32 / EVAL_WAVES;
  return n > cap ? cap : n;
}

// Sum of `v` over the 64 lanes, returned wave-uniform (in scalar registers). Cross-lane moves are DPP modifiers
// (quad permutes, row mirrors, row broadcasts), not LDS permutes: ~6 short steps. The order of the additions differs
// from a sequential sum, so callers use it only where the sum is exact (order-independent).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_f64(double v) {
  const unsigned long long u = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)u, CTRL, ROW_MASK, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, ROW_MASK, 0xF, false);
  return __longlong_as_double(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
// The double that lane `src` (wave-uniform) holds, returned wave-uniform: two 32-bit readlanes.
__device__ __forceinline__ double readlane_f64(double v, int src) {
  const unsigned long long u = __double_as_longlong(v);
  const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)u, src);
  const unsigned hi = __builtin_amdgcn_readlane((int)(unsigned)(u >> 32), src);
  return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double wave_sum_f64(double v) {
  v += dpp_f64<0xB1, 0xF>(v);   // quad_perm [1,0,3,2]
  v += dpp_f64<0x4E, 0xF>(v);   // quad_perm [2,3,0,1]
  v += dpp_f64<0x141, 0xF>(v);  // row_half_mirror
  v += dpp_f64<0x140, 0xF>(v);  // row_mirror: every lane now holds the total of its row of 16
  v += dpp_f64<0x142, 0xA>(v);  // row_bcast15 into rows 1 and 3 (masked rows add 0)
  v += dpp_f64<0x143, 0xC>(v);  // row_bcast31 into rows 2 and 3: lane 63 holds the wave total
  return readlane_f64(v, 63);
}
// Number of set bits of the ballot `mask` below the calling lane: its rank among the lanes that voted.
__device__ __forceinline__ int lane_rank(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
}

#endif  // CC_EVAL_COMMON_H
