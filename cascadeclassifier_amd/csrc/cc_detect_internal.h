// Declarations shared by the detection-side translation units: the detector (cc_detector.h and its four files), cc_front.hip
// (pyramid and integral images), cc_negmine.hip (negative mining for training), cc_spec.hip (the run-time specialiser) and
// cc_group.hip (ordering and grouping on the device). What only the detector's own files share is in cc_detector.h;
// everything else stays static in the file that uses it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "cc_hip_util.h"
#include "cc_internal.h"

namespace ccamd {

#include "cc_eval_common.h"

// Scale (or level, or group) of a block: `first` holds the first block of each of the n segments, ascending.
__device__ __forceinline__ int find_segment(const int* __restrict__ first, int n, int idx) {
  int s = 0;
  while (s + 1 < n && first[s + 1] <= idx) s++;  // n <= a few hundred, wave-uniform
  return s;
}

inline int align_up(int v, int a) { return (v + a - 1) / a * a; }

// ------------------------------------------------------------------------------------------------
// Front end: pyramid (k_resize), integral images (k_integral_carry, k_integral_band) and tilted integral (k_diag_sums,
// k_tilted_cols) of every level of nf frames. The detector, the negative miner and the building-block entry points all
// lay it out with front_layout, upload it with FrontTables::upload and launch it with launch_front.
// ------------------------------------------------------------------------------------------------
// Host tables of the front end for levels of the given sizes, each resized from a src_w x src_h source.
struct FrontLayout {
  int src_w = 0, src_h = 0;
  std::vector<ScaleDev> sd;  // front-end fields set (w h pitch8 pitchI img_ofs int_ofs h_ofs nbands xtab_ofs ytab_ofs), the rest 0
  // block maps, ns + 1 entries: first block (band, group) of each level, the total last
  std::vector<int> resize_first, band_first, col_first, diag_first, tcol_first;
  std::vector<int> xofs, yofs;  // resize taps: columns (padded, see append_column_taps), rows
  std::vector<uint16_t> xw1, yw1;
  std::vector<long long> tseg_ofs;  // tilted only: where each level's segment totals start in a frame's, ns + 1 entries
  int max_nseg = 0;                 // tilted only: segments of the tallest level (0: no tilted integral)
  // per frame: pyramid bytes, integral elements per channel, band-total elements per channel, segment-total elements
  size_t pyr_frame_bytes = 0, int_frame_elems = 0, h_frame_elems = 0, tseg_frame_elems = 0;
};
FrontLayout front_layout(int src_w, int src_h, const std::vector<int2>& sizes, bool tilted);

// A layout and its tables on the device. Callers set the layout, add their own ScaleDev fields, then upload once: the
// detector's captured hipGraph replays these pointers, so a plan's tables are never reallocated.
struct FrontTables {
  FrontLayout L;
  DevBuf<ScaleDev> d_sd;
  DevBuf<int> d_resize_first, d_band_first, d_col_first, d_diag_first, d_tcol_first, d_xofs, d_yofs;
  DevBuf<uint16_t> d_xw1, d_yw1;
  DevBuf<long long> d_tseg_ofs;
  // Ends with a synchronisation of `st`, so earlier uploads of the caller on `st` have landed too.
  hipError_t upload(hipStream_t st) {
    for (hipError_t e : {d_sd.upload(L.sd, st), d_resize_first.upload(L.resize_first, st), d_band_first.upload(L.band_first, st),
                         d_col_first.upload(L.col_first, st), d_diag_first.upload(L.diag_first, st), d_tcol_first.upload(L.tcol_first, st),
                         d_xofs.upload(L.xofs, st), d_yofs.upload(L.yofs, st), d_xw1.upload(L.xw1, st), d_yw1.upload(L.yw1, st),
                         L.tseg_ofs.empty() ? hipSuccess : d_tseg_ofs.upload(L.tseg_ofs, st)})
      if (e != hipSuccess) return e;
    return hipStreamSynchronize(st);
  }
};

enum { FRONT_RESIZE = 1, FRONT_INTEGRALS = 2 };  // launch_front parts

// Caller-owned buffers of launch_front, frame f of each at f times its per-frame size.
struct FrontIO {
  // FRONT_RESIZE: the source frames, src_w x src_h. FRONT_INTEGRALS: set = FRONT_RESIZE ran with this very FrontIO (in
  // this call or the one before it on the stream) and left the band column sums in hbuf; null = the caller filled pyr
  // itself and launch_front adds them up first (k_band_colsums).
  const uint8_t* src = nullptr;
  size_t row_stride = 0, frame_stride = 0;
  uint8_t* pyr = nullptr;      // L.pyr_frame_bytes per frame: the levels (FRONT_INTEGRALS alone: filled by the caller)
  int32_t* integ = nullptr;    // nchan x L.int_frame_elems per frame: channel 0 sum, 1 sqsum (sq), tilt_chan tilted (tilted layouts)
  // nchan x L.h_frame_elems per frame, [band][pitchI] per level: the bands' column sums (sum, and sum of squares when sq),
  // written by FRONT_RESIZE when set, scanned down the bands in place by FRONT_INTEGRALS. Null: FRONT_RESIZE alone.
  int32_t* hbuf = nullptr;
  int32_t* diag = nullptr;     // tilted: 2 x L.int_frame_elems per frame, diagonal sums
  int32_t* tseg = nullptr;     // tilted: L.tseg_frame_elems per frame, segment totals
  int nchan = 1, tilt_chan = 2;
  bool sq = false;
  int sq_odd_rows_only = 0;  // k_integral_band: squared sums of ystep-2 levels only where the detector reads them
};

// Launches the front end's `parts` for nf frames on `st`. Only launches: no allocation, no synchronisation (the detector
// runs it inside a hipGraph capture).
void launch_front(hipStream_t st, const FrontTables& T, const FrontIO& io, int nf, int parts);

// ---- colour frames (CC_PIX_*, include/cascadeclassifier_amd.h) ----
// Bytes per pixel of a row (1 for the planar format, whose planes are rows of one channel); 0 for an unknown format.
inline int pix_bytes(int fmt) {
  switch (fmt) {
    case CC_PIX_GRAY8: case CC_PIX_RGB8_PLANAR: return 1;
    case CC_PIX_BGR8: case CC_PIX_RGB8: return 3;
    case CC_PIX_BGRA8: case CC_PIX_RGBA8: return 4;
    default: return 0;
  }
}
// Rows of `row_stride` bytes that one frame of the format spans (the planar format: three planes of `height` rows).
inline int pix_rows(int fmt, int height) { return fmt == CC_PIX_RGB8_PLANAR ? 3 * height : height; }
// k_to_gray: nf frames of format `fmt` (frame f at src + f * frame_stride) -> gray frames at dst + f * dst_frame_stride,
// rows dst_stride apart. dst and dst_stride must be multiples of 4; src and row_stride may be anything. Only the launch.
void launch_to_gray(hipStream_t st, int fmt, const uint8_t* src, size_t row_stride, size_t frame_stride, int w, int h, int nf,
                    uint8_t* dst, size_t dst_stride, size_t dst_frame_stride);

// ---- checks shared by the entry points (defined in cc_detect_api.hip) ----
// Detection and its run-time specialisation are Haar / LBP only: nothing in the reference defines detection with a HOG
// cascade. Every detector entry point calls this before the model reaches a kernel or a table builder (the LBP branches
// would read lbp_rects, which a HOG model leaves empty).
cc_status refuse_hog(const Cascade& m, const char* who);

// True when, for every stage, any partial sum of leaf values is exactly representable in double: all leaves are
// integer multiples of q = 2^(emin-24) (emin = smallest frexp exponent among the stage's nonzero leaves) and the sum of the
// larger leaf magnitudes divided by q stays below 2^53. Then the double accumulation never rounds, so its result
// does not depend on the order of the additions.
bool stage_sums_order_independent(const Cascade& m, double headroom = 1.0);
// Stage s alone, for int32 vote sums: true when its leaves are all multiples of q = 2^(emin-24) and the sum of the larger
// leaf magnitudes divided by q stays below 2^31 - 1; q is set then. False for a stage without a nonzero leaf. The caller
// has established finite leaves (stage_sums_order_independent). Both are defined in cc_host.cpp.
bool stage_quantum(const Cascade& m, int s, double& q);

// ---- stump tables of the cascade kernels (detector and specialiser) ----
// `at(y, x)` maps a corner inside the window to what the record stores: an LDS offset of one of the tile layouts, or
// (y << 16 | x) for the records whose corners are read from global memory (GlobalReader). tilt_shift: distance of the
// tilted tile behind the sum tile.
// The two record kinds (stump, tree node) share their corner fields; the builders add thr / left / right.
template <class R, class At>
void fill_haar_corners(const Cascade& m, int fi, R& d, At at, int tilt_shift) {  // ofs, w, nrect of feature fi
  d.nrect = 2;
  for (int j = 0; j < 3; j++) {
    const int32_t* r = &m.haar_rects[(size_t)fi * 12 + j * 4];
    const float wt = m.haar_weights[(size_t)fi * 3 + j];
    d.w[j] = wt;
    // rects after the first zero weight contribute w*0 upstream (offsets stay 0): keep corner offsets equal
    const bool used = j < 2 || wt != 0.0f;
    if (j == 2 && wt != 0.0f) d.nrect = 3;
    const int x = used ? r[0] : 0, y = used ? r[1] : 0, rw = used ? r[2] : 0, rh = used ? r[3] : 0;
    if (!m.haar_tilted[fi]) {
      d.ofs[j][0] = at(y, x);
      d.ofs[j][1] = at(y, x + rw);
      d.ofs[j][2] = at(y + rh, x);
      d.ofs[j][3] = at(y + rh, x + rw);
    } else {  // corners of the 45-degree rectangle (CV_TILTED_OFFSETS), read from the tilted tile behind the sum tile
      d.ofs[j][0] = tilt_shift + at(y, x);
      d.ofs[j][1] = tilt_shift + at(y + rh, x - rh);
      d.ofs[j][2] = tilt_shift + at(y + rw, x + rw);
      d.ofs[j][3] = tilt_shift + at(y + rw + rh, x + rw - rh);
    }
  }
}
template <class R, class At>
void fill_lbp_cells(const Cascade& m, int fi, size_t i, R& d, At at) {  // ofs of feature fi, subset of stump / node i
  const int32_t* r = &m.lbp_rects[(size_t)fi * 4];
  for (int rr = 0; rr < 4; rr++)
    for (int cc = 0; cc < 4; cc++) d.ofs[4 * rr + cc] = at(r[1] + rr * r[3], r[0] + cc * r[2]);
  for (int j = 0; j < 8; j++) d.subset[j] = m.node_subset[i * 8 + j];
}
template <class At>
void build_haar_stumps_at(const Cascade& m, std::vector<HaarStumpDev>& out, At at, int tilt_shift) {
  out.resize(m.stump_feature.size());
  for (size_t i = 0; i < out.size(); i++) {
    HaarStumpDev& d = out[i];
    std::memset(&d, 0, sizeof(d));
    fill_haar_corners(m, m.stump_feature[i], d, at, tilt_shift);
    d.thr = m.stump_threshold[i];
    d.left = m.stump_left[i];
    d.right = m.stump_right[i];
    d.pad = (int)i;  // the stump's index: survives the re-ordering of schedule_for_wave_phase
  }
}
template <int STEP>
void build_haar_stumps(const Cascade& m, std::vector<HaarStumpDev>& out) {
  const TileGeom<STEP> G(m.win_w, m.win_h);
  build_haar_stumps_at(m, out, [&](int y, int x) { return G.at(y, x); }, tile_words_padded(G.words()));
}
template <class At>
void build_lbp_stumps_at(const Cascade& m, std::vector<LbpStumpDev>& out, At at) {
  out.resize(m.stump_feature.size());
  for (size_t i = 0; i < out.size(); i++) {
    LbpStumpDev& d = out[i];
    std::memset(&d, 0, sizeof(d));
    fill_lbp_cells(m, m.stump_feature[i], i, d, at);
    d.left = m.stump_left[i];
    d.right = m.stump_right[i];
  }
}
template <int STEP>
void build_lbp_stumps(const Cascade& m, std::vector<LbpStumpDev>& out) {
  const TileGeom<STEP> G(m.win_w, m.win_h);
  build_lbp_stumps_at(m, out, [&](int y, int x) { return G.at(y, x); });
}
inline void build_lbp_stumps16(const Cascade& m, std::vector<LbpStumpDev>& out) {  // STEP-2 tile with 16-bit entries
  const TileGeom16 G(m.win_w, m.win_h);
  build_lbp_stumps_at(m, out, [&](int y, int x) { return G.at(y, x); });
}

// Layout of the STEP-2 tiles of a specialised kernel: 32-bit entries in two column planes (TileGeom<2>) or 16-bit entries
// (TileGeom16).
enum { TILE_32 = 0, TILE_16 = 1 };

// A rectangle sum read from 16-bit entries is exact when 255 * area < 2^16.
inline bool fits16(long long area) { return 255LL * area <= 65535LL; }

// ---- run-time specialisation (cc_spec.hip) ----
// One compiled module of the run-time specialised kernel: the tiles it covers (0 = all, 1 / 2 = the tiles of STEP-1 / STEP-2
// scales) and the tile height it was compiled for.
struct SpecCode {
  std::vector<char> code;
  int only_step = 0;
  int tile_y = TILE_Y;
};

// Host half of the specialisation: source for the first stages (whole stages within the code-size budget) compiled for
// `arch`. No device calls: safe on a background thread.
cc_status spec_build(const Cascade& m, int n_stages, const std::string& arch, std::vector<SpecCode>& codes, int& k_out, int& tmode_out);

// One loaded module of the specialised kernel: its entry point, the dynamic LDS bytes a block of it requests, and the tiles
// it runs over (window rows per tile; 0 = the tiles of all scales, 1 / 2 = of the STEP-1 / STEP-2 scales).
struct SpecModule {
  hipModule_t mod = nullptr;
  hipFunction_t fn = nullptr;
  size_t lds = 0;
  int tile_y = TILE_Y;
  int only_step = 0;
  int wave_below = -1;  // >= 0: the module's own EvalArgs::wave_below (spec_install); -1: the detector's
};

// EvalArgs::wave_below of the launches of a module over the tiles of step `only_step` at `tile_y` window rows, given the
// detector's value; -1 = the detector's value.
int spec_wave_below(int detector_value, int only_step, int tile_y);

// Device half: the code objects of spec_build as loaded modules, out[0] the one for all tiles or the STEP-2 tiles, out[1]
// the STEP-1 module if any. `base_lds`: the LDS request of the ahead-of-time kernels. Owning thread only.
cc_status spec_load(const Cascade& m, const std::vector<SpecCode>& codes, int tmode, size_t base_lds, SpecModule out[2], int* n_out);

// ---- ordering and grouping on the device (cc_group.hip) ----
// What lets the kernels of a detector pass drop out: counts = the pass's {raw, filtered} candidate counts on the device, the
// capacity its lists were launched with, and the detector's abort word (set by a pass that overflowed, for the passes behind
// it). All null / 0 for rectangles that come from a caller (cc_group_rectangles_device).
struct GroupGuard {
  const int* counts = nullptr;
  int cand_cap = 0;
  int* abort = nullptr;
};
constexpr int GROUP_WS_INTS = 7;          // workspace ints per rectangle of k_group_frames
constexpr int GROUP_WS_INTS_SCORED = 10;  // of k_group_frames_scored: + the class level and the class weight's 64-bit image
// The scored form of both helpers (cv::groupRectangles with rejectLevels and levelWeights): a level and a weight per input
// rectangle (levels null: const_level for all of them, the detector's case) and where the survivors' go, beside `out`.
// Default: unscored.
struct GroupScores {
  bool scored = false;
  const int32_t* levels = nullptr;
  int const_level = 0;
  const double* weights = nullptr;
  int32_t* out_levels = nullptr;
  double* out_weights = nullptr;
  explicit operator bool() const { return scored; }
};
// Device workspace of the two launch helpers below, owned by the caller; ensure() only grows it (the detector sizes it for
// its candidate capacity and pass size, so a warm pass allocates nothing). What only scored calls use -- the ordered weights,
// the staged levels and weights, the wider ws -- is allocated by the first ensure(scored = true).
struct GroupBufs {
  DevBuf<cc_rect> ordered, grouped;  // a pass's rectangles in candidate order; each frame's result at its input offset
  DevBuf<unsigned long long> keys;
  DevBuf<int> src, seg, frame_cnt, out_count, ws;  // seg: frames + 1 segment offsets of `ordered`; ws: GROUP_WS_INTS(_SCORED) per rectangle
  DevBuf<double> ordered_weights, grouped_weights;  // scored: beside ordered / grouped
  DevBuf<int32_t> grouped_levels;
  hipError_t ensure(size_t rects, size_t frames, bool ordering, bool scored = false);
};
// Only launches, on `st`. The filtered candidates of a pass of nf frames -> B.ordered in (frame, scale, gy, gx) order with
// B.seg as its per-frame offsets; scored: their stage sums -> B.ordered_weights in the same order.
void launch_order_candidates(hipStream_t st, GroupGuard g, const CandOut* cands, int nf, GroupBufs& B, bool scored = false);
// cv::groupRectangles on each of nf frames (frame f: rects[offsets[f] .. offsets[f + 1])). The results go to `out` from
// *total on, frame after frame, only what lies below cap being written; out_offsets[0 .. nf] receives their offsets and *total
// moves on by their number. sc: with levels and weights, B sized by ensure(scored = true).
void launch_group_frames(hipStream_t st, GroupGuard g, const cc_rect* rects, const int* offsets, int nf, int group_threshold, double eps,
                         GroupBufs& B, cc_rect* out, int cap, int32_t* out_offsets, int* total, const GroupScores& sc = GroupScores{});

}  // namespace ccamd
