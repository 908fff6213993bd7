// Detection on gfx950: sliding-window cascade evaluation with early exit (the kernels of cc_eval_kernel.inc), the stage-0
// skip-rule filter, and the detector that drives them (cc_detector: plans, pass loop, graph capture, staging, batches,
// grouping, installing run-time specialised kernels). The pyramid and integral images come from cc_front.hip, the
// specialised kernels' source and code objects from cc_spec.hip. Replaces cv::CascadeClassifier::detectMultiScale as called
// by the reference's detection tool (tools/detection/Cpp/main.cpp:42-45); behaviour follows SURVEY.md Appendix A.
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
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <future>
#include <memory>
#include <thread>

#include <atomic>
#include <map>
#include <mutex>
#include <unordered_set>

#include "cc_detect_internal.h"

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

struct Plan {
  int w = 0, h = 0;
  cc_detect_params p{};
  std::vector<ScaleGeom> geom;
  FrontTables front;  // its ScaleDev records carry the detector's fields too (mask_ofs win_ofs ystep nx ny nxw scale win_w win_h)
  size_t mask_frame_words = 0;
  long long windows = 0, integral_elems = 0;
  int n_grid_rows = 0;
  struct TileList {
    int n = 0;
    DevBuf<int4> d;
  };
  // Tile lists by (window rows per tile, step of the scales covered or 0 = all), see plan_tiles: (TILE_Y, 0) for the
  // ahead-of-time kernels, the others for the specialised kernel's modules. An entry is never reallocated or moved while the
  // plan lives (map nodes stay where they are): captured graphs replay its pointer.
  std::map<std::pair<int, int>, TileList> tiles;
  DevBuf<int> d_gridrow_first;
  // Single-image calls (the detection tool's shape) are launch-bound: ~10 launches, memsets and copies for well under a
  // millisecond of device work. After a first ordinary call has sized every buffer, the whole pass (H2D copy of the
  // image, pyramid, integrals, cascade kernel, skip filter, copy-back of the counters) is captured into a hipGraph and
  // replayed with one launch for as long as the buffers and kernels it recorded stay the same (`graph_key`). One graph per
  // pixel format (CC_PIX_*; a colour pass starts with the copy of the colour bytes and k_to_gray), so that gray and colour
  // calls on one plan both stay on graph launches.
  static constexpr int kFormats = CC_PIX_RGB8_PLANAR + 1;
  bool graph_warm[kFormats] = {};
  hipGraphExec_t graph_exec[kFormats] = {};
  std::vector<const void*> graph_key[kFormats];
  ~Plan() {
    for (hipGraphExec_t g : graph_exec)
      if (g) (void)hipGraphExecDestroy(g);
  }
};

struct TimingEvent {
  hipEvent_t a, b;
  int kind;
};

// Where the filtered candidates of a batch's passes go (called on the host thread that retires the pass), and the first
// error met while retiring one of its passes from another call (cc_detect_batch_submit of the NEXT batch).
struct BatchSink {
  std::function<void(int f0, int nf, std::vector<CandOut>& cands)> consume;
  cc_status status = CC_OK;
  std::string error;
  // Submitted batches (cc_detect_batch_submit): the host side of a retired pass -- sorting and grouping its candidates,
  // ~1.3 ms for 19 Full-HD frames -- runs on a helper thread, so that the submitting thread goes straight on to launch
  // the next pass / the next batch; cc_detect_batch_collect waits for the helpers. (Doing all of it in collect instead was
  // measured too: 18.5 -> 23.5 ms per step, the device idles while the host groups 64 frames in one go.)
  bool async_consume = false;
  std::vector<std::future<void>> jobs;
  void wait_jobs() {
    for (auto& j : jobs)
      if (j.valid()) j.get();
    jobs.clear();
  }
};

// The frames of a call as the caller describes them: n_frames frames of pixel format `fmt` (CC_PIX_*), frame_stride bytes
// apart, in host memory or (on_device) on the detector's card.
struct FrameSet {
  const uint8_t* frames;
  int on_device, n_frames, width, height;
  size_t row_stride, frame_stride;
  int fmt;
};
inline FrameSet host_image(const uint8_t* img, int width, int height, size_t row_stride, int fmt = CC_PIX_GRAY8) {
  return FrameSet{img, 0, 1, width, height, row_stride, row_stride * (size_t)pix_rows(fmt, height), fmt};
}

// Where the grouped rectangles of a device-output pass go (cc_detect_batch_to_device): the caller's device buffers, with
// d_offsets already at the pass's first frame. d_offsets null: a host-output pass, whose candidates go to its sink.
// d_weights set: with scores (cc_detect_batch_to_device_levels), d_levels / d_weights beside d_out, every level = `level`.
struct DeviceOutput {
  cc_rect* d_out = nullptr;
  int cap = 0;
  int32_t* d_offsets = nullptr;
  int min_neighbors = 0;
  int32_t* d_levels = nullptr;
  double* d_weights = nullptr;
  int level = 0;
  explicit operator bool() const { return d_offsets != nullptr; }
};

// How run_batch runs a batch. want_results false: launches only, nothing is read back (cc_detect_batch_device_only).
// debug: the windows' exit codes and sums are kept (cc_detect_debug_windows). defer_last: the batch's last pass stays pending
// when the call returns (cc_detect_batch_submit). dev: a device-output batch.
struct BatchOptions {
  bool want_results = true, debug = false, defer_last = false;
  DeviceOutput dev;
};

}  // namespace ccamd

using namespace ccamd;

constexpr int kStageSlots = 3;  // staging slots for host frames (stage_pass: why three)

struct cc_detector {
  Cascade m;
  unsigned long long serial = 0;  // unique per created detector (tickets name their owner by it, not by address alone)
  int device = 0;
  int max_batch = 1;
  int pass_capacity = 1;  // frames the per-pass workspace is sized for: the largest pass seen so far (<= max_batch)
  hipStream_t own_stream = nullptr, stream = nullptr;
  // cascade tables on the device (one per tile layout)
  DevBuf<int> d_stage_ntrees, d_stage_first;
  DevBuf<int> d_group_first;  // stage groups of the cascade kernel (EvalArgs::group_first), n_groups + 1 entries
  int n_groups = 0;
  int dense_from = 0x7fffffff;  // first stage group whose queue is a plain list instead of a bank-class table (EvalArgs::dense_from)
  DevBuf<float> d_stage_thr;
  int wave_below = 0;
  int last_call_graph = 0;  // the last single-image call was one hipGraph launch (cc_detector_graph_active)
  int stop_after = -1;
  int split_stumps = 0;
  DevBuf<HaarStumpDev> d_haar1, d_haar2;
  DevBuf<HaarStumpDev> d_haar1w, d_haar2w;  // the same stumps dealt to lanes for the wave phase (bank-aware order)
  DevBuf<HaarStumpDev> d_haar_g;            // corners as window coordinates (GlobalReader; kernels with 16-bit tiles)
  DevBuf<LbpStumpDev> d_lbp_g, d_lbp16;      // LBP: window coordinates (GlobalReader) / 16-bit STEP-2 tile offsets (LBP wave phase)
  int lbp16_all = 0;                        // every LBP cell of the cascade sums below 2^16
  DevBuf<LbpStumpDev> d_lbp1, d_lbp2;
  DevBuf<HaarNodeDev> d_hnode1, d_hnode2;  // cascades with trees deeper than stumps
  DevBuf<LbpNodeDev> d_lnode1, d_lnode2;
  DevBuf<int> d_tree_root, d_tree_leaf0;
  DevBuf<float> d_leaves;
  size_t lds = 0;  // dynamic LDS bytes per tile (larger of the two layouts)
  // plans + workspace
  std::vector<std::unique_ptr<Plan>> plans;
  DevBuf<uint8_t> d_frames, d_pyr;
  // The integral images are double-buffered: pyramid + integrals of pass i+1 are built on `front_stream` while the
  // cascade kernel of pass i (LDS/VALU-bound, leaves wave slots and all of HBM idle) runs on `stream`.
  DevBuf<int32_t> d_integ[2], d_hbuf, d_diag, d_tseg;
  hipStream_t front_stream = nullptr;
  hipEvent_t front_done[2] = {nullptr, nullptr}, eval_done[2] = {nullptr, nullptr}, batch_begin = nullptr;
  bool eval_pending[2] = {false, false};
  int overlap_front = 1;
  // run-time specialised cascade kernel (cc_detector_specialize, spec_load); n_spec 0 = table-driven kernel. spec[0] covers
  // every tile, or the tiles of STEP-2 scales when spec[1] exists: that one covers the tiles of STEP-1 scales.
  SpecModule spec[2];
  int n_spec = 0;
  int last_stamp_tiles = 0;  // CCAMD_DEBUG_STAMPS: tiles of the last pass (all launches)
  int spec_stages = 0;
  // background build of the specialised module (cc_detector_specialize_async / CCAMD_AUTO_SPECIALIZE): a host thread
  // generates and compiles; the next detection call on the owning thread loads the module and switches over
  std::thread spec_thread;
  std::atomic<int> spec_bg_state{0};  // 0 idle, 1 building, 2 ready to install, 3 failed
  std::vector<SpecCode> spec_bg_code;
  int spec_bg_stages = 0;
  int spec_bg_tmode = 0;
  std::string spec_bg_error;
  // Per slot, like the results. (Round 3 also ran the cascade kernels of consecutive passes on two streams, so that the next
  // one starts on the CUs the previous one's last blocks leave free: 18.50 -> 19.24 ms per step, two kernels of this size
  // only get in each other's way. Not kept.)
  DevBuf<unsigned long long> d_masks[2];
  DevBuf<CandRaw> d_cands[2];
  // Results of a pass are double-buffered so that the host can fetch and group pass i while the device runs pass i+1.
  DevBuf<CandOut> d_out[2];
  DevBuf<int> d_counts[2];  // [0] raw count, [1] filtered count
  // cc_detect_batch_to_device: the workspace of the ordering and grouping kernels (cc_group.hip), sized for cand_cap
  // candidates and pass_capacity frames, and two words on the device: [0] rectangles written so far in the batch, [1] set by
  // a pass whose candidate list overflowed (GroupGuard::abort).
  GroupBufs group;
  DevBuf<int> d_group_state;
  int* h_counts = nullptr;  // pinned, 2 x 2 ints
  uint8_t* h_frame = nullptr;  // pinned staging copy of a single host image (graph path)
  size_t h_frame_bytes = 0;
  uint8_t* h_color_frame = nullptr;  // the same for a single colour image (its own buffer: the gray graphs keep theirs)
  size_t h_color_frame_bytes = 0;
  // Colour frames from the host land here (stage_host_frames) and k_to_gray writes them into a gray staging slot, both on
  // the front stream: stream order makes one buffer of pass_capacity frames enough. Allocated on the first colour batch.
  DevBuf<uint8_t> d_color;
  uint8_t* h_stage = nullptr;  // pinned staging area for batches of host frames, kStageSlots slots like d_frames (stage_host_frames)
  size_t h_stage_bytes = 0;    // kStageSlots equal slots of h_stage_bytes / kStageSlots bytes, whatever the frames' format
  long long graph_captures = 0;  // hipGraph captures made (cc_detector_graph_captures)
  int stage_slot = 0;          // staging slot the next pass of host frames takes (round-robin, also across calls)
  int use_graph = 1;  // single-image calls replay a captured hipGraph; cleared when a capture fails
  int early_skip = 1, pipeline_passes = 4, pipeline_passes_set = 0;  // tuning knobs, read once at creation
  hipStream_t copy_stream = nullptr;
  hipEvent_t pass_done[2] = {nullptr, nullptr};
  int cand_cap = 0;
  // The pass launched last, not yet fetched (run_batch): inside a batch that is what lets the host side of pass i overlap
  // the device side of pass i + 1; across calls (cc_detect_batch_submit) it lets the first pass of the next batch overlap
  // the last pass of this one. `sink` receives the pass's candidates when it is retired. A device-output pass (`dev`) is a
  // pass like any other whose launch is followed by the ordering and grouping kernels (enqueue_group): retiring it only
  // looks at its raw count, and there is nothing to fetch unless it has to be redone (retire_pending).
  struct PendingPass {
    bool active = false;
    Plan* plan = nullptr;
    int f0 = 0, nf = 0, slot = 0;
    const uint8_t* dptr = nullptr;
    size_t rs = 0, fs = 0;
    int cap = 0;       // capacity of the candidate lists the pass was launched with
    unsigned gen = 0;  // generation of the candidate lists it wrote into
    bool debug = false;
    ccamd::DeviceOutput dev;
    std::shared_ptr<ccamd::BatchSink> sink;
    void drop() { active = false, sink.reset(); }  // nobody fetches it: its results are left where they are
  } pending;
  unsigned list_gen = 0;  // bumped whenever the candidate lists are released and regrown
  int next_slot = 0;      // result / integral slot the next pass uses (alternates, also across calls)
  DevBuf<unsigned long long> d_stamps;  // CCAMD_DEBUG_STAMPS experiments
  DevBuf<int32_t> d_dbg_codes;
  DevBuf<double> d_dbg_sums;
  DevBuf<uint8_t> d_dbg_visited;
  // profiling
  bool profiling = false;
  std::vector<TimingEvent> events;
  cc_detector_timings tm{};

  void unload_spec() {  // back to the table-driven kernel; the caller has made sure that no launch of the modules is in flight
    for (int i = 0; i < n_spec; i++) (void)hipModuleUnload(spec[i].mod);
    spec[0] = spec[1] = SpecModule{};
    n_spec = 0;
    spec_stages = 0;
  }
  ~cc_detector() {
    for (auto& e : events) {
      (void)hipEventDestroy(e.a);
      (void)hipEventDestroy(e.b);
    }
    if (own_stream) (void)hipStreamDestroy(own_stream);
    if (copy_stream) (void)hipStreamDestroy(copy_stream);

    if (front_stream) (void)hipStreamDestroy(front_stream);
    if (spec_thread.joinable()) spec_thread.join();
    unload_spec();
    for (hipEvent_t e : {pass_done[0], pass_done[1], front_done[0], front_done[1], eval_done[0], eval_done[1], batch_begin})
      if (e) (void)hipEventDestroy(e);
    if (h_counts) (void)hipHostFree(h_counts);
    if (h_frame) (void)hipHostFree(h_frame);
    if (h_color_frame) (void)hipHostFree(h_color_frame);
    if (h_stage) (void)hipHostFree(h_stage);
  }
};

namespace ccamd {

cc_status refuse_hog(const Cascade& m, const char* who) {
  if (m.feature_type == CC_FEATURE_HAAR || m.feature_type == CC_FEATURE_LBP) return CC_OK;
  return set_error(CC_ERR_UNSUPPORTED, "%s: %s cascades are not supported for detection (Haar and LBP only)", who,
                   m.feature_type == CC_FEATURE_HOG ? "HOG" : "unknown-type");
}

cc_status ensure_device(int device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return set_error(CC_ERR_NO_DEVICE, "no usable HIP device (%s); this library has no CPU fallback",
                     e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
  if (device < 0 || device >= n) return set_error(CC_ERR_INVALID_ARG, "device %d out of range (devices: %d)", device, n);
  CC_HIP(hipSetDevice(device));
  return CC_OK;
}

// Wave phase: lane l of step k evaluates stump (64 k + l) of the stage, so the 32 lanes of a half-wavefront read 32
// unrelated LDS words per corner slot (~3.8-way bank conflicts in file order). The stage sums are order-independent
// when this phase is used, so the stumps of a stage may be dealt to the lanes in any order, and the two '+' and the
// two '-' corners of a rectangle may swap slots: a greedy pass fills one 32-lane group at a time with the stump
// (and corner arrangement) that adds the fewest conflict cycles. Returns a reordered copy of the table.
static std::vector<HaarStumpDev> schedule_for_wave_phase(const Cascade& m, const std::vector<HaarStumpDev>& t) {
  std::vector<HaarStumpDev> out;
  out.reserve(t.size());
  auto variant = [](const HaarStumpDev& s, int v) {  // v: 6 bits, per rect swap of slots (0,3) and of slots (1,2)
    HaarStumpDev r = s;
    for (int j = 0; j < 3; j++) {
      if (v & (1 << (2 * j))) std::swap(r.ofs[j][0], r.ofs[j][3]);
      if (v & (2 << (2 * j))) std::swap(r.ofs[j][1], r.ofs[j][2]);
    }
    return r;
  };
  for (size_t s = 0; s < m.stage_ntrees.size(); s++) {
    const int first = m.stage_first[s], nt = m.stage_ntrees[s];
    std::vector<char> used((size_t)nt, 0);
    int left = nt;
    while (left > 0) {
      // per slot: how many distinct words each bank already holds in this 32-lane group
      std::vector<std::vector<int>> words(12 * 32);
      int mx[12] = {0};
      for (int lane = 0; lane < 32 && left > 0; lane++) {
        int best = -1, best_v = 0, best_cost = 1 << 30;
        int looked = 0;
        for (int i = 0; i < nt && looked < 48; i++) {  // bounded look-ahead keeps detector creation fast
          if (used[(size_t)i]) continue;
          looked++;
          const HaarStumpDev& c = t[(size_t)first + i];
          const int nslots = c.nrect == 3 ? 12 : 8;
          for (int v = 0; v < (c.nrect == 3 ? 64 : 16); v++) {
            const HaarStumpDev r = variant(c, v);
            int cost = 0;
            for (int k = 0; k < nslots; k++) {
              const int o = r.ofs[k >> 2][k & 3];
              const std::vector<int>& w = words[(size_t)k * 32 + (o & 31)];
              const bool present = std::find(w.begin(), w.end(), o) != w.end();
              const int load = (int)w.size() + (present ? 0 : 1);
              if (load > mx[k]) cost += load - mx[k];
            }
            if (cost < best_cost) {
              best_cost = cost;
              best = i;
              best_v = v;
              if (cost == 0) break;
            }
          }
          if (best_cost == 0) break;
        }
        const HaarStumpDev r = variant(t[(size_t)first + best], best_v);
        const int nslots = r.nrect == 3 ? 12 : 8;
        for (int k = 0; k < nslots; k++) {
          const int o = r.ofs[k >> 2][k & 3];
          std::vector<int>& w = words[(size_t)k * 32 + (o & 31)];
          if (std::find(w.begin(), w.end(), o) == w.end()) w.push_back(o);
          mx[k] = std::max(mx[k], (int)w.size());
        }
        out.push_back(r);
        used[(size_t)best] = 1;
        left--;
      }
    }
  }
  return out;
}

template <int STEP>
static void build_haar_nodes(const Cascade& m, std::vector<HaarNodeDev>& out) {
  const TileGeom<STEP> G(m.win_w, m.win_h);
  out.resize(m.node_feature.size());
  for (size_t i = 0; i < out.size(); i++) {
    HaarNodeDev& d = out[i];
    std::memset(&d, 0, sizeof(d));
    const int fi = m.node_feature[i];
    d.nrect = 2;
    for (int j = 0; j < 3; j++) {
      const int32_t* r = &m.haar_rects[(size_t)fi * 12 + j * 4];
      const float wt = m.haar_weights[(size_t)fi * 3 + j];
      d.w[j] = wt;
      const bool used = j < 2 || wt != 0.0f;
      if (j == 2 && wt != 0.0f) d.nrect = 3;
      const int x = used ? r[0] : 0, y = used ? r[1] : 0, rw = used ? r[2] : 0, rh = used ? r[3] : 0;
      if (!m.haar_tilted[fi]) {
        d.ofs[j][0] = G.at(y, x);
        d.ofs[j][1] = G.at(y, x + rw);
        d.ofs[j][2] = G.at(y + rh, x);
        d.ofs[j][3] = G.at(y + rh, x + rw);
      } else {
        const int shift = tile_words_padded(G.words());
        d.ofs[j][0] = shift + G.at(y, x);
        d.ofs[j][1] = shift + G.at(y + rh, x - rh);
        d.ofs[j][2] = shift + G.at(y + rw, x + rw);
        d.ofs[j][3] = shift + G.at(y + rw + rh, x + rw - rh);
      }
    }
    d.thr = m.node_threshold[i];
    d.left = m.node_left[i];
    d.right = m.node_right[i];
  }
}

template <int STEP>
static void build_lbp_nodes(const Cascade& m, std::vector<LbpNodeDev>& out) {
  const TileGeom<STEP> G(m.win_w, m.win_h);
  out.resize(m.node_feature.size());
  for (size_t i = 0; i < out.size(); i++) {
    LbpNodeDev& d = out[i];
    std::memset(&d, 0, sizeof(d));
    const int32_t* r = &m.lbp_rects[(size_t)m.node_feature[i] * 4];
    for (int rr = 0; rr < 4; rr++)
      for (int cc = 0; cc < 4; cc++) d.ofs[4 * rr + cc] = G.at(r[1] + rr * r[3], r[0] + cc * r[2]);
    d.left = m.node_left[i];
    d.right = m.node_right[i];
    for (int j = 0; j < 8; j++) d.subset[j] = m.node_subset[i * 8 + j];
  }
}

static int window_xy(int y, int x) { return (y << 16) | x; }  // GlobalReader records (upright features only)
static void build_haar_gstumps(const Cascade& m, std::vector<HaarStumpDev>& out) { build_haar_stumps_at(m, out, window_xy, 0); }
static void build_lbp_gstumps(const Cascade& m, std::vector<LbpStumpDev>& out) { build_lbp_stumps_at(m, out, window_xy); }

static bool same_params(const cc_detect_params& a, const cc_detect_params& b) {
  return a.scale_factor == b.scale_factor && a.min_w == b.min_w && a.min_h == b.min_h && a.max_w == b.max_w && a.max_h == b.max_h;
}

// Tile list {scale, tx, ty, 0} of a plan for tiles of `tile_y` window rows.
// Workgroups are dealt round-robin over the 8 XCDs (blocks b and b+8 share an L2): the list is permuted so that the tiles
// one XCD receives are neighbours in the image and share their halo rows/columns in that XCD's L2. Placement only changes
// speed, never results.
static std::vector<int4> plan_tile_list(const std::vector<ScaleGeom>& geom, int tile_y, int only_step) {
  std::vector<int4> tiles;
  for (size_t i = 0; i < geom.size(); i++) {
    const ScaleGeom& g = geom[i];
    if (only_step && g.ystep != only_step) continue;
    const int ntx = (g.nx + TILE_X - 1) / TILE_X, nty = (g.ny + tile_y - 1) / tile_y;
    for (int ty_ = 0; ty_ < nty; ty_++)
      for (int tx_ = 0; tx_ < ntx; tx_++) tiles.push_back(make_int4((int)i, tx_, ty_, 0));
  }
  const size_t n = tiles.size(), per = (n + 7) / 8;
  std::vector<int4> perm;
  perm.reserve(n);
  for (size_t j = 0; j < per; j++)
    for (size_t x = 0; x < 8; x++) {
      const size_t src = x * per + j;
      if (src < n) perm.push_back(tiles[src]);
    }
  return perm;
}

// The plan's list of tiles of `tile_y` window rows over the scales of step `only_step` (0 = all). `create`: a missing list
// is built and uploaded -- through the detector's own stream, and waited for there: a copy on the legacy stream (plain
// hipMemcpy) is refused while ANY thread of the process captures a graph, and fails that thread's capture with it (two
// detectors on two host threads, one of them capturing its single-image pass). Otherwise a missing list is an error.
static cc_status plan_tiles(cc_detector* d, Plan* P, int tile_y, int only_step, bool create, const Plan::TileList** out) {
  const std::pair<int, int> key(tile_y, only_step);
  auto it = P->tiles.find(key);
  if (it == P->tiles.end()) {
    if (!create) return set_error(CC_ERR_HIP, "internal: no tile list for tiles of %d window rows (step %d)", tile_y, only_step);
    const std::vector<int4> tv = plan_tile_list(P->geom, tile_y, only_step);
    it = P->tiles.try_emplace(key).first;
    it->second.n = (int)tv.size();
    hipError_t e = it->second.d.upload(tv, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);  // tv ends here
    if (e != hipSuccess) {
      P->tiles.erase(it);
      return set_error(CC_ERR_HIP, "uploading a tile list failed: %s", hipGetErrorString(e));
    }
  }
  *out = &it->second;
  return CC_OK;
}

static cc_status build_plan(cc_detector* d, int w, int h, const cc_detect_params& p, Plan** out) {
  for (auto& pl : d->plans)
    if (pl->w == w && pl->h == h && same_params(pl->p, p)) {
      *out = pl.get();
      return CC_OK;
    }
  std::unique_ptr<Plan> P(new Plan());
  P->w = w;
  P->h = h;
  P->p = p;
  scale_plan(d->m.win_w, d->m.win_h, w, h, p, P->geom);
  const int ns = (int)P->geom.size();
  std::vector<int2> sizes(ns);
  for (int i = 0; i < ns; i++) sizes[i] = make_int2(P->geom[i].w, P->geom[i].h);
  P->front.L = front_layout(w, h, sizes, d->m.feature_type == CC_FEATURE_HAAR && d->m.has_tilted);
  std::vector<int> gridrow_first(ns + 1, 0);
  long long mask_ofs = 0, win_ofs = 0;
  for (int i = 0; i < ns; i++) {
    const ScaleGeom& g = P->geom[i];
    ScaleDev& S = P->front.L.sd[i];
    S.mask_ofs = mask_ofs;
    S.win_ofs = win_ofs;
    S.ystep = g.ystep;
    S.nx = g.nx;
    S.ny = g.ny;
    S.nxw = (g.nx + 63) / 64;
    S.scale = g.scale;
    S.win_w = g.win_w;
    S.win_h = g.win_h;
    mask_ofs += (long long)S.nxw * g.ny;
    win_ofs += (long long)g.nx * g.ny;
    P->integral_elems += (long long)(g.w + 1) * (g.h + 1);
    gridrow_first[i + 1] = gridrow_first[i] + g.ny;
  }
  P->mask_frame_words = (size_t)mask_ofs;
  P->windows = win_ofs;
  P->n_grid_rows = gridrow_first[ns];
  hipStream_t st = d->stream;
  CC_HIP(P->d_gridrow_first.upload(gridrow_first, st));
  CC_HIP(P->front.upload(st));  // synchronises: the host vectors above go out of scope
  const Plan::TileList* own = nullptr;  // the ahead-of-time kernels' list, made like any other
  if (cc_status ts = plan_tiles(d, P.get(), TILE_Y, 0, true, &own); ts != CC_OK) return ts;
  *out = P.get();
  if (d->plans.size() >= 8) d->plans.erase(d->plans.begin());
  d->plans.push_back(std::move(P));
  return CC_OK;
}

enum { EV_RESIZE = 0, EV_INTEGRAL = 1, EV_EVAL = 2, EV_FILTER = 3, EV_EVAL_STEP1 = 4, EV_GROUP = 5 };

struct EvScope {  // records a pair of events around a group of launches when profiling is on
  cc_detector* d;
  int kind;
  hipEvent_t a = nullptr, b = nullptr;
  hipStream_t st;
  EvScope(cc_detector* d_, int kind_, hipStream_t st_) : d(d_), kind(kind_), st(st_) {
    if (!d->profiling || kind < 0) return;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
      a = b = nullptr;
      return;
    }
    (void)hipEventRecord(a, st);
  }
  ~EvScope() {
    if (!a) return;
    (void)hipEventRecord(b, st);
    d->events.push_back(TimingEvent{a, b, kind});
  }
};

static void collect_events(cc_detector* d) {
  for (auto& e : d->events) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
      switch (e.kind) {
        case EV_RESIZE: d->tm.resize_ms += ms; d->tm.resize_launches++; break;
        case EV_INTEGRAL: d->tm.integral_ms += ms; d->tm.integral_launches++; break;
        case EV_EVAL: d->tm.eval_ms += ms; d->tm.eval_launches++; break;
        case EV_EVAL_STEP1: d->tm.eval_step1_ms += ms; break;
        case EV_FILTER: d->tm.finalize_ms += ms; d->tm.finalize_launches++; break;
        case EV_GROUP: d->tm.group_ms += ms; d->tm.group_launches++; break;
      }
    }
    (void)hipEventDestroy(e.a);
    (void)hipEventDestroy(e.b);
  }
  d->events.clear();
}

// The cascade-kernel launches of a pass: one ahead-of-time kernel (fn null) over the plan's TILE_Y tiles, or the specialised
// kernel's module(s), each over the list of its own tile height (and of its step's tiles when there is a module per step).
struct EvalLaunch {
  hipFunction_t fn;
  size_t lds;
  int n_tiles;
  const int4* tiles;
};
static cc_status pass_launches(cc_detector* d, Plan* P, bool create_lists, EvalLaunch out[2], int* n_out) {
  const bool run_spec = d->n_spec > 0 && d->m.max_nodes_per_tree <= 1;
  const int n = run_spec ? d->n_spec : 1;
  for (int i = 0; i < n; i++) {
    const SpecModule aot{nullptr, nullptr, d->lds, TILE_Y, 0};
    const SpecModule& M = run_spec ? d->spec[i] : aot;
    const Plan::TileList* tl = nullptr;
    if (cc_status st = plan_tiles(d, P, M.tile_y, M.only_step, create_lists, &tl); st != CC_OK) return st;
    out[i] = EvalLaunch{M.fn, M.lds, tl->n, tl->d.p};
  }
  *n_out = n;
  return CC_OK;
}

// The specialised kernel may use other tile heights than the ahead-of-time kernels: its tile lists are built on first use,
// before the pass is launched and never from inside a hipGraph capture (run_device_pass only looks them up).
static cc_status ensure_spec_tiles(cc_detector* d, Plan* P) {
  EvalLaunch launches[2];
  int n = 0;
  return pass_launches(d, P, true, launches, &n);
}

// Workspace of a pass in `slot`, sized for pass_capacity frames (only allocations, nothing is enqueued).
static cc_status ensure_pass_workspace(cc_detector* d, const Plan* P, int slot, int nchan, bool tilt, bool debug) {
  const FrontLayout& FL = P->front.L;
  const size_t cap = (size_t)d->pass_capacity;
  CC_HIP(d->d_pyr.ensure(FL.pyr_frame_bytes * cap));
  CC_HIP(d->d_integ[slot].ensure(FL.int_frame_elems * (size_t)nchan * cap));
  CC_HIP(d->d_hbuf.ensure(std::max<size_t>(FL.h_frame_elems * (size_t)nchan * cap, 4)));
  if (tilt) {
    CC_HIP(d->d_diag.ensure(FL.int_frame_elems * 2 * cap));
    CC_HIP(d->d_tseg.ensure(std::max<size_t>(FL.tseg_frame_elems * cap, 1)));
  }
  CC_HIP(d->d_masks[slot].ensure(std::max<size_t>(P->mask_frame_words * cap, 1)));
  if (d->cand_cap == 0) d->cand_cap = 1 << 18;
  CC_HIP(d->d_cands[slot].ensure((size_t)d->cand_cap));
  CC_HIP(d->d_out[slot].ensure((size_t)d->cand_cap));
  if (debug) {
    CC_HIP(d->d_dbg_codes.ensure((size_t)std::max<long long>(P->windows, 1)));
    CC_HIP(d->d_dbg_sums.ensure((size_t)std::max<long long>(P->windows, 1)));
    CC_HIP(d->d_dbg_visited.ensure((size_t)std::max<long long>(P->windows, 1)));
  }
  return CC_OK;
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

// The cascade-kernel launches of a pass over nf frames, one after the other on `st`.
static cc_status launch_eval(cc_detector* d, EvalArgs A, const EvalLaunch* launches, int n_launches, int nf, bool haar, hipStream_t st) {
  for (int i = 0; i < n_launches; i++) {
    const EvalLaunch& L = launches[i];
    if (L.n_tiles == 0) continue;
    A.tiles = L.tiles;
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

// CCAMD_DEBUG_STAMPS=<path>: waits for the pass and writes its stamps, [n_tiles * nf][STAMP_SLOTS] u64 (overwritten per pass).
static cc_status dump_stamps(cc_detector* d, const char* path, int nf) {
  CC_HIP(hipStreamSynchronize(d->stream));
  const int n_tiles_run = d->last_stamp_tiles;
  std::vector<unsigned long long> h((size_t)n_tiles_run * (size_t)nf * STAMP_SLOTS);
  CC_HIP(hipMemcpyAsync(h.data(), d->d_stamps.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, d->stream));
  CC_HIP(hipStreamSynchronize(d->stream));
  if (FILE* f = std::fopen(path, "wb")) {
    const int hdr[4] = {n_tiles_run, nf, STAMP_SLOTS, 0};
    std::fwrite(hdr, sizeof(int), 4, f);
    std::fwrite(h.data(), sizeof(unsigned long long), h.size(), f);
    std::fclose(f);
  }
  return CC_OK;
}

// Device pipeline for up to max_batch frames already resident on the device. Leaves the filtered candidate list
// (d_out[slot], d_counts[slot][1]) on the device; no synchronisation.
static cc_status run_device_pass(cc_detector* d, Plan* P, const uint8_t* dframes, int nf, size_t row_stride,
                                 size_t frame_stride, bool debug, int slot, bool single_stream = false) {
  const int ns = (int)P->front.L.sd.size();
  hipStream_t st = d->stream;
  hipStream_t fs = d->overlap_front && !single_stream ? d->front_stream : d->stream;  // pyramid + integrals
  const bool haar = d->m.feature_type == CC_FEATURE_HAAR;
  const bool tilt = haar && d->m.has_tilted;
  const int nchan = haar ? (tilt ? 3 : 2) : 1;  // sum, sqsum, tilted
  CC_HIP(d->d_counts[slot].ensure(2));
  CC_HIP(hipMemsetAsync(d->d_counts[slot].p, 0, 2 * sizeof(int), st));
  if (ns == 0 || nf == 0) return CC_OK;
  // even window sizes: the variance rectangle's corners of step-2 scales sit on odd rows and odd columns only
  const int sq_compact = (haar && d->m.win_w % 2 == 0 && d->m.win_h % 2 == 0) ? 1 : 0;
  if (cc_status ws = ensure_pass_workspace(d, P, slot, nchan, tilt, debug); ws != CC_OK) return ws;
  // this slot's integrals may still be read by the cascade kernel launched two passes ago
  if (fs != st && d->eval_pending[slot]) CC_HIP(hipStreamWaitEvent(fs, d->eval_done[slot], 0));
  FrontIO io;
  io.src = dframes;
  io.row_stride = row_stride;
  io.frame_stride = frame_stride;
  io.pyr = d->d_pyr.p;
  io.integ = d->d_integ[slot].p;
  io.hbuf = d->d_hbuf.p;
  io.diag = d->d_diag.p;
  io.tseg = d->d_tseg.p;
  io.nchan = nchan;
  io.sq = haar;
  io.sq_odd_rows_only = sq_compact;
  {
    EvScope ev(d, EV_RESIZE, fs);
    launch_front(fs, P->front, io, nf, FRONT_RESIZE);
  }
  {
    EvScope ev(d, EV_INTEGRAL, fs);
    launch_front(fs, P->front, io, nf, FRONT_INTEGRALS);
  }
  if (fs != st) {
    CC_HIP(hipEventRecord(d->front_done[slot], fs));
    CC_HIP(hipStreamWaitEvent(st, d->front_done[slot], 0));
  }
  {
    EvScope ev(d, EV_EVAL, st);
    EvalArgs A = eval_args(d, P, slot, nchan, tilt, sq_compact, debug);
    EvalLaunch launches[2];
    int n_launches = 0;
    if (cc_status ls = pass_launches(d, P, false, launches, &n_launches); ls != CC_OK) return ls;
    size_t stamp_tiles = 0;
    for (int i = 0; i < n_launches; i++) stamp_tiles += (size_t)launches[i].n_tiles;
    if (std::getenv("CCAMD_DEBUG_STAMPS")) {  // timing experiments: per-block phase stamps of the cascade kernel (launch after launch)
      CC_HIP(d->d_stamps.ensure(std::max<size_t>(stamp_tiles * (size_t)nf * STAMP_SLOTS, 1)));
      CC_HIP(hipMemsetAsync(d->d_stamps.p, 0, stamp_tiles * (size_t)nf * STAMP_SLOTS * sizeof(unsigned long long), st));
      A.stamps = d->d_stamps.p;
    }
    if (cc_status es = launch_eval(d, A, launches, n_launches, nf, haar, st); es != CC_OK) return es;
    d->last_stamp_tiles = (int)stamp_tiles;
  }
  if (fs != st) {
    CC_HIP(hipEventRecord(d->eval_done[slot], st));
    d->eval_pending[slot] = true;
  }
  {
    EvScope ev(d, EV_FILTER, st);
    hipLaunchKernelGGL(k_filter_candidates, dim3(64), dim3(256), 0, st, d->d_cands[slot].p, d->d_counts[slot].p, d->cand_cap, P->front.d_sd.p,
                       d->d_masks[slot].p, P->mask_frame_words, d->d_out[slot].p, d->d_counts[slot].p + 1);
    if (debug && P->n_grid_rows)
      hipLaunchKernelGGL(k_debug_visited, dim3(P->n_grid_rows), dim3(256), 0, st, P->front.d_sd.p, ns, P->d_gridrow_first.p,
                         d->d_masks[slot].p, d->d_dbg_visited.p);
  }
  CC_HIP(hipGetLastError());
  if (const char* path = std::getenv("CCAMD_DEBUG_STAMPS"))
    if (cc_status ds = dump_stamps(d, path, nf); ds != CC_OK) return ds;
  d->tm.frames += nf;
  d->tm.grid_windows += P->windows * nf;
  d->tm.integral_elems += P->integral_elems * nf;
  return CC_OK;
}

// Colour formats: row_stride counts bytes (width * bytes per pixel at least) and, with more than one frame, frame_stride must
// hold a whole frame of the format. Gray frames are checked as they always were.
static cc_status check_frame_args(const cc_detector* d, const FrameSet& F, const cc_detect_params* p, const char* who) {
  if (!d || !p || (!F.frames && F.n_frames > 0)) return set_error(CC_ERR_INVALID_ARG, "%s: null argument", who);
  const int bpp = pix_bytes(F.fmt);
  if (bpp == 0) return set_error(CC_ERR_INVALID_ARG, "%s: unknown pixel format %d", who, F.fmt);
  if (F.n_frames < 0 || F.width < 1 || F.height < 1 || F.row_stride < (size_t)F.width * bpp)
    return set_error(CC_ERR_INVALID_ARG, "%s: bad frame geometry (%dx%d, stride %zu, n %d)", who, F.width, F.height, F.row_stride, F.n_frames);
  if (F.fmt != CC_PIX_GRAY8 && F.n_frames > 1 &&
      F.frame_stride < (size_t)(pix_rows(F.fmt, F.height) - 1) * F.row_stride + (size_t)F.width * bpp)
    return set_error(CC_ERR_INVALID_ARG, "%s: frame stride %zu shorter than one frame of pixel format %d", who, F.frame_stride, F.fmt);
  if (F.width > 32768 || F.height > 32768) return set_error(CC_ERR_UNSUPPORTED, "%s: frames larger than 32768 px per side", who);
  if (!(p->scale_factor > 1.0)) return set_error(CC_ERR_INVALID_ARG, "%s: scaleFactor must be > 1", who);
  return CC_OK;
}

// The candidate lists of BOTH slots are freed (run_device_pass allocates them again, `raw` and half as many entries long),
// so every pass launched before this belongs to an older generation of the lists.
static void grow_candidate_lists(cc_detector* d, int raw) {
  d->cand_cap = raw + raw / 2;
  for (int s = 0; s < 2; s++) {
    d->d_cands[s].release();
    d->d_out[s].release();
  }
  d->list_gen++;
}

// A pass's two counters (raw and filtered candidates) travel to the pinned h_counts behind its kernels; pass_done[slot]
// tells when they have arrived.
static cc_status read_back_counts(cc_detector* d, int slot) {
  CC_HIP(hipMemcpyAsync(d->h_counts + 2 * slot, d->d_counts[slot].p, 2 * sizeof(int), hipMemcpyDeviceToHost, d->stream));
  CC_HIP(hipEventRecord(d->pass_done[slot], d->stream));
  return CC_OK;
}

// Device-output pass: behind the pass's kernels on the detector's stream, the ordering and grouping kernels append its
// rectangles to the caller's buffers at the batch's running total (d_group_state[0]). They drop out when the pass's list
// overflowed or a pass before it set the abort word (GroupGuard). Runs for a plan without scales too (run_device_pass has
// zeroed the counters by then): that is what writes such a pass's offsets.
static cc_status enqueue_group(cc_detector* d, const cc_detector::PendingPass& ps) {
  // sized here, where cand_cap is known; allocates only while the detector's lists or passes are still growing
  const bool scored = ps.dev.d_weights != nullptr;  // the scored buffers come with the detector's first scored pass
  CC_HIP(d->group.ensure((size_t)std::max(d->cand_cap, 1), (size_t)d->pass_capacity, true, scored));
  const GroupGuard g{d->d_counts[ps.slot].p, d->cand_cap, d->d_group_state.p + 1};
  const GroupScores sc{scored, nullptr, ps.dev.level, d->group.ordered_weights.p, ps.dev.d_levels, ps.dev.d_weights};
  {
    EvScope ev(d, EV_GROUP, d->stream);
    launch_order_candidates(d->stream, g, d->d_out[ps.slot].p, ps.nf, d->group, scored);
    launch_group_frames(d->stream, g, d->group.ordered.p, d->group.seg.p, ps.nf, ps.dev.min_neighbors, 0.2, d->group, ps.dev.d_out,
                        ps.dev.cap, ps.dev.d_offsets, d->d_group_state.p, sc);
  }
  CC_HIP(hipGetLastError());
  return CC_OK;
}

// Fetches the results of the pending pass and hands them to its sink. On candidate-list overflow the lists grow and the
// pass is redone synchronously. Growing frees the lists of BOTH slots; a pass is judged against the capacity it was
// launched with and against the generation of the lists it wrote into (stale generation => redone as well).
// Device-output passes append at a running total, so unlike host-output passes they must be redone in batch order. One that
// overflowed has written nothing and has set the abort word, so the pass launched behind it has written nothing either;
// that pass is stale by then (an overflow always grows the lists: raw > ps.cap at the current generation means ps.cap ==
// cand_cap), and run_batch retires it, and so redoes it from its frames, still in their staging slot, before it launches the
// next pass. Here the redo clears the abort word first and runs the grouping kernels again behind the pass.
static cc_status retire_pending(cc_detector* d) {
  if (!d->pending.active) return CC_OK;
  cc_detector::PendingPass ps = d->pending;
  d->pending.drop();
  std::vector<CandOut> got;
  for (;;) {
    CC_HIP(hipEventSynchronize(d->pass_done[ps.slot]));
    const int raw = d->h_counts[2 * ps.slot], kept = d->h_counts[2 * ps.slot + 1];
    if (raw > ps.cap || ps.gen != d->list_gen) {
      CC_HIP(hipStreamSynchronize(d->stream));
      if (raw > d->cand_cap) grow_candidate_lists(d, raw);
      if (ps.dev) CC_HIP(hipMemsetAsync(d->d_group_state.p + 1, 0, sizeof(int), d->stream));
      cc_status st2 = run_device_pass(d, ps.plan, ps.dptr, ps.nf, ps.rs, ps.fs, ps.debug, ps.slot, false);
      if (st2 != CC_OK) return st2;
      ps.cap = d->cand_cap;
      ps.gen = d->list_gen;
      if (cc_status gs = ps.dev ? enqueue_group(d, ps) : CC_OK; gs != CC_OK) return gs;
      if (cc_status cs = read_back_counts(d, ps.slot); cs != CC_OK) return cs;
      continue;
    }
    if (ps.dev) return CC_OK;  // its rectangles are in the caller's buffers: nothing to fetch, nobody to hand them to
    got.resize((size_t)kept);
    if (kept > 0) {  // the copy stream is free to run while the main stream executes the next pass
      CC_HIP(hipMemcpyAsync(got.data(), d->d_out[ps.slot].p, (size_t)kept * sizeof(CandOut), hipMemcpyDeviceToHost, d->copy_stream));
      CC_HIP(hipStreamSynchronize(d->copy_stream));
      for (CandOut& c : got) c.frame += ps.f0;
    }
    if (ps.sink && ps.sink->async_consume) {
      std::shared_ptr<BatchSink> sk = ps.sink;
      const int jf0 = ps.f0, jnf = ps.nf;
      auto cands = std::make_shared<std::vector<CandOut>>(std::move(got));
      sk->jobs.push_back(std::async(std::launch::async, [sk, jf0, jnf, cands]() { sk->consume(jf0, jnf, *cands); }));
    } else if (ps.sink && ps.sink->consume)
      ps.sink->consume(ps.f0, ps.nf, got);
    return CC_OK;
  }
}
// Retires a pass that belongs to another batch than the caller's: its failure is that batch's, reported when it is collected.
static void retire_foreign(cc_detector* d) {
  if (!d->pending.active) return;
  std::shared_ptr<BatchSink> sink = d->pending.sink;
  const cc_status st = retire_pending(d);
  if (st != CC_OK && sink && sink->status == CC_OK) {
    sink->status = st;
    sink->error = cc_last_error();
  }
}

// Host frames -> the device staging area of `slot`, on the front stream. Pageable memory (what a caller of the reference's
// shape hands over, tools/detection/Cpp/main.cpp:27-45) cannot be copied asynchronously: the runtime stages it through
// its own pinned chunks on the calling thread, copy after copy, and the call returns when the last one is on the device
// (round 3: a step of 64 Full-HD frames took 19.9 ms this way against 17.2 with resident frames). So the detector keeps
// its own pinned staging area, kStageSlots slots like the device one: the frames of a pass are copied into it by a few host
// threads (tight rows), then ONE asynchronous copy on the front stream moves the pass to the device while the cascade
// kernels of the pass before run -- and the caller's frames are free again when the call returns. A pinned slot is
// reused kStageSlots passes later; run_batch has retired its pass by then (it stages pass i + 1 only after pass i - 2 is
// retired), so its copy is long complete. Frames that already live in pinned memory (hipHostMalloc / hipHostRegister)
// skip the staging copy: those must stay valid until the call that retires their pass (include/cascadeclassifier_amd.h).
// The slots have ONE pitch for all passes (h_stage_bytes / kStageSlots), not the pass's own frame size: gray and colour
// passes of one plan stage different byte counts per frame, and a pending pass of the other format may still be copying out
// of its slot when the next call fills its own (a pitch per format would make the slots of the two formats overlap). The
// area only grows, after the front stream has finished every copy out of it.
static cc_status stage_host_frames(cc_detector* d, const uint8_t* src, int nf, int width, int height, size_t row_stride,
                                   size_t frame_stride, uint8_t* dev, size_t rs, size_t fs, int slot, hipStream_t front) {
  hipPointerAttribute_t attr;
  bool pinned = false;
  if (hipPointerGetAttributes(&attr, src) == hipSuccess)
    pinned = attr.type == hipMemoryTypeHost;
  else
    (void)hipGetLastError();  // ordinary pageable memory is "invalid value" to this query on some runtimes
  static const bool no_stage = std::getenv("CCAMD_NO_PINNED_STAGING") != nullptr;  // the round-3 path, for A/B runs
  if (pinned || no_stage) {
    for (int f = 0; f < nf; f++)
      CC_HIP(hipMemcpy2DAsync(dev + (size_t)f * fs, rs, src + (size_t)f * frame_stride, row_stride, (size_t)width, (size_t)height,
                              hipMemcpyHostToDevice, front));
    return CC_OK;
  }
  const size_t need = fs * (size_t)d->pass_capacity * kStageSlots;
  if (d->h_stage_bytes / kStageSlots < fs * (size_t)d->pass_capacity) {
    if (d->h_stage) {
      CC_HIP(hipStreamSynchronize(front));  // no copy may still be reading the old area
      (void)hipHostFree(d->h_stage);
    }
    d->h_stage = nullptr;
    d->h_stage_bytes = 0;
    CC_HIP(hipHostMalloc(reinterpret_cast<void**>(&d->h_stage), need, hipHostMallocDefault));
    d->h_stage_bytes = need;
  }
  uint8_t* hs = d->h_stage + (size_t)slot * (d->h_stage_bytes / kStageSlots);
  auto copy_frames = [&](int fa, int fb) {
    for (int f = fa; f < fb; f++) {
      const uint8_t* sf = src + (size_t)f * frame_stride;
      uint8_t* df = hs + (size_t)f * fs;
      if (row_stride == rs)
        std::memcpy(df, sf, (size_t)(height - 1) * rs + (size_t)width);
      else
        for (int y = 0; y < height; y++) std::memcpy(df + (size_t)y * rs, sf + (size_t)y * row_stride, (size_t)width);
    }
  };
  static const int want_threads = []() {
    const unsigned hc = std::thread::hardware_concurrency();
    return (int)std::max(1u, std::min(8u, hc / 2));  // 64 Full-HD frames per step: 2 threads 18.2, 4 17.9, 8 17.85 ms (resident frames 17.44)
  }();
  const size_t total = fs * (size_t)nf;
  const int nt = (int)std::min<size_t>((size_t)std::min(want_threads, nf), std::max<size_t>(1, total >> 21));  // >= 2 MB per thread
  if (nt <= 1) {
    copy_frames(0, nf);
  } else {
    std::vector<std::future<void>> jobs;
    try {
      for (int t = 1; t < nt; t++) {
        const int fa = (int)((long long)nf * t / nt), fb = (int)((long long)nf * (t + 1) / nt);
        jobs.push_back(std::async(std::launch::async, copy_frames, fa, fb));
      }
      copy_frames(0, nf / nt);
      for (auto& j : jobs) j.get();
    } catch (const std::exception& e) {
      for (auto& j : jobs)
        if (j.valid()) j.wait();
      return set_error(CC_ERR_HIP, "staging host frames: %s", e.what());
    }
  }
  CC_HIP(hipMemcpyAsync(dev, hs, total, hipMemcpyHostToDevice, front));
  return CC_OK;
}

static void spec_poll(cc_detector* d);  // installs a finished background specialisation

// Retires the pending pass, if any, on behalf of the batch that delivers to `sink`: as its own when it is that batch's (an
// error is the caller's), as a foreign one otherwise (an error is kept for the batch it belongs to).
static cc_status retire_for(cc_detector* d, const std::shared_ptr<BatchSink>& sink) {
  if (!d->pending.active) return CC_OK;
  if (d->pending.sink == sink) return retire_pending(d);
  retire_foreign(d);
  return CC_OK;
}

// The streams, events and pinned counters of the pass loop, created by the first detection call.
static cc_status ensure_pipeline_objects(cc_detector* d) {
  if (d->copy_stream) return CC_OK;
  CC_HIP(hipStreamCreateWithFlags(&d->copy_stream, hipStreamNonBlocking));
  CC_HIP(hipEventCreateWithFlags(&d->pass_done[0], hipEventDisableTiming));
  CC_HIP(hipEventCreateWithFlags(&d->pass_done[1], hipEventDisableTiming));
  CC_HIP(hipHostMalloc(reinterpret_cast<void**>(&d->h_counts), 4 * sizeof(int), hipHostMallocDefault));
  {  // the pyramid / integral stream only fills what the cascade kernel leaves idle: lowest priority
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    CC_HIP(hipStreamCreateWithPriority(&d->front_stream, hipStreamNonBlocking, least));
  }
  for (hipEvent_t* e : {&d->front_done[0], &d->front_done[1], &d->eval_done[0], &d->eval_done[1], &d->batch_begin})
    CC_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
  d->overlap_front = std::getenv("CCAMD_NO_FRONT_OVERLAP") ? 0 : 1;
  return CC_OK;
}

// Single host image: one pass on one stream, replayed from a hipGraph once the buffers are sized. Hands the candidates to
// `sink` and sets `delivered`, or leaves it false when the candidate lists overflowed: the ordinary path then grows the
// lists and redoes the pass.
static cc_status run_single_image_graph(cc_detector* d, Plan* P, const FrameSet& F, BatchSink& sink, bool* delivered) {
  *delivered = false;
  const size_t rs = (size_t)align_up(F.width, 4), fs = rs * (size_t)F.height;
  const bool color = F.fmt != CC_PIX_GRAY8;
  // colour: rows of width * bpp bytes (planar: 3 * height rows of width) at a pitch of their own
  const int crows = pix_rows(F.fmt, F.height);
  const size_t cw = (size_t)F.width * pix_bytes(F.fmt), cpitch = (size_t)align_up((int)cw, 4), cfs = cpitch * (size_t)crows;
  uint8_t*& hbuf = color ? d->h_color_frame : d->h_frame;
  size_t& hbytes = color ? d->h_color_frame_bytes : d->h_frame_bytes;
  const size_t hneed = color ? cfs : fs;
  if (hbytes < hneed) {
    if (hbuf) (void)hipHostFree(hbuf);
    hbuf = nullptr;
    hbytes = 0;
    CC_HIP(hipHostMalloc(reinterpret_cast<void**>(&hbuf), hneed, hipHostMallocDefault));
    hbytes = hneed;
  }
  if (color)
    for (int y = 0; y < crows; y++) std::memcpy(hbuf + (size_t)y * cpitch, F.frames + (size_t)y * F.row_stride, cw);
  else
    for (int y = 0; y < F.height; y++) std::memcpy(d->h_frame + (size_t)y * rs, F.frames + (size_t)y * F.row_stride, (size_t)F.width);
  CC_HIP(d->d_frames.ensure(fs * (size_t)d->pass_capacity * 2));
  if (color) {
    if (d->d_color.n < cfs && d->d_color.p && d->front_stream) CC_HIP(hipStreamSynchronize(d->front_stream));  // batch conversions
    CC_HIP(d->d_color.ensure(cfs));
  }
  auto body = [&]() -> cc_status {
    if (color) {
      CC_HIP(hipMemcpyAsync(d->d_color.p, d->h_color_frame, cfs, hipMemcpyHostToDevice, d->stream));
      launch_to_gray(d->stream, F.fmt, d->d_color.p, cpitch, cfs, F.width, F.height, 1, d->d_frames.p, rs, fs);
    } else
      CC_HIP(hipMemcpyAsync(d->d_frames.p, d->h_frame, fs, hipMemcpyHostToDevice, d->stream));
    cc_status s2 = run_device_pass(d, P, d->d_frames.p, 1, rs, fs, false, 0, true);
    if (s2 != CC_OK) return s2;
    CC_HIP(hipMemcpyAsync(d->h_counts, d->d_counts[0].p, 2 * sizeof(int), hipMemcpyDeviceToHost, d->stream));
    return CC_OK;
  };
  auto key_now = [&]() {
    return std::vector<const void*>{d->d_frames.p, hbuf, color ? d->d_color.p : nullptr, d->d_pyr.p, d->d_integ[0].p, d->d_hbuf.p, d->d_diag.p, d->d_tseg.p, d->d_masks[0].p, d->d_cands[0].p,
                                    d->d_out[0].p, d->d_counts[0].p, d->h_counts, (const void*)d->spec[0].fn, (const void*)d->spec[1].fn, (const void*)d->stream,
                                    (const void*)(size_t)d->cand_cap, (const void*)(size_t)d->wave_below, (const void*)(size_t)(d->stop_after + 16)};
  };
  if (d->eval_pending[0] || d->eval_pending[1]) {  // a batch call may still be using the buffers on the other stream
    CC_HIP(hipStreamSynchronize(d->front_stream));
    d->eval_pending[0] = d->eval_pending[1] = false;
  }
  bool launched = false;
  d->last_call_graph = 0;
  hipGraphExec_t& gexec = P->graph_exec[F.fmt];
  if (gexec && P->graph_key[F.fmt] == key_now()) {
    CC_HIP(hipGraphLaunch(gexec, d->stream));
    launched = true;
    d->last_call_graph = 1;
  } else if (P->graph_warm[F.fmt]) {
    if (gexec) (void)hipGraphExecDestroy(gexec);
    gexec = nullptr;
    hipGraph_t graph = nullptr;
    // Relaxed mode: this thread's stream-ordered calls are captured, nobody's legacy-stream calls are policed (other
    // host threads may be inside synchronous copies of their own handles; under the stricter modes HIP fails those
    // calls and invalidates this capture). One capture at a time per process; if a capture does not come out, the
    // detector simply stops using graphs.
    static std::mutex capture_mu;
    hipError_t ce = hipSuccess, ie = hipSuccess;
    cc_status s2 = CC_OK;
    {
      std::lock_guard<std::mutex> capture_lock(capture_mu);
      ce = std::getenv("CCAMD_DEBUG_FAIL_CAPTURE") ? hipErrorStreamCaptureUnsupported  // tests: the fallback path
                                                   : hipStreamBeginCapture(d->stream, hipStreamCaptureModeRelaxed);
      if (ce == hipSuccess) {
        s2 = body();
        ce = hipStreamEndCapture(d->stream, &graph);
      }
    }
    if (ce == hipSuccess && s2 == CC_OK && graph) ie = hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0);
    if (graph) (void)hipGraphDestroy(graph);
    if (ce != hipSuccess || s2 != CC_OK || ie != hipSuccess || !gexec) {
      // said once per detector, on stderr: the call still succeeds, only the launch-bound single-image path gets slower
      std::fprintf(stderr, "[ccamd] hipGraph capture of the single-image pass failed (begin/end: %s, body status %d, instantiate: %s): "
                           "this detector uses ordinary launches from now on\n",
                   hipGetErrorString(ce), (int)s2, hipGetErrorString(ie));
      (void)hipGetLastError();
      gexec = nullptr;
      d->use_graph = 0;  // ordinary launches from now on (this call included)
    } else {
      P->graph_key[F.fmt] = key_now();
      d->graph_captures++;
      CC_HIP(hipGraphLaunch(gexec, d->stream));
      launched = true;
      d->last_call_graph = 1;
    }
  }
  if (!launched) {
    const cc_status stt = body();
    if (stt != CC_OK) return stt;
    P->graph_warm[F.fmt] = true;  // every buffer now has its size: the next call can be captured
  }
  CC_HIP(hipStreamSynchronize(d->stream));
  const int raw = d->h_counts[0], kept = d->h_counts[1];
  if (raw <= d->cand_cap) {
    std::vector<CandOut> got((size_t)kept);
    if (kept > 0) {
      CC_HIP(hipMemcpyAsync(got.data(), d->d_out[0].p, (size_t)kept * sizeof(CandOut), hipMemcpyDeviceToHost, d->stream));
      CC_HIP(hipStreamSynchronize(d->stream));
    }
    if (sink.consume) sink.consume(0, 1, got);
    *delivered = true;
  }
  return CC_OK;
}

// Stages frames [pf0, pf0 + pnf) of the batch (host frames, or colour frames wherever they are) into the next staging slot,
// on `front`; `where` receives the slot's gray frames. `sink`: the calling batch's, for a pending pass that must go first.
// Host frames: THREE staging slots (device and pinned), handed out round-robin across passes and calls. The frames of
// pass i + 1 are staged and their copy issued right after pass i is launched and BEFORE the pass before it is fetched
// (a blocking wait), so the host copy and the H2D transfer of a pass run a whole pass ahead of the kernels that read
// them. Two slots are not enough for that: the slot of pass i + 1 would be the one of pass i - 1, which is still
// unfetched at that point and re-reads its frames if it has to be redone (candidate-list overflow). With three, the slot
// that is overwritten belongs to pass i - 2, fetched when pass i - 1 was launched.
// Colour frames take the same slots: k_to_gray writes the pass's gray frames there (from the caller's device buffer, or from
// d_color, where stage_host_frames has put host frames), so a redone pass re-reads gray frames like any other. The rule holds
// only while every pass uses the same slot pitch: the device slots are gray frames of the plan (a pending pass of another
// plan is retired first), the pinned slots have one pitch for every format (stage_host_frames).
static cc_status stage_pass(cc_detector* d, const std::shared_ptr<BatchSink>& sink, const FrameSet& F, hipStream_t front, int pf0, int pnf,
                            const uint8_t** where) {
  const size_t rs = (size_t)align_up(F.width, 4), fs = rs * (size_t)F.height;
  const size_t need = fs * (size_t)d->pass_capacity * kStageSlots;
  if (d->d_frames.n < need && d->pending.active) {
    // Growing the staging area frees it, and the unfetched pass still names its frames there (round-3 advisor finding).
    const cc_status st2 = retire_for(d, sink);
    if (st2 != CC_OK) return st2;
  }
  if (d->d_frames.n < need) d->stage_slot = 0;
  CC_HIP(d->d_frames.ensure(need));
  const int sslot = d->stage_slot;
  d->stage_slot = (d->stage_slot + 1) % kStageSlots;
  uint8_t* stage = d->d_frames.p + (size_t)sslot * fs * (size_t)d->pass_capacity;
  if (F.fmt == CC_PIX_GRAY8) {
    const cc_status st2 = stage_host_frames(d, F.frames + (size_t)pf0 * F.frame_stride, pnf, F.width, F.height, F.row_stride, F.frame_stride, stage, rs,
                                            fs, sslot, front);
    if (st2 != CC_OK) return st2;
    *where = stage;
    return CC_OK;
  }
  const uint8_t* csrc = F.frames + (size_t)pf0 * F.frame_stride;
  size_t crs = F.row_stride, cfs = F.frame_stride;
  if (!F.on_device) {  // the colour bytes travel as they are, like gray frames, into d_color
    const int crows = pix_rows(F.fmt, F.height);
    const size_t cw = (size_t)F.width * pix_bytes(F.fmt);
    crs = (size_t)align_up((int)cw, 4);
    cfs = crs * (size_t)crows;
    const size_t cneed = cfs * (size_t)d->pass_capacity;
    if (d->d_color.n < cneed && d->d_color.p) CC_HIP(hipStreamSynchronize(front));  // the last k_to_gray may still read it
    CC_HIP(d->d_color.ensure(cneed));
    const cc_status st2 = stage_host_frames(d, csrc, pnf, (int)cw, crows, F.row_stride, F.frame_stride, d->d_color.p, crs, cfs, sslot, front);
    if (st2 != CC_OK) return st2;
    csrc = d->d_color.p;
  }
  {
    EvScope ev(d, EV_RESIZE, front);  // the conversion's time counts as pyramid time (include/cascadeclassifier_amd.h)
    launch_to_gray(front, F.fmt, csrc, crs, cfs, F.width, F.height, pnf, stage, rs, fs);
  }
  CC_HIP(hipGetLastError());
  *where = stage;
  return CC_OK;
}

// The pass loop of run_batch: runs the batch in passes. `sink->consume` (optional) receives the filtered candidates of each
// pass (frame indices made global) on the calling thread. With two or more frames the batch is cut into at least two passes
// and the host side of pass i (copy-back + consume) overlaps the device side of pass i+1.
// `opt.defer_last`: the batch's last pass stays pending when the call returns (cc_detect_batch_submit); its candidates reach
// `consume` when the next call -- or cc_detect_batch_collect -- retires it.
// `opt.dev`: a device-output batch. Its passes go through this same loop; each is followed by enqueue_group, and retiring
// one delivers nothing (retire_pending, which also has the rule that keeps their output in order).
// `F.fmt` (CC_PIX_*): colour frames become gray frames in the staging slots (stage_pass) before the pass reads them.
static cc_status run_batch_passes(cc_detector* d, const FrameSet& F, const cc_detect_params* p, const std::shared_ptr<BatchSink>& sink,
                                  const BatchOptions& opt) {
  const bool want_results = opt.want_results, debug = opt.debug, defer_last = opt.defer_last, to_device = (bool)opt.dev;
  const int n_frames = F.n_frames;
  cc_status stt = ensure_device(d->device);
  if (stt != CC_OK) return stt;
  // A pass of an earlier (submitted) batch may still be pending. It can stay so -- and overlap this call's first pass --
  // only if this call runs ordinary host-output passes on the same plan; everything else fetches it first.
  const bool single_image_graph = n_frames == 1 && !F.on_device && want_results && !debug && !to_device && !d->profiling && d->use_graph;
  if (d->pending.active) {
    bool same_plan = false;
    for (auto& pl : d->plans)
      if (pl.get() == d->pending.plan && pl->w == F.width && pl->h == F.height && same_params(pl->p, *p)) same_plan = true;
    if (!same_plan || debug || !want_results || to_device || single_image_graph || n_frames < 1) retire_foreign(d);  // (a new plan may evict the pending pass's)
  }
  spec_poll(d);
  Plan* P = nullptr;
  if (stt = build_plan(d, F.width, F.height, *p, &P); stt != CC_OK) return stt;
  if (stt = ensure_spec_tiles(d, P); stt != CC_OK) return stt;
  if (stt = ensure_pipeline_objects(d); stt != CC_OK) return stt;
  hipStream_t front = d->overlap_front ? d->front_stream : d->stream;
  // Frames produced by earlier work on a stream the CALLER gave us (cc_detector_set_stream) must be complete before the
  // pyramid reads them. On the detector's own stream there is only our own earlier work -- a pending pass of the batch
  // submitted before -- and waiting for that would serialise exactly what cc_detect_batch_submit exists to overlap.
  if (front != d->stream && d->stream != d->own_stream) {
    CC_HIP(hipEventRecord(d->batch_begin, d->stream));
    CC_HIP(hipStreamWaitEvent(front, d->batch_begin, 0));
  }
  if (single_image_graph) {
    bool delivered = false;
    stt = run_single_image_graph(d, P, F, *sink, &delivered);
    if (stt != CC_OK || delivered) return stt;
  }
  const std::vector<int> sizes = pass_sizes(n_frames, d->max_batch, d->pipeline_passes, d->pipeline_passes_set != 0, want_results, defer_last);
  for (int v : sizes) d->pass_capacity = std::max(d->pass_capacity, v);  // the workspace only ever grows
  if (to_device) {  // the batch's running total and the abort word start at zero; a batch without frames has one offset
    CC_HIP(d->d_group_state.ensure(2));
    CC_HIP(hipMemsetAsync(d->d_group_state.p, 0, 2 * sizeof(int), d->stream));
    if (sizes.empty()) CC_HIP(hipMemsetAsync(opt.dev.d_offsets, 0, sizeof(int32_t), d->stream));
  }
  const bool staged = !F.on_device || F.fmt != CC_PIX_GRAY8;
  const uint8_t* prestaged = nullptr;
  // spec_poll may have installed another kernel: a pending pass keeps the results it was launched for, nothing to redo.
  int f0 = 0;
  for (size_t pi = 0; pi < sizes.size(); f0 += sizes[pi], pi++) {
    const int slot = d->next_slot;
    cc_detector::PendingPass ps;
    ps.plan = P;
    ps.f0 = f0;
    ps.nf = sizes[pi];
    ps.slot = slot;
    ps.rs = F.row_stride;
    ps.fs = F.frame_stride;
    ps.debug = debug;
    ps.dev = opt.dev;
    if (to_device) ps.dev.d_offsets += f0;
    ps.sink = sink;
    if (!staged) {
      ps.dptr = F.frames + (size_t)f0 * F.frame_stride;
    } else {
      ps.rs = (size_t)align_up(F.width, 4);
      ps.fs = ps.rs * (size_t)F.height;
      if (!prestaged) {
        if (stt = stage_pass(d, sink, F, front, f0, sizes[pi], &prestaged); stt != CC_OK) return stt;
      }
      ps.dptr = prestaged;
      prestaged = nullptr;
    }
    // the slot's result buffers are free: the pass that used them last was retired when the pass after it was launched
    static const bool trace_host = std::getenv("CCAMD_TRACE_HOST") != nullptr;  // host-side timeline of the pass loop (stderr)
    const auto th0 = std::chrono::steady_clock::now();
    auto th = [&](const char* what) {
      if (trace_host)
        std::fprintf(stderr, "[ccamd host] pass %zu %-18s +%.3f ms\n", pi, what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - th0).count());
    };
    if (stt = run_device_pass(d, P, ps.dptr, ps.nf, ps.rs, ps.fs, debug, slot); stt != CC_OK) return stt;
    ps.cap = d->cand_cap;
    ps.gen = d->list_gen;
    if (stt = to_device ? enqueue_group(d, ps) : CC_OK; stt != CC_OK) return stt;
    th("launched");
    if (staged && pi + 1 < sizes.size() && want_results) {  // the next pass's frames travel while this pass runs
      if (stt = stage_pass(d, sink, F, front, f0 + sizes[pi], sizes[pi + 1], &prestaged); stt != CC_OK) return stt;
      th("next pass staged");
    }
    if (want_results) {
      if (stt = read_back_counts(d, slot); stt != CC_OK) return stt;
      // fetch the pass launched before this one -- of this batch or, for the first pass, of the batch submitted before --
      // while the device runs this one
      if (stt = retire_for(d, sink); stt != CC_OK) return stt;
      th("previous retired");
      ps.active = true;
      d->pending = ps;
      // device output: dead behind a pass that overflowed, so redone now, before the next pass is launched (retire_pending)
      if (to_device && ps.gen != d->list_gen)
        if (stt = retire_pending(d); stt != CC_OK) return stt;
    }
    d->next_slot ^= 1;
  }
  if (!(defer_last && d->pending.sink == sink))
    if (stt = retire_for(d, sink); stt != CC_OK) return stt;
  // Profiling: the event pairs of this call are read once their kernels are done. A submitted batch must not wait for that
  // here (the synchronisation would undo the overlap with the next batch -- which is how the round-3 bench first measured
  // its own instrumentation instead of the pipeline): its events are read by cc_detector_get_timings or by the next
  // synchronous call.
  if (d->profiling && !defer_last) {
    CC_HIP(hipStreamSynchronize(d->stream));
    if (d->front_stream) CC_HIP(hipStreamSynchronize(d->front_stream));
    collect_events(d);
  }
  return CC_OK;
}

// A batch that failed leaves none of its passes pending: a later call must not deliver to (or, for device output, redo a pass
// into the buffers of) a call that has returned.
static cc_status run_batch(cc_detector* d, const FrameSet& F, const cc_detect_params* p, const std::shared_ptr<BatchSink>& sink,
                           const BatchOptions& opt = BatchOptions{}) {
  const cc_status st = run_batch_passes(d, F, p, sink, opt);
  if (st != CC_OK && d->pending.active && d->pending.sink == sink) d->pending.drop();
  return st;
}

static void sort_candidates(std::vector<CandOut>& v) {
  std::sort(v.begin(), v.end(), [](const CandOut& a, const CandOut& b) {
    if (a.frame != b.frame) return a.frame < b.frame;
    if (a.scale != b.scale) return a.scale < b.scale;
    if (a.gy != b.gy) return a.gy < b.gy;
    return a.gx < b.gx;
  });
}

// A frame's reject levels and level weights, beside its rectangles (cc_detect_batch_levels_fmt).
struct FrameScores {
  std::vector<int> levels;
  std::vector<double> weights;
};

// Host side of one pass (called while the device already runs the next pass). Per frame: order the candidates (scale, y, x)
// = OpenCV's single-threaded order, then group. Frames are independent, so they are spread over a few host threads.
// scores: grouped as cc_detect_multiscale_levels_fmt groups, every candidate with `level` and its last stage's sum.
static void group_pass(int min_neighbors, int f0, int nf, std::vector<CandOut>& cands, std::vector<std::vector<cc_rect>>& grouped,
                       std::vector<FrameScores>* scores = nullptr, int level = 0) {
  std::vector<std::vector<CandOut>> per_frame((size_t)nf);
  for (const CandOut& c : cands) per_frame[(size_t)(c.frame - f0)].push_back(c);
  auto work = [&](int a0, int a1) {
    for (int f = a0; f < a1; f++) {
      sort_candidates(per_frame[(size_t)f]);
      std::vector<cc_rect>& rects = grouped[(size_t)(f0 + f)];
      rects.reserve(per_frame[(size_t)f].size());
      for (const CandOut& c : per_frame[(size_t)f]) rects.push_back(cc_rect{c.x, c.y, c.w, c.h});
      if (scores) {
        FrameScores& fs = (*scores)[(size_t)(f0 + f)];
        fs.levels.assign(rects.size(), level);
        fs.weights.reserve(rects.size());
        for (const CandOut& c : per_frame[(size_t)f]) fs.weights.push_back(c.sum);
        group_rectangles(rects, min_neighbors, 0.2, &fs.levels, &fs.weights);
      } else
        group_rectangles(rects, min_neighbors, 0.2);  // GROUP_EPS
    }
  };
  const int nthr = std::max(1, std::min({nf, (int)std::thread::hardware_concurrency(), 16}));
  if (nthr <= 1 || cands.size() < 2048)
    work(0, nf);
  else {
    std::vector<std::thread> th;
    for (int t = 0; t < nthr; t++) th.emplace_back(work, (int)((long long)nf * t / nthr), (int)((long long)nf * (t + 1) / nthr));
    for (auto& t : th) t.join();
  }
}

// The frames' rectangles one after the other into out (below cap) and their offsets into offsets; returns how many there are.
static long long flatten_grouped(const std::vector<std::vector<cc_rect>>& grouped, cc_rect* out, int cap, int32_t* offsets) {
  long long total = 0;
  for (size_t f = 0; f < grouped.size(); f++) {
    offsets[f] = (int32_t)total;
    for (const cc_rect& r : grouped[f]) {
      if (total < cap) out[total] = r;
      total++;
    }
  }
  offsets[grouped.size()] = (int32_t)total;
  return total;
}

// One host image through run_batch: the candidates of all its passes in OpenCV's single-threaded order.
static cc_status image_candidates(cc_detector* d, const FrameSet& F, const cc_detect_params* p, bool debug, std::vector<CandOut>& cands) {
  auto sink = std::make_shared<BatchSink>();
  sink->consume = [&cands](int, int, std::vector<CandOut>& c) { cands.insert(cands.end(), c.begin(), c.end()); };
  BatchOptions opt;
  opt.debug = debug;
  const cc_status st = run_batch(d, F, p, sink, opt);
  if (st == CC_OK) sort_candidates(cands);
  return st;
}

// Switches the detector over to the compiled modules (spec_load is the device half). Owning thread only.
static cc_status spec_install(cc_detector* d, const std::vector<SpecCode>& codes, int k, int tmode) {
  retire_foreign(d);  // a pass still unfetched was launched with the old kernel (and its tile lists): fetch it before the switch
  CC_HIP(hipStreamSynchronize(d->stream));  // no launch of the old modules is in flight any more
  SpecModule fresh[2];
  int n_fresh = 0;
  if (cc_status st = spec_load(d->m, codes, tmode, d->lds, fresh, &n_fresh); st != CC_OK) return st;  // the old kernel stays
  d->unload_spec();
  for (int i = 0; i < n_fresh; i++) d->spec[i] = fresh[i];
  d->n_spec = n_fresh;
  d->spec_stages = k;
  return CC_OK;
}

static cc_status device_arch(int device, std::string& arch) {
  hipDeviceProp_t prop;
  CC_HIP(hipGetDeviceProperties(&prop, device));
  arch = prop.gcnArchName;
  arch = arch.substr(0, arch.find(':'));
  return CC_OK;
}

// Picks up a finished background build (called at the start of every detection call).
static void spec_poll(cc_detector* d) {
  const int st = d->spec_bg_state.load(std::memory_order_acquire);
  if (st != 2 && st != 3) return;
  if (d->spec_thread.joinable()) d->spec_thread.join();
  if (st == 2 && spec_install(d, d->spec_bg_code, d->spec_bg_stages, d->spec_bg_tmode) != CC_OK) d->spec_bg_error = cc_last_error();
  d->spec_bg_code.clear();
  d->spec_bg_state.store(0, std::memory_order_release);
}

static cc_status spec_start_background(cc_detector* d, int n_stages) {
  if (d->m.max_nodes_per_tree > 1) return set_error(CC_ERR_UNSUPPORTED, "cc_detector_specialize: stump cascades only");
  if (d->spec_bg_state.load(std::memory_order_acquire) == 1) return CC_OK;  // a build is already running
  spec_poll(d);
  std::string arch;
  cc_status st = device_arch(d->device, arch);
  if (st != CC_OK) return st;
  d->spec_bg_error.clear();
  d->spec_bg_state.store(1, std::memory_order_release);
  d->spec_thread = std::thread([d, n_stages, arch]() {
    std::vector<SpecCode> code;
    int k = 0;
    int tmode = 0;
    const cc_status s2 = spec_build(d->m, n_stages, arch, code, k, tmode);
    if (s2 == CC_OK) {
      d->spec_bg_code.swap(code);
      d->spec_bg_stages = k;
      d->spec_bg_tmode = tmode;
      d->spec_bg_state.store(2, std::memory_order_release);
    } else {
      d->spec_bg_error = cc_last_error();  // this thread's message
      d->spec_bg_state.store(3, std::memory_order_release);
    }
  });
  return CC_OK;
}

}  // namespace ccamd

// Parity instrumentation of inv_sqrt_as_float (cc_eval_kernel.inc): counts values nf for which it differs from
// (float)(1.0 / sqrt(nf)). nf is drawn as the kernels form it -- area * valsqsum - valsum^2 for a random window size, pixel
// sum and squared sum (an integer-valued double) -- and, every fourth draw, as an arbitrary integer below 2^52.
namespace ccamd {
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
}  // namespace ccamd

extern "C" {

int cc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// Serial numbers of the detectors alive in this process. op 0: new serial (registered); 1: unregister `serial`;
// 2: is `serial` alive (returns 1 / 0).
static unsigned long long detector_registry(int op, unsigned long long serial) {
  static std::mutex mu;
  static std::unordered_set<unsigned long long> live;
  static unsigned long long next = 0;
  std::lock_guard<std::mutex> lk(mu);
  if (op == 0) {
    live.insert(++next);
    return next;
  }
  if (op == 1) {
    live.erase(serial);
    return 0;
  }
  return live.count(serial) ? 1 : 0;
}

// The cascade's tree / stump records in the layouts the kernels read (one table per tile layout), built and uploaded on the
// detector's stream. Every branch ends synchronised: its host vectors go out of scope.
static cc_status upload_cascade_tables(cc_detector* d) {
  const bool haar = d->m.feature_type == CC_FEATURE_HAAR;
  const bool trees = d->m.max_nodes_per_tree > 1;
  if (trees) {
    std::vector<int> root(d->m.tree_first_node.begin(), d->m.tree_first_node.end()), leaf0(d->m.tree_first_leaf.begin(), d->m.tree_first_leaf.end());
    CC_HIP(d->d_tree_root.upload(root, d->stream));
    CC_HIP(d->d_tree_leaf0.upload(leaf0, d->stream));
    CC_HIP(d->d_leaves.upload(d->m.leaves, d->stream));
    if (haar) {
      std::vector<HaarNodeDev> n1, n2;
      build_haar_nodes<1>(d->m, n1);
      build_haar_nodes<2>(d->m, n2);
      CC_HIP(d->d_hnode1.upload(n1, d->stream));
      CC_HIP(d->d_hnode2.upload(n2, d->stream));
      CC_HIP(hipStreamSynchronize(d->stream));
    } else {
      std::vector<LbpNodeDev> n1, n2;
      build_lbp_nodes<1>(d->m, n1);
      build_lbp_nodes<2>(d->m, n2);
      CC_HIP(d->d_lnode1.upload(n1, d->stream));
      CC_HIP(d->d_lnode2.upload(n2, d->stream));
      CC_HIP(hipStreamSynchronize(d->stream));
    }
  } else if (haar) {
    std::vector<HaarStumpDev> s1, s2;
    build_haar_stumps<1>(d->m, s1);
    build_haar_stumps<2>(d->m, s2);
    CC_HIP(d->d_haar1.upload(s1, d->stream));
    CC_HIP(d->d_haar2.upload(s2, d->stream));
    std::vector<HaarStumpDev> sg;
    if (!d->m.has_tilted) build_haar_gstumps(d->m, sg);
    CC_HIP(d->d_haar_g.upload(sg, d->stream));
    CC_HIP(hipStreamSynchronize(d->stream));
    if (d->wave_below > 0) {
      const std::vector<HaarStumpDev> w1 = schedule_for_wave_phase(d->m, s1), w2 = schedule_for_wave_phase(d->m, s2);
      CC_HIP(d->d_haar1w.upload(w1, d->stream));
      CC_HIP(d->d_haar2w.upload(w2, d->stream));
      CC_HIP(hipStreamSynchronize(d->stream));
    }
  } else {
    std::vector<LbpStumpDev> s1, s2;
    build_lbp_stumps<1>(d->m, s1);
    build_lbp_stumps<2>(d->m, s2);
    CC_HIP(d->d_lbp1.upload(s1, d->stream));
    CC_HIP(d->d_lbp2.upload(s2, d->stream));
    std::vector<LbpStumpDev> sg, s16;
    build_lbp_gstumps(d->m, sg);
    CC_HIP(d->d_lbp_g.upload(sg, d->stream));
    d->lbp16_all = 1;
    for (size_t i = 0; i < d->m.stump_feature.size(); i++) {
      const int32_t* r = &d->m.lbp_rects[(size_t)d->m.stump_feature[i] * 4];
      if (!fits16((long long)r[2] * r[3])) d->lbp16_all = 0;
    }
    if (d->lbp16_all) {
      build_lbp_stumps16(d->m, s16);
      CC_HIP(d->d_lbp16.upload(s16, d->stream));
    }
    CC_HIP(hipStreamSynchronize(d->stream));
  }
  return CC_OK;
}

cc_status cc_detector_create(const cc_cascade* c, int device, int max_batch, cc_detector** out) {
  if (!c || !out) return set_error(CC_ERR_INVALID_ARG, "cc_detector_create: null argument");
  *out = nullptr;
  if (max_batch < 1 || max_batch > 4096) return set_error(CC_ERR_INVALID_ARG, "cc_detector_create: max_batch %d out of range", max_batch);
  if (cc_status hs = refuse_hog(c->m, "cc_detector_create"); hs != CC_OK) return hs;

  cc_status st = ensure_device(device);
  if (st != CC_OK) return st;
  std::unique_ptr<cc_detector> d(new cc_detector());
  d->m = c->m;
  d->serial = detector_registry(0, 0);
  d->device = device;
  d->max_batch = max_batch;
  CC_HIP(hipStreamCreateWithFlags(&d->own_stream, hipStreamNonBlocking));
  d->stream = d->own_stream;
  const TileGeom<1> G1(d->m.win_w, d->m.win_h);
  const TileGeom<2> G2(d->m.win_w, d->m.win_h);
  d->lds = eval_lds_bytes(std::max(G1.words(), G2.words()), d->m.has_tilted, d->m.feature_type == CC_FEATURE_HAAR);
  if ((int)d->m.stage_ntrees.size() >= MAX_STAGES)
    return set_error(CC_ERR_UNSUPPORTED, "cc_detector_create: cascades with %zu stages are not supported (limit %d)",
                     d->m.stage_ntrees.size(), MAX_STAGES - 1);
  if (d->lds > 160 * 1024 - 256)
    return set_error(CC_ERR_UNSUPPORTED, "cc_detector_create: %dx%d window needs %zu bytes of LDS per tile (limit 160 KiB)",
                     d->m.win_w, d->m.win_h, d->lds);
  const bool haar = d->m.feature_type == CC_FEATURE_HAAR;
  if (d->lds > 64 * 1024) {
    if (haar)
      CC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_eval_haar), hipFuncAttributeMaxDynamicSharedMemorySize, (int)d->lds));
    else
      CC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_eval_lbp), hipFuncAttributeMaxDynamicSharedMemorySize, (int)d->lds));
  }
  std::vector<int> ntrees(d->m.stage_ntrees.begin(), d->m.stage_ntrees.end());
  std::vector<int> sfirst(d->m.stage_first.begin(), d->m.stage_first.end());
  CC_HIP(d->d_stage_ntrees.upload(ntrees, d->stream));
  CC_HIP(d->d_stage_first.upload(sfirst, d->stream));
  // One wavefront per window (parallel reduction of a stage's votes) is only bit-identical to the sequential CPU sum
  // when every partial sum is exact in double; LBP stages are too short for it to pay.
  const bool trees = d->m.max_nodes_per_tree > 1;  // general trees: thread-per-window phases only, sequential sums
  const bool exact = !trees && stage_sums_order_independent(d->m);
  d->wave_below = (haar && exact) ? 24 : 0;
  if (!haar && !trees) {
    // LBP wave phase (lanes = the stumps of several whole stages; sums in stump order, so no exactness condition): needs
    // every stage to fit a wavefront. Threshold measured on the stock cascade (tools/sweeps/r3_l.txt).
    bool fits = true;
    for (int v : d->m.stage_ntrees) fits = fits && v <= 64;
    d->wave_below = fits ? 24 : 0;  // 8 ... 32 within 3 % of each other, 48 +5 %, 64 +11 %, off +23 %
  }
  d->split_stumps = exact ? 1 : 0;
  if (const char* e = std::getenv("CCAMD_SPLIT_STUMPS")) d->split_stumps = d->split_stumps && std::atoi(e) != 0;
  if (const char* e = std::getenv("CCAMD_DEBUG_STOP_AFTER_STAGE")) d->stop_after = std::atoi(e);  // timing experiments
  d->early_skip = std::getenv("CCAMD_NO_EARLY_SKIP") ? 0 : 1;
  if (const char* e = std::getenv("CCAMD_PIPELINE_PASSES")) {
    d->pipeline_passes = std::max(1, std::atoi(e));
    d->pipeline_passes_set = 1;
  }
  if (const char* e = std::getenv("CCAMD_CAND_CAP")) d->cand_cap = std::max(16, std::atoi(e));  // initial candidate-list capacity (tests: forces the overflow path)
  if (const char* e = std::getenv("CCAMD_WAVE_BELOW"))  // tuning knob; only honoured where the wave phase is valid at all
    if (d->wave_below) d->wave_below = std::max(0, std::min(64, std::atoi(e)));  // the wave phase holds one window per lane
  CC_HIP(d->d_stage_thr.upload(d->m.stage_threshold, d->stream));
  {
    // Stage groups and queue form (stage_groups, where the numbers behind the defaults are): LBP stump cascades group their
    // short stages from stage 2 on, up to 14 stumps, and switch to the list queue there; everything else keeps one stage per
    // group and the bank-class table.
    const bool lbp = !haar && !trees;
    int budget = lbp ? 14 : 0;
    const int from = lbp ? 2 : 1;
    if (const char* e = std::getenv("CCAMD_GROUP_STUMPS")) budget = trees ? 0 : std::max(0, std::atoi(e));  // tuning
    int dense_stage = lbp ? 2 : -1;
    if (const char* e = std::getenv("CCAMD_DENSE_FROM")) dense_stage = std::atoi(e);
    std::vector<int> gf;
    stage_groups(d->m.stage_ntrees, from, budget, dense_stage, gf, d->dense_from);
    d->n_groups = (int)gf.size() - 1;
    CC_HIP(d->d_group_first.upload(gf, d->stream));
    CC_HIP(hipStreamSynchronize(d->stream));
  }
  if (cc_status ts = upload_cascade_tables(d.get()); ts != CC_OK) return ts;
  // CCAMD_AUTO_SPECIALIZE=<stages>: build the specialised kernel in the background; detection starts on the table-driven
  // kernel and switches over when the module is ready (no change to the calling code)
  if (const char* e = std::getenv("CCAMD_AUTO_SPECIALIZE")) {
    const int k = std::atoi(e);
    if (k > 0 && d->m.max_nodes_per_tree == 1) (void)spec_start_background(d.get(), k);
  }
  *out = d.release();
  return CC_OK;
}

void cc_detector_destroy(cc_detector* d) {
  if (!d) return;
  detector_registry(1, d->serial);
  (void)hipSetDevice(d->device);
  if (d->pending.active) {  // a submitted batch nobody collected: let the device finish, drop the results
    (void)hipStreamSynchronize(d->stream);
    d->pending.drop();
  }
  delete d;
}

cc_status cc_detector_set_stream(cc_detector* d, void* hip_stream) {
  if (!d) return set_error(CC_ERR_INVALID_ARG, "cc_detector_set_stream: null detector");
  d->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : d->own_stream;
  return CC_OK;
}

cc_status cc_detector_specialize(cc_detector* d, int n_stages) {
  if (!d) return set_error(CC_ERR_INVALID_ARG, "cc_detector_specialize: null detector");
  if (cc_status hs = refuse_hog(d->m, "cc_detector_specialize"); hs != CC_OK) return hs;
  cc_status st = ensure_device(d->device);
  if (st != CC_OK) return st;
  if (d->spec_thread.joinable()) d->spec_thread.join();  // a background build, if any, is superseded
  d->spec_bg_state.store(0, std::memory_order_release);
  d->spec_bg_code.clear();
  if (n_stages <= 0) {  // back to the table-driven kernel
    CC_HIP(hipStreamSynchronize(d->stream));
    d->unload_spec();
    return CC_OK;
  }
  std::string arch;
  st = device_arch(d->device, arch);
  if (st != CC_OK) return st;
  std::vector<SpecCode> code;
  int k = 0;
  int tmode = 0;
  st = spec_build(d->m, n_stages, arch, code, k, tmode);
  if (st != CC_OK) return st;
  return spec_install(d, code, k, tmode);
}

cc_status cc_detector_specialize_async(cc_detector* d, int n_stages) {
  if (!d) return set_error(CC_ERR_INVALID_ARG, "cc_detector_specialize_async: null detector");
  if (n_stages <= 0) return set_error(CC_ERR_INVALID_ARG, "cc_detector_specialize_async: n_stages must be positive");
  if (cc_status hs = refuse_hog(d->m, "cc_detector_specialize_async"); hs != CC_OK) return hs;
  cc_status st = ensure_device(d->device);
  if (st != CC_OK) return st;
  return spec_start_background(d, n_stages);
}

int cc_detector_specialized_stages(const cc_detector* d) { return d ? d->spec_stages : 0; }

int cc_detector_graph_active(const cc_detector* d) {
  if (!d) return (int)set_error(CC_ERR_INVALID_ARG, "cc_detector_graph_active: null detector");
  return d->last_call_graph;
}

int64_t cc_detector_graph_captures(const cc_detector* d) {
  if (!d) return (int64_t)set_error(CC_ERR_INVALID_ARG, "cc_detector_graph_captures: null detector");
  return d->graph_captures;
}

cc_status cc_detector_set_profiling(cc_detector* d, int enabled) {
  if (!d) return set_error(CC_ERR_INVALID_ARG, "cc_detector_set_profiling: null detector");
  d->profiling = enabled != 0;
  return CC_OK;
}

int cc_detector_candidate_capacity(const cc_detector* d) { return d ? d->cand_cap : -1; }

cc_status cc_detector_get_timings(cc_detector* d, cc_detector_timings* t, int reset) {
  if (!d || !t) return set_error(CC_ERR_INVALID_ARG, "cc_detector_get_timings: null argument");
  if (!d->events.empty()) {  // event pairs of submitted batches: their kernels may still be running
    cc_status st = ensure_device(d->device);
    if (st != CC_OK) return st;
    CC_HIP(hipStreamSynchronize(d->stream));
    if (d->front_stream) CC_HIP(hipStreamSynchronize(d->front_stream));
    collect_events(d);
  }
  *t = d->tm;
  if (reset) std::memset(&d->tm, 0, sizeof(d->tm));
  return CC_OK;
}

cc_status cc_detect_batch_device_only(cc_detector* d, const uint8_t* frames, int on_device, int n_frames, int width, int height,
                                      size_t row_stride, size_t frame_stride, const cc_detect_params* p) {
  const FrameSet F{frames, on_device, n_frames, width, height, row_stride, frame_stride, CC_PIX_GRAY8};
  cc_status st = check_frame_args(d, F, p, "cc_detect_batch_device_only");
  if (st != CC_OK) return st;
  BatchOptions opt;
  opt.want_results = false;
  return run_batch(d, F, p, std::make_shared<BatchSink>(), opt);
}

cc_status cc_detect_batch(cc_detector* d, const uint8_t* frames, int on_device, int n_frames, int width, int height,
                          size_t row_stride, size_t frame_stride, const cc_detect_params* p, cc_rect* out, int cap,
                          int32_t* offsets) {
  return cc_detect_batch_fmt(d, frames, on_device, n_frames, width, height, row_stride, frame_stride, CC_PIX_GRAY8, p, out, cap, offsets);
}

cc_status cc_detect_batch_fmt(cc_detector* d, const uint8_t* frames, int on_device, int n_frames, int width, int height,
                              size_t row_stride, size_t frame_stride, int pixel_format, const cc_detect_params* p, cc_rect* out,
                              int cap, int32_t* offsets) {
  const FrameSet F{frames, on_device, n_frames, width, height, row_stride, frame_stride, pixel_format};
  cc_status st = check_frame_args(d, F, p, "cc_detect_batch");
  if (st != CC_OK) return st;
  if (!offsets || (cap > 0 && !out) || cap < 0) return set_error(CC_ERR_INVALID_ARG, "cc_detect_batch: bad output buffers");
  const auto t_start = std::chrono::steady_clock::now();
  double group_ms = 0;
  size_t n_cands = 0;
  std::vector<std::vector<cc_rect>> grouped((size_t)n_frames);
  const int min_neighbors = p->min_neighbors;
  auto sink = std::make_shared<BatchSink>();
  sink->consume = [&](int f0, int nf, std::vector<CandOut>& cands) {
    const auto t0 = std::chrono::steady_clock::now();
    n_cands += cands.size();
    group_pass(min_neighbors, f0, nf, cands, grouped);
    group_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  };
  st = run_batch(d, F, p, sink);
  if (st != CC_OK) return st;
  const long long total = flatten_grouped(grouped, out, cap, offsets);
  if (std::getenv("CCAMD_TIMING")) {
    const auto t1 = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[ccamd] detect_batch: total %.3f ms, of which sort+group on the host %.3f ms (overlapped), %zu candidates\n",
                 std::chrono::duration<double, std::milli>(t1 - t_start).count(), group_ms, n_cands);
  }
  if (total > cap) return set_error(CC_ERR_BUFFER_TOO_SMALL, "cc_detect_batch: %lld rectangles, capacity %d", total, cap);
  return CC_OK;
}

// cc_detect_batch_fmt with scores: the same passes, and a sink that groups with levels and weights.
cc_status cc_detect_batch_levels_fmt(cc_detector* d, const uint8_t* frames, int on_device, int n_frames, int width, int height,
                                     size_t row_stride, size_t frame_stride, int pixel_format, const cc_detect_params* p, cc_rect* out,
                                     int32_t* reject_levels, double* level_weights, int cap, int32_t* offsets) {
  const FrameSet F{frames, on_device, n_frames, width, height, row_stride, frame_stride, pixel_format};
  cc_status st = check_frame_args(d, F, p, "cc_detect_batch_levels");
  if (st != CC_OK) return st;
  if (!offsets || cap < 0 || (cap > 0 && (!out || !reject_levels || !level_weights)))
    return set_error(CC_ERR_INVALID_ARG, "cc_detect_batch_levels: bad output buffers");
  std::vector<std::vector<cc_rect>> grouped((size_t)n_frames);
  std::vector<FrameScores> scores((size_t)n_frames);
  const int min_neighbors = p->min_neighbors, nstages = (int)d->m.stage_ntrees.size();
  auto sink = std::make_shared<BatchSink>();
  sink->consume = [&](int f0, int nf, std::vector<CandOut>& cands) { group_pass(min_neighbors, f0, nf, cands, grouped, &scores, nstages); };
  st = run_batch(d, F, p, sink);
  if (st != CC_OK) return st;
  const long long total = flatten_grouped(grouped, out, cap, offsets);
  long long at = 0;
  for (const FrameScores& fs : scores)
    for (size_t i = 0; i < fs.levels.size(); i++, at++)
      if (at < cap) {
        reject_levels[at] = fs.levels[i];
        level_weights[at] = fs.weights[i];
      }
  if (total > cap) return set_error(CC_ERR_BUFFER_TOO_SMALL, "cc_detect_batch_levels: %lld rectangles, capacity %d", total, cap);
  return CC_OK;
}

// The device-output batch: the passes of cc_detect_batch through the same loop (run_batch), each followed on the detector's
// stream by the ordering and grouping kernels, which append to the caller's buffers (enqueue_group). The host reads back the
// batch's total at the end and nothing else of the results.
// `scored`: cc_detect_batch_to_device_levels, whose passes run the scored kernels and write d_levels / d_weights as well.
static cc_status detect_batch_to_device(cc_detector* d, const FrameSet& F, const cc_detect_params* p, cc_rect* d_out, bool scored,
                                        int32_t* d_levels, double* d_weights, int cap, int32_t* d_offsets, int* n_total) {
  cc_status st = check_frame_args(d, F, p, "cc_detect_batch_to_device");
  if (st != CC_OK) return st;
  if (!d_offsets || !n_total || (cap > 0 && !d_out) || cap < 0 || (scored && (!d_levels || !d_weights)))
    return set_error(CC_ERR_INVALID_ARG, "cc_detect_batch_to_device: bad output buffers");
  BatchOptions opt;
  opt.dev = DeviceOutput{d_out, cap, d_offsets, p->min_neighbors};
  if (scored) {
    opt.dev.d_levels = d_levels;
    opt.dev.d_weights = d_weights;
    opt.dev.level = (int)d->m.stage_ntrees.size();
  }
  st = run_batch(d, F, p, std::make_shared<BatchSink>(), opt);
  if (st != CC_OK) return st;
  int total = 0;
  CC_HIP(copy_sync(&total, d->d_group_state.p, sizeof(int), hipMemcpyDeviceToHost, d->stream));
  *n_total = total;
  if (total > cap) return set_error(CC_ERR_BUFFER_TOO_SMALL, "cc_detect_batch_to_device: %d rectangles, capacity %d", total, cap);
  return CC_OK;
}

cc_status cc_detect_batch_to_device(cc_detector* d, const uint8_t* frames, int on_device, int n_frames, int width, int height,
                                    size_t row_stride, size_t frame_stride, int pixel_format, const cc_detect_params* p,
                                    cc_rect* d_out, int cap, int32_t* d_offsets, int* n_total) {
  const FrameSet F{frames, on_device, n_frames, width, height, row_stride, frame_stride, pixel_format};
  return detect_batch_to_device(d, F, p, d_out, false, nullptr, nullptr, cap, d_offsets, n_total);
}

cc_status cc_detect_batch_to_device_levels(cc_detector* d, const uint8_t* frames, int on_device, int n_frames, int width, int height,
                                           size_t row_stride, size_t frame_stride, int pixel_format, const cc_detect_params* p,
                                           cc_rect* d_out, int32_t* d_levels, double* d_weights, int cap, int32_t* d_offsets,
                                           int* n_total) {
  const FrameSet F{frames, on_device, n_frames, width, height, row_stride, frame_stride, pixel_format};
  return detect_batch_to_device(d, F, p, d_out, true, d_levels, d_weights, cap, d_offsets, n_total);
}

struct cc_batch_ticket {
  cc_detector* owner = nullptr;
  unsigned long long owner_serial = 0;  // cc_detector::serial of the owner: an address can be reused by a later detector
  std::shared_ptr<BatchSink> sink;
  // Shared with the sink's consume function, NOT owned by the ticket alone: the detector may still hold the sink of a pass
  // it has not fetched when the ticket ends on an error path, and that pass's helper then writes here (round-3 advisor
  // finding: the function used to capture the ticket's address).
  std::shared_ptr<std::vector<std::vector<cc_rect>>> grouped;
  ~cc_batch_ticket() {
    if (sink) {
      try {
        sink->wait_jobs();
      } catch (...) {
      }
    }
  }
};

// The helper threads of a submitted batch run std::sort / std::vector code: what they throw (bad_alloc) surfaces in
// future::get and must not cross the C ABI.
static cc_status wait_sink_jobs(BatchSink& sink, const char* who) {
  try {
    sink.wait_jobs();
  } catch (const std::exception& e) {
    sink.jobs.clear();
    return set_error(CC_ERR_HIP, "%s: grouping a pass failed on the host: %s", who, e.what());
  } catch (...) {
    sink.jobs.clear();
    return set_error(CC_ERR_HIP, "%s: grouping a pass failed on the host", who);
  }
  return CC_OK;
}

cc_status cc_detect_batch_submit(cc_detector* d, const uint8_t* frames, int on_device, int n_frames, int width, int height,
                                 size_t row_stride, size_t frame_stride, const cc_detect_params* p, cc_batch_ticket** ticket) {
  return cc_detect_batch_submit_fmt(d, frames, on_device, n_frames, width, height, row_stride, frame_stride, CC_PIX_GRAY8, p, ticket);
}

cc_status cc_detect_batch_submit_fmt(cc_detector* d, const uint8_t* frames, int on_device, int n_frames, int width, int height,
                                     size_t row_stride, size_t frame_stride, int pixel_format, const cc_detect_params* p,
                                     cc_batch_ticket** ticket) {
  if (!ticket) return set_error(CC_ERR_INVALID_ARG, "cc_detect_batch_submit: null ticket pointer");
  *ticket = nullptr;
  const FrameSet F{frames, on_device, n_frames, width, height, row_stride, frame_stride, pixel_format};
  cc_status st = check_frame_args(d, F, p, "cc_detect_batch_submit");
  if (st != CC_OK) return st;
  std::unique_ptr<cc_batch_ticket> t(new cc_batch_ticket);
  t->owner = d;
  t->owner_serial = d->serial;
  t->grouped = std::make_shared<std::vector<std::vector<cc_rect>>>((size_t)n_frames);
  t->sink = std::make_shared<BatchSink>();
  std::shared_ptr<std::vector<std::vector<cc_rect>>> grouped = t->grouped;
  const int min_neighbors = p->min_neighbors;
  t->sink->consume = [grouped, min_neighbors](int f0, int nf, std::vector<CandOut>& cands) { group_pass(min_neighbors, f0, nf, cands, *grouped); };
  t->sink->async_consume = true;  // passes of a batch cover disjoint frames: their helpers never touch the same entry of `grouped`
  BatchOptions opt;
  opt.defer_last = true;
  st = run_batch(d, F, p, t->sink, opt);
  if (st != CC_OK) return st;
  *ticket = t.release();
  return CC_OK;
}

// A ticket is only ever ended by the detector it came from: with any other detector (or one that was destroyed and whose
// address a new detector took over -- `serial` tells them apart) the call fails and the ticket stays valid.
static bool ticket_is_of(const cc_detector* d, const cc_batch_ticket* t) { return d && t->owner == d && t->owner_serial == d->serial; }

cc_status cc_detect_batch_collect(cc_detector* d, cc_batch_ticket* t, cc_rect* out, int cap, int32_t* offsets) {
  if (!t) return set_error(CC_ERR_INVALID_ARG, "cc_detect_batch_collect: null ticket");
  if (!ticket_is_of(d, t)) return set_error(CC_ERR_INVALID_ARG, "cc_detect_batch_collect: the ticket belongs to another detector (it stays valid)");
  std::unique_ptr<cc_batch_ticket> own(t);  // from here on the ticket ends with this call (except CC_ERR_BUFFER_TOO_SMALL)
  if (!offsets || (cap > 0 && !out) || cap < 0) {
    if (d->pending.active && d->pending.sink == t->sink) (void)retire_pending(d);
    return set_error(CC_ERR_INVALID_ARG, "cc_detect_batch_collect: bad output buffers");
  }
  cc_status st = ensure_device(d->device);
  if (st != CC_OK) {
    (void)own.release();  // nothing was fetched: the caller may collect or discard again
    return st;
  }
  if (d->pending.active && d->pending.sink == t->sink) {  // its last pass has not been fetched by a later submit
    st = retire_pending(d);
    if (st != CC_OK) return st;
  }
  if (t->sink->status != CC_OK) return set_error(t->sink->status, "cc_detect_batch_collect: %s", t->sink->error.c_str());
  st = wait_sink_jobs(*t->sink, "cc_detect_batch_collect");  // the helper threads that sort + group what the passes delivered
  if (st != CC_OK) return st;
  const long long total = flatten_grouped(*t->grouped, out, cap, offsets);
  if (total > cap) {
    (void)own.release();  // the results stay in the ticket: collect again with room for offsets[n_frames] rectangles
    return set_error(CC_ERR_BUFFER_TOO_SMALL, "cc_detect_batch_collect: %lld rectangles, capacity %d", total, cap);
  }
  return CC_OK;
}

cc_status cc_detect_batch_discard(cc_detector* d, cc_batch_ticket* t) {
  if (!t) return CC_OK;
  if (!detector_registry(2, t->owner_serial)) {  // the owner was destroyed (it waited for the device and dropped the pass)
    delete t;
    return CC_OK;
  }
  if (!ticket_is_of(d, t)) return set_error(CC_ERR_INVALID_ARG, "cc_detect_batch_discard: the ticket belongs to another detector (it stays valid)");
  std::unique_ptr<cc_batch_ticket> own(t);
  if (d->pending.active && d->pending.sink == t->sink) {  // let its last pass finish and drop what it delivers
    cc_status st = ensure_device(d->device);
    if (st != CC_OK) {  // the pass cannot be fetched: cut it loose (its helper, if any, keeps `grouped` alive by itself)
      d->pending.drop();
      return st;
    }
    (void)retire_pending(d);
  }
  (void)wait_sink_jobs(*t->sink, "cc_detect_batch_discard");
  return CC_OK;
}

cc_status cc_detect_multiscale(cc_detector* d, const uint8_t* gray, int width, int height, size_t row_stride,
                               const cc_detect_params* p, cc_rect* out, int cap, int* n) {
  return cc_detect_multiscale_fmt(d, gray, width, height, row_stride, CC_PIX_GRAY8, p, out, cap, n);
}

cc_status cc_detect_multiscale_fmt(cc_detector* d, const uint8_t* img, int width, int height, size_t row_stride, int pixel_format,
                                   const cc_detect_params* p, cc_rect* out, int cap, int* n) {
  if (!n) return set_error(CC_ERR_INVALID_ARG, "cc_detect_multiscale: null count pointer");
  int32_t offsets[2] = {0, 0};
  cc_status st = cc_detect_batch_fmt(d, img, 0, 1, width, height, row_stride, row_stride * (size_t)pix_rows(pixel_format, height),
                                     pixel_format, p, out, cap, offsets);
  if (st == CC_OK || st == CC_ERR_BUFFER_TOO_SMALL) *n = offsets[1];
  return st;
}

cc_status cc_detect_multiscale_levels(cc_detector* d, const uint8_t* gray, int width, int height, size_t row_stride,
                                      const cc_detect_params* p, cc_rect* out, int32_t* reject_levels, double* level_weights,
                                      int cap, int* n) {
  return cc_detect_multiscale_levels_fmt(d, gray, width, height, row_stride, CC_PIX_GRAY8, p, out, reject_levels, level_weights, cap, n);
}

cc_status cc_detect_multiscale_levels_fmt(cc_detector* d, const uint8_t* img, int width, int height, size_t row_stride,
                                          int pixel_format, const cc_detect_params* p, cc_rect* out, int32_t* reject_levels,
                                          double* level_weights, int cap, int* n) {
  const FrameSet F = host_image(img, width, height, row_stride, pixel_format);
  cc_status st = check_frame_args(d, F, p, "cc_detect_multiscale_levels");
  if (st != CC_OK) return st;
  if (!n || cap < 0 || (cap > 0 && (!out || !reject_levels || !level_weights)))
    return set_error(CC_ERR_INVALID_ARG, "cc_detect_multiscale_levels: bad output buffers");
  std::vector<CandOut> cands;
  st = image_candidates(d, F, p, false, cands);
  if (st != CC_OK) return st;
  std::vector<cc_rect> rects;
  std::vector<int> levels;
  std::vector<double> weights;
  const int nstages = (int)d->m.stage_ntrees.size();
  for (const CandOut& c : cands) {  // only windows that passed every stage are reported: level = number of stages
    rects.push_back(cc_rect{c.x, c.y, c.w, c.h});
    levels.push_back(nstages);
    weights.push_back(c.sum);
  }
  group_rectangles(rects, p->min_neighbors, 0.2, &levels, &weights);
  *n = (int)rects.size();
  for (int i = 0; i < (int)rects.size() && i < cap; i++) {
    out[i] = rects[(size_t)i];
    reject_levels[i] = levels[(size_t)i];
    level_weights[i] = weights[(size_t)i];
  }
  if ((int)rects.size() > cap) return set_error(CC_ERR_BUFFER_TOO_SMALL, "cc_detect_multiscale_levels: %zu rectangles, capacity %d", rects.size(), cap);
  return CC_OK;
}

cc_status cc_detect_raw(cc_detector* d, const uint8_t* gray, int width, int height, size_t row_stride, const cc_detect_params* p,
                        int32_t* cand, int cap, int* n) {
  const FrameSet F = host_image(gray, width, height, row_stride);
  cc_status st = check_frame_args(d, F, p, "cc_detect_raw");
  if (st != CC_OK) return st;
  if (!n || (cap > 0 && !cand)) return set_error(CC_ERR_INVALID_ARG, "cc_detect_raw: bad output buffers");
  std::vector<CandOut> cands;
  st = image_candidates(d, F, p, false, cands);
  if (st != CC_OK) return st;
  *n = (int)cands.size();
  for (int i = 0; i < (int)cands.size() && i < cap; i++) {
    const CandOut& c = cands[i];
    const int32_t v[7] = {c.scale, c.gx, c.gy, c.x, c.y, c.w, c.h};
    std::memcpy(cand + 7 * (size_t)i, v, sizeof(v));
  }
  if ((int)cands.size() > cap) return set_error(CC_ERR_BUFFER_TOO_SMALL, "cc_detect_raw: %zu candidates, capacity %d", cands.size(), cap);
  return CC_OK;
}

cc_status cc_detect_debug_windows(cc_detector* d, const uint8_t* gray, int width, int height, size_t row_stride,
                                  const cc_detect_params* p, int32_t* codes, double* sums, uint8_t* visited, int64_t cap,
                                  int64_t* n_windows) {
  const FrameSet F = host_image(gray, width, height, row_stride);
  cc_status st = check_frame_args(d, F, p, "cc_detect_debug_windows");
  if (st != CC_OK) return st;
  if (!n_windows) return set_error(CC_ERR_INVALID_ARG, "cc_detect_debug_windows: null count pointer");
  std::vector<CandOut> cands;  // not reported: the windows' codes and sums are
  st = image_candidates(d, F, p, true, cands);
  if (st != CC_OK) return st;
  Plan* P = nullptr;
  st = build_plan(d, width, height, *p, &P);
  if (st != CC_OK) return st;
  *n_windows = P->windows;
  if (P->windows > cap) return set_error(CC_ERR_BUFFER_TOO_SMALL, "cc_detect_debug_windows: %lld windows, capacity %lld", P->windows, (long long)cap);
  const size_t nw = (size_t)P->windows;
  if (nw) {
    // through the detector's stream, not the legacy one: see plan_tiles
    if (codes) CC_HIP(hipMemcpyAsync(codes, d->d_dbg_codes.p, nw * sizeof(int32_t), hipMemcpyDeviceToHost, d->stream));
    if (sums) CC_HIP(hipMemcpyAsync(sums, d->d_dbg_sums.p, nw * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    if (visited) CC_HIP(hipMemcpyAsync(visited, d->d_dbg_visited.p, nw, hipMemcpyDeviceToHost, d->stream));
    CC_HIP(hipStreamSynchronize(d->stream));
  }
  return CC_OK;
}

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
