// The detector behind cc_detector_*: its plans, its device and pinned buffers, streams and events, and what crosses its four
// translation units -- cc_detect.hip (kernels and their launchers), cc_tables.hip (cascade tables, creation-time settings),
// cc_pass.hip (plans and the pass loop) and cc_detect_api.hip (host grouping, specialisation, entry points).
// HIP only, never included by a .cpp. Every resource frees itself; what must happen in an order is in ~cc_detector().
#pragma once
#include <atomic>
#include <functional>
#include <future>
#include <map>
#include <memory>
#include <thread>

#include "cc_detect_internal.h"

namespace ccamd {

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

struct TimingEvent {  // a recorded pair (EvScope) until collect_events reads it
  OwnEvent a, b;
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
  OwnStream own_stream;
  hipStream_t stream = nullptr;  // own_stream.s, or the caller's (cc_detector_set_stream)
  // cascade tables on the device (one per tile layout)
  DevBuf<int> d_stage_ntrees, d_stage_first;
  std::vector<int> group_first;  // stage groups of the cascade kernel (EvalArgs::group_first), n_groups + 1 entries
  DevBuf<int> d_group_first;
  int n_groups = 0;
  int dense_from = 0x7fffffff;  // first stage group whose queue is a plain list instead of a bank-class table (EvalArgs::dense_from)
  DevBuf<float> d_stage_thr;
  int wave_below = 0;
  int last_call_graph = 0;  // the last single-image call was one hipGraph launch (cc_detector_graph_active)
  int stop_after = -1;
  int split_stumps = 0;
  DevBuf<HaarStumpDev> d_haar1, d_haar2;
  DevBuf<HaarStumpDev> d_haar1w, d_haar2w;  // the same stumps dealt to lanes for the wave phase (bank-aware order)
  // Integer form of the wave phase's stage sums (wave_int_tables; CCAMD_WAVE_INT=0: no stage has one). The leaf words of
  // d_haar1w / d_haar2w hold int32 multiples of the quantum in the stages where wave_int.q is not 0.
  int wave_int_enabled = 1;
  WaveIntTables wave_int;
  DevBuf<double> d_wave_q;
  DevBuf<int> d_wave_thr_q;
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
  OwnStream front_stream;
  OwnEvent front_done[2], eval_done[2], batch_begin;
  bool eval_pending[2] = {false, false};
  int overlap_front = 1;
  // run-time specialised cascade kernel (cc_detector_specialize, spec_load); n_spec 0 = table-driven kernel. spec[0] covers
  // every tile, or the tiles of STEP-2 scales when spec[1] exists: that one covers the tiles of STEP-1 scales.
  SpecModule spec[2];
  int n_spec = 0;
  int last_stamp_tiles = 0;  // CCAMD_DEBUG_STAMPS: tiles of the last pass (all launches)
  int spec_stages = 0;
  int auto_specialize = 0;  // CCAMD_AUTO_SPECIALIZE: stages to specialise in the background from creation on
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
  PinnedBuf h_counts;  // 2 x 2 ints
  int* counts(int slot) const { return static_cast<int*>(h_counts.p) + 2 * slot; }
  PinnedBuf h_frame;        // staging copy of a single host image (graph path)
  PinnedBuf h_color_frame;  // the same for a single colour image (its own buffer: the gray graphs keep theirs)
  // Colour frames from the host land here (stage_host_frames) and k_to_gray writes them into a gray staging slot, both on
  // the front stream: stream order makes one buffer of pass_capacity frames enough. Allocated on the first colour batch.
  DevBuf<uint8_t> d_color;
  // pinned staging area for batches of host frames, kStageSlots slots like d_frames (stage_host_frames): equal slots of
  // h_stage.bytes / kStageSlots bytes, whatever the frames' format
  PinnedBuf h_stage;
  long long graph_captures = 0;  // hipGraph captures made (cc_detector_graph_captures)
  int stage_slot = 0;          // staging slot the next pass of host frames takes (round-robin, also across calls)
  int use_graph = 1;  // single-image calls replay a captured hipGraph; cleared when a capture fails
  int early_skip = 1, pipeline_passes = 4, pipeline_passes_set = 0;  // tuning knobs, read once at creation
  OwnStream copy_stream;
  OwnEvent pass_done[2];
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
  ~cc_detector() {  // only what has an order: the builder thread reads the detector, the modules go once nothing builds them
    if (spec_thread.joinable()) spec_thread.join();
    unload_spec();
  }
};

namespace ccamd {

enum { EV_RESIZE = 0, EV_INTEGRAL = 1, EV_EVAL = 2, EV_FILTER = 3, EV_EVAL_STEP1 = 4, EV_GROUP = 5 };

struct EvScope {  // records a pair of events around a group of launches when profiling is on (cc_pass.hip)
  cc_detector* d;
  int kind;
  OwnEvent a, b;
  hipStream_t st;
  EvScope(cc_detector* d_, int kind_, hipStream_t st_);
  ~EvScope();
};
void collect_events(cc_detector* d);  // adds the recorded pairs' times to d->tm, after their kernels are done

// ---- cc_detect.hip ----
// The cascade-kernel launches of a pass: one ahead-of-time kernel (fn null) over the plan's TILE_Y tiles, or the specialised
// kernel's module(s), each over the list of its own tile height (and of its step's tiles when there is a module per step).
struct EvalLaunch {
  hipFunction_t fn;
  size_t lds;
  int n_tiles;
  const int4* tiles;
  int wave_below = -1;  // >= 0: this launch's EvalArgs::wave_below; -1: the detector's
};
// The cascade-kernel launches of a pass over nf frames in `slot`, one after the other on `st`. stamps: null, or where the
// blocks' phase stamps go (CCAMD_DEBUG_STAMPS), eval_stamp_slots() words per block, launch after launch.
cc_status launch_eval(cc_detector* d, const Plan* P, int slot, int nchan, bool tilt, int sq_compact, bool debug, unsigned long long* stamps,
                      const EvalLaunch* launches, int n_launches, int nf, hipStream_t st);
int eval_stamp_slots();  // STAMP_SLOTS of cc_eval_kernel.inc (a function: nothing is added to the device code)
// The skip-rule filter of the pass in `slot` (k_filter_candidates); for debug passes, the visited flags of frame 0's windows.
void launch_filter_candidates(cc_detector* d, const Plan* P, int slot, hipStream_t st);
void launch_debug_visited(cc_detector* d, const Plan* P, int slot, hipStream_t st);
// The ahead-of-time kernel of the detector's feature type may request d->lds bytes of LDS (above the 64 KiB default).
cc_status allow_large_lds(const cc_detector* d);

// ---- cc_tables.hip ----
// Everything derived from the cascade and the CCAMD_* knobs of creation: LDS per tile, wave phase, split stumps, stage
// groups, pass and candidate-list settings. Every getenv of creation is here. No device calls.
void configure_detector(cc_detector* d);
// The cascade's stage tables and its tree / stump records in the layouts the kernels read (one table per tile layout), built
// and uploaded on the detector's stream. Every branch ends synchronised: its host vectors go out of scope.
cc_status upload_cascade_tables(cc_detector* d);

// ---- cc_pass.hip ----
// The plan for frames of w x h with parameters p: the detector's if it has one, else built, uploaded and kept (the last 8).
cc_status build_plan(cc_detector* d, int w, int h, const cc_detect_params& p, Plan** out);
// Colour formats: row_stride counts bytes (width * bytes per pixel at least) and, with more than one frame, frame_stride must
// hold a whole frame of the format. Gray frames are checked as they always were.
cc_status check_frame_args(const cc_detector* d, const FrameSet& F, const cc_detect_params* p, const char* who);
// Fetches the results of the pending pass and hands them to its sink. On candidate-list overflow the lists grow and the
// pass is redone synchronously. Growing frees the lists of BOTH slots; a pass is judged against the capacity it was
// launched with and against the generation of the lists it wrote into (stale generation => redone as well).
// Device-output passes append at a running total, so unlike host-output passes they must be redone in batch order. One that
// overflowed has written nothing and has set the abort word, so the pass launched behind it has written nothing either;
// that pass is stale by then (an overflow always grows the lists: raw > ps.cap at the current generation means ps.cap ==
// cand_cap), and run_batch retires it, and so redoes it from its frames, still in their staging slot, before it launches the
// next pass. Here the redo clears the abort word first and runs the grouping kernels again behind the pass.
cc_status retire_pending(cc_detector* d);
// Retires a pass that belongs to another batch than the caller's: its failure is that batch's, reported when it is collected.
void retire_foreign(cc_detector* d);
// Runs the batch through the pass loop (run_batch_passes). A batch that failed leaves none of its passes pending: a later call
// must not deliver to (or, for device output, redo a pass into the buffers of) a call that has returned.
cc_status run_batch(cc_detector* d, const FrameSet& F, const cc_detect_params* p, const std::shared_ptr<BatchSink>& sink,
                    const BatchOptions& opt = BatchOptions{});

// ---- cc_detect_api.hip ----
void spec_poll(cc_detector* d);  // picks up a finished background specialisation (called at the start of every detection call)

}  // namespace ccamd
