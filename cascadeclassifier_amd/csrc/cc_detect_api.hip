// The detector's entry points (the cc_detector_* and cc_detect_* functions of include/cascadeclassifier_amd.h) with what only
// they need: ordering and grouping a pass's candidates on the host, installing run-time specialised kernels (cc_spec.hip builds
// them), the registry of live detectors and the tickets of submitted batches. The passes themselves are run by cc_pass.hip.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <mutex>
#include <unordered_set>

#include "cc_detector.h"

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
  for (int i = 0; i < n_fresh; i++) {
    d->spec[i] = fresh[i];
    d->spec[i].wave_below = spec_wave_below(d->wave_below, fresh[i].only_step, fresh[i].tile_y);
  }
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

void spec_poll(cc_detector* d) {
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

using namespace ccamd;

// Serial numbers of the detectors alive in this process (tickets name their owner by one): a set behind a mutex.
static std::mutex live_mu;
static std::unordered_set<unsigned long long> live_serials;
static unsigned long long register_detector() {
  static unsigned long long next = 0;
  std::lock_guard<std::mutex> lk(live_mu);
  live_serials.insert(++next);
  return next;
}
static void unregister_detector(unsigned long long serial) {
  std::lock_guard<std::mutex> lk(live_mu);
  live_serials.erase(serial);
}
static bool detector_is_alive(unsigned long long serial) {
  std::lock_guard<std::mutex> lk(live_mu);
  return live_serials.count(serial) != 0;
}

extern "C" {

int cc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
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
  d->serial = register_detector();
  d->device = device;
  d->max_batch = max_batch;
  CC_HIP(d->own_stream.create());
  d->stream = d->own_stream.s;
  if ((int)d->m.stage_ntrees.size() >= MAX_STAGES)
    return set_error(CC_ERR_UNSUPPORTED, "cc_detector_create: cascades with %zu stages are not supported (limit %d)",
                     d->m.stage_ntrees.size(), MAX_STAGES - 1);
  configure_detector(d.get());
  if (d->lds > 160 * 1024 - 256)
    return set_error(CC_ERR_UNSUPPORTED, "cc_detector_create: %dx%d window needs %zu bytes of LDS per tile (limit 160 KiB)",
                     d->m.win_w, d->m.win_h, d->lds);
  if (st = allow_large_lds(d.get()); st != CC_OK) return st;
  if (st = upload_cascade_tables(d.get()); st != CC_OK) return st;
  if (d->auto_specialize > 0 && d->m.max_nodes_per_tree == 1) (void)spec_start_background(d.get(), d->auto_specialize);
  *out = d.release();
  return CC_OK;
}

void cc_detector_destroy(cc_detector* d) {
  if (!d) return;
  unregister_detector(d->serial);
  (void)hipSetDevice(d->device);
  if (d->pending.active) {  // a submitted batch nobody collected: let the device finish, drop the results
    (void)hipStreamSynchronize(d->stream);
    d->pending.drop();
  }
  // nothing of the detector's may still run when its members free their buffers, in whatever order they are declared
  for (hipStream_t s : {d->own_stream.s, d->front_stream.s, d->copy_stream.s})
    if (s) (void)hipStreamSynchronize(s);
  delete d;
}

cc_status cc_detector_set_stream(cc_detector* d, void* hip_stream) {
  if (!d) return set_error(CC_ERR_INVALID_ARG, "cc_detector_set_stream: null detector");
  d->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : d->own_stream.s;
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
    if (d->front_stream.s) CC_HIP(hipStreamSynchronize(d->front_stream.s));
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
  if (!detector_is_alive(t->owner_serial)) {  // the owner was destroyed (it waited for the device and dropped the pass)
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

}  // extern "C"
