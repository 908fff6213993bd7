// The detector's pass machinery: scale plans and their tile lists, the device pipeline of one pass, staging of host and colour
// frames, retiring passes, the single-image hipGraph path and the pass loop of a batch (run_batch). The kernels and their
// launchers are in cc_detect.hip, the pyramid and integral images in cc_front.hip, the grouping kernels in cc_group.hip.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <mutex>

#include "cc_detector.h"

namespace ccamd {

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

cc_status build_plan(cc_detector* d, int w, int h, const cc_detect_params& p, Plan** out) {
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

EvScope::EvScope(cc_detector* d_, int kind_, hipStream_t st_) : d(d_), kind(kind_), st(st_) {
  if (!d->profiling || kind < 0) return;
  if (a.create() != hipSuccess || b.create() != hipSuccess) {
    a = OwnEvent();
    return;
  }
  (void)hipEventRecord(a.e, st);
}
EvScope::~EvScope() {
  if (!a.e) return;
  (void)hipEventRecord(b.e, st);
  d->events.push_back(TimingEvent{std::move(a), std::move(b), kind});
}

void collect_events(cc_detector* d) {
  for (auto& e : d->events) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, e.a.e, e.b.e) != hipSuccess) continue;
    switch (e.kind) {
      case EV_RESIZE: d->tm.resize_ms += ms; d->tm.resize_launches++; break;
      case EV_INTEGRAL: d->tm.integral_ms += ms; d->tm.integral_launches++; break;
      case EV_EVAL: d->tm.eval_ms += ms; d->tm.eval_launches++; break;
      case EV_EVAL_STEP1: d->tm.eval_step1_ms += ms; break;
      case EV_FILTER: d->tm.finalize_ms += ms; d->tm.finalize_launches++; break;
      case EV_GROUP: d->tm.group_ms += ms; d->tm.group_launches++; break;
    }
  }
  d->events.clear();
}

// The cascade-kernel launches of a pass, see EvalLaunch. create_lists: a missing tile list is built (plan_tiles).
static cc_status pass_launches(cc_detector* d, Plan* P, bool create_lists, EvalLaunch out[2], int* n_out) {
  const bool run_spec = d->n_spec > 0 && d->m.max_nodes_per_tree <= 1;
  const int n = run_spec ? d->n_spec : 1;
  for (int i = 0; i < n; i++) {
    const SpecModule aot{nullptr, nullptr, d->lds, TILE_Y, 0};
    const SpecModule& M = run_spec ? d->spec[i] : aot;
    const Plan::TileList* tl = nullptr;
    if (cc_status st = plan_tiles(d, P, M.tile_y, M.only_step, create_lists, &tl); st != CC_OK) return st;
    out[i] = EvalLaunch{M.fn, M.lds, tl->n, tl->d.p, M.wave_below};
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

// CCAMD_DEBUG_STAMPS=<path>: waits for the pass and writes its stamps, [n_tiles * nf][eval_stamp_slots()] u64 (overwritten per pass).
static cc_status dump_stamps(cc_detector* d, const char* path, int nf) {
  CC_HIP(hipStreamSynchronize(d->stream));
  const int n_tiles_run = d->last_stamp_tiles;
  std::vector<unsigned long long> h((size_t)n_tiles_run * (size_t)nf * eval_stamp_slots());
  CC_HIP(hipMemcpyAsync(h.data(), d->d_stamps.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, d->stream));
  CC_HIP(hipStreamSynchronize(d->stream));
  if (FILE* f = std::fopen(path, "wb")) {
    const int hdr[4] = {n_tiles_run, nf, eval_stamp_slots(), 0};
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
  hipStream_t fs = d->overlap_front && !single_stream ? d->front_stream.s : d->stream;  // pyramid + integrals
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
  if (fs != st && d->eval_pending[slot]) CC_HIP(hipStreamWaitEvent(fs, d->eval_done[slot].e, 0));
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
    CC_HIP(hipEventRecord(d->front_done[slot].e, fs));
    CC_HIP(hipStreamWaitEvent(st, d->front_done[slot].e, 0));
  }
  {
    EvScope ev(d, EV_EVAL, st);
    unsigned long long* stamps = nullptr;
    EvalLaunch launches[2];
    int n_launches = 0;
    if (cc_status ls = pass_launches(d, P, false, launches, &n_launches); ls != CC_OK) return ls;
    size_t stamp_tiles = 0;
    for (int i = 0; i < n_launches; i++) stamp_tiles += (size_t)launches[i].n_tiles;
    if (std::getenv("CCAMD_DEBUG_STAMPS")) {  // timing experiments: per-block phase stamps of the cascade kernel (launch after launch)
      CC_HIP(d->d_stamps.ensure(std::max<size_t>(stamp_tiles * (size_t)nf * eval_stamp_slots(), 1)));
      CC_HIP(hipMemsetAsync(d->d_stamps.p, 0, stamp_tiles * (size_t)nf * eval_stamp_slots() * sizeof(unsigned long long), st));
      stamps = d->d_stamps.p;
    }
    if (cc_status es = launch_eval(d, P, slot, nchan, tilt, sq_compact, debug, stamps, launches, n_launches, nf, st); es != CC_OK) return es;
    d->last_stamp_tiles = (int)stamp_tiles;
  }
  if (fs != st) {
    CC_HIP(hipEventRecord(d->eval_done[slot].e, st));
    d->eval_pending[slot] = true;
  }
  {
    EvScope ev(d, EV_FILTER, st);
    launch_filter_candidates(d, P, slot, st);
    if (debug && P->n_grid_rows) launch_debug_visited(d, P, slot, st);
  }
  CC_HIP(hipGetLastError());
  if (const char* path = std::getenv("CCAMD_DEBUG_STAMPS"))
    if (cc_status ds = dump_stamps(d, path, nf); ds != CC_OK) return ds;
  d->tm.frames += nf;
  d->tm.grid_windows += P->windows * nf;
  d->tm.integral_elems += P->integral_elems * nf;
  return CC_OK;
}

cc_status check_frame_args(const cc_detector* d, const FrameSet& F, const cc_detect_params* p, const char* who) {
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
  CC_HIP(hipMemcpyAsync(d->counts(slot), d->d_counts[slot].p, 2 * sizeof(int), hipMemcpyDeviceToHost, d->stream));
  CC_HIP(hipEventRecord(d->pass_done[slot].e, d->stream));
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

cc_status retire_pending(cc_detector* d) {
  if (!d->pending.active) return CC_OK;
  cc_detector::PendingPass ps = d->pending;
  d->pending.drop();
  std::vector<CandOut> got;
  for (;;) {
    CC_HIP(hipEventSynchronize(d->pass_done[ps.slot].e));
    const int raw = d->counts(ps.slot)[0], kept = d->counts(ps.slot)[1];
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
      CC_HIP(hipMemcpyAsync(got.data(), d->d_out[ps.slot].p, (size_t)kept * sizeof(CandOut), hipMemcpyDeviceToHost, d->copy_stream.s));
      CC_HIP(hipStreamSynchronize(d->copy_stream.s));
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
void retire_foreign(cc_detector* d) {
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
// The slots have ONE pitch for all passes (h_stage.bytes / kStageSlots), not the pass's own frame size: gray and colour
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
  if (d->h_stage.bytes / kStageSlots < fs * (size_t)d->pass_capacity) {
    if (d->h_stage.p) CC_HIP(hipStreamSynchronize(front));  // no copy may still be reading the old area
    CC_HIP(d->h_stage.ensure(fs * (size_t)d->pass_capacity * kStageSlots));
  }
  uint8_t* hs = static_cast<uint8_t*>(d->h_stage.p) + (size_t)slot * (d->h_stage.bytes / kStageSlots);
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
  if (d->copy_stream.s) return CC_OK;
  CC_HIP(d->copy_stream.create());
  CC_HIP(d->pass_done[0].create(hipEventDisableTiming));
  CC_HIP(d->pass_done[1].create(hipEventDisableTiming));
  CC_HIP(d->h_counts.ensure(4 * sizeof(int)));
  {  // the pyramid / integral stream only fills what the cascade kernel leaves idle: lowest priority
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    CC_HIP(d->front_stream.create(least));
  }
  for (OwnEvent* e : {&d->front_done[0], &d->front_done[1], &d->eval_done[0], &d->eval_done[1], &d->batch_begin}) CC_HIP(e->create(hipEventDisableTiming));
  d->overlap_front = std::getenv("CCAMD_NO_FRONT_OVERLAP") ? 0 : 1;
  return CC_OK;
}

// A single host image on the graph path: its gray frame on the device (rows rs apart, fs bytes), the rows as they travel
// (crows rows of cw bytes at pitch cpitch, cfs in all; colour: width * bpp bytes, planar 3 * height rows of width; gray: the
// gray frame itself) and the pinned block its pass copies from, one per kind: the gray graphs keep theirs.
struct SingleImage {
  const FrameSet& F;
  const bool color;
  const size_t rs, fs;
  const int crows;
  const size_t cw, cpitch, cfs;
  PinnedBuf& pin;
  SingleImage(cc_detector* d, const FrameSet& F_)
      : F(F_), color(F.fmt != CC_PIX_GRAY8), rs((size_t)align_up(F.width, 4)), fs(rs * (size_t)F.height), crows(pix_rows(F.fmt, F.height)),
        cw((size_t)F.width * pix_bytes(F.fmt)), cpitch((size_t)align_up((int)cw, 4)), cfs(cpitch * (size_t)crows),
        pin(color ? d->h_color_frame : d->h_frame) {}
};

// The image into its pinned block, and the device buffers it lands in at their sizes.
static cc_status stage_single_image(cc_detector* d, const SingleImage& I) {
  CC_HIP(I.pin.ensure(I.cfs));
  for (int y = 0; y < I.crows; y++)
    std::memcpy(static_cast<uint8_t*>(I.pin.p) + (size_t)y * I.cpitch, I.F.frames + (size_t)y * I.F.row_stride, I.cw);
  CC_HIP(d->d_frames.ensure(I.fs * (size_t)d->pass_capacity * 2));
  if (I.color) {
    if (d->d_color.n < I.cfs && d->d_color.p && d->front_stream.s) CC_HIP(hipStreamSynchronize(d->front_stream.s));  // batch conversions
    CC_HIP(d->d_color.ensure(I.cfs));
  }
  return CC_OK;
}

// The pass of a single image on the detector's stream: copy in, (conversion,) pipeline, counters back. This is what a graph records.
static cc_status enqueue_single_image(cc_detector* d, Plan* P, const SingleImage& I) {
  if (I.color) {
    CC_HIP(hipMemcpyAsync(d->d_color.p, I.pin.p, I.cfs, hipMemcpyHostToDevice, d->stream));
    launch_to_gray(d->stream, I.F.fmt, d->d_color.p, I.cpitch, I.cfs, I.F.width, I.F.height, 1, d->d_frames.p, I.rs, I.fs);
  } else
    CC_HIP(hipMemcpyAsync(d->d_frames.p, I.pin.p, I.fs, hipMemcpyHostToDevice, d->stream));
  cc_status s2 = run_device_pass(d, P, d->d_frames.p, 1, I.rs, I.fs, false, 0, true);
  if (s2 != CC_OK) return s2;
  CC_HIP(hipMemcpyAsync(d->counts(0), d->d_counts[0].p, 2 * sizeof(int), hipMemcpyDeviceToHost, d->stream));
  return CC_OK;
}

// Everything a recorded pass names: a graph is replayed only while all of it is what it was at the capture.
static std::vector<const void*> graph_key(const cc_detector* d, const SingleImage& I) {
  return {d->d_frames.p, I.pin.p, I.color ? d->d_color.p : nullptr, d->d_pyr.p, d->d_integ[0].p, d->d_hbuf.p, d->d_diag.p, d->d_tseg.p, d->d_masks[0].p,
          d->d_cands[0].p, d->d_out[0].p, d->d_counts[0].p, d->h_counts.p, (const void*)d->spec[0].fn, (const void*)d->spec[1].fn, (const void*)d->stream,
          (const void*)(size_t)d->cand_cap, (const void*)(size_t)d->wave_below, (const void*)(size_t)(d->stop_after + 16)};
}

// Records the pass into a new graph for `gexec` (the old one ends). False: no graph came out; the detector says so once on
// stderr and uses ordinary launches from now on (this call included): the call still succeeds, only the launch-bound
// single-image path gets slower.
static bool capture_single_image(cc_detector* d, Plan* P, const SingleImage& I, hipGraphExec_t& gexec) {
  if (gexec) (void)hipGraphExecDestroy(gexec);
  gexec = nullptr;
  hipGraph_t graph = nullptr;
  // Relaxed mode: this thread's stream-ordered calls are captured, nobody's legacy-stream calls are policed (other
  // host threads may be inside synchronous copies of their own handles; under the stricter modes HIP fails those
  // calls and invalidates this capture). One capture at a time per process.
  static std::mutex capture_mu;
  hipError_t ce = hipSuccess, ie = hipSuccess;
  cc_status s2 = CC_OK;
  {
    std::lock_guard<std::mutex> capture_lock(capture_mu);
    ce = std::getenv("CCAMD_DEBUG_FAIL_CAPTURE") ? hipErrorStreamCaptureUnsupported  // tests: the fallback path
                                                 : hipStreamBeginCapture(d->stream, hipStreamCaptureModeRelaxed);
    if (ce == hipSuccess) {
      s2 = enqueue_single_image(d, P, I);
      ce = hipStreamEndCapture(d->stream, &graph);
    }
  }
  if (ce == hipSuccess && s2 == CC_OK && graph) ie = hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0);
  if (graph) (void)hipGraphDestroy(graph);
  if (ce == hipSuccess && s2 == CC_OK && ie == hipSuccess && gexec) return true;
  std::fprintf(stderr, "[ccamd] hipGraph capture of the single-image pass failed (begin/end: %s, body status %d, instantiate: %s): "
                       "this detector uses ordinary launches from now on\n",
               hipGetErrorString(ce), (int)s2, hipGetErrorString(ie));
  (void)hipGetLastError();
  gexec = nullptr;
  d->use_graph = 0;
  return false;
}

// Single host image: one pass on one stream, replayed from a hipGraph once the buffers are sized (a plan's first call per
// format is never captured). Hands the candidates to `sink` and sets `delivered`, or leaves it false when the candidate
// lists overflowed: the ordinary path then grows the lists and redoes the pass.
static cc_status run_single_image_graph(cc_detector* d, Plan* P, const FrameSet& F, BatchSink& sink, bool* delivered) {
  *delivered = false;
  const SingleImage I(d, F);
  if (cc_status st = stage_single_image(d, I); st != CC_OK) return st;
  if (d->eval_pending[0] || d->eval_pending[1]) {  // a batch call may still be using the buffers on the other stream
    CC_HIP(hipStreamSynchronize(d->front_stream.s));
    d->eval_pending[0] = d->eval_pending[1] = false;
  }
  d->last_call_graph = 0;
  hipGraphExec_t& gexec = P->graph_exec[F.fmt];
  bool replay = gexec && P->graph_key[F.fmt] == graph_key(d, I);
  if (!replay && P->graph_warm[F.fmt] && capture_single_image(d, P, I, gexec)) {
    P->graph_key[F.fmt] = graph_key(d, I);
    d->graph_captures++;
    replay = true;
  }
  if (replay) {
    CC_HIP(hipGraphLaunch(gexec, d->stream));
    d->last_call_graph = 1;
  } else {
    if (cc_status st = enqueue_single_image(d, P, I); st != CC_OK) return st;
    P->graph_warm[F.fmt] = true;  // every buffer now has its size: the next call can be captured
  }
  CC_HIP(hipStreamSynchronize(d->stream));
  const int raw = d->counts(0)[0], kept = d->counts(0)[1];
  if (raw > d->cand_cap) return CC_OK;  // overflow: falls through to the ordinary path
  std::vector<CandOut> got((size_t)kept);
  if (kept > 0) {
    CC_HIP(hipMemcpyAsync(got.data(), d->d_out[0].p, (size_t)kept * sizeof(CandOut), hipMemcpyDeviceToHost, d->stream));
    CC_HIP(hipStreamSynchronize(d->stream));
  }
  if (sink.consume) sink.consume(0, 1, got);
  *delivered = true;
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
  hipStream_t front = d->overlap_front ? d->front_stream.s : d->stream;
  // Frames produced by earlier work on a stream the CALLER gave us (cc_detector_set_stream) must be complete before the
  // pyramid reads them. On the detector's own stream there is only our own earlier work -- a pending pass of the batch
  // submitted before -- and waiting for that would serialise exactly what cc_detect_batch_submit exists to overlap.
  if (front != d->stream && d->stream != d->own_stream.s) {
    CC_HIP(hipEventRecord(d->batch_begin.e, d->stream));
    CC_HIP(hipStreamWaitEvent(front, d->batch_begin.e, 0));
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
    if (d->front_stream.s) CC_HIP(hipStreamSynchronize(d->front_stream.s));
    collect_events(d);
  }
  return CC_OK;
}

cc_status run_batch(cc_detector* d, const FrameSet& F, const cc_detect_params* p, const std::shared_ptr<BatchSink>& sink,
                           const BatchOptions& opt) {
  const cc_status st = run_batch_passes(d, F, p, sink, opt);
  if (st != CC_OK && d->pending.active && d->pending.sink == sink) d->pending.drop();
  return st;
}

}  // namespace ccamd
