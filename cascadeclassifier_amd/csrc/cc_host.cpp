// Host-side pieces of the hot path that are tiny and serial in the reference too: error plumbing, the scale
// pyramid geometry, the tap tables of the fixed-point bilinear resize, rectangle grouping and the feature catalogs.
// Everything that scales with pixels / windows / samples runs in the HIP kernels (cc_detect.hip, cc_front.hip, cc_group.hip, cc_eval_*.hip).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <numeric>

#include "cc_internal.h"
#include "cc_resize_arith.h"

namespace ccamd {

static thread_local std::string g_last_error;

cc_status set_error(cc_status code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

// cvRound: round half to even, as the SSE conversion does under the default rounding mode.
static inline int rnd_f(float v) { return (int)std::nearbyintf(v); }
static inline int rnd_d(double v) { return (int)std::nearbyint(v); }

// Scale list and per-scale geometry of detectMultiScale (OpenCV 4.6.0 cascadedetect.cpp
// detectMultiScaleNoGrouping + FeatureEvaluator::updateScaleData + the stripe split of the scan loop).
void scale_plan(int W0, int H0, int imgw, int imgh, const cc_detect_params& p, std::vector<ScaleGeom>& out) {
  out.clear();
  int maxW = p.max_w, maxH = p.max_h;
  if (maxW == 0 || maxH == 0) {
    maxW = imgw;
    maxH = imgh;
  }
  if (imgh < H0 || imgw < W0) return;
  std::vector<float> all, scales;
  for (double factor = 1;; factor *= p.scale_factor) {
    const int ww = rnd_d(W0 * factor), wh = rnd_d(H0 * factor);
    if (ww > imgw || wh > imgh) break;
    all.push_back((float)factor);
    if (all.size() > 100000) break;
  }
  for (float s : all) {
    const int ww = rnd_f(W0 * s), wh = rnd_f(H0 * s);
    if (ww > maxW || wh > maxH) break;
    if (ww < p.min_w || wh < p.min_h) continue;
    scales.push_back(s);
  }
  if (scales.empty() && !all.empty()) {  // minSize == maxSize off the grid: closest scale
    size_t best = 0;
    double dbest = 0;
    for (size_t v = 0; v < all.size(); v++) {
      const int ww = rnd_f(W0 * all[v]), wh = rnd_f(H0 * all[v]);
      const double d = (double)(p.min_w - ww) * (p.min_w - ww) + (double)(p.min_h - wh) * (p.min_h - wh);
      if (v == 0 || dbest > d) {
        dbest = d;
        best = v;
      }
    }
    scales.push_back(all[best]);
  }
  int nstripes = 1;
  for (size_t i = 0; i < scales.size(); i++) {
    ScaleGeom g;
    g.scale = scales[i];
    g.w = rnd_f(imgw / g.scale);
    g.h = rnd_f(imgh / g.scale);
    g.ystep = g.scale >= 2 ? 1 : 2;
    const int szw_w = std::max(g.w + 1 - W0, 0), szw_h = std::max(g.h + 1 - H0, 0);
    if (i == 0) nstripes = std::max((int)std::ceil(szw_w / 32.), 1);
    const int stripe = std::max((szw_h / g.ystep + nstripes - 1) / nstripes, 1) * g.ystep;
    const int y_end = std::min(nstripes * stripe, szw_h);
    g.nx = (szw_w + g.ystep - 1) / g.ystep;
    g.ny = (y_end + g.ystep - 1) / g.ystep;
    if (szw_w <= 0 || y_end <= 0) g.nx = g.ny = 0;
    g.win_w = rnd_f(W0 * g.scale);
    g.win_h = rnd_f(H0 * g.scale);
    out.push_back(g);
  }
}

// INTER_LINEAR_EXACT tap table of one axis: f = scale*(d+0.5)-0.5, scale = 1/((double)dst/src).
void linear_exact_taps(int src, int dst, AxisTaps& t) {
  t.ofs.resize(dst);
  t.w1.resize(dst);
  for (int d = 0; d < dst; d++) linear_exact_tap(src, dst, d, t.ofs[d], t.w1[d]);
}

// Pass sizes. With results wanted the batch is cut into a few passes so that the host side of pass i (copy-back +
// grouping) overlaps the device side of pass i+1 and the pyramid/integrals of pass i+1 overlap the cascade kernel of
// pass i. Nothing overlaps the LAST pass's host work, so with three or more passes it is the short one: every pass before
// it carries ceil(2n / (2 passes - 1)) frames and the last what is left, half a pass or less (32 frames in 4 passes ->
// 10, 10, 10, 2; a small first pass, to start the cascade kernel earlier, measured no better). A SUBMITTED batch has its last
// pass overlapped by the batch after it, so it is cut into two even passes only (bench step 17.51 ms against 17.86 / 18.25
// for 1 / 4 passes, profiles/r03_kernel_experiments.txt). Without results the passes are as large as max_batch allows.
std::vector<int> pass_sizes(int n_frames, int max_batch, int pipeline_passes, bool pipeline_passes_set, bool want_results,
                            bool defer_last) {
  std::vector<int> sizes;
  if (want_results && n_frames >= 2) {
    const bool submitted = defer_last && !pipeline_passes_set;
    const int passes = std::min(submitted ? 2 : pipeline_passes, n_frames);
    int per = (n_frames + passes - 1) / passes;
    if (passes >= 3 && !submitted) {
      const int big = (2 * n_frames + 2 * passes - 2) / (2 * passes - 1);
      if (big >= 2 && big * (passes - 1) < n_frames) per = big;
    }
    for (int f = 0; f < n_frames; f += per) sizes.push_back(std::min(per, n_frames - f));
  } else {
    for (int f = 0; f < n_frames; f += max_batch) sizes.push_back(std::min(max_batch, n_frames - f));
  }
  // normalise: sizes within max_batch, summing to n_frames (a pass larger than max_batch is cut down where it stands and
  // the frames it loses make up further passes at the end: 64 frames at max_batch 16 -> 16, 16, 16, 7, 9)
  std::vector<int> fixed;
  int left = n_frames;
  for (size_t i = 0; left > 0; i++) {
    int v = i < sizes.size() ? sizes[i] : left;
    v = std::max(1, std::min({v, max_batch, left}));
    fixed.push_back(v);
    left -= v;
  }
  return fixed;
}

// Stage groups (EvalArgs::group_first). Every stage boundary inside the cascade kernel costs the block a barrier, the
// class counts and a queue rebuild -- about as much as a pass over 25 stumps -- while what it buys is that the windows
// rejected by the stage stop occupying lanes. For short stages (the stock LBP cascade has 3-10 stumps per stage) the
// boundary costs more than it saves, so consecutive stages are put into one group while the group stays within
// `budget` stumps; a stage longer than the budget is a group of its own (the form every stage had before). Grouping
// never changes a result: a window's exit stage and stage sum are recorded where it fails, whatever the lanes around
// it do. Cascades with deeper trees keep one stage per group (budget 0).
// Measured (round 3, stock LBP cascade, ms per 32 Full-HD frames alone on the device; tools/sweeps/r3_*.txt): grouping
// from stage 1 on is slower at every budget but 12 stumps (-3 %), because the lanes of windows that died inside a
// group keep executing; the gain is in the LATE stages, where a handful of windows per tile pay a barrier round per
// stage. Hence two knobs: groups start at stage `from`, and hold up to `budget` stumps.
// LBP with its wave phase (which takes over below 24 windows), round 3 (tiles of 8 rows, bank-class table): groups of
// <= 20 stumps from stage 2 on 4.91-5.06, 12 from stage 1: 5.04-5.25, one stage per group 5.29, 30 from stage 2: 5.36.
// Round 4 (list queue from stage 2; specialised kernel on tiles of 20 rows): <= 14 stumps 3.70, <= 20 3.87, <= 30 4.17;
// at 8 rows 4.84 / 4.87 / 5.13.
void stage_groups(const std::vector<int32_t>& stage_ntrees, int from, int budget, int dense_stage, std::vector<int>& group_first,
                  int& dense_from) {
  std::vector<int>& gf = group_first;
  gf.clear();
  const int nst = (int)stage_ntrees.size();
  for (int s0 = 0; s0 < nst;) {
    gf.push_back(s0);
    const int cap = s0 < from ? 0 : budget;  // stage 0 is the dense phase: always alone
    int s1 = s0 + 1, sum = stage_ntrees[(size_t)s0];
    while (s1 < nst && sum + stage_ntrees[(size_t)s1] <= cap) sum += stage_ntrees[(size_t)s1++];
    s0 = s1;
  }
  gf.push_back(nst);
  if (gf.size() < 2) gf.push_back(nst);  // no stage at all: one empty group, the kernels read group_first[1]
  // Queue form (EvalArgs::dense_from): LBP stump cascades switch from the bank-class table to a plain list at stage 2.
  // There the tile is down to ~100 of its 512 windows: the table needs 6.2 rows for them (its fullest class) where a list
  // needs 3.1, i.e. four wavefront passes over the group's 19 stumps instead of two, and the LBP kernel is bound by the
  // vector ALU (73 % busy; LDS 52 %, profiles/r04_pmc_eval_lbp.json), not by the ~2.5-way bank conflicts the list costs.
  // Haar cascades keep the table everywhere (LDS-bound; CCAMD_DENSE_FROM=<stage> to experiment).
  dense_from = 0x7fffffff;
  if (dense_stage >= 1)
    for (int g = (int)gf.size() - 2; g >= 1; g--)
      if (gf[(size_t)g] >= dense_stage) dense_from = g;
}

// Range proofs over a cascade's leaf values that decide, at load time, which arithmetic a kernel may use for the stage
// sums (declared in cc_detect_internal.h; tests/cpp/test_detect_host.cpp sits on their bounds).
bool stage_sums_order_independent(const Cascade& m, double headroom) {
  for (size_t s = 0; s < m.stage_ntrees.size(); s++) {
    int emin = INT32_MAX;
    double mag = 0;
    for (int i = 0; i < m.stage_ntrees[s]; i++) {
      const size_t k = (size_t)m.stage_first[s] + i;
      const float l = m.stump_left[k], r = m.stump_right[k];
      if (!std::isfinite(l) || !std::isfinite(r)) return false;
      mag += std::max(std::fabs((double)l), std::fabs((double)r));
      for (float v : {l, r})
        if (v != 0.0f) {
          int e;
          std::frexp(v, &e);
          emin = std::min(emin, e);
        }
    }
    if (emin == INT32_MAX) continue;
    // v = f * 2^e with f in [0.5, 1) and a 24-bit significand: v is a multiple of 2^(e-24); subnormals only get coarser
    const double q = std::ldexp(1.0, emin - 24);
    if (mag * headroom / q >= 9007199254740992.0) return false;
  }
  return true;
}

// Fixed-point votes of a generated stage (cc_spec.hip): true when the stage's leaves are all multiples of q = 2^k and the
// sum of their larger magnitudes stays below (2^31 - 1) q, so that the stage sum of ANY subset of votes is an int32
// multiple of q. A stage without a nonzero leaf has no quantum.
bool stage_quantum(const Cascade& m, int s, double& q) {
  int emin = INT32_MAX;
  double mag = 0;
  for (int i = 0; i < m.stage_ntrees[(size_t)s]; i++) {
    const size_t k = (size_t)m.stage_first[(size_t)s] + i;
    const float l = m.stump_left[k], r = m.stump_right[k];
    mag += std::max(std::fabs((double)l), std::fabs((double)r));
    for (float v : {l, r})
      if (v != 0.0f) {
        int e;
        std::frexp(v, &e);
        emin = std::min(emin, e);
      }
  }
  if (emin == INT32_MAX) return false;
  q = std::ldexp(1.0, emin - 24);  // every leaf is a multiple of q (see stage_sums_order_independent)
  return mag / q < 2147483647.0;
}

// Integer form of the Haar wave phase's stage sums (WaveIntTables, cc_detect_internal.h). With x = threshold / q (exact: q
// is a power of two), an integer n has n * q >= threshold exactly when n >= ceil(x). A reachable n has |n| <= 2^31 - 2
// (stage_quantum), so a threshold beyond either end saturates to the int32 limit that always passes / never does.
WaveIntTables wave_int_tables(const Cascade& m, bool enabled) {
  const size_t ns = m.stage_ntrees.size();
  WaveIntTables t;
  t.q.assign(ns, 0.0);
  t.thr_q.assign(ns, 0);
  t.left_q.assign(m.stump_left.size(), 0);
  t.right_q.assign(m.stump_left.size(), 0);
  if (!enabled || m.feature_type != CC_FEATURE_HAAR || m.max_nodes_per_tree != 1 || !stage_sums_order_independent(m, 1.0)) return t;
  for (size_t s = 0; s < ns; s++) {
    double q;
    const double thr = (double)m.stage_threshold[s];
    if (std::isnan(thr) || !stage_quantum(m, (int)s, q)) continue;  // (a NaN threshold passes every sum: left to the double form)
    const double x = std::ceil(thr / q);
    t.q[s] = q;
    t.thr_q[s] = x >= 2147483647.0 ? INT32_MAX : x <= -2147483648.0 ? INT32_MIN : (int32_t)x;
    for (int i = 0; i < m.stage_ntrees[s]; i++) {
      const size_t k = (size_t)m.stage_first[s] + i;
      t.left_q[k] = (int32_t)((double)m.stump_left[k] / q);  // exact, and below 2^31 - 1 in magnitude (stage_quantum)
      t.right_q[k] = (int32_t)((double)m.stump_right[k] / q);
    }
  }
  return t;
}

// cv::groupRectangles. Classes are the connected components of the SimilarRects graph, labelled in
// order of first appearance, which is what cv::partition yields.
void group_rectangles(std::vector<cc_rect>& rects, int group_threshold, double eps, std::vector<int>* levels,
                      std::vector<double>* level_weights) {
  const int n = (int)rects.size();
  if (group_threshold <= 0 || n == 0) return;  // (with both vectors given, upstream leaves them untouched here as well)
  std::vector<int> parent(n), rank_(n, 0);
  std::iota(parent.begin(), parent.end(), 0);
  auto find = [&](int a) {
    int r = a;
    while (parent[r] != r) r = parent[r];
    while (parent[a] != r) {
      int nx = parent[a];
      parent[a] = r;
      a = nx;
    }
    return r;
  };
  // SimilarRects needs |a.x - b.x| <= delta <= eps * (a.w + a.h) / 2, so after sorting by x only a short run of
  // followers can be similar to a rectangle: a sweep instead of all n^2 pairs (same components, same labels).
  std::vector<int> order(n);
  std::iota(order.begin(), order.end(), 0);
  std::sort(order.begin(), order.end(), [&](int a, int b) { return rects[a].x < rects[b].x; });
  for (int oi = 0; oi < n; oi++) {
    const int i = order[oi];
    const cc_rect& a = rects[i];
    const double reach = eps * (a.width + a.height) * 0.5;
    for (int oj = oi + 1; oj < n; oj++) {
      const int j = order[oj];
      const cc_rect& b = rects[j];
      if (b.x - a.x > reach) break;
      const double delta = eps * (std::min(a.width, b.width) + std::min(a.height, b.height)) * 0.5;
      if (std::abs(a.x - b.x) <= delta && std::abs(a.y - b.y) <= delta &&
          std::abs(a.x + a.width - b.x - b.width) <= delta && std::abs(a.y + a.height - b.y - b.height) <= delta) {
        int ra = find(i), rb = find(j);
        if (ra == rb) continue;
        if (rank_[ra] < rank_[rb]) std::swap(ra, rb);
        parent[rb] = ra;
        if (rank_[ra] == rank_[rb]) rank_[ra]++;
      }
    }
  }
  std::vector<int> cls_of_root(n, -1), label(n);
  int nclasses = 0;
  for (int i = 0; i < n; i++) {
    const int r = find(i);
    if (cls_of_root[r] < 0) cls_of_root[r] = nclasses++;
    label[i] = cls_of_root[r];
  }
  std::vector<cc_rect> acc(nclasses, cc_rect{0, 0, 0, 0});
  std::vector<int> cnt(nclasses, 0);
  for (int i = 0; i < n; i++) {
    cc_rect& a = acc[label[i]];
    a.x += rects[i].x;
    a.y += rects[i].y;
    a.width += rects[i].width;
    a.height += rects[i].height;
    cnt[label[i]]++;
  }
  for (int i = 0; i < nclasses; i++) {
    const float s = 1.f / cnt[i];
    acc[i] = cc_rect{rnd_f(acc[i].x * s), rnd_f(acc[i].y * s), rnd_f(acc[i].width * s), rnd_f(acc[i].height * s)};
  }
  // outputRejectLevels variant: per class the highest level among its members and, among those, the largest weight
  std::vector<int> cls_level(nclasses, 0), out_levels;
  std::vector<double> cls_weight(nclasses, DBL_MIN), out_weights;
  const bool with_levels = levels && level_weights && !levels->empty() && !level_weights->empty();
  if (with_levels)
    for (int i = 0; i < n; i++) {
      const int c = label[i];
      if ((*levels)[(size_t)i] > cls_level[c]) {
        cls_level[c] = (*levels)[(size_t)i];
        cls_weight[c] = (*level_weights)[(size_t)i];
      } else if ((*levels)[(size_t)i] == cls_level[c] && (*level_weights)[(size_t)i] > cls_weight[c])
        cls_weight[c] = (*level_weights)[(size_t)i];
    }
  std::vector<cc_rect> out;
  for (int i = 0; i < nclasses; i++) {
    const cc_rect r1 = acc[i];
    const int n1 = cnt[i];
    if (n1 <= group_threshold) continue;
    int j;
    for (j = 0; j < nclasses; j++) {
      const int n2 = cnt[j];
      if (j == i || n2 <= group_threshold) continue;
      const cc_rect r2 = acc[j];
      const int dx = rnd_d(r2.width * eps), dy = rnd_d(r2.height * eps);
      if (r1.x >= r2.x - dx && r1.y >= r2.y - dy && r1.x + r1.width <= r2.x + r2.width + dx &&
          r1.y + r1.height <= r2.y + r2.height + dy && (n2 > std::max(3, n1) || n1 < 3))
        break;
    }
    if (j == nclasses) {
      out.push_back(r1);
      out_levels.push_back(with_levels ? cls_level[i] : n1);  // "useDefaultWeights": the class size
      out_weights.push_back(cls_weight[i]);
    }
  }
  rects.swap(out);
  if (levels) levels->swap(out_levels);
  if (level_weights) level_weights->swap(out_weights);
}

// Haar catalog in the reference's order (traincascade/lib/src/haarfeatures.cpp:127-251); the feature index is part of
// the contract because valCache rows / var_idx are catalog indices.
void haar_catalog(int W, int H, int mode, std::vector<HaarFeature>& out) {
  out.clear();
  auto add = [&](bool tilted, int x0, int y0, int w0, int h0, float t0, int x1, int y1, int w1, int h1, float t1,
                 int x2 = 0, int y2 = 0, int w2 = 0, int h2 = 0, float t2 = 0.f) {
    HaarFeature f;
    const int32_t r[3][4] = {{x0, y0, w0, h0}, {x1, y1, w1, h1}, {x2, y2, w2, h2}};
    std::memcpy(f.r, r, sizeof(r));
    f.w[0] = t0;
    f.w[1] = t1;
    f.w[2] = t2;
    f.tilted = tilted ? 1 : 0;
    out.push_back(f);
  };
  const bool core = mode != CC_HAAR_BASIC, all = mode == CC_HAAR_ALL;
  for (int x = 0; x < W; x++)
    for (int y = 0; y < H; y++)
      for (int dx = 1; dx <= W; dx++)
        for (int dy = 1; dy <= H; dy++) {
          const bool fx1 = x + dx <= W, fy1 = y + dy <= H;
          if (x + 2 * dx <= W && fy1) add(false, x, y, 2 * dx, dy, -1, x + dx, y, dx, dy, 2);          // x2
          if (fx1 && y + 2 * dy <= H) add(false, x, y, dx, 2 * dy, -1, x, y + dy, dx, dy, 2);          // y2
          if (x + 3 * dx <= W && fy1) add(false, x, y, 3 * dx, dy, -1, x + dx, y, dx, dy, 2);          // x3 (weight 2, as coded)
          if (fx1 && y + 3 * dy <= H) add(false, x, y, dx, 3 * dy, -1, x, y + dy, dx, dy, 2);          // y3
          if (core && x + 4 * dx <= W && fy1) add(false, x, y, 4 * dx, dy, -1, x + dx, y, 2 * dx, dy, 2);  // x4
          if (core && fx1 && y + 4 * dy <= H) add(false, x, y, dx, 4 * dy, -1, x, y + dy, dx, 2 * dy, 2);  // y4
          if (x + 2 * dx <= W && y + 2 * dy <= H)
            add(false, x, y, 2 * dx, 2 * dy, -1, x, y, dx, dy, 2, x + dx, y + dy, dx, dy, 2);          // x2_y2
          if (core && x + 3 * dx <= W && y + 3 * dy <= H)
            add(false, x, y, 3 * dx, 3 * dy, -1, x + dx, y + dy, dx, dy, 9);                            // centre
          if (all) {
            if (x + 2 * dx <= W && y + 2 * dx + dy <= H && x - dy >= 0) add(true, x, y, 2 * dx, dy, -1, x, y, dx, dy, 2);
            if (fx1 && y + dx + 2 * dy <= H && x - 2 * dy >= 0) add(true, x, y, dx, 2 * dy, -1, x, y, dx, dy, 2);
            if (x + 3 * dx <= W && y + 3 * dx + dy <= H && x - dy >= 0) add(true, x, y, 3 * dx, dy, -1, x + dx, y + dx, dx, dy, 3);
            if (fx1 && y + dx + 3 * dy <= H && x - 3 * dy >= 0) add(true, x, y, dx, 3 * dy, -1, x - dy, y + dy, dx, dy, 3);
            if (x + 4 * dx <= W && y + 4 * dx + dy <= H && x - dy >= 0) add(true, x, y, 4 * dx, dy, -1, x + dx, y + dx, 2 * dx, dy, 2);
            if (fx1 && y + dx + 4 * dy <= H && x - 4 * dy >= 0) add(true, x, y, dx, 4 * dy, -1, x - dy, y + dy, dx, 2 * dy, 2);
          }
        }
}

// LBP catalog (traincascade/lib/src/lbpfeatures.cpp:35-45): one cell (x y w h) of the 3x3 grid per feature.
void lbp_catalog(int W, int H, std::vector<int32_t>& rects) {
  rects.clear();
  for (int x = 0; x < W; x++)
    for (int y = 0; y < H; y++)
      for (int w = 1; w <= W / 3; w++)
        for (int h = 1; h <= H / 3; h++)
          if (x + 3 * w <= W && y + 3 * h <= H) {
            rects.push_back(x);
            rects.push_back(y);
            rects.push_back(w);
            rects.push_back(h);
          }
}

// HOG catalog (HOGfeatures.cpp:67-106): cell size t = 8, 16, ... while t <= W / 2; per t three block shapes (2t x 2t,
// 2t x 4t, 4t x 2t in pixels; cells t x t, t x 2t, 2t x t), each placed with step 4, x outer and y inner.
void hog_catalog(int W, int H, std::vector<int32_t>& blocks) {
  blocks.clear();
  for (int t = 8; t <= W / 2; t += 8) {
    const int cell[3][2] = {{t, t}, {t, 2 * t}, {2 * t, t}};
    for (const auto& c : cell)
      for (int x = 0; x <= W - 2 * c[0]; x += 4)
        for (int y = 0; y <= H - 2 * c[1]; y += 4) blocks.insert(blocks.end(), {x, y, c[0], c[1]});
  }
}

// ------------------------------------------------------------------------------------------------
// Categorical split: category ordering + scan (o_cvboostree.cpp:289-357 classification, :466-515 regression).
// The accumulation over samples happened on the device; this is the O(n_cat log n_cat) remainder. std::sort with a
// plain `<` on the keys is the reference's call (LessThanPtr over pointers compares the same doubles), so categories
// with equal keys come out in the same order as there.
// ------------------------------------------------------------------------------------------------
void split_categories(const double* hist, int n_cat, bool is_classifier, bool gini, CatSplit& out) {
  const double feps = (double)FLT_EPSILON;
  out.found = false;
  out.quality = -1;
  out.n_left = 0;
  std::memset(out.subset, 0, sizeof(out.subset));
  // scratch on the stack for the usual 256 categories (8 464 calls per node search: no allocator traffic)
  constexpr int kStack = 256;
  int order_s[kStack];
  double key_s[kStack], tot_s[kStack], cnt_s[kStack];
  std::vector<int> order_v;
  std::vector<double> key_v, tot_v, cnt_v;
  int* order = order_s;
  double *key = key_s, *tot = tot_s, *cnt = cnt_s;
  if (n_cat > kStack) {
    order_v.resize((size_t)n_cat);
    key_v.resize((size_t)n_cat);
    tot_v.resize((size_t)n_cat);
    cnt_v.resize((size_t)n_cat);
    order = order_v.data();
    key = key_v.data();
    tot = tot_v.data();
    cnt = cnt_v.data();
  }
  for (int c = 0; c < n_cat; c++) order[(size_t)c] = c;
  double best = -1.0;  // init_quality of a search on its own
  int best_pos = -1;
  if (!is_classifier) {
    double right_w = 0, right_s = 0;
    for (int c = 0; c < n_cat; c++) {
      const double s = hist[2 * c], w = hist[2 * c + 1];
      right_w += w;
      right_s += s;
      cnt[(size_t)c] = w;
      key[(size_t)c] = std::fabs(w) > DBL_EPSILON ? s / w : 0;  // average response of the category
    }
    std::sort(order, order + n_cat, [&](int a, int b) { return key[(size_t)a] < key[(size_t)b]; });
    for (int c = 0; c < n_cat; c++) tot[(size_t)c] = key[(size_t)c] * cnt[(size_t)c];  // "revert back to unnormalized sums"
    double left_w = 0, left_s = 0;
    for (int pos = 0; pos < n_cat - 1; pos++) {
      const int c = order[(size_t)pos];
      const double w = cnt[(size_t)c];
      if (!(w > feps)) continue;
      const double s = tot[(size_t)c];
      left_s += s;
      left_w += w;
      right_s -= s;
      right_w -= w;
      if (left_w > feps && right_w > feps) {
        const double val = (left_s * left_s * right_w + right_s * right_s * left_w) / (left_w * right_w);
        if (best < val) {
          best = val;
          best_pos = pos;
        }
      }
    }
  } else {
    double lcw[2] = {0, 0}, rcw[2] = {0, 0};
    for (int c = 0; c < n_cat; c++) {
      rcw[0] += hist[2 * c];
      rcw[1] += hist[2 * c + 1];
      key[(size_t)c] = hist[2 * c + 1];  // weight of the category's class-1 samples
    }
    double left_w = 0, right_w = rcw[0] + rcw[1];
    std::sort(order, order + n_cat, [&](int a, int b) { return key[(size_t)a] < key[(size_t)b]; });
    for (int pos = 0; pos < n_cat - 1; pos++) {
      const int c = order[(size_t)pos];
      const double w0 = hist[2 * c], w1 = hist[2 * c + 1];
      const double weight = w0 + w1;
      if (weight < feps) continue;
      lcw[0] += w0;
      rcw[0] -= w0;
      lcw[1] += w1;
      rcw[1] -= w1;
      if (gini) {
        const double lsum2 = lcw[0] * lcw[0] + lcw[1] * lcw[1];
        const double rsum2 = rcw[0] * rcw[0] + rcw[1] * rcw[1];
        left_w += weight;
        right_w -= weight;
        if (left_w > feps && right_w > feps) {
          const double val = (lsum2 * right_w + rsum2 * left_w) / (left_w * right_w);
          if (best < val) {
            best = val;
            best_pos = pos;
          }
        }
      } else {
        const double a = lcw[0] + rcw[1], b = lcw[1] + rcw[0];
        const double val = a > b ? a : b;
        if (best < val) {
          best = val;
          best_pos = pos;
        }
      }
    }
  }
  if (best_pos < 0) return;
  out.found = true;
  out.quality = best;
  out.n_left = best_pos + 1;
  for (int pos = 0; pos <= best_pos; pos++) {
    const int c = order[(size_t)pos];
    out.subset[c >> 5] |= 1 << (c & 31);
  }
}

}  // namespace ccamd

using namespace ccamd;

extern "C" {

const char* cc_last_error(void) { return g_last_error.c_str(); }
int cc_version(void) { return 100; }

cc_status cc_scale_plan(int win_w, int win_h, int width, int height, const cc_detect_params* p, cc_scale_info* out, int cap,
                        int* n) {
  if (!p || !n) return set_error(CC_ERR_INVALID_ARG, "cc_scale_plan: null argument");
  if (!(p->scale_factor > 1.0)) return set_error(CC_ERR_INVALID_ARG, "cc_scale_plan: scaleFactor must be > 1");
  if (win_w < 3 || win_h < 3 || width < 1 || height < 1) return set_error(CC_ERR_INVALID_ARG, "cc_scale_plan: bad sizes");
  std::vector<ScaleGeom> g;
  scale_plan(win_w, win_h, width, height, *p, g);
  *n = (int)g.size();
  for (int i = 0; i < (int)g.size() && i < cap && out; i++)
    out[i] = cc_scale_info{g[i].scale, g[i].w, g[i].h, g[i].ystep, g[i].nx, g[i].ny, g[i].win_w, g[i].win_h};
  if ((int)g.size() > cap) return set_error(CC_ERR_BUFFER_TOO_SMALL, "cc_scale_plan: %zu scales, capacity %d", g.size(), cap);
  return CC_OK;
}

cc_status cc_group_rectangles(const cc_rect* rects, int n, int group_threshold, double eps, cc_rect* out, int cap,
                              int* n_out) {
  if ((n > 0 && !rects) || !n_out || n < 0) return set_error(CC_ERR_INVALID_ARG, "cc_group_rectangles: bad argument");
  std::vector<cc_rect> v(rects, rects + n);
  group_rectangles(v, group_threshold, eps);
  *n_out = (int)v.size();
  for (int i = 0; i < (int)v.size() && i < cap && out; i++) out[i] = v[i];
  if ((int)v.size() > cap) return set_error(CC_ERR_BUFFER_TOO_SMALL, "cc_group_rectangles: %zu rects, capacity %d", v.size(), cap);
  return CC_OK;
}

cc_status cc_group_rectangles_levels(const cc_rect* rects, const int32_t* levels, const double* weights, int n, int group_threshold,
                                     double eps, cc_rect* out, int32_t* out_levels, double* out_weights, int cap, int* n_out) {
  if ((n > 0 && (!rects || !levels || !weights)) || !n_out || n < 0)
    return set_error(CC_ERR_INVALID_ARG, "cc_group_rectangles_levels: bad argument");
  std::vector<cc_rect> v(rects, rects + n);
  std::vector<int> l(levels, levels + n);
  std::vector<double> w(weights, weights + n);
  group_rectangles(v, group_threshold, eps, &l, &w);
  *n_out = (int)v.size();
  for (int i = 0; i < (int)v.size() && i < cap && out && out_levels && out_weights; i++) {
    out[i] = v[(size_t)i];
    out_levels[i] = l[(size_t)i];
    out_weights[i] = w[(size_t)i];
  }
  if ((int)v.size() > cap) return set_error(CC_ERR_BUFFER_TOO_SMALL, "cc_group_rectangles_levels: %zu rects, capacity %d", v.size(), cap);
  return CC_OK;
}

}  // extern "C"
