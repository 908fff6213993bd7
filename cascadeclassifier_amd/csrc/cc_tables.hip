// The detector's cascade tables and creation-time settings: the stage tables and the tree / stump records in the layouts the
// kernels of cc_detect.hip read, and everything cc_detector_create derives from the cascade and the CCAMD_* knobs.
#include <algorithm>
#include <cstdlib>

#include "cc_detector.h"

namespace ccamd {

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

// The wave phase's copy of the stump table, stages with an integer form (WaveIntTables): the two leaf words of a record carry
// the leaves as int32 multiples of the stage's quantum. The copy is read by the wave phase only; `pad` is the stump's index.
static void put_integer_leaves(const Cascade& m, const WaveIntTables& t, std::vector<HaarStumpDev>& w) {
  for (size_t s = 0; s < m.stage_ntrees.size(); s++) {
    if (t.q[s] == 0.0) continue;
    for (int i = 0; i < m.stage_ntrees[s]; i++) {
      HaarStumpDev& r = w[(size_t)m.stage_first[s] + i];
      static_assert(sizeof(r.left) == sizeof(int32_t), "leaf words");
      std::memcpy(&r.left, &t.left_q[(size_t)r.pad], sizeof(int32_t));
      std::memcpy(&r.right, &t.right_q[(size_t)r.pad], sizeof(int32_t));
    }
  }
}
static bool wave_int_wanted() {
  const char* e = std::getenv("CCAMD_WAVE_INT");
  return !e || std::atoi(e) != 0;
}

// Tree nodes: the corners of the stump records (fill_haar_corners / fill_lbp_cells), children instead of leaf values.
template <int STEP>
static void build_haar_nodes(const Cascade& m, std::vector<HaarNodeDev>& out) {
  const TileGeom<STEP> G(m.win_w, m.win_h);
  out.resize(m.node_feature.size());
  for (size_t i = 0; i < out.size(); i++) {
    HaarNodeDev& d = out[i];
    std::memset(&d, 0, sizeof(d));
    fill_haar_corners(m, m.node_feature[i], d, [&](int y, int x) { return G.at(y, x); }, tile_words_padded(G.words()));
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
    fill_lbp_cells(m, m.node_feature[i], i, d, [&](int y, int x) { return G.at(y, x); });
    d.left = m.node_left[i];
    d.right = m.node_right[i];
  }
}

static int window_xy(int y, int x) { return (y << 16) | x; }  // GlobalReader records (upright features only)
static void build_haar_gstumps(const Cascade& m, std::vector<HaarStumpDev>& out) { build_haar_stumps_at(m, out, window_xy, 0); }
static void build_lbp_gstumps(const Cascade& m, std::vector<LbpStumpDev>& out) { build_lbp_stumps_at(m, out, window_xy); }

void configure_detector(cc_detector* d) {
  const bool haar = d->m.feature_type == CC_FEATURE_HAAR;
  const TileGeom<1> G1(d->m.win_w, d->m.win_h);
  const TileGeom<2> G2(d->m.win_w, d->m.win_h);
  d->lds = eval_lds_bytes(std::max(G1.words(), G2.words()), d->m.has_tilted, haar);
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
  // Haar wave phase: int32 vote sums in the stages that have a quantum. CCAMD_WAVE_INT=0: double sums in every stage (A/B runs, tests).
  d->wave_int_enabled = wave_int_wanted();
  d->wave_int = wave_int_tables(d->m, d->wave_int_enabled && haar && d->wave_below > 0);
  // Stage groups and queue form (stage_groups, where the numbers behind the defaults are): LBP stump cascades group their
  // short stages from stage 2 on, up to 14 stumps, and switch to the list queue there; everything else keeps one stage per
  // group and the bank-class table.
  const bool lbp = !haar && !trees;
  int budget = lbp ? 14 : 0;
  const int from = lbp ? 2 : 1;
  if (const char* e = std::getenv("CCAMD_GROUP_STUMPS")) budget = trees ? 0 : std::max(0, std::atoi(e));  // tuning
  int dense_stage = lbp ? 2 : -1;
  if (const char* e = std::getenv("CCAMD_DENSE_FROM")) dense_stage = std::atoi(e);
  stage_groups(d->m.stage_ntrees, from, budget, dense_stage, d->group_first, d->dense_from);
  d->n_groups = (int)d->group_first.size() - 1;
  // CCAMD_AUTO_SPECIALIZE=<stages>: build the specialised kernel in the background; detection starts on the table-driven
  // kernel and switches over when the module is ready (no change to the calling code)
  if (const char* e = std::getenv("CCAMD_AUTO_SPECIALIZE")) d->auto_specialize = std::atoi(e);
}

cc_status upload_cascade_tables(cc_detector* d) {
  const bool haar = d->m.feature_type == CC_FEATURE_HAAR;
  const bool trees = d->m.max_nodes_per_tree > 1;
  CC_HIP(d->d_stage_ntrees.upload(d->m.stage_ntrees, d->stream));
  CC_HIP(d->d_stage_first.upload(d->m.stage_first, d->stream));
  CC_HIP(d->d_stage_thr.upload(d->m.stage_threshold, d->stream));
  CC_HIP(d->d_group_first.upload(d->group_first, d->stream));
  CC_HIP(hipStreamSynchronize(d->stream));
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
      std::vector<HaarStumpDev> w1 = schedule_for_wave_phase(d->m, s1), w2 = schedule_for_wave_phase(d->m, s2);
      put_integer_leaves(d->m, d->wave_int, w1);
      put_integer_leaves(d->m, d->wave_int, w2);
      CC_HIP(d->d_haar1w.upload(w1, d->stream));
      CC_HIP(d->d_haar2w.upload(w2, d->stream));
      CC_HIP(d->d_wave_q.upload(d->wave_int.q, d->stream));
      CC_HIP(d->d_wave_thr_q.upload(d->wave_int.thr_q, d->stream));
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

}  // namespace ccamd

extern "C" cc_status cc_debug_wave_int_tables(const cc_cascade* c, double* q, int32_t* thr_q, int32_t* left_q, int32_t* right_q) {
  if (!c) return set_error(CC_ERR_INVALID_ARG, "cc_debug_wave_int_tables: null cascade");
  const WaveIntTables t = wave_int_tables(c->m, wave_int_wanted());
  if (q) std::copy(t.q.begin(), t.q.end(), q);
  if (thr_q) std::copy(t.thr_q.begin(), t.thr_q.end(), thr_q);
  if (left_q) std::copy(t.left_q.begin(), t.left_q.end(), left_q);
  if (right_q) std::copy(t.right_q.begin(), t.right_q.end(), right_q);
  return CC_OK;
}
