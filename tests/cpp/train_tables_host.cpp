// Host-only parts of csrc/cc_train_device.h under AddressSanitizer + UBSan: the plain-offset catalogs (what the host
// mirror and k_eval_list read) and the node records k_predict walks, built from cascades given on the command line. Every
// offset must lie inside a window's integral and every child index inside its tree; the shared feature functions are
// run on the host over a ramp image through the records. Stand-alone (own main, no device call):
//   hipcc -x hip --offload-host-only -Xarch_host -fsanitize=address,undefined -Iinclude -Icascadeclassifier_amd/csrc \
//         tests/cpp/train_tables_host.cpp cascadeclassifier_amd/csrc/{cc_xml,cc_cascade,cc_host}.cpp
//   usage: train_tables_host <cascade.xml>...
#include <cstdio>
#include <vector>

#include "cc_train_device.h"

namespace ccamd {
bool stage_sums_order_independent(const Cascade& m, double headroom);  // cc_host.cpp (declared in cc_detect_internal.h)
}
using namespace ccamd;

static int fails = 0;
#define CHECK(c, ...)                  \
  do {                                 \
    if (!(c)) {                        \
      fails++;                         \
      std::fprintf(stderr, __VA_ARGS__); \
      std::fprintf(stderr, "\n");      \
    }                                  \
  } while (0)

static std::vector<int32_t> ramp_integral(int W, int H) {  // integral of the image px(y, x) = (3 * x + 5 * y) & 255
  std::vector<int32_t> s((size_t)(W + 1) * (H + 1), 0);
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++)
      s[(size_t)(y + 1) * (W + 1) + x + 1] = ((3 * x + 5 * y) & 255) + s[(size_t)y * (W + 1) + x + 1] + s[(size_t)(y + 1) * (W + 1) + x] - s[(size_t)y * (W + 1) + x];
  return s;
}

static void check_catalogs(int W, int H) {
  const int cols = (W + 1) * (H + 1);
  const std::vector<int32_t> s = ramp_integral(W, H);
  auto at = [&](int o) { return s[(size_t)o]; };
  for (int mode = 0; mode < 3; mode++) {
    std::vector<HaarFeature> cat;
    haar_catalog(W, H, mode, cat);
    const std::vector<HaarFeatDev> dev = haar_catalog_dev(cat, W);
    CHECK(dev.size() == cat.size(), "haar catalog %dx%d mode %d: size", W, H, mode);
    double sum = 0;
    for (size_t i = 0; i < dev.size(); i++) {
      for (int j = 0; j < 3; j++)
        for (int k = 0; k < 4; k++) CHECK(dev[i].p[j][k] >= 0 && dev[i].p[j][k] < cols, "haar %zu: offset %d outside %d", i, dev[i].p[j][k], cols);
      sum += haar_value(haar_sum(dev[i], at), 37.5f);
    }
    std::printf("haar %dx%d mode %d: %zu features, checksum %.6g\n", W, H, mode, dev.size(), sum);
  }
  std::vector<int32_t> rects;
  lbp_catalog(W, H, rects);
  const std::vector<LbpFeatDev> dev = lbp_catalog_dev(rects, W);
  CHECK(dev.size() * 4 == rects.size(), "lbp catalog %dx%d: size", W, H);
  long codes = 0;
  for (size_t i = 0; i < dev.size(); i++) {
    for (int k = 0; k < 16; k++) CHECK(dev[i].p[k] >= 0 && dev[i].p[k] < cols, "lbp %zu: offset %d outside %d", i, dev[i].p[k], cols);
    const int code = lbp_code_at(dev[i], at);
    CHECK(code >= 0 && code < 256, "lbp %zu: code %d", i, code);
    codes += code;
  }
  std::printf("lbp %dx%d: %zu features, code sum %ld\n", W, H, dev.size(), codes);
}

// children of node n of a tree with nn nodes and nl leaves stay inside it
static void check_children(const Cascade& m, size_t n, int left, int right) {
  size_t t = 0;
  while (t + 1 < m.tree_first_node.size() && (size_t)m.tree_first_node[t + 1] <= n) t++;
  const int nn = m.tree_nnodes[t];
  const int nl = (t + 1 < m.tree_first_leaf.size() ? m.tree_first_leaf[t + 1] : (int)m.leaves.size()) - m.tree_first_leaf[t];
  for (int c : {left, right}) CHECK(c > 0 ? c < nn : -c < nl, "node %zu: child %d outside its tree (%d nodes, %d leaves)", n, c, nn, nl);
}

static void check_cascade(const char* path) {
  cc_cascade* c = nullptr;
  if (cc_cascade_load_xml(path, &c) != CC_OK) {
    CHECK(false, "%s: %s", path, cc_last_error());
    return;
  }
  const Cascade& m = c->m;
  const int cols = (m.win_w + 1) * (m.win_h + 1);
  CHECK(m.stage_first.size() == m.stage_ntrees.size() && m.stage_threshold.size() == m.stage_ntrees.size(), "%s: stage tables", path);
  CHECK(m.tree_first_node.size() == m.tree_first_leaf.size(), "%s: tree tables", path);
  for (size_t s = 0; s < m.stage_ntrees.size(); s++)
    CHECK(m.stage_first[s] >= 0 && (size_t)(m.stage_first[s] + m.stage_ntrees[s]) <= m.tree_first_node.size(), "%s: stage %zu leaves the trees", path, s);
  size_t n = 0;
  if (m.feature_type == CC_FEATURE_HAAR) {
    const std::vector<HaarPredictNode> nodes = haar_predict_nodes(m);
    n = nodes.size();
    for (size_t i = 0; i < n; i++) {
      for (int j = 0; j < 3; j++)
        for (int k = 0; k < 4; k++) CHECK(nodes[i].f.p[j][k] >= 0 && nodes[i].f.p[j][k] < cols, "%s: node %zu reads offset %d", path, i, nodes[i].f.p[j][k]);
      CHECK(nodes[i].thr == m.node_threshold[i], "%s: node %zu threshold", path, i);
      check_children(m, i, nodes[i].left, nodes[i].right);
    }
  } else if (m.feature_type == CC_FEATURE_LBP) {
    const std::vector<LbpPredictNode> nodes = lbp_predict_nodes(m);
    n = nodes.size();
    for (size_t i = 0; i < n; i++) {
      for (int k = 0; k < 16; k++) CHECK(nodes[i].f.p[k] >= 0 && nodes[i].f.p[k] < cols, "%s: node %zu reads offset %d", path, i, nodes[i].f.p[k]);
      check_children(m, i, nodes[i].left, nodes[i].right);
    }
  }
  int widest = 0;
  for (int nt : m.stage_ntrees) widest = std::max(widest, nt);
  // the negative miner's choice between one wavefront and one thread per window (mine_begin, cc_negmine.hip)
  const bool wave = m.max_nodes_per_tree == 1 && stage_sums_order_independent(m, 1.0);
  std::printf("%s: %zu stages, %zu trees, %zu node records, widest stage %d, wave walk %d\n", path, m.stage_ntrees.size(),
              m.tree_first_node.size(), n, widest, wave ? 1 : 0);
  cc_cascade_destroy(c);
}

int main(int argc, char** argv) {
  check_catalogs(24, 24);
  check_catalogs(7, 5);
  for (int i = 1; i < argc; i++) check_cascade(argv[i]);
  std::printf(fails ? "FAILED: %d checks\n" : "ok\n", fails);
  return fails ? 1 : 0;
}
