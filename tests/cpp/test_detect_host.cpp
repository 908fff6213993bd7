// The detector's device-free arithmetic (cc_internal.h, defined in cc_host.cpp): how a batch is cut into passes
// (pass_sizes), how a cascade's stages are put into groups (stage_groups), and the two range proofs over a cascade's leaves
// that decide which arithmetic a kernel may use for the stage sums (stage_sums_order_independent, stage_quantum), on the
// leaf sets of tests/cascade_edges.py that sit on their bounds. Compiled with g++ against cc_host.cpp and run by
// tests/test_host_logic.py; no GPU, no HIP.
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <limits>
#include <utility>
#include <vector>

#include "cc_internal.h"

namespace ccamd {
// as in cc_detect_internal.h, which needs the HIP headers
bool stage_sums_order_independent(const Cascade& m, double headroom);
bool stage_quantum(const Cascade& m, int s, double& q);
}  // namespace ccamd

using namespace ccamd;

static int g_failures = 0;

#define CHECK(cond, ...)                                 \
  do {                                                   \
    if (!(cond)) {                                       \
      std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                          \
      std::printf("\n");                                 \
      if (++g_failures > 20) return;                     \
    }                                                    \
  } while (0)

static void print_list(const char* what, const std::vector<int>& v) {
  std::printf("%s:", what);
  for (int x : v) std::printf(" %d", x);
  std::printf("\n");
}

static void test_pass_sizes_properties() {
  for (int n = 0; n <= 130; n++)
    for (int max_batch : {1, 4, 16, 64})
      for (int passes : {1, 2, 3, 4, 7})
        for (int flags = 0; flags < 8; flags++) {
          const bool set = flags & 1, want = flags & 2, defer = flags & 4;
          const std::vector<int> s = pass_sizes(n, max_batch, passes, set, want, defer);
          long long sum = 0;
          for (int v : s) {
            sum += v;
            CHECK(v >= 1 && v <= max_batch, "size %d: n %d max_batch %d passes %d flags %d", v, n, max_batch, passes, flags);
          }
          CHECK(sum == n, "sum %lld: n %d max_batch %d passes %d flags %d", sum, n, max_batch, passes, flags);
          CHECK(n != 0 || s.empty(), "n 0 gives %zu passes", s.size());
        }
}

// What the pass loop did before pass_sizes was cut out of it, row by row.
static void test_pass_sizes_values() {
  struct Row {
    int n, max_batch, passes;
    bool set, want, defer;
    std::vector<int> sizes;
  };
  const Row rows[] = {
      {1, 64, 4, false, true, false, {1}},
      {2, 64, 4, false, true, false, {1, 1}},
      {5, 64, 4, false, true, false, {2, 2, 1}},
      {32, 64, 4, false, true, false, {10, 10, 10, 2}},
      {64, 64, 4, false, true, false, {19, 19, 19, 7}},
      {64, 64, 4, false, true, true, {32, 32}},
      {7, 64, 4, false, true, true, {4, 3}},
      {64, 64, 3, true, true, true, {26, 26, 12}},
      {64, 64, 1, true, true, false, {64}},
      {64, 16, 4, false, true, false, {16, 16, 16, 7, 9}},  // odd, and what the code has always done
      {40, 8, 4, false, true, false, {8, 8, 8, 4, 8, 4}},
      {10, 4, 4, false, false, false, {4, 4, 2}},
  };
  for (const Row& r : rows) {
    const std::vector<int> got = pass_sizes(r.n, r.max_batch, r.passes, r.set, r.want, r.defer);
    if (got != r.sizes) {
      print_list("got ", got);
      print_list("want", r.sizes);
    }
    CHECK(got == r.sizes, "n %d max_batch %d passes %d set %d want_results %d defer_last %d", r.n, r.max_batch, r.passes, (int)r.set,
          (int)r.want, (int)r.defer);
  }
}

static void check_groups(const std::vector<int32_t>& nt, int from, int budget, int dense_stage) {
  std::vector<int> gf{-7, -7, -7};  // stale contents must not survive
  int dense_from = -1;
  stage_groups(nt, from, budget, dense_stage, gf, dense_from);
  const int nst = (int)nt.size();
  CHECK(gf.size() >= 2 && gf.front() == 0 && gf.back() == nst, "ends: %zu entries, stages %d", gf.size(), nst);
  if (nst == 0) {
    CHECK(gf.size() == 2, "no stages: %zu entries", gf.size());
  } else {
    for (size_t g = 0; g + 1 < gf.size(); g++) CHECK(gf[g] < gf[g + 1], "group %zu: %d then %d", g, gf[g], gf[g + 1]);
    CHECK(gf[1] == 1, "stage 0 shares a group: group_first[1] = %d (from %d, budget %d)", gf[1], from, budget);
  }
  for (size_t g = 0; g + 1 < gf.size(); g++) {
    int sum = 0;
    for (int s = gf[g]; s < gf[g + 1]; s++) sum += nt[(size_t)s];
    const int len = gf[g + 1] - gf[g];
    if (gf[g] >= from) CHECK(len <= 1 || sum <= budget, "group %zu holds %d stumps in %d stages, budget %d", g, sum, len, budget);
    if (gf[g] < from) CHECK(len <= 1, "group %zu starts before stage %d and holds %d stages", g, from, len);
    if (budget == 0) CHECK(len <= 1, "budget 0: group %zu holds %d stages", g, len);
    // greedy: the next stage did not fit
    if (gf[g] >= from && gf[g + 1] < nst && len >= 1 && budget > 0 && sum <= budget)
      CHECK(sum + nt[(size_t)gf[g + 1]] > budget, "group %zu (%d stumps) stops before a stage of %d that fits %d", g, sum, nt[(size_t)gf[g + 1]], budget);
  }
  // dense_from: the first group >= 1 that starts at dense_stage or later; none -- and any dense_stage below 1, which asks for
  // the bank-class table everywhere -- is 0x7fffffff
  int want = 0x7fffffff;
  if (dense_stage >= 1)
    for (int g = 1; g + 1 < (int)gf.size(); g++)
      if (gf[(size_t)g] >= dense_stage) {
        want = g;
        break;
      }
  CHECK(dense_from == want, "dense_from %d, expected %d (dense_stage %d)", dense_from, want, dense_stage);
}

static void test_stage_groups() {
  const std::vector<int32_t> lbp = {3, 4, 4, 5, 5, 5, 5, 6, 7, 7, 7, 7, 8, 9, 10, 9, 9, 9, 10, 10};  // data/lbpcascade_frontalface.xml
  std::vector<std::vector<int32_t>> cascades = {{}, {5}, {1, 1, 1}, {9, 16, 27, 32, 52, 53, 62, 72, 83, 91, 99}, {3, 70, 5, 4}, lbp};
  unsigned x = 12345u;  // a few pseudo-random cascades of short and long stages
  for (int c = 0; c < 40; c++) {
    std::vector<int32_t> nt;
    const int nst = 1 + (int)((x = x * 1664525u + 1013904223u) >> 27);
    for (int s = 0; s < nst; s++) nt.push_back(1 + (int)(((x = x * 1664525u + 1013904223u) >> 16) % (c % 2 ? 12 : 40)));
    cascades.push_back(nt);
  }
  for (const auto& nt : cascades)
    for (int from : {1, 2})
      for (int budget : {0, 1, 5, 14, 20, 1000})
        for (int dense_stage : {-1, 0, 1, 2, 3, 5, 100}) check_groups(nt, from, budget, dense_stage);
  // the stock LBP cascade under the detector's defaults for it, as the code inline in cc_detector_create grouped it
  std::vector<int> gf;
  int dense_from = 0;
  stage_groups(lbp, 2, 14, 2, gf, dense_from);
  const std::vector<int> want = {0, 1, 2, 5, 7, 9, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20};
  if (gf != want) print_list("got ", gf);
  CHECK(gf == want, "stock LBP cascade: group_first");
  CHECK(dense_from == 2, "stock LBP cascade: dense_from %d", dense_from);
}

// A stump cascade of the given stages, each a list of (left, right) leaves.
using Leaves = std::vector<std::pair<float, float>>;
static Cascade cascade_of(const std::vector<Leaves>& stages) {
  Cascade m;
  m.max_nodes_per_tree = 1;
  for (const Leaves& st : stages) {
    m.stage_first.push_back((int32_t)m.stump_left.size());
    m.stage_ntrees.push_back((int32_t)st.size());
    for (const auto& lr : st) {
      m.stump_left.push_back(lr.first);
      m.stump_right.push_back(lr.second);
    }
  }
  return m;
}

static Leaves repeat(int n, float l, float r) { return Leaves((size_t)n, {l, r}); }
static Leaves operator+(Leaves a, const Leaves& b) {
  a.insert(a.end(), b.begin(), b.end());
  return a;
}

static void test_order_independence_bound() {
  const float odd = 1.f + std::ldexp(1.f, -23);  // exponent 1: q = 2^-23, so the bound 2^53 q is 2^30 and a quarter of it 2^28
  const Leaves ordinary = {{0.5f, -0.25f}, {-0.75f, 0.125f}};
  struct Row {
    const char* what;
    Leaves critical;
    bool with1, with4;
  };
  const float x27 = std::ldexp(1.f, 27), x28 = std::ldexp(1.f, 28), x29 = std::ldexp(1.f, 29);
  const Row rows[] = {
      {"sum max / q = 2^51 - 2^43 + 2^23 + 1", {{x27 - std::ldexp(1.f, 19), 0.f}, {-1.f, x27 - std::ldexp(1.f, 19)}, {odd, -1.f}}, true, true},
      {"2^51 exactly", {{x27, -x27}, {x27 - 8.f, 1.f}, {odd, -1.f}, {2.f - std::ldexp(1.f, -23), 0.f}, {5.f, -1.f}}, true, false},
      {"2^51 - 1", {{x27, -x27}, {x27 - 8.f, 1.f}, {odd, -1.f}, {2.f - std::ldexp(1.f, -22), 0.f}, {5.f, -1.f}}, true, true},
      {"2^52 + ...", {{x28, -x28}, {-x28, x28}, {odd, -odd}}, true, false},
      {"2^53 - 1", {{x29, x29}, {-(x29 - 32.f), 0.f}, {odd, -1.f}, {2.f - std::ldexp(1.f, -22), 0.f}, {29.f, -1.f}}, true, false},
      {"2^53 exactly", {{x29, x29}, {-(x29 - 32.f), 0.f}, {odd, -1.f}, {2.f - std::ldexp(1.f, -23), 0.f}, {29.f, -1.f}}, false, false},
      {"witness at the bound: 2^54 + ...", {{-x29, x29}, {1.5f, -1.5f}, {-odd, odd}, {-2.f * x29, 2.f * x29}, {x29, -x29}, {2.f * x29, 0.f}}, false, false},
      {"2^40 beside multiples of 2^-15", {{std::ldexp(1.f, 40), 0.f}, {40 * std::ldexp(1.f, -15), 22 * std::ldexp(1.f, -15)}}, false, false},
      {"a subnormal leaf: q = 2^-149, 1.0 is 2^149 q", {{std::ldexp(1.f, -149), 1.f}}, false, false},
      {"subnormal leaves alone", {{std::ldexp(1.f, -149), -std::ldexp(1.f, -140)}, {std::ldexp(3.f, -149), 0.f}}, true, true},
      {"a zero leaf does not lower q", {{0.f, x27 - 8.f}, {x27 - 8.f, -0.f}, {odd, 0.f}}, true, true},
      {"an all-zero stage", {{0.f, -0.f}, {0.f, 0.f}}, true, true},
      {"an empty stage", {}, true, true},
      {"+inf", {{std::numeric_limits<float>::infinity(), 1.f}}, false, false},
      {"-inf", {{1.f, -std::numeric_limits<float>::infinity()}}, false, false},
      {"NaN", {{std::numeric_limits<float>::quiet_NaN(), 1.f}}, false, false},
      {"largest floats: FLT_MAX / 2^104 < 2^24", {{std::numeric_limits<float>::max(), -std::numeric_limits<float>::max()}}, true, true},
  };
  for (const Row& r : rows)
    for (int where = 0; where < 3; where++) {  // the critical stage first, in the middle, last
      std::vector<Leaves> st = {ordinary, ordinary};
      st.insert(st.begin() + where, r.critical);
      const Cascade m = cascade_of(st);
      CHECK(stage_sums_order_independent(m, 1.0) == r.with1, "%s (stage %d), headroom 1", r.what, where);
      CHECK(stage_sums_order_independent(m, 4.0) == r.with4, "%s (stage %d), headroom 4", r.what, where);
    }
}

static void test_stage_quantum_bound() {
  const float below1 = 1.f - std::ldexp(1.f, -24), below2 = 1.f - std::ldexp(1.f, -23);  // exponent 0: q = 2^-24
  struct Row {
    const char* what;
    Leaves stage;
    bool ok;
    double q;
  };
  const Row rows[] = {
      {"2^31 - 2", repeat(127, 1.f, -1.f) + Leaves{{below2, -below2}}, true, std::ldexp(1.0, -24)},
      {"2^31 - 2, the larger leaf on the right", repeat(127, 0.5f, -1.f) + Leaves{{0.f, below2}}, true, std::ldexp(1.0, -24)},
      {"2^31 - 1", repeat(127, 1.f, -1.f) + Leaves{{below1, -below1}}, false, 0.},
      {"2^31", repeat(128, -1.f, 1.f) + Leaves{{0.5f, 0.f}, {0.f, -0.5f}}, false, 0.},
      {"2^31 + 2^24 - 1", repeat(128, 1.f, -1.f) + Leaves{{below1, -below1}}, false, 0.},
      {"one leaf: 2^24 - 1 quanta", {{below1, 0.f}}, true, std::ldexp(1.0, -24)},
      {"powers of two: q follows the smallest leaf", {{4.f, -2.f}, {0.f, 0.25f}}, true, std::ldexp(1.0, -25)},
      {"a subnormal leaf beside 1.0", {{std::ldexp(1.f, -149), 1.f}}, false, 0.},
      {"subnormal leaves alone", {{std::ldexp(1.f, -149), std::ldexp(5.f, -149)}}, true, std::ldexp(1.0, -172)},
      {"an all-zero stage has no quantum", {{0.f, -0.f}, {0.f, 0.f}}, false, 0.},
      {"an empty stage", {}, false, 0.},
  };
  for (const Row& r : rows) {
    const Cascade m = cascade_of({{{0.5f, -0.5f}}, r.stage, {{3.f, 1.f}}});
    double q = -1.;
    const bool ok = stage_quantum(m, 1, q);
    CHECK(ok == r.ok, "%s: got %d", r.what, (int)ok);
    if (ok && r.ok) {
      CHECK(q == r.q, "%s: q %a, expected %a", r.what, q, r.q);
      for (const auto& lr : r.stage)  // every leaf is an integer number of quanta, and they fit int32 together
        for (float v : {lr.first, lr.second}) CHECK((double)v / q == std::nearbyint((double)v / q), "%s: leaf %a is no multiple of q", r.what, (double)v);
    }
    double q0 = -1., q2 = -1.;
    CHECK(stage_quantum(m, 0, q0) && q0 == std::ldexp(1.0, -24) && stage_quantum(m, 2, q2) && q2 == std::ldexp(1.0, -23), "%s: the neighbours", r.what);
  }
}

int main() {
  test_pass_sizes_properties();
  test_pass_sizes_values();
  test_stage_groups();
  test_order_independence_bound();
  test_stage_quantum_bound();
  if (g_failures) {
    std::printf("test_detect_host: %d check(s) failed\n", g_failures);
    return 1;
  }
  std::printf("test_detect_host OK\n");
  return 0;
}
