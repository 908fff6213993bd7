// Host-side check of cc_cascade_from_stumps, built with g++ -fsanitize=address,undefined (no HIP): cascades from random
// and from hostile arguments for the three feature types; every built model is saved, loaded again and compared. Every
// call must return a status without tripping a sanitizer.
//   usage: stumps_host <iterations> <tmpdir>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "cascadeclassifier_amd.h"

// by value: the writer prints -0.0 as "0."
static bool same_floats(const float* a, const float* b, int n) {
  for (int i = 0; i < n; i++)
    if (!(a[i] == b[i])) return false;
  return true;
}

static bool same_model(const cc_cascade* a, const cc_cascade* b) {
  cc_cascade_info ia, ib;
  if (cc_cascade_info_get(a, &ia) != CC_OK || cc_cascade_info_get(b, &ib) != CC_OK || std::memcmp(&ia, &ib, sizeof(ia)) != 0) return false;
  const int32_t *fa, *fb, *na, *nb, *sa, *sb;
  const float *ta, *tb, *la, *lb, *ra, *rb;
  cc_cascade_stages(a, &fa, &na, &ta);
  cc_cascade_stages(b, &fb, &nb, &tb);
  if (std::memcmp(na, nb, 4 * ia.n_stages) || !same_floats(ta, tb, ia.n_stages) || std::memcmp(fa, fb, 4 * ia.n_stages)) return false;
  cc_cascade_stumps(a, &fa, &ta, &la, &ra, &sa);
  cc_cascade_stumps(b, &fb, &tb, &lb, &rb, &sb);
  if (std::memcmp(fa, fb, 4 * ia.n_weak) || !same_floats(ta, tb, ia.n_weak) || !same_floats(la, lb, ia.n_weak) || !same_floats(ra, rb, ia.n_weak)) return false;
  if (ia.subset_size && std::memcmp(sa, sb, 4 * ia.n_weak * ia.subset_size)) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const int iters = std::atoi(argv[1]);
  const std::string path = std::string(argv[2]) + "/stumps.xml";
  std::mt19937 rng(2024);
  int built = 0, refused = 0;
  for (int it = 0; it < iters; it++) {
    const bool hostile = it % 3 == 2;
    const int type = hostile && rng() % 5 == 0 ? (int)(rng() % 7) - 2 : (int)(rng() % 3);
    const int W = type == 2 ? 16 + 8 * (int)(rng() % 3) : 6 + (int)(rng() % 20), H = type == 2 ? 16 + 8 * (int)(rng() % 3) : 6 + (int)(rng() % 20);
    const int n_stages = 1 + (int)(rng() % 4);
    std::vector<int32_t> n_weak((size_t)n_stages);
    int total = 0;
    for (int32_t& v : n_weak) total += v = 1 + (int)(rng() % 5);
    std::vector<float> thr((size_t)n_stages), ord((size_t)total), left((size_t)total), right((size_t)total);
    std::vector<int32_t> var((size_t)total), subsets((size_t)total * 8);
    for (float& v : thr) v = (float)((int)(rng() % 2001) - 1000) / 257.f;
    for (int t = 0; t < total; t++) {
      var[(size_t)t] = (int32_t)(rng() % 60);  // small windows have few variables: some of these are out of range
      ord[(size_t)t] = (float)((int)(rng() % 2001) - 1000) / 1013.f;
      left[(size_t)t] = (float)((int)(rng() % 2001) - 1000) / 999.f;
      right[(size_t)t] = -left[(size_t)t];
      for (int j = 0; j < 8; j++) subsets[(size_t)t * 8 + j] = (int32_t)rng();
    }
    int given = total, w = W, h = H, mode = (int)(rng() % 3);
    if (hostile) {
      switch (rng() % 6) {
        case 0: var[rng() % (size_t)total] = rng() & 1 ? -1 : 0x7fffffff; break;
        case 1: given = total + (rng() & 1 ? 1 : -1); break;
        case 2: n_weak[rng() % (size_t)n_stages] = rng() & 1 ? 0 : -3; break;
        case 3: w = rng() & 1 ? 2 : 5000; break;
        case 4: mode = 9; break;
        default: h = -1;
      }
    }
    cc_cascade* c = nullptr;
    const cc_status st = cc_cascade_from_stumps(type, mode, w, h, n_stages, n_weak.data(), given, thr.data(), var.data(), type == 1 ? nullptr : ord.data(),
                                                type == 1 ? subsets.data() : nullptr, left.data(), right.data(), &c);
    if (st != CC_OK) {
      if (c) return 3;
      if (!cc_last_error()[0]) return 4;  // a refusal carries a message
      refused++;
      continue;
    }
    built++;
    cc_cascade* back = nullptr;
    if (cc_cascade_save_xml(c, path.c_str()) != CC_OK || cc_cascade_load_xml(path.c_str(), &back) != CC_OK || !same_model(c, back)) {
      std::fprintf(stderr, "ERROR: iteration %d: the saved cascade does not load as the built one\n", it);
      return 5;
    }
    cc_cascade_destroy(back);
    cc_cascade_destroy(c);
  }
  std::printf("built %d refused %d\n", built, refused);
  return built > 0 && refused > 0 ? 0 : 6;
}
