// Host-side check of cc_cascade_from_trees, built with g++ -fsanitize=address,undefined (no HIP): cascades of trees from
// random and from hostile arguments for the three feature types; every built model is saved, loaded again and saved once
// more, and the two files must be equal. Every call must return a status without tripping a sanitizer.
//   usage: trees_host <iterations> <tmpdir>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "cascadeclassifier_amd.h"

static std::string slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  std::stringstream ss;
  ss << f.rdbuf();
  return ss.str();
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const int iters = std::atoi(argv[1]);
  const std::string path = std::string(argv[2]) + "/trees.xml", path2 = std::string(argv[2]) + "/trees_again.xml";
  std::mt19937 rng(2025);
  int built = 0, refused = 0, deep = 0;
  for (int it = 0; it < iters; it++) {
    const bool hostile = it % 3 == 2;
    const int type = (int)(rng() % 3);
    const int W = type == 2 ? 16 + 8 * (int)(rng() % 3) : 6 + (int)(rng() % 20), H = type == 2 ? 16 + 8 * (int)(rng() % 3) : 6 + (int)(rng() % 20);
    const int n_stages = 1 + (int)(rng() % 3);
    std::vector<int32_t> n_weak((size_t)n_stages), n_nodes;
    std::vector<float> thr((size_t)n_stages), leaves;
    std::vector<cc_tree_node> nodes;
    int total = 0;
    for (int s = 0; s < n_stages; s++) {
      total += n_weak[(size_t)s] = 1 + (int)(rng() % 4);
      thr[(size_t)s] = (float)((int)(rng() % 2001) - 1000) / 257.f;
    }
    for (int t = 0; t < total; t++) {
      const int nn = 1 + (int)(rng() % 5);
      n_nodes.push_back(nn);
      // the writer's layout: either the full tree of three nodes or a chain with the inner child on a random side
      const bool full = nn == 3 && (rng() & 1);
      int next_leaf = 0;
      for (int k = 0; k < nn; k++) {
        cc_tree_node nd;
        std::memset(&nd, 0, sizeof(nd));
        if (full && k == 0) {
          nd.left = 1;
          nd.right = 2;
        } else {
          const bool inner = !full && k + 1 < nn;
          const bool inner_left = rng() & 1;
          nd.left = inner && inner_left ? k + 1 : -(next_leaf++);
          nd.right = inner && !inner_left ? k + 1 : -(next_leaf++);
        }
        nd.var_idx = (int32_t)(rng() % 40);  // small windows have few variables: some of these are out of range
        nd.ord_c = (float)((int)(rng() % 2001) - 1000) / 1013.f;
        for (int j = 0; j < 8; j++) nd.subset[j] = (int32_t)rng();
        nodes.push_back(nd);
      }
      if (nn > 1) deep++;
      for (int k = 0; k < nn + 1; k++) leaves.push_back((float)((int)(rng() % 2001) - 1000) / 999.f);
    }
    int given = total, given_nodes = (int)nodes.size(), w = W, h = H, mode = (int)(rng() % 3), ftype = type;
    if (hostile) {
      cc_tree_node& victim = nodes[rng() % nodes.size()];
      switch (rng() % 9) {
        case 0: victim.var_idx = rng() & 1 ? -1 : 0x7fffffff; break;
        case 1: given = total + (rng() & 1 ? 1 : -1); break;
        case 2: n_weak[rng() % (size_t)n_stages] = rng() & 1 ? 0 : -3; break;
        case 3: w = rng() & 1 ? 2 : 5000; break;
        case 4: n_nodes[rng() % n_nodes.size()] = rng() & 1 ? 0 : -2; break;
        case 5: given_nodes += rng() & 1 ? 1 : -1; break;
        case 6: victim.left = rng() & 1 ? 0x7fffffff : (int32_t)0x80000000; break;
        case 7: victim.right = (int32_t)(rng() % 13) - 6; break;  // often a cycle, a leaf twice or past the end
        default: ftype = (int)(rng() % 7) - 2;
      }
    }
    cc_cascade* c = nullptr;
    const cc_status st = cc_cascade_from_trees(ftype, mode, w, h, n_stages, n_weak.data(), given, thr.data(), n_nodes.data(), given_nodes, nodes.data(),
                                               leaves.data(), &c);
    if (st != CC_OK) {
      if (c) return 3;
      if (!cc_last_error()[0]) return 4;  // a refusal carries a message
      refused++;
      continue;
    }
    built++;
    cc_cascade* back = nullptr;
    if (cc_cascade_save_xml(c, path.c_str()) != CC_OK || cc_cascade_load_xml(path.c_str(), &back) != CC_OK ||
        cc_cascade_save_xml(back, path2.c_str()) != CC_OK || slurp(path) != slurp(path2) || slurp(path).empty()) {
      std::fprintf(stderr, "ERROR: iteration %d: the saved cascade does not load as the built one: %s\n", it, cc_last_error());
      return 5;
    }
    cc_cascade_destroy(back);
    cc_cascade_destroy(c);
  }
  std::printf("built %d refused %d trees with more than one node %d\n", built, refused, deep);
  return built > 0 && refused > 0 && deep > 0 ? 0 : 6;
}
