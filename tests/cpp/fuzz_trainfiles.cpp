// Stand-alone driver for the trainer's file readers and writers (section 6d of the C ABI) under AddressSanitizer + UBSan:
// writes a params.xml and stage files of every node layout, reads them back, then reads thousands of mutated copies.
// Every call must return a status; nothing may trip a sanitizer. usage: fuzz_trainfiles <iterations> <tmpdir>
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

static void spit(const std::string& path, const std::string& text) {
  std::ofstream f(path, std::ios::binary);
  f.write(text.data(), (std::streamsize)text.size());
}

static std::string mutate(const std::string& src, std::mt19937& rng) {
  std::string s = src;
  static const char* const bits[] = {"<", ">", "</", "-", "1e999", "nan", " ", "\n", "<!--", "-->", "2147483648", "-2147483649", "<_>", "</_>", "."};
  const int edits = 1 + (int)(rng() % 4);
  for (int e = 0; e < edits && !s.empty(); e++) {
    const size_t at = rng() % s.size();
    switch (rng() % 10) {
      case 0: s[at] = (char)(rng() % 256); break;
      case 1: s.erase(at, 1 + rng() % 16); break;
      case 2: s.insert(at, bits[rng() % (sizeof(bits) / sizeof(bits[0]))]); break;
      case 3: s.resize(at); break;
      case 4: s.insert(at, s.substr(rng() % s.size(), rng() % 64)); break;
      default: {  // another number in place of a digit: the file stays XML, the trees change
        size_t d = at;
        while (d < s.size() && !(s[d] >= '0' && s[d] <= '9')) d++;
        if (d < s.size()) s.replace(d, 1, std::to_string((int)(rng() % 40) - 8));
      }
    }
  }
  return s;
}

static bool same(const cc_train_params& a, const cc_train_params& b) {
  return a.feature_type == b.feature_type && a.win_w == b.win_w && a.win_h == b.win_h && a.boost_type == b.boost_type &&
         a.min_hit_rate == b.min_hit_rate && a.max_false_alarm == b.max_false_alarm && a.weight_trim_rate == b.weight_trim_rate &&
         a.max_depth == b.max_depth && a.max_weak_count == b.max_weak_count && a.max_cat_count == b.max_cat_count &&
         a.feat_size == b.feat_size && a.haar_mode == b.haar_mode;
}

static int read_stage(const std::string& path, int max_cat, int n_vars, int* statuses) {
  float thr = 0;
  int n_weak = 0, n_total = 0;
  cc_status st = cc_stage_load_xml(path.c_str(), max_cat, n_vars, &thr, &n_weak, nullptr, 0, &n_total, nullptr, 0, nullptr);
  if (st != CC_ERR_BUFFER_TOO_SMALL) {
    statuses[st == CC_OK ? 0 : 1]++;
    return st;
  }
  std::vector<int32_t> n_nodes((size_t)n_weak);
  std::vector<cc_tree_node> nodes((size_t)n_total);
  std::vector<float> leaves((size_t)n_total + (size_t)n_weak);
  st = cc_stage_load_xml(path.c_str(), max_cat, n_vars, &thr, &n_weak, n_nodes.data(), n_weak, &n_total, nodes.data(), n_total, leaves.data());
  statuses[st == CC_OK ? 0 : 1]++;
  return st;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const int iters = std::atoi(argv[1]);
  const std::string dir = argv[2];
  std::mt19937 rng(12345);
  int fails = 0;

  // params.xml for every feature type
  std::vector<std::string> params_text;
  for (int ft = 0; ft < 3; ft++) {
    cc_train_params p = {ft, 24, 20, ft + 1, 0.995f, 0.5f, 1.0 - 1.0 / 9007199254740992.0, 2, 100, ft == 1 ? 256 : 0, ft == 2 ? 36 : 1, ft == 0 ? 2 : 0};
    cc_train_params q;
    const std::string path = dir + "/params.xml";
    if (cc_train_params_save_xml(&p, path.c_str(), nullptr) != CC_OK || cc_train_params_load_xml(path.c_str(), &q) != CC_OK || !same(p, q)) {
      std::printf("params round trip failed for feature type %d: %s\n", ft, cc_last_error());
      fails++;
    }
    params_text.push_back(slurp(path));
  }
  // stage files: stumps and a depth-3 tree, ordered and categorical
  std::vector<std::pair<std::string, int>> stage_text;
  for (int max_cat : {0, 256}) {
    const int32_t n_nodes[3] = {1, 7, 2};
    cc_tree_node nodes[10];
    std::memset(nodes, 0, sizeof(nodes));
    float leaves[13];
    for (int i = 0; i < 13; i++) leaves[i] = 0.37f * (float)i - 1.f;
    for (int i = 0; i < 10; i++) {
      nodes[i].var_idx = 17 * i;
      nodes[i].ord_c = i == 3 ? 1e-40f : -0.5f * (float)i;
      for (int w = 0; w < 8; w++) nodes[i].subset[w] = w == 0 ? INT32_MIN : w == 1 ? INT32_MAX : -w * i;
    }
    nodes[0].left = 0, nodes[0].right = -1;
    const int kids[7][2] = {{1, 2}, {3, 4}, {5, 6}, {0, -1}, {-2, -3}, {-4, -5}, {-6, -7}};
    for (int i = 0; i < 7; i++) nodes[1 + i].left = kids[i][0], nodes[1 + i].right = kids[i][1];
    nodes[8].left = 0, nodes[8].right = 1;
    nodes[9].left = -1, nodes[9].right = -2;
    const std::string path = dir + "/stage4.xml";
    int statuses[2] = {0, 0};
    if (cc_stage_save_xml(path.c_str(), nullptr, max_cat, -0.25f, 3, n_nodes, 10, nodes, leaves) != CC_OK || read_stage(path, max_cat, 17 * 9 + 1, statuses) != CC_OK) {
      std::printf("stage round trip failed for max_cat_count %d: %s\n", max_cat, cc_last_error());
      fails++;
    }
    stage_text.emplace_back(slurp(path), max_cat);
  }
  int statuses[2] = {0, 0}, p_ok = 0, p_bad = 0;
  const std::string path = dir + "/mutant.xml";
  for (int it = 0; it < iters; it++) {
    const auto& st = stage_text[(size_t)it % stage_text.size()];
    spit(path, mutate(st.first, rng));
    read_stage(path, st.second, it % 3 == 0 ? 100 : 0, statuses);
    read_stage(path, 256 - st.second, 0, statuses);  // and with the other node step
    spit(path, mutate(params_text[(size_t)it % params_text.size()], rng));
    cc_train_params q;
    (cc_train_params_load_xml(path.c_str(), &q) == CC_OK ? p_ok : p_bad)++;
    cc_cascade* c = nullptr;  // a cascade reader looking for a parameter block in the same text
    if (cc_cascade_load_xml(path.c_str(), &c) == CC_OK) cc_cascade_destroy(c);
  }
  std::printf("stages: %d read, %d refused; params: %d read, %d refused; failures %d\n", statuses[0], statuses[1], p_ok, p_bad, fails);
  return fails ? 1 : 0;
}
