// Cascade model in memory: the builders from trained stumps and trees, the C ABI accessors of section 1 of
// include/cascadeclassifier_amd.h, and what the readers and writers of trees share (cc_cascade_xml.cpp: cascade.xml;
// cc_trainfiles.cpp: the trainer's files): tokens and numbers of FileStorage text, the child-reference rule, one weak
// classifier's XML, appending a tree to a Cascade. Host code only.
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>

#include "cc_internal.h"

namespace ccamd {

void split_tokens(const std::string& s, std::vector<std::string>& out) {
  out.clear();
  size_t i = 0, n = s.size();
  while (i < n) {
    while (i < n && std::isspace((unsigned char)s[i])) i++;
    size_t j = i;
    while (j < n && !std::isspace((unsigned char)s[j])) j++;
    if (j > i) out.emplace_back(s, i, j - i);
    i = j;
  }
}

bool to_int(const std::string& t, int32_t& v) {
  errno = 0;
  char* e = nullptr;
  long long r = std::strtoll(t.c_str(), &e, 10);
  if (e == t.c_str() || errno) return false;
  if (*e == '.') {  // FileStorage writes some ints as "6." when read through a float path; accept integral reals
    double d = std::strtod(t.c_str(), &e);
    if (*e || d != std::floor(d)) return false;
    r = (long long)d;
  } else if (*e)
    return false;
  if (r < INT32_MIN || r > INT32_MAX) return false;
  v = (int32_t)r;
  return true;
}

bool to_double(const std::string& t, double& v) {
  errno = 0;
  char* e = nullptr;
  v = std::strtod(t.c_str(), &e);
  return e != t.c_str() && *e == 0;
}

bool node_int(const XmlNode* n, int32_t& v) {
  if (!n) return false;
  std::vector<std::string> tk;
  split_tokens(n->text, tk);
  return tk.size() == 1 && to_int(tk[0], v);
}

bool node_double(const XmlNode* n, double& v) {
  if (!n) return false;
  std::vector<std::string> tk;
  split_tokens(n->text, tk);
  return tk.size() == 1 && to_double(tk[0], v);
}

std::string trimmed(const std::string& s) {
  size_t a = 0, b = s.size();
  while (a < b && std::isspace((unsigned char)s[a])) a++;
  while (b > a && std::isspace((unsigned char)s[b - 1])) b--;
  return s.substr(a, b - a);
}

const char* const kFeatureNames[3] = {"HAAR", "LBP", "HOG"};
const char* const kBoostNames[4] = {"DAB", "RAB", "LB", "GAB"};
const char* const kModeNames[3] = {"BASIC", "CORE", "ALL"};

int name_index(const std::string& s, const char* const* names, int n) {
  for (int i = 0; i < n; i++)
    if (s == names[i]) return i;
  return -1;
}

static std::string real_text(double v, const char* fmt) {
  char b[64];
  if (v == (double)(long long)v && v > -1e9 && v < 1e9)
    snprintf(b, sizeof(b), "%lld.", (long long)v);
  else
    snprintf(b, sizeof(b), fmt, v);
  return b;
}
std::string real_text(float v) { return real_text((double)v, "%.8e"); }  // 8 significant digits + exponent round-trip a float
std::string real_text_d(double v) { return real_text(v, "%.16e"); }      // node values in the legacy layout, weightTrimRate

cc_status read_text_file(const char* path, std::string& text) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return set_error(CC_ERR_IO, "cannot open '%s'", path);
  std::stringstream ss;
  ss << f.rdbuf();
  text = ss.str();
  return CC_OK;
}

cc_status write_text_file(const char* path, const std::string& text) {
  std::ofstream f(path, std::ios::binary);
  if (!f) return set_error(CC_ERR_IO, "cannot open '%s' for writing", path);
  f.write(text.data(), (std::streamsize)text.size());
  if (!f) return set_error(CC_ERR_IO, "write to '%s' failed", path);
  return CC_OK;
}

// ---- trees ------------------------------------------------------------------------------------------

const char* child_ref_fault(int32_t left, int32_t right, int j, int nn) {
  if (left >= nn || right >= nn || left < -nn || right < -nn) return "lies outside the tree (child index out of range)";
  if ((left > 0 && left <= j) || (right > 0 && right <= j)) return "does not lie behind it (child index does not increase: a cycle)";
  return nullptr;
}

cc_status check_node_counts(const char* who, const int32_t* n_nodes, size_t n_trees, int n_nodes_total) {
  size_t total = 0;
  for (size_t t = 0; t < n_trees; t++) {
    const int nn = n_nodes ? n_nodes[t] : 1;
    if (nn < 1) return set_error(CC_ERR_INVALID_ARG, "%s: weak classifier %zu has %d nodes", who, t, nn);
    total += (size_t)nn;
  }
  if (n_nodes_total < 0 || total != (size_t)n_nodes_total)
    return set_error(CC_ERR_INVALID_ARG, "%s: n_nodes adds up to %zu nodes, %d were given", who, total, n_nodes_total);
  return CC_OK;
}

cc_status read_weak_xml(const XmlNode& wn, int subset_words, int feature_bound, const char* where, int t, std::vector<cc_tree_node>& nodes,
                        std::vector<float>& leaves) {
  const XmlNode* in = wn.child("internalNodes");
  const XmlNode* ln = wn.child("leafValues");
  if (!in) return set_error(CC_ERR_PARSE, "%s: weak classifier %d has no <internalNodes>", where, t);
  if (!ln) return set_error(CC_ERR_PARSE, "%s: weak classifier %d has no <leafValues>", where, t);
  const size_t step = 3 + (subset_words > 0 ? (size_t)subset_words : 1);
  std::vector<std::string> tk, lt;
  split_tokens(in->text, tk);
  if (tk.empty() || tk.size() % step)
    return set_error(CC_ERR_PARSE, "%s: <internalNodes> of weak classifier %d holds %zu numbers, no multiple of the node step %zu", where, t, tk.size(), step);
  const int nn = (int)(tk.size() / step);
  split_tokens(ln->text, lt);
  if ((int)lt.size() != nn + 1)  // upstream advances its leaf cursor by nodeCount + 1 per tree
    return set_error(CC_ERR_PARSE, "%s: <leafValues> of weak classifier %d holds %zu values, a tree of %d nodes has %d", where, t, lt.size(), nn, nn + 1);
  for (int j = 0; j < nn; j++) {
    const std::string* f = &tk[(size_t)j * step];
    cc_tree_node nd;
    std::memset(&nd, 0, sizeof(nd));
    if (!to_int(f[0], nd.left) || !to_int(f[1], nd.right) || !to_int(f[2], nd.var_idx))
      return set_error(CC_ERR_PARSE, "%s: <internalNodes> of weak classifier %d: node %d is malformed", where, t, j);
    if (const char* fault = child_ref_fault(nd.left, nd.right, j, nn))
      return set_error(CC_ERR_PARSE, "%s: <internalNodes> of weak classifier %d: a child of node %d %s", where, t, j, fault);
    if (nd.var_idx < 0 || (feature_bound > 0 && nd.var_idx >= feature_bound))
      return set_error(CC_ERR_PARSE, "%s: <internalNodes> of weak classifier %d: featureIdx %d outside [0, %d)", where, t, nd.var_idx, feature_bound);
    if (subset_words > 0) {
      for (int w = 0; w < subset_words; w++)
        if (!to_int(f[3 + w], nd.subset[w])) return set_error(CC_ERR_PARSE, "%s: <internalNodes> of weak classifier %d: malformed category subset", where, t);
    } else {
      double c = 0;
      if (!to_double(f[3], c)) return set_error(CC_ERR_PARSE, "%s: <internalNodes> of weak classifier %d: malformed threshold", where, t);
      nd.ord_c = (float)c;
    }
    nodes.push_back(nd);
  }
  for (const std::string& s : lt) {
    double v = 0;
    if (!to_double(s, v)) return set_error(CC_ERR_PARSE, "%s: <leafValues> of weak classifier %d: malformed value", where, t);
    leaves.push_back((float)v);
  }
  return CC_OK;
}

void write_weak_xml(std::ostream& o, int indent, const cc_tree_node* nodes, int nn, int subset_words, const float* leaves) {
  const std::string in((size_t)indent, ' ');
  o << in << "<_>\n" << in << "  <internalNodes>\n" << in << "   ";
  for (int j = 0; j < nn; j++) {
    o << " " << nodes[j].left << " " << nodes[j].right << " " << nodes[j].var_idx;
    if (subset_words > 0)
      for (int w = 0; w < subset_words; w++) o << " " << nodes[j].subset[w];
    else
      o << " " << real_text(nodes[j].ord_c);
  }
  o << "</internalNodes>\n" << in << "  <leafValues>\n" << in << "   ";
  for (int j = 0; j < nn + 1; j++) o << " " << real_text(leaves[j]);
  o << "</leafValues></_>\n";
}

void append_tree(Cascade& c, const cc_tree_node* nodes, int nn, const float* leaves, const int32_t* var_map) {
  c.tree_first_node.push_back((int32_t)c.node_left.size());
  c.tree_nnodes.push_back(nn);
  c.tree_first_leaf.push_back((int32_t)c.leaves.size());
  for (int j = 0; j < nn; j++) {
    const cc_tree_node& nd = nodes[j];
    c.node_left.push_back(nd.left);
    c.node_right.push_back(nd.right);
    c.node_feature.push_back(var_map ? var_map[nd.var_idx] : nd.var_idx);
    c.node_threshold.push_back(c.subset_size > 0 ? 0.f : nd.ord_c);
    for (int w = 0; w < c.subset_size; w++) c.node_subset.push_back(nd.subset[w]);
  }
  for (int j = 0; j < nn + 1; j++) c.leaves.push_back(leaves[j]);
  c.max_nodes_per_tree = std::max(c.max_nodes_per_tree, nn);
}

// Stump view, as upstream builds it: left = leafValues[0], right = leafValues[1] (the writer always emits child refs 0 / -1
// for a stump, o_cvcascadeboosttree.cpp:60-77). Tree t of one-node trees is node t with leaves 2 t and 2 t + 1.
void build_stump_view(Cascade& c) {
  if (c.max_nodes_per_tree != 1) return;
  for (size_t t = 0; t < c.node_feature.size(); t++) {
    c.stump_feature.push_back(c.node_feature[t]);
    c.stump_threshold.push_back(c.node_threshold[t]);
    c.stump_left.push_back(c.leaves[2 * t]);
    c.stump_right.push_back(c.leaves[2 * t + 1]);
  }
}

}  // namespace ccamd

using namespace ccamd;

namespace {

// The model CvCascadeClassifier::save would write (cascadeclassifier.cpp:421-456) for trees given node by node in the
// writer's order: what cc_cascade_from_stumps and cc_cascade_from_trees share, after the checks they share.
cc_status check_shape(const char* who, int feature_type, int haar_mode, int win_w, int win_h, int n_stages, const int32_t* n_weak, int n_weak_total,
                      size_t* total_out) {
  if (feature_type != CC_FEATURE_HAAR && feature_type != CC_FEATURE_LBP && feature_type != CC_FEATURE_HOG)
    return set_error(CC_ERR_INVALID_ARG, "%s: unknown feature type %d", who, feature_type);
  if (feature_type == CC_FEATURE_HAAR && (haar_mode < 0 || haar_mode > 2)) return set_error(CC_ERR_INVALID_ARG, "%s: unknown Haar mode %d", who, haar_mode);
  if (win_w < 3 || win_h < 3 || win_w > 4096 || win_h > 4096) return set_error(CC_ERR_INVALID_ARG, "%s: window %dx%d", who, win_w, win_h);
  if (n_stages < 1) return set_error(CC_ERR_INVALID_ARG, "%s: no stages", who);
  size_t total = 0;
  for (int s = 0; s < n_stages; s++) {
    if (n_weak[s] < 1) return set_error(CC_ERR_INVALID_ARG, "%s: stage %d has %d weak classifiers", who, s, n_weak[s]);
    total += (size_t)n_weak[s];
  }
  if (n_weak_total < 0 || total != (size_t)n_weak_total)
    return set_error(CC_ERR_INVALID_ARG, "%s: n_weak adds up to %zu weak classifiers, %d were given", who, total, n_weak_total);
  *total_out = total;
  return CC_OK;
}

// Arguments that passed check_shape. n_nodes == nullptr: one node per tree.
cc_status cascade_from_nodes(const char* who, int feature_type, int haar_mode, int win_w, int win_h, int n_stages, const int32_t* n_weak, size_t total,
                             const float* stage_threshold, const int32_t* n_nodes, int n_nodes_total, const cc_tree_node* nodes, const float* leaves,
                             cc_cascade** out) {
  const bool lbp = feature_type == CC_FEATURE_LBP;
  if (cc_status st = check_node_counts(who, n_nodes, total, n_nodes_total); st != CC_OK) return st;
  std::vector<HaarFeature> haar;
  std::vector<int32_t> cat;  // LBP rects [n][4] or HOG blocks [n][4]
  int n_vars = 0;
  if (feature_type == CC_FEATURE_HAAR) {
    haar_catalog(win_w, win_h, haar_mode, haar);
    n_vars = (int)haar.size();
  } else if (lbp) {
    lbp_catalog(win_w, win_h, cat);
    n_vars = (int)(cat.size() / 4);
  } else {
    hog_catalog(win_w, win_h, cat);
    n_vars = (int)(cat.size() / 4) * 36;
  }
  // markUsedFeaturesInMap (boost.cpp:566-573) over every node (markFeaturesInMap, o_cvcascadeboosttree.cpp:349-359) + the
  // numbering of CvCascadeClassifier::save (cascadeclassifier.cpp:421-437): used variables in catalog order
  std::vector<int32_t> map((size_t)n_vars, -1);
  {
    size_t k = 0;
    for (size_t t = 0; t < total; t++) {
      const int nn = n_nodes ? n_nodes[t] : 1;
      for (int j = 0; j < nn; j++, k++) {
        const cc_tree_node& nd = nodes[k];
        if (nd.var_idx < 0 || nd.var_idx >= n_vars)
          return set_error(CC_ERR_OUT_OF_RANGE, "%s: variable %d of weak classifier %zu outside the catalog (%d)", who, nd.var_idx, t, n_vars);
        if (const char* fault = child_ref_fault(nd.left, nd.right, j, nn))
          return set_error(CC_ERR_OUT_OF_RANGE, "%s: <internalNodes> of weak classifier %zu: a child of node %d %s", who, t, j, fault);
        map[(size_t)nd.var_idx] = 0;
      }
    }
  }
  std::unique_ptr<cc_cascade> c(new cc_cascade());
  Cascade& m = c->m;
  m.feature_type = feature_type;
  m.win_w = win_w;
  m.win_h = win_h;
  m.max_cat_count = lbp ? 256 : 0;
  m.subset_size = lbp ? 8 : 0;
  int next = 0;
  for (int v = 0; v < n_vars; v++) {
    if (map[(size_t)v] < 0) continue;
    map[(size_t)v] = next++;
    if (feature_type == CC_FEATURE_HAAR) {
      const HaarFeature& f = haar[(size_t)v];
      for (int j = 0; j < 3; j++) {
        for (int k = 0; k < 4; k++) m.haar_rects.push_back(f.r[j][k]);
        m.haar_weights.push_back(f.w[j]);
      }
      m.haar_tilted.push_back(f.tilted != 0);
      m.has_tilted = m.has_tilted || f.tilted != 0;
    } else if (lbp) {
      for (int k = 0; k < 4; k++) m.lbp_rects.push_back(cat[(size_t)v * 4 + k]);
    } else {
      for (int k = 0; k < 4; k++) m.hog_feats.push_back(cat[(size_t)(v / 36) * 4 + k]);
      m.hog_feats.push_back(v % 36);
    }
  }
  size_t t = 0, k = 0;
  for (int s = 0; s < n_stages; s++) {
    m.stage_first.push_back((int32_t)t);
    m.stage_ntrees.push_back(n_weak[s]);
    m.stage_threshold.push_back(stage_threshold[s] - 1e-5f);  // THRESHOLD_EPS, as the reader stores it
    for (int i = 0; i < n_weak[s]; i++, t++) {
      const int nn = n_nodes ? n_nodes[t] : 1;
      append_tree(m, nodes + k, nn, leaves + k + t, map.data());
      k += (size_t)nn;
    }
  }
  build_stump_view(m);
  *out = c.release();
  return CC_OK;
}

}  // namespace

extern "C" {

void cc_cascade_destroy(cc_cascade* c) { delete c; }

cc_status cc_cascade_from_stumps(int feature_type, int haar_mode, int win_w, int win_h, int n_stages, const int32_t* n_weak,
                                 int n_weak_total, const float* stage_threshold, const int32_t* var_idx, const float* ord_c, const int32_t* subsets,
                                 const float* left, const float* right, cc_cascade** out) {
  const char* who = "cc_cascade_from_stumps";
  if (!out) return set_error(CC_ERR_INVALID_ARG, "%s: null argument", who);
  *out = nullptr;
  if (!n_weak || !stage_threshold || !var_idx || !left || !right) return set_error(CC_ERR_INVALID_ARG, "%s: null argument", who);
  size_t total = 0;
  if (cc_status st = check_shape(who, feature_type, haar_mode, win_w, win_h, n_stages, n_weak, n_weak_total, &total); st != CC_OK) return st;
  const bool lbp = feature_type == CC_FEATURE_LBP;
  if (lbp ? !subsets : !ord_c) return set_error(CC_ERR_INVALID_ARG, "%s: %s", who, lbp ? "subsets required for LBP" : "ord_c required for HAAR / HOG");
  // a stump is the tree of one node with the writer's child references 0 / -1 (o_cvcascadeboosttree.cpp:60-77)
  std::vector<cc_tree_node> nodes(total);
  std::vector<float> leaves(2 * total);
  for (size_t t = 0; t < total; t++) {
    cc_tree_node& nd = nodes[t];
    std::memset(&nd, 0, sizeof(nd));
    nd.right = -1;
    nd.var_idx = var_idx[t];
    if (ord_c) nd.ord_c = ord_c[t];
    if (subsets) std::memcpy(nd.subset, subsets + t * 8, sizeof(nd.subset));
    leaves[2 * t] = left[t];
    leaves[2 * t + 1] = right[t];
  }
  return cascade_from_nodes(who, feature_type, haar_mode, win_w, win_h, n_stages, n_weak, total, stage_threshold, nullptr, n_weak_total, nodes.data(),
                            leaves.data(), out);
}

cc_status cc_cascade_from_trees(int feature_type, int haar_mode, int win_w, int win_h, int n_stages, const int32_t* n_weak, int n_weak_total,
                                const float* stage_threshold, const int32_t* n_nodes, int n_nodes_total, const cc_tree_node* nodes, const float* leaves,
                                cc_cascade** out) {
  const char* who = "cc_cascade_from_trees";
  if (!out) return set_error(CC_ERR_INVALID_ARG, "%s: null argument", who);
  *out = nullptr;
  if (!n_weak || !stage_threshold || !n_nodes || !nodes || !leaves) return set_error(CC_ERR_INVALID_ARG, "%s: null argument", who);
  size_t total = 0;
  if (cc_status st = check_shape(who, feature_type, haar_mode, win_w, win_h, n_stages, n_weak, n_weak_total, &total); st != CC_OK) return st;
  return cascade_from_nodes(who, feature_type, haar_mode, win_w, win_h, n_stages, n_weak, total, stage_threshold, n_nodes, n_nodes_total, nodes, leaves, out);
}

cc_status cc_cascade_info_get(const cc_cascade* c, cc_cascade_info* info) {
  if (!c || !info) return set_error(CC_ERR_INVALID_ARG, "cc_cascade_info_get: null argument");
  const Cascade& m = c->m;
  info->feature_type = m.feature_type;
  info->win_w = m.win_w;
  info->win_h = m.win_h;
  info->n_stages = (int32_t)m.stage_ntrees.size();
  info->n_weak = (int32_t)m.tree_first_node.size();
  info->n_nodes = (int32_t)m.node_left.size();
  info->n_leaves = (int32_t)m.leaves.size();
  info->n_features = m.n_features();
  info->max_cat_count = m.max_cat_count;
  info->subset_size = m.subset_size;
  info->max_nodes_per_tree = m.max_nodes_per_tree;
  info->has_tilted = m.has_tilted ? 1 : 0;
  return CC_OK;
}

cc_status cc_cascade_stages(const cc_cascade* c, const int32_t** first_weak, const int32_t** n_weak, const float** threshold) {
  if (!c) return set_error(CC_ERR_INVALID_ARG, "cc_cascade_stages: null cascade");
  if (first_weak) *first_weak = c->m.stage_first.data();
  if (n_weak) *n_weak = c->m.stage_ntrees.data();
  if (threshold) *threshold = c->m.stage_threshold.data();
  return CC_OK;
}

cc_status cc_cascade_stumps(const cc_cascade* c, const int32_t** feature_idx, const float** threshold, const float** left,
                            const float** right, const int32_t** subsets) {
  if (!c) return set_error(CC_ERR_INVALID_ARG, "cc_cascade_stumps: null cascade");
  if (c->m.max_nodes_per_tree != 1) return set_error(CC_ERR_UNSUPPORTED, "cc_cascade_stumps: cascade has trees deeper than stumps");
  if (feature_idx) *feature_idx = c->m.stump_feature.data();
  if (threshold) *threshold = c->m.stump_threshold.data();
  if (left) *left = c->m.stump_left.data();
  if (right) *right = c->m.stump_right.data();
  if (subsets) *subsets = c->m.subset_size ? c->m.node_subset.data() : nullptr;
  return CC_OK;
}

cc_status cc_cascade_features(const cc_cascade* c, const int32_t** rects, const float** weights, const int32_t** tilted) {
  if (!c) return set_error(CC_ERR_INVALID_ARG, "cc_cascade_features: null cascade");
  const Cascade& m = c->m;
  const bool haar = m.feature_type == CC_FEATURE_HAAR;
  if (rects) *rects = haar ? m.haar_rects.data() : m.feature_type == CC_FEATURE_HOG ? m.hog_feats.data() : m.lbp_rects.data();
  if (weights) *weights = haar ? m.haar_weights.data() : nullptr;
  if (tilted) *tilted = haar ? m.haar_tilted.data() : nullptr;
  return CC_OK;
}

}  // extern "C"
