// Cascade model: reader of the new-format cascade.xml (the format CvCascadeClassifier::save writes,
// traincascade/lib/src/cascadeclassifier.cpp:439-456 with the tags of cascadeclassifier.h:27-73) and the
// C ABI accessors of section 1 of include/cascadeclassifier_amd.h. Host code only.
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>

#include "cc_internal.h"

namespace ccamd {
namespace {

bool split_tokens(const std::string& s, std::vector<std::string>& out) {
  out.clear();
  size_t i = 0, n = s.size();
  while (i < n) {
    while (i < n && std::isspace((unsigned char)s[i])) i++;
    size_t j = i;
    while (j < n && !std::isspace((unsigned char)s[j])) j++;
    if (j > i) out.emplace_back(s, i, j - i);
    i = j;
  }
  return true;
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

// a string value: FileStorage quotes one that would not read back as a string otherwise
std::string string_value(const XmlNode* n) {
  std::string s = n ? trimmed(n->text) : std::string();
  if (s.size() >= 2 && s.front() == '"' && s.back() == '"') s = s.substr(1, s.size() - 2);
  return s;
}

const char* const kFeatureNames[3] = {"HAAR", "LBP", "HOG"};
const char* const kBoostNames[4] = {"DAB", "RAB", "LB", "GAB"};  // CvBoost's DISCRETE, REAL, LOGIT, GENTLE
const char* const kModeNames[3] = {"BASIC", "CORE", "ALL"};

int name_index(const std::string& s, const char* const* names, int n) {
  for (int i = 0; i < n; i++)
    if (s == names[i]) return i;
  return -1;
}

// The parameter block of a params.xml or a cascade.xml with the checks of CvCascadeParams::read (cascadeclassifier.cpp:48-73),
// CvCascadeBoostParams::read (boost.cpp:73-95), CvFeatureParams::read (features.cpp:53-60) and CvHaarFeatureParams::read
// (haarfeatures.cpp:38-52). `where` starts every message (the file's name).
cc_status train_params_from_xml(const XmlNode& b, const char* where, cc_train_params& p) {
  std::memset(&p, 0, sizeof(p));
  if (string_value(b.child("stageType")) != "BOOST") return set_error(CC_ERR_PARSE, "%s: <stageType> must be BOOST", where);
  p.feature_type = name_index(string_value(b.child("featureType")), kFeatureNames, 3);
  if (p.feature_type < 0) return set_error(CC_ERR_PARSE, "%s: <featureType> must be HAAR, LBP or HOG", where);
  if (!node_int(b.child("height"), p.win_h) || p.win_h <= 0) return set_error(CC_ERR_PARSE, "%s: <height> must be a positive integer", where);
  if (!node_int(b.child("width"), p.win_w) || p.win_w <= 0) return set_error(CC_ERR_PARSE, "%s: <width> must be a positive integer", where);
  const XmlNode* sp = b.child("stageParams");
  if (!sp) return set_error(CC_ERR_PARSE, "%s: <stageParams> is missing", where);
  if (!sp->child("boostType"))
    return set_error(CC_ERR_NO_TRAIN_PARAMS, "%s: no training parameters (<stageParams> has no <boostType>)", where);
  p.boost_type = name_index(string_value(sp->child("boostType")), kBoostNames, 4);
  if (p.boost_type < 0) return set_error(CC_ERR_PARSE, "%s: <boostType> must be DAB, RAB, LB or GAB (unsupported Boost type)", where);
  double hit = 0, fa = 0, trim = 0;
  if (!node_double(sp->child("minHitRate"), hit) || !((float)hit > 0 && (float)hit <= 1))
    return set_error(CC_ERR_PARSE, "%s: <minHitRate> must lie in (0, 1] (bad parameters range)", where);
  if (!node_double(sp->child("maxFalseAlarm"), fa) || !((float)fa > 0 && (float)fa <= 1))
    return set_error(CC_ERR_PARSE, "%s: <maxFalseAlarm> must lie in (0, 1] (bad parameters range)", where);
  if (!node_double(sp->child("weightTrimRate"), trim) || !(trim > 0 && trim <= 1))
    return set_error(CC_ERR_PARSE, "%s: <weightTrimRate> must lie in (0, 1] (bad parameters range)", where);
  p.min_hit_rate = (float)hit;
  p.max_false_alarm = (float)fa;
  p.weight_trim_rate = trim;
  if (!node_int(sp->child("maxDepth"), p.max_depth) || p.max_depth <= 0)
    return set_error(CC_ERR_PARSE, "%s: <maxDepth> must be a positive integer (bad parameters range)", where);
  if (!node_int(sp->child("maxWeakCount"), p.max_weak_count) || p.max_weak_count <= 0)
    return set_error(CC_ERR_PARSE, "%s: <maxWeakCount> must be a positive integer (bad parameters range)", where);
  const XmlNode* fp = b.child("featureParams");
  if (!fp) fp = b.child("featuhreParams");  // historical typo carried by some stock files
  if (!fp) return set_error(CC_ERR_PARSE, "%s: <featureParams> is missing", where);
  p.max_cat_count = p.feature_type == CC_FEATURE_LBP ? 256 : 0;
  p.feat_size = p.feature_type == CC_FEATURE_HOG ? 36 : 1;
  if (fp->child("maxCatCount") && (!node_int(fp->child("maxCatCount"), p.max_cat_count) || p.max_cat_count < 0))
    return set_error(CC_ERR_PARSE, "%s: <maxCatCount> must be an integer >= 0", where);
  if (fp->child("featSize") && (!node_int(fp->child("featSize"), p.feat_size) || p.feat_size < 1))
    return set_error(CC_ERR_PARSE, "%s: <featSize> must be an integer >= 1", where);
  if (p.feature_type == CC_FEATURE_HAAR) {
    p.haar_mode = name_index(string_value(fp->child("mode")), kModeNames, 3);
    if (p.haar_mode < 0) return set_error(CC_ERR_PARSE, "%s: <mode> must be BASIC, CORE or ALL", where);
  }
  return CC_OK;
}

// the object under <opencv_storage> (FileStorage::getFirstTopLevelNode), or the root itself
const XmlNode* first_top_level(const XmlNode& root) {
  if (root.name != "opencv_storage") return &root;
  return root.children.empty() ? nullptr : &root.children[0];
}

}  // namespace

cc_status cascade_from_xml(const XmlNode& root, Cascade& c) {
  const XmlNode* casc = nullptr;
  if (root.name == "opencv_storage") {
    casc = root.child("cascade");
    if (!casc && !root.children.empty()) casc = &root.children[0];
  } else
    casc = &root;
  if (!casc) return set_error(CC_ERR_PARSE, "cascade XML: <opencv_storage> has no cascade node");
  const XmlNode* st = casc->child("stageType");
  if (!st) {
    if (casc->child("size") || casc->child("stages"))
      return set_error(CC_ERR_UNSUPPORTED,
                       "cascade XML: old-format (opencv-haar-classifier) cascade; only the new format written by "
                       "traincascade is supported");
    return set_error(CC_ERR_PARSE, "cascade XML: missing <stageType>");
  }
  if (trimmed(st->text) != "BOOST") return set_error(CC_ERR_PARSE, "cascade XML: stageType must be BOOST");
  const XmlNode* ft = casc->child("featureType");
  if (!ft) return set_error(CC_ERR_PARSE, "cascade XML: missing <featureType>");
  std::string fts = trimmed(ft->text);
  if (fts == "HAAR")
    c.feature_type = CC_FEATURE_HAAR;
  else if (fts == "LBP")
    c.feature_type = CC_FEATURE_LBP;
  else if (fts == "HOG")
    c.feature_type = CC_FEATURE_HOG;
  else
    return set_error(CC_ERR_PARSE, "cascade XML: unknown featureType '%s'", fts.c_str());
  int32_t w = 0, h = 0;
  if (!node_int(casc->child("width"), w) || !node_int(casc->child("height"), h) || w < 3 || h < 3 || w > 4096 || h > 4096)
    return set_error(CC_ERR_PARSE, "cascade XML: bad <width>/<height>");
  c.win_w = w;
  c.win_h = h;
  const XmlNode* fp = casc->child("featureParams");
  if (!fp) fp = casc->child("featuhreParams");  // historical typo carried by some stock files
  int32_t maxcat = c.feature_type == CC_FEATURE_LBP ? 256 : 0;
  if (fp && fp->child("maxCatCount") && !node_int(fp->child("maxCatCount"), maxcat))
    return set_error(CC_ERR_PARSE, "cascade XML: bad <maxCatCount>");
  if (maxcat < 0 || maxcat > 256 || (c.feature_type == CC_FEATURE_LBP && maxcat != 256) ||
      (c.feature_type == CC_FEATURE_HAAR && maxcat != 0))
    return set_error(CC_ERR_PARSE, "cascade XML: maxCatCount %d does not match featureType %s", maxcat, fts.c_str());
  if (c.feature_type == CC_FEATURE_HOG) {  // a HOG variable is one of N_BINS * N_CELLS components (HOGfeatures.cpp:9-14)
    if (maxcat != 0) return set_error(CC_ERR_PARSE, "cascade XML: maxCatCount %d does not match featureType HOG", maxcat);
    int32_t fs = 36;
    if (fp && fp->child("featSize") && !node_int(fp->child("featSize"), fs)) return set_error(CC_ERR_PARSE, "cascade XML: bad <featSize>");
    if (fs != 36) return set_error(CC_ERR_PARSE, "cascade XML: featSize %d does not match featureType HOG (36)", fs);
  }
  c.max_cat_count = maxcat;
  c.subset_size = maxcat > 0 ? (maxcat + 31) / 32 : 0;
  const int node_step = 3 + (maxcat > 0 ? c.subset_size : 1);

  // ---- features first (stage nodes are validated against their count)
  const XmlNode* feats = casc->child("features");
  if (!feats) return set_error(CC_ERR_PARSE, "cascade XML: missing <features>");
  std::vector<std::string> tk;
  for (const XmlNode& f : feats->children) {
    if (f.name != "_") continue;
    if (c.feature_type == CC_FEATURE_HAAR) {
      const XmlNode* rects = f.child("rects");
      if (!rects) return set_error(CC_ERR_PARSE, "cascade XML: Haar feature without <rects>");
      int32_t r[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
      float wt[3] = {0, 0, 0};
      int ri = 0;
      int32_t tilted = 0;
      if (f.child("tilted") && !node_int(f.child("tilted"), tilted)) return set_error(CC_ERR_PARSE, "cascade XML: bad <tilted>");
      tilted = tilted != 0;
      for (const XmlNode& rn : rects->children) {
        if (rn.name != "_") continue;
        if (ri >= 3) return set_error(CC_ERR_PARSE, "cascade XML: more than 3 rects in a Haar feature");
        split_tokens(rn.text, tk);
        double wd = 0;
        if (tk.size() != 5 || !to_int(tk[0], r[ri][0]) || !to_int(tk[1], r[ri][1]) || !to_int(tk[2], r[ri][2]) ||
            !to_int(tk[3], r[ri][3]) || !to_double(tk[4], wd))
          return set_error(CC_ERR_PARSE, "cascade XML: malformed Haar rect '%s'", rn.text.c_str());
        wt[ri] = (float)wd;
        // every integral entry the rect touches must lie inside the (W+1)x(H+1) window integral
        const int x = r[ri][0], y = r[ri][1], rw = r[ri][2], rh = r[ri][3];
        bool ok = rw >= 0 && rh >= 0 && x >= 0 && y >= 0;
        if (!tilted)
          ok = ok && x + rw <= w && y + rh <= h;
        else
          ok = ok && x - rh >= 0 && x + rw <= w && y + rw + rh <= h;
        if (!ok)
          return set_error(CC_ERR_PARSE, "cascade XML: Haar rect (%d %d %d %d%s) leaves the %dx%d window", x, y, rw, rh,
                           tilted ? " tilted" : "", w, h);
        ri++;
      }
      if (ri < 1) return set_error(CC_ERR_PARSE, "cascade XML: Haar feature with no rect");
      for (int j = 0; j < 3; j++) {
        for (int k = 0; k < 4; k++) c.haar_rects.push_back(r[j][k]);
        c.haar_weights.push_back(wt[j]);
      }
      c.haar_tilted.push_back(tilted);
      c.has_tilted = c.has_tilted || tilted;
    } else if (c.feature_type == CC_FEATURE_LBP) {
      const XmlNode* rn = f.child("rect");
      int32_t r[4];
      if (!rn) return set_error(CC_ERR_PARSE, "cascade XML: LBP feature without <rect>");
      split_tokens(rn->text, tk);
      if (tk.size() != 4 || !to_int(tk[0], r[0]) || !to_int(tk[1], r[1]) || !to_int(tk[2], r[2]) || !to_int(tk[3], r[3]))
        return set_error(CC_ERR_PARSE, "cascade XML: malformed LBP rect '%s'", rn->text.c_str());
      if (r[0] < 0 || r[1] < 0 || r[2] < 1 || r[3] < 1 || r[0] + 3 * r[2] > w || r[1] + 3 * r[3] > h)
        return set_error(CC_ERR_PARSE, "cascade XML: LBP rect (%d %d %d %d) leaves the %dx%d window", r[0], r[1], r[2], r[3], w, h);
      for (int k = 0; k < 4; k++) c.lbp_rects.push_back(r[k]);
    } else {
      // HOG: cell 0 of the block and the component (HOGfeatures.cpp:155-160); the block is 2 x 2 cells
      const XmlNode* rn = f.child("rect");
      int32_t r[5];
      if (!rn) return set_error(CC_ERR_PARSE, "cascade XML: HOG feature without <rect>");
      split_tokens(rn->text, tk);
      if (tk.size() != 5 || !to_int(tk[0], r[0]) || !to_int(tk[1], r[1]) || !to_int(tk[2], r[2]) || !to_int(tk[3], r[3]) ||
          !to_int(tk[4], r[4]))
        return set_error(CC_ERR_PARSE, "cascade XML: malformed HOG rect '%s'", rn->text.c_str());
      if (r[4] < 0 || r[4] >= 36) return set_error(CC_ERR_PARSE, "cascade XML: HOG component %d outside [0, 36)", r[4]);
      // the device kernels index the window's planes with these numbers: the whole block must lie inside the window
      if (r[0] < 0 || r[1] < 0 || r[2] < 1 || r[3] < 1 || r[2] > w || r[3] > h || r[0] + 2 * r[2] > w || r[1] + 2 * r[3] > h)
        return set_error(CC_ERR_PARSE, "cascade XML: HOG block of cell (%d %d %d %d) leaves the %dx%d window", r[0], r[1], r[2], r[3], w, h);
      for (int k = 0; k < 5; k++) c.hog_feats.push_back(r[k]);
    }
  }
  const int nfeat = c.n_features();
  if (nfeat == 0) return set_error(CC_ERR_PARSE, "cascade XML: empty <features>");

  // ---- stages
  const XmlNode* stages = casc->child("stages");
  if (!stages) return set_error(CC_ERR_PARSE, "cascade XML: missing <stages>");
  c.max_nodes_per_tree = 0;
  for (const XmlNode& sn : stages->children) {
    if (sn.name != "_") continue;
    double thr = 0;
    if (!node_double(sn.child("stageThreshold"), thr)) return set_error(CC_ERR_PARSE, "cascade XML: bad <stageThreshold>");
    const XmlNode* weak = sn.child("weakClassifiers");
    if (!weak) return set_error(CC_ERR_PARSE, "cascade XML: stage without <weakClassifiers>");
    c.stage_first.push_back((int32_t)c.tree_first_node.size());
    c.stage_threshold.push_back((float)thr - 1e-5f);  // THRESHOLD_EPS
    int ntrees = 0;
    for (const XmlNode& wn : weak->children) {
      if (wn.name != "_") continue;
      const XmlNode* in = wn.child("internalNodes");
      const XmlNode* lv = wn.child("leafValues");
      if (!in || !lv) return set_error(CC_ERR_PARSE, "cascade XML: weak classifier without internalNodes/leafValues");
      split_tokens(in->text, tk);
      if (tk.empty() || tk.size() % node_step) return set_error(CC_ERR_PARSE, "cascade XML: internalNodes length %zu is not a multiple of %d", tk.size(), node_step);
      const int nn = (int)tk.size() / node_step;
      std::vector<std::string> lt;
      split_tokens(lv->text, lt);
      const int nl = (int)lt.size();
      if (nl != nn + 1)  // upstream advances its leaf cursor by nodeCount + 1 per tree
        return set_error(CC_ERR_PARSE, "cascade XML: a tree with %d nodes must have %d leaf values (found %d)", nn, nn + 1, nl);
      c.tree_first_node.push_back((int32_t)c.node_left.size());
      c.tree_nnodes.push_back(nn);
      c.tree_first_leaf.push_back((int32_t)c.leaves.size());
      for (int k = 0; k < nn; k++) {
        const std::string* t = &tk[(size_t)k * node_step];
        int32_t l, r, fi;
        if (!to_int(t[0], l) || !to_int(t[1], r) || !to_int(t[2], fi)) return set_error(CC_ERR_PARSE, "cascade XML: malformed internalNodes");
        // child > 0: internal node index inside this tree; child <= 0: leaf index -child
        if (l >= nn || r >= nn || -l >= nl || -r >= nl) return set_error(CC_ERR_PARSE, "cascade XML: tree child index out of range");
        // the writer numbers internal nodes breadth-first, so a child's index exceeds its parent's; insisting on it
        // guarantees that walking the tree terminates (a cyclic file would otherwise hang a kernel)
        if ((l > 0 && l <= k) || (r > 0 && r <= k)) return set_error(CC_ERR_PARSE, "cascade XML: tree child index does not increase (cycle)");
        if (fi < 0 || fi >= nfeat) return set_error(CC_ERR_PARSE, "cascade XML: featureIdx %d out of range (features: %d)", fi, nfeat);
        c.node_left.push_back(l);
        c.node_right.push_back(r);
        c.node_feature.push_back(fi);
        if (c.subset_size > 0) {
          for (int j = 0; j < c.subset_size; j++) {
            int32_t sw;
            if (!to_int(t[3 + j], sw)) return set_error(CC_ERR_PARSE, "cascade XML: malformed category subset");
            c.node_subset.push_back(sw);
          }
          c.node_threshold.push_back(0.f);
        } else {
          double td;
          if (!to_double(t[3], td)) return set_error(CC_ERR_PARSE, "cascade XML: malformed node threshold");
          c.node_threshold.push_back((float)td);
        }
      }
      for (int k = 0; k < nl; k++) {
        double v;
        if (!to_double(lt[k], v)) return set_error(CC_ERR_PARSE, "cascade XML: malformed leaf value");
        c.leaves.push_back((float)v);
      }
      if (nn > c.max_nodes_per_tree) c.max_nodes_per_tree = nn;
      ntrees++;
    }
    if (ntrees == 0) return set_error(CC_ERR_PARSE, "cascade XML: stage with no weak classifier");
    c.stage_ntrees.push_back(ntrees);
  }
  if (c.stage_ntrees.empty()) return set_error(CC_ERR_PARSE, "cascade XML: no stages");

  if (c.max_nodes_per_tree == 1) {
    // Stump view, as upstream builds it: left = leafValues[0], right = leafValues[1] (the writer always emits child
    // refs 0 / -1 for a stump, o_cvcascadeboosttree.cpp:60-77); two leaves per stump are required.
    const size_t nt = c.tree_first_node.size();
    for (size_t t = 0; t < nt; t++) {
      const int n0 = c.tree_first_node[t], l0 = c.tree_first_leaf[t];
      const int nl = (t + 1 < nt ? c.tree_first_leaf[t + 1] : (int)c.leaves.size()) - l0;
      if (nl != 2) return set_error(CC_ERR_PARSE, "cascade XML: stump %zu has %d leaf values (expected 2)", t, nl);
      c.stump_feature.push_back(c.node_feature[n0]);
      c.stump_threshold.push_back(c.node_threshold[n0]);
      c.stump_left.push_back(c.leaves[l0]);
      c.stump_right.push_back(c.leaves[l0 + 1]);
    }
  }
  // the training parameters, where the file holds a whole block that passes the trainer's checks; the model does not depend on them
  cc_train_params tp;
  if (train_params_from_xml(*casc, "cascade XML", tp) == CC_OK && tp.feature_type == c.feature_type && tp.win_w == c.win_w && tp.win_h == c.win_h) {
    c.has_train_params = true;
    c.train_params = tp;
  }
  return CC_OK;
}

}  // namespace ccamd

using namespace ccamd;

namespace {
// FileStorage prints float reals with "%.8e" and integral reals as "2." (8 significant digits + exponent round-trip a float)
std::string real_text(float v) {
  char b[64];
  if (v == (float)(long long)v && v > -1e9f && v < 1e9f)
    snprintf(b, sizeof(b), "%lld.", (long long)v);
  else
    snprintf(b, sizeof(b), "%.8e", (double)v);
  return b;
}
// doubles (node values in the legacy layout) go out with "%.16e"
std::string real_text_d(double v) {
  char b[64];
  if (v == (double)(long long)v && v > -1e9 && v < 1e9)
    snprintf(b, sizeof(b), "%lld.", (long long)v);
  else
    snprintf(b, sizeof(b), "%.16e", v);
  return b;
}
// the raw <stageThreshold> whose (float)t - 1e-5f is the stored value; false if no float maps onto it
bool stage_threshold_preimage(float stored, float& t) {
  t = stored + 1e-5f;
  for (int k = 0; k < 64 && (float)(t - 1e-5f) != stored; k++) t = (float)(t - 1e-5f) < stored ? std::nextafterf(t, INFINITY) : std::nextafterf(t, -INFINITY);
  return (float)(t - 1e-5f) == stored;
}
cc_status write_text_file(const char* path, const std::string& text) {
  std::ofstream f(path, std::ios::binary);
  if (!f) return set_error(CC_ERR_IO, "cannot open '%s' for writing", path);
  f.write(text.data(), (std::streamsize)text.size());
  if (!f) return set_error(CC_ERR_IO, "write to '%s' failed", path);
  return CC_OK;
}

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
  size_t total_nodes = 0;
  for (size_t t = 0; t < total; t++) {
    const int nn = n_nodes ? n_nodes[t] : 1;
    if (nn < 1) return set_error(CC_ERR_INVALID_ARG, "%s: weak classifier %zu has %d nodes", who, t, nn);
    total_nodes += (size_t)nn;
  }
  if (n_nodes_total < 0 || total_nodes != (size_t)n_nodes_total)
    return set_error(CC_ERR_INVALID_ARG, "%s: n_nodes adds up to %zu nodes, %d were given", who, total_nodes, n_nodes_total);
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
        // what the XML reader asks of child references (cascade_from_xml): inside the tree, and an internal child behind its parent
        if (nd.left >= nn || nd.right >= nn || nd.left < -nn || nd.right < -nn)
          return set_error(CC_ERR_OUT_OF_RANGE, "%s: child index of node %d of weak classifier %zu out of range", who, j, t);
        if ((nd.left > 0 && nd.left <= j) || (nd.right > 0 && nd.right <= j))
          return set_error(CC_ERR_OUT_OF_RANGE, "%s: child index of node %d of weak classifier %zu does not increase (cycle)", who, j, t);
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
  m.max_nodes_per_tree = 0;
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
      m.tree_first_node.push_back((int32_t)k);
      m.tree_nnodes.push_back(nn);
      m.tree_first_leaf.push_back((int32_t)(k + t));
      for (int j = 0; j < nn + 1; j++) m.leaves.push_back(leaves[k + t + (size_t)j]);
      for (int j = 0; j < nn; j++, k++) {
        const cc_tree_node& nd = nodes[k];
        m.node_left.push_back(nd.left);
        m.node_right.push_back(nd.right);
        m.node_feature.push_back(map[(size_t)nd.var_idx]);
        m.node_threshold.push_back(lbp ? 0.f : nd.ord_c);
        if (lbp)
          for (int w = 0; w < 8; w++) m.node_subset.push_back(nd.subset[w]);
      }
      m.max_nodes_per_tree = std::max(m.max_nodes_per_tree, nn);
    }
  }
  if (m.max_nodes_per_tree == 1)  // the stump view, as the reader builds it
    for (size_t i = 0; i < total; i++) {
      m.stump_feature.push_back(m.node_feature[i]);
      m.stump_threshold.push_back(m.node_threshold[i]);
      m.stump_left.push_back(m.leaves[2 * i]);
      m.stump_right.push_back(m.leaves[2 * i + 1]);
    }
  *out = c.release();
  return CC_OK;
}
cc_status parse_xml_file(const char* path, XmlNode& root) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return set_error(CC_ERR_IO, "cannot open '%s'", path);
  std::stringstream ss;
  ss << f.rdbuf();
  const std::string s = ss.str();
  std::string err;
  if (!xml_parse(s.data(), s.size(), root, err)) return set_error(CC_ERR_PARSE, "%s: %s", path, err.c_str());
  return CC_OK;
}

// FileStorage::getDefaultObjectName: the file's name without directory and extension, made an identifier
std::string default_object_name(const char* path) {
  std::string s(path);
  const size_t slash = s.find_last_of("/\\");
  if (slash != std::string::npos) s.erase(0, slash + 1);
  if (s.size() > 3 && s.compare(s.size() - 3, 3, ".gz") == 0) s.erase(s.size() - 3);
  const size_t dot = s.find_last_of('.');
  if (dot != std::string::npos) s.erase(dot);
  for (char& ch : s)
    if (!std::isalnum((unsigned char)ch) && ch != '-' && ch != '_') ch = '_';
  if (s.empty() || !(std::isalpha((unsigned char)s[0]) || s[0] == '_')) s.insert(s.begin(), '_');
  return s;
}

cc_status check_param_names(const char* who, const cc_train_params& p) {
  if (p.feature_type < 0 || p.feature_type > 2) return set_error(CC_ERR_INVALID_ARG, "%s: unknown feature type %d", who, p.feature_type);
  if (p.boost_type < 0 || p.boost_type > 3) return set_error(CC_ERR_INVALID_ARG, "%s: unknown boost type %d", who, p.boost_type);
  if (p.feature_type == CC_FEATURE_HAAR && (p.haar_mode < 0 || p.haar_mode > 2)) return set_error(CC_ERR_INVALID_ARG, "%s: unknown Haar mode %d", who, p.haar_mode);
  return CC_OK;
}

// <stageType> .. <featureParams>: CvCascadeParams::write (cascadeclassifier.cpp:33-46) and the two blocks of writeParams (:359-364),
// at the depth params.xml and cascade.xml hold them. p == nullptr: the short blocks cc_cascade_save_xml writes, from the last three arguments.
void write_params_text(std::ostringstream& o, int feature_type, int win_w, int win_h, const cc_train_params* p, int max_weak, int max_cat, int feat_size) {
  o << "  <stageType>BOOST</stageType>\n  <featureType>" << kFeatureNames[feature_type] << "</featureType>\n";
  o << "  <height>" << win_h << "</height>\n  <width>" << win_w << "</width>\n";
  o << "  <stageParams>\n";
  if (p) {  // CvCascadeBoostParams::write, boost.cpp:58-71
    o << "    <boostType>" << kBoostNames[p->boost_type] << "</boostType>\n    <minHitRate>" << real_text(p->min_hit_rate) << "</minHitRate>\n";
    o << "    <maxFalseAlarm>" << real_text(p->max_false_alarm) << "</maxFalseAlarm>\n    <weightTrimRate>" << real_text_d(p->weight_trim_rate)
      << "</weightTrimRate>\n    <maxDepth>" << p->max_depth << "</maxDepth>\n";
  }
  o << "    <maxWeakCount>" << (p ? p->max_weak_count : max_weak) << "</maxWeakCount></stageParams>\n";
  o << "  <featureParams>\n    <maxCatCount>" << (p ? p->max_cat_count : max_cat) << "</maxCatCount>\n    <featSize>" << (p ? p->feat_size : feat_size)
    << "</featSize>";
  if (p && feature_type == CC_FEATURE_HAAR) o << "\n    <mode>" << kModeNames[p->haar_mode] << "</mode>";  // haarfeatures.cpp:28-36
  o << "</featureParams>\n";
}

// cc_cascade_save_xml (p == nullptr) and cc_cascade_save_xml_params
cc_status save_cascade_xml(const char* who, const Cascade& m, const cc_train_params* p, const char* path) {
  const CNumericLocale c_numbers;  // "%.8e" / strtod must not follow the host program's LC_NUMERIC
  const bool haar = m.feature_type == CC_FEATURE_HAAR, hog = m.feature_type == CC_FEATURE_HOG;
  std::ostringstream o;
  int max_weak = 0;
  for (int n : m.stage_ntrees) max_weak = std::max(max_weak, n);
  o << "<?xml version=\"1.0\"?>\n<opencv_storage>\n<cascade>\n";
  write_params_text(o, m.feature_type, m.win_w, m.win_h, p, max_weak, m.max_cat_count, hog ? 36 : 1);
  o << "  <stageNum>" << m.stage_ntrees.size() << "</stageNum>\n  <stages>\n";
  for (size_t s = 0; s < m.stage_ntrees.size(); s++) {
    // the model keeps (float)stageThreshold - 1e-5f; write back a value that parses to the same float after the
    // reader subtracts the epsilon again: search the neighbourhood of thr + 1e-5f
    float t;
    if (!stage_threshold_preimage(m.stage_threshold[s], t)) return set_error(CC_ERR_UNSUPPORTED, "%s: stage threshold %zu has no float pre-image", who, s);
    o << "    <_>\n      <maxWeakCount>" << m.stage_ntrees[s] << "</maxWeakCount>\n      <stageThreshold>" << real_text(t)
      << "</stageThreshold>\n      <weakClassifiers>\n";
    for (int i = 0; i < m.stage_ntrees[s]; i++) {
      const size_t t_i = (size_t)m.stage_first[s] + i;
      const int n0 = m.tree_first_node[t_i], nn = m.tree_nnodes[t_i], l0 = m.tree_first_leaf[t_i];
      o << "        <_>\n          <internalNodes>\n           ";
      for (int k = 0; k < nn; k++) {
        o << " " << m.node_left[n0 + k] << " " << m.node_right[n0 + k] << " " << m.node_feature[n0 + k];
        if (m.subset_size > 0)
          for (int j = 0; j < m.subset_size; j++) o << " " << m.node_subset[(size_t)(n0 + k) * m.subset_size + j];
        else
          o << " " << real_text(m.node_threshold[n0 + k]);
      }
      o << "</internalNodes>\n          <leafValues>\n           ";
      for (int k = 0; k < nn + 1; k++) o << " " << real_text(m.leaves[l0 + k]);
      o << "</leafValues></_>\n";
    }
    o << "      </weakClassifiers></_>\n";
  }
  o << "  </stages>\n  <features>\n";
  const int nf = m.n_features();
  for (int f = 0; f < nf; f++) {
    if (haar) {
      o << "    <_>\n      <rects>\n";
      for (int j = 0; j < 3; j++) {
        const int32_t* r = &m.haar_rects[(size_t)f * 12 + j * 4];
        const float w = m.haar_weights[(size_t)f * 3 + j];
        if (j > 0 && r[2] == 0 && w == 0.0f) break;  // Feature::write stops at the first rect of zero width
        o << "        <_>\n          " << r[0] << " " << r[1] << " " << r[2] << " " << r[3] << " " << real_text(w) << "</_>\n";
      }
      o << "      </rects>\n      <tilted>" << (m.haar_tilted[f] ? 1 : 0) << "</tilted></_>\n";
    } else if (hog) {
      const int32_t* r = &m.hog_feats[(size_t)f * 5];
      o << "    <_>\n      <rect>\n        " << r[0] << " " << r[1] << " " << r[2] << " " << r[3] << " " << r[4] << "</rect></_>\n";
    } else {
      const int32_t* r = &m.lbp_rects[(size_t)f * 4];
      o << "    <_>\n      <rect>\n        " << r[0] << " " << r[1] << " " << r[2] << " " << r[3] << "</rect></_>\n";
    }
  }
  o << "  </features>\n</cascade>\n</opencv_storage>\n";
  return write_text_file(path, o.str());
}

}  // namespace

extern "C" {

cc_status cc_cascade_load_xml_mem(const char* text, size_t len, cc_cascade** out) {
  const CNumericLocale c_numbers;  // "%.8e" / strtod must not follow the host program's LC_NUMERIC
  if (!text || !out) return set_error(CC_ERR_INVALID_ARG, "cc_cascade_load_xml_mem: null argument");
  *out = nullptr;
  XmlNode root;
  std::string err;
  if (!xml_parse(text, len, root, err)) return set_error(CC_ERR_PARSE, "cascade XML: %s", err.c_str());
  cc_cascade* c = new cc_cascade();
  cc_status st = cascade_from_xml(root, c->m);
  if (st != CC_OK) {
    delete c;
    return st;
  }
  *out = c;
  return CC_OK;
}

cc_status cc_cascade_load_xml(const char* path, cc_cascade** out) {
  if (!path || !out) return set_error(CC_ERR_INVALID_ARG, "cc_cascade_load_xml: null argument");
  *out = nullptr;
  std::ifstream f(path, std::ios::binary);
  if (!f) return set_error(CC_ERR_IO, "cannot open '%s'", path);
  std::stringstream ss;
  ss << f.rdbuf();
  std::string s = ss.str();
  return cc_cascade_load_xml_mem(s.data(), s.size(), out);
}

void cc_cascade_destroy(cc_cascade* c) { delete c; }

cc_status cc_cascade_save_xml(const cc_cascade* c, const char* path) {
  if (!c || !path) return set_error(CC_ERR_INVALID_ARG, "cc_cascade_save_xml: null argument");
  return save_cascade_xml("cc_cascade_save_xml", c->m, nullptr, path);
}

cc_status cc_cascade_save_xml_params(const cc_cascade* c, const cc_train_params* p, const char* path) {
  const char* who = "cc_cascade_save_xml_params";
  if (!c || !p || !path) return set_error(CC_ERR_INVALID_ARG, "%s: null argument", who);
  if (cc_status st = check_param_names(who, *p); st != CC_OK) return st;
  if (p->feature_type != c->m.feature_type || p->win_w != c->m.win_w || p->win_h != c->m.win_h)
    return set_error(CC_ERR_INVALID_ARG, "%s: the parameters are for feature type %d and a %dx%d window, the cascade has %d and %dx%d", who,
                     p->feature_type, p->win_w, p->win_h, c->m.feature_type, c->m.win_w, c->m.win_h);
  return save_cascade_xml(who, c->m, p, path);
}

cc_status cc_cascade_train_params(const cc_cascade* c, cc_train_params* out) {
  if (!c || !out) return set_error(CC_ERR_INVALID_ARG, "cc_cascade_train_params: null argument");
  if (!c->m.has_train_params) return set_error(CC_ERR_NO_TRAIN_PARAMS, "cc_cascade_train_params: the cascade carries no training parameters");
  *out = c->m.train_params;
  return CC_OK;
}

cc_status cc_train_params_save_xml(const cc_train_params* p, const char* path, const char* object_name) {
  const CNumericLocale c_numbers;
  const char* who = "cc_train_params_save_xml";
  if (!p || !path) return set_error(CC_ERR_INVALID_ARG, "%s: null argument", who);
  if (cc_status st = check_param_names(who, *p); st != CC_OK) return st;
  const std::string name = object_name ? object_name : default_object_name(path);
  std::ostringstream o;
  o << "<?xml version=\"1.0\"?>\n<opencv_storage>\n<" << name << ">\n";
  write_params_text(o, p->feature_type, p->win_w, p->win_h, p, 0, 0, 0);
  // FileStorage closes a map on the line of its last entry
  std::string text = o.str();
  text.pop_back();
  text += "</" + name + ">\n</opencv_storage>\n";
  return write_text_file(path, text);
}

cc_status cc_train_params_load_xml(const char* path, cc_train_params* out) {
  const CNumericLocale c_numbers;
  if (!path || !out) return set_error(CC_ERR_INVALID_ARG, "cc_train_params_load_xml: null argument");
  XmlNode root;
  if (cc_status st = parse_xml_file(path, root); st != CC_OK) return st;
  const XmlNode* top = first_top_level(root);
  if (!top) return set_error(CC_ERR_PARSE, "%s: <opencv_storage> is empty", path);
  return train_params_from_xml(*top, path, *out);
}

cc_status cc_stage_save_xml(const char* path, const char* object_name, int max_cat_count, float stage_threshold, int n_weak,
                            const int32_t* n_nodes, int n_nodes_total, const cc_tree_node* nodes, const float* leaves) {
  const CNumericLocale c_numbers;
  const char* who = "cc_stage_save_xml";
  if (!path || !n_nodes || !nodes || !leaves) return set_error(CC_ERR_INVALID_ARG, "%s: null argument", who);
  if (max_cat_count < 0 || max_cat_count > 256) return set_error(CC_ERR_INVALID_ARG, "%s: max_cat_count %d outside [0, 256]", who, max_cat_count);
  if (n_weak < 1) return set_error(CC_ERR_INVALID_ARG, "%s: a stage has at least one weak classifier", who);
  const int words = (max_cat_count + 31) / 32;
  size_t total = 0;
  for (int t = 0; t < n_weak; t++) {
    if (n_nodes[t] < 1) return set_error(CC_ERR_INVALID_ARG, "%s: weak classifier %d has %d nodes", who, t, n_nodes[t]);
    total += (size_t)n_nodes[t];
  }
  if (n_nodes_total < 0 || total != (size_t)n_nodes_total)
    return set_error(CC_ERR_INVALID_ARG, "%s: n_nodes adds up to %zu nodes, %d were given", who, total, n_nodes_total);
  const std::string name = object_name ? object_name : default_object_name(path);
  std::ostringstream o;
  o << "<?xml version=\"1.0\"?>\n<opencv_storage>\n<" << name << ">\n";
  o << "  <maxWeakCount>" << n_weak << "</maxWeakCount>\n  <stageThreshold>" << real_text(stage_threshold) << "</stageThreshold>\n  <weakClassifiers>\n";
  size_t k = 0;
  for (int t = 0; t < n_weak; t++) {
    const int nn = n_nodes[t];
    o << "    <_>\n      <internalNodes>\n       ";
    for (int j = 0; j < nn; j++) {
      const cc_tree_node& nd = nodes[k + (size_t)j];
      // what the reader asks of child references: inside the tree, and an internal child behind its parent
      if (nd.left >= nn || nd.right >= nn || nd.left < -nn || nd.right < -nn || (nd.left > 0 && nd.left <= j) || (nd.right > 0 && nd.right <= j))
        return set_error(CC_ERR_OUT_OF_RANGE, "%s: child index of node %d of weak classifier %d out of range", who, j, t);
      if (nd.var_idx < 0) return set_error(CC_ERR_OUT_OF_RANGE, "%s: variable %d of weak classifier %d", who, nd.var_idx, t);
      o << " " << nd.left << " " << nd.right << " " << nd.var_idx;
      if (words > 0)
        for (int w = 0; w < words; w++) o << " " << nd.subset[w];
      else
        o << " " << real_text(nd.ord_c);
    }
    o << "</internalNodes>\n      <leafValues>\n       ";
    for (int j = 0; j < nn + 1; j++) o << " " << real_text(leaves[k + (size_t)t + (size_t)j]);
    o << "</leafValues></_>\n";
    k += (size_t)nn;
  }
  o << "  </weakClassifiers></" << name << ">\n</opencv_storage>\n";
  return write_text_file(path, o.str());
}

cc_status cc_stage_load_xml(const char* path, int max_cat_count, int n_variables, float* stage_threshold, int* n_weak, int32_t* n_nodes,
                            int weak_cap, int* n_nodes_total, cc_tree_node* nodes, int node_cap, float* leaves) {
  const CNumericLocale c_numbers;
  if (!path || !stage_threshold || !n_weak || !n_nodes_total) return set_error(CC_ERR_INVALID_ARG, "cc_stage_load_xml: null argument");
  if (max_cat_count < 0 || max_cat_count > 256) return set_error(CC_ERR_INVALID_ARG, "cc_stage_load_xml: max_cat_count %d outside [0, 256]", max_cat_count);
  *n_weak = *n_nodes_total = 0;
  XmlNode root;
  if (cc_status st = parse_xml_file(path, root); st != CC_OK) return st;
  const XmlNode* top = first_top_level(root);
  if (!top) return set_error(CC_ERR_PARSE, "%s: <opencv_storage> is empty", path);
  const int words = (max_cat_count + 31) / 32, step = 3 + (words > 0 ? words : 1);
  double thr = 0;
  if (!node_double(top->child("stageThreshold"), thr)) return set_error(CC_ERR_PARSE, "%s: bad or missing <stageThreshold>", path);
  const XmlNode* weak = top->child("weakClassifiers");
  if (!weak) return set_error(CC_ERR_PARSE, "%s: <weakClassifiers> is missing", path);
  std::vector<int32_t> counts;
  std::vector<cc_tree_node> all;
  std::vector<float> lv;
  std::vector<std::string> tk, lt;
  for (const XmlNode& wn : weak->children) {
    if (wn.name != "_") continue;
    const int t = (int)counts.size();
    const XmlNode* in = wn.child("internalNodes");
    const XmlNode* ln = wn.child("leafValues");
    if (!in) return set_error(CC_ERR_PARSE, "%s: weak classifier %d has no <internalNodes>", path, t);
    if (!ln) return set_error(CC_ERR_PARSE, "%s: weak classifier %d has no <leafValues>", path, t);
    split_tokens(in->text, tk);
    if (tk.empty() || tk.size() % (size_t)step)
      return set_error(CC_ERR_PARSE, "%s: <internalNodes> of weak classifier %d holds %zu numbers, no multiple of the node step %d", path, t, tk.size(), step);
    const int nn = (int)(tk.size() / (size_t)step);
    split_tokens(ln->text, lt);
    if ((int)lt.size() != nn + 1)
      return set_error(CC_ERR_PARSE, "%s: <leafValues> of weak classifier %d holds %zu values, a tree of %d nodes has %d", path, t, lt.size(), nn, nn + 1);
    for (int j = 0; j < nn; j++) {
      const std::string* f = &tk[(size_t)j * (size_t)step];
      cc_tree_node nd;
      std::memset(&nd, 0, sizeof(nd));
      if (!to_int(f[0], nd.left) || !to_int(f[1], nd.right) || !to_int(f[2], nd.var_idx))
        return set_error(CC_ERR_PARSE, "%s: <internalNodes> of weak classifier %d: node %d is malformed", path, t, j);
      if (nd.left >= nn || nd.right >= nn || nd.left < -nn || nd.right < -nn)
        return set_error(CC_ERR_PARSE, "%s: <internalNodes> of weak classifier %d: a child of node %d lies outside the tree", path, t, j);
      if ((nd.left > 0 && nd.left <= j) || (nd.right > 0 && nd.right <= j))
        return set_error(CC_ERR_PARSE, "%s: <internalNodes> of weak classifier %d: a child of node %d does not lie behind it (cycle)", path, t, j);
      if (nd.var_idx < 0 || (n_variables > 0 && nd.var_idx >= n_variables))
        return set_error(CC_ERR_PARSE, "%s: <internalNodes> of weak classifier %d: featureIdx %d outside [0, %d)", path, t, nd.var_idx, n_variables);
      if (words > 0) {
        for (int w = 0; w < words; w++)
          if (!to_int(f[3 + w], nd.subset[w])) return set_error(CC_ERR_PARSE, "%s: <internalNodes> of weak classifier %d: malformed category subset", path, t);
      } else {
        double c = 0;
        if (!to_double(f[3], c)) return set_error(CC_ERR_PARSE, "%s: <internalNodes> of weak classifier %d: malformed threshold", path, t);
        nd.ord_c = (float)c;
      }
      all.push_back(nd);
    }
    for (const std::string& s : lt) {
      double v = 0;
      if (!to_double(s, v)) return set_error(CC_ERR_PARSE, "%s: <leafValues> of weak classifier %d: malformed value", path, t);
      lv.push_back((float)v);
    }
    counts.push_back(nn);
  }
  if (counts.empty()) return set_error(CC_ERR_PARSE, "%s: <weakClassifiers> holds no weak classifier", path);
  *stage_threshold = (float)thr;
  *n_weak = (int)counts.size();
  *n_nodes_total = (int)all.size();
  if (!n_nodes || !nodes || !leaves || weak_cap < *n_weak || node_cap < *n_nodes_total)
    return set_error(CC_ERR_BUFFER_TOO_SMALL, "cc_stage_load_xml: %d weak classifiers with %d nodes need larger buffers", *n_weak, *n_nodes_total);
  std::copy(counts.begin(), counts.end(), n_nodes);
  std::copy(all.begin(), all.end(), nodes);
  std::copy(lv.begin(), lv.end(), leaves);
  return CC_OK;
}

cc_status cc_cascade_save_xml_legacy(const cc_cascade* c, const char* path) {
  const CNumericLocale c_numbers;  // "%.8e" / strtod must not follow the host program's LC_NUMERIC
  if (!c || !path) return set_error(CC_ERR_INVALID_ARG, "cc_cascade_save_xml_legacy: null argument");
  const Cascade& m = c->m;
  if (m.feature_type != CC_FEATURE_HAAR)
    return set_error(CC_ERR_UNSUPPORTED, "old file format is used for Haar-like features only");
  std::ostringstream o;
  o << "<?xml version=\"1.0\"?>\n<opencv_storage>\n<cascade type_id=\"opencv-haar-classifier\">\n";
  o << "  <size>\n    " << m.win_w << " " << m.win_h << "</size>\n  <stages>\n";
  for (size_t s = 0; s < m.stage_ntrees.size(); s++) {
    float thr;
    if (!stage_threshold_preimage(m.stage_threshold[s], thr))
      return set_error(CC_ERR_UNSUPPORTED, "cc_cascade_save_xml_legacy: stage threshold %zu has no float pre-image", s);
    o << "    <_>\n      <trees>\n";
    for (int i = 0; i < m.stage_ntrees[s]; i++) {
      const size_t t_i = (size_t)m.stage_first[s] + i;
      const int n0 = m.tree_first_node[t_i], l0 = m.tree_first_leaf[t_i];
      o << "        <_>\n";
      // breadth-first walk from the root; an inner child gets the next free number when it is queued
      std::vector<int> queue(1, 0);
      int next_idx = 0;
      for (size_t q = 0; q < queue.size(); q++) {
        const int k = n0 + queue[q];
        const int f = m.node_feature[k];
        o << "          <_>\n            <feature>\n              <rects>\n";
        for (int j = 0; j < 3; j++) {
          const int32_t* r = &m.haar_rects[(size_t)f * 12 + j * 4];
          const float w = m.haar_weights[(size_t)f * 3 + j];
          if (j > 0 && r[2] == 0 && w == 0.0f) break;
          o << "                <_>\n                  " << r[0] << " " << r[1] << " " << r[2] << " " << r[3] << " " << real_text(w) << "</_>\n";
        }
        o << "              </rects>\n              <tilted>" << (m.haar_tilted[f] ? 1 : 0) << "</tilted></feature>\n";
        o << "            <threshold>" << real_text(m.node_threshold[k]) << "</threshold>\n";
        const int child[2] = {m.node_left[k], m.node_right[k]};
        const char* node_tag[2] = {"left_node", "right_node"};
        const char* val_tag[2] = {"left_val", "right_val"};
        for (int side = 0; side < 2; side++) {
          if (child[side] > 0) {
            queue.push_back(child[side]);
            o << "            <" << node_tag[side] << ">" << ++next_idx << "</" << node_tag[side] << ">";
          } else {
            o << "            <" << val_tag[side] << ">" << real_text_d((double)m.leaves[l0 - child[side]]) << "</" << val_tag[side] << ">";
          }
          o << (side == 0 ? "\n" : "</_>\n");
        }
      }
      o << "        </_>\n";
    }
    o << "      </trees>\n      <stage_threshold>" << real_text(thr) << "</stage_threshold>\n      <parent>" << (int)s - 1
      << "</parent>\n      <next>-1</next></_>\n";
  }
  o << "  </stages>\n</cascade>\n</opencv_storage>\n";
  return write_text_file(path, o.str());
}

cc_status cc_vec_read(const char* path, int32_t* count, int32_t* vec_size, uint8_t* pixels, int cap_samples) {
  if (!path || !count || !vec_size) return set_error(CC_ERR_INVALID_ARG, "cc_vec_read: null argument");
  std::ifstream f(path, std::ios::binary);
  if (!f) return set_error(CC_ERR_IO, "cannot open '%s'", path);
  int32_t hdr[2];
  int16_t mm[2];
  f.read(reinterpret_cast<char*>(hdr), 8);
  f.read(reinterpret_cast<char*>(mm), 4);
  if (!f || hdr[0] < 0 || hdr[1] <= 0) return set_error(CC_ERR_PARSE, "wrong file format for %s", path);
  f.seekg(0, std::ios::end);
  const long long fsize = (long long)f.tellg();
  if (12 + (long long)hdr[0] * (1 + 2LL * hdr[1]) > fsize)
    return set_error(CC_ERR_PARSE, "%s: header promises %d samples of %d values but the file has %lld bytes", path, hdr[0], hdr[1], fsize);
  f.seekg(12, std::ios::beg);
  *count = hdr[0];
  *vec_size = hdr[1];
  if (!pixels) return CC_OK;
  std::vector<int16_t> rec((size_t)hdr[1]);
  const int n = std::min(hdr[0], std::max(cap_samples, 0));
  for (int i = 0; i < n; i++) {
    char zero;
    f.read(&zero, 1);
    f.read(reinterpret_cast<char*>(rec.data()), (std::streamsize)rec.size() * 2);
    if (!f) return set_error(CC_ERR_PARSE, "%s: sample %d is truncated (vec-file has incorrect structure)", path, i);
    for (int k = 0; k < hdr[1]; k++) pixels[(size_t)i * hdr[1] + k] = (uint8_t)rec[(size_t)k];
  }
  return CC_OK;
}

cc_status cc_vec_write(const char* path, const uint8_t* pixels, int count, int width, int height) {
  if (!path || (count > 0 && !pixels) || count < 0 || width < 1 || height < 1) return set_error(CC_ERR_INVALID_ARG, "cc_vec_write: bad argument");
  std::ofstream f(path, std::ios::binary);
  if (!f) return set_error(CC_ERR_IO, "cannot open '%s' for writing", path);
  const int32_t hdr[2] = {count, width * height};
  const int16_t mm[2] = {0, 0};
  f.write(reinterpret_cast<const char*>(hdr), 8);
  f.write(reinterpret_cast<const char*>(mm), 4);
  std::vector<int16_t> rec((size_t)width * height);
  for (int i = 0; i < count; i++) {
    const char zero = 0;
    for (size_t k = 0; k < rec.size(); k++) rec[k] = pixels[(size_t)i * rec.size() + k];
    f.write(&zero, 1);
    f.write(reinterpret_cast<const char*>(rec.data()), (std::streamsize)rec.size() * 2);
  }
  if (!f) return set_error(CC_ERR_IO, "write to '%s' failed", path);
  return CC_OK;
}

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
  if (c->m.feature_type == CC_FEATURE_HAAR) {
    if (rects) *rects = c->m.haar_rects.data();
    if (weights) *weights = c->m.haar_weights.data();
    if (tilted) *tilted = c->m.haar_tilted.data();
  } else if (c->m.feature_type == CC_FEATURE_HOG) {
    if (rects) *rects = c->m.hog_feats.data();
    if (weights) *weights = nullptr;
    if (tilted) *tilted = nullptr;
  } else {
    if (rects) *rects = c->m.lbp_rects.data();
    if (weights) *weights = nullptr;
    if (tilted) *tilted = nullptr;
  }
  return CC_OK;
}

}  // extern "C"
