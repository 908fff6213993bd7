// cascade.xml: reader of the new format (the one CvCascadeClassifier::save writes, traincascade/lib/src/cascadeclassifier.cpp:439-456
// with the tags of cascadeclassifier.h:27-73), its writer with and without the training parameters, and the writer of the
// legacy "opencv-haar-classifier" layout (both: cascadeclassifier.cpp:439-531). Host code only.
#include <algorithm>
#include <cmath>
#include <sstream>

#include "cc_internal.h"

namespace ccamd {

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
  const std::string fts = trimmed(ft->text);
  c.feature_type = name_index(fts, kFeatureNames, 3);
  if (c.feature_type < 0) return set_error(CC_ERR_PARSE, "cascade XML: unknown featureType '%s'", fts.c_str());
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
  std::vector<cc_tree_node> nodes;
  std::vector<float> leaves;
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
      nodes.clear();
      leaves.clear();
      if (cc_status s = read_weak_xml(wn, c.subset_size, nfeat, "cascade XML", (int)c.tree_first_node.size(), nodes, leaves); s != CC_OK) return s;
      append_tree(c, nodes.data(), (int)nodes.size(), leaves.data(), nullptr);
      ntrees++;
    }
    if (ntrees == 0) return set_error(CC_ERR_PARSE, "cascade XML: stage with no weak classifier");
    c.stage_ntrees.push_back(ntrees);
  }
  if (c.stage_ntrees.empty()) return set_error(CC_ERR_PARSE, "cascade XML: no stages");
  build_stump_view(c);
  // The training parameters, where the file holds a whole block that passes the trainer's checks; the model does not depend on
  // them. The two sets of header checks meet here and stay apart on purpose: the ones above are what the kernels rely on (a
  // window within 3..4096, a maxCatCount that fits the feature type); train_params_from_xml's are the reference trainer's
  // looser range checks, with a status of their own for a file without <boostType>.
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

// the raw <stageThreshold> whose (float)t - 1e-5f is the stored value; false if no float maps onto it
bool stage_threshold_preimage(float stored, float& t) {
  t = stored + 1e-5f;
  for (int k = 0; k < 64 && (float)(t - 1e-5f) != stored; k++) t = (float)(t - 1e-5f) < stored ? std::nextafterf(t, INFINITY) : std::nextafterf(t, -INFINITY);
  return (float)(t - 1e-5f) == stored;
}

// <rects> and <tilted> of Haar feature f (Feature::write, haarfeatures.cpp:311-320), `indent` spaces deep; the caller closes the map
void write_haar_feature(std::ostream& o, int indent, const Cascade& m, int f) {
  const std::string in((size_t)indent, ' ');
  o << in << "<rects>\n";
  for (int j = 0; j < 3; j++) {
    const int32_t* r = &m.haar_rects[(size_t)f * 12 + j * 4];
    const float w = m.haar_weights[(size_t)f * 3 + j];
    if (j > 0 && r[2] == 0 && w == 0.0f) break;  // Feature::write stops at the first rect of zero width
    o << in << "  <_>\n" << in << "    " << r[0] << " " << r[1] << " " << r[2] << " " << r[3] << " " << real_text(w) << "</_>\n";
  }
  o << in << "</rects>\n" << in << "<tilted>" << (m.haar_tilted[f] ? 1 : 0) << "</tilted>";
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
  std::vector<cc_tree_node> nodes;
  for (size_t s = 0; s < m.stage_ntrees.size(); s++) {
    // the model keeps (float)stageThreshold - 1e-5f; write back a value that parses to the same float after the
    // reader subtracts the epsilon again: search the neighbourhood of thr + 1e-5f
    float t;
    if (!stage_threshold_preimage(m.stage_threshold[s], t)) return set_error(CC_ERR_UNSUPPORTED, "%s: stage threshold %zu has no float pre-image", who, s);
    o << "    <_>\n      <maxWeakCount>" << m.stage_ntrees[s] << "</maxWeakCount>\n      <stageThreshold>" << real_text(t)
      << "</stageThreshold>\n      <weakClassifiers>\n";
    for (int i = 0; i < m.stage_ntrees[s]; i++) {
      const size_t t_i = (size_t)m.stage_first[s] + i;
      const int n0 = m.tree_first_node[t_i], nn = m.tree_nnodes[t_i];
      nodes.assign((size_t)nn, cc_tree_node());  // append_tree, backwards
      for (int k = 0; k < nn; k++) {
        cc_tree_node& nd = nodes[(size_t)k];
        nd.left = m.node_left[n0 + k];
        nd.right = m.node_right[n0 + k];
        nd.var_idx = m.node_feature[n0 + k];
        nd.ord_c = m.node_threshold[n0 + k];
        std::copy_n(m.node_subset.begin() + (size_t)(n0 + k) * m.subset_size, m.subset_size, nd.subset);
      }
      write_weak_xml(o, 8, nodes.data(), nn, m.subset_size, &m.leaves[m.tree_first_leaf[t_i]]);
    }
    o << "      </weakClassifiers></_>\n";
  }
  o << "  </stages>\n  <features>\n";
  const int nf = m.n_features();
  for (int f = 0; f < nf; f++) {
    if (haar) {
      o << "    <_>\n";
      write_haar_feature(o, 6, m, f);
      o << "</_>\n";
    } else {  // LBP: the 3 x 3 grid's first cell; HOG: the block's first cell and the component
      const int32_t* r = hog ? &m.hog_feats[(size_t)f * 5] : &m.lbp_rects[(size_t)f * 4];
      o << "    <_>\n      <rect>\n        " << r[0] << " " << r[1] << " " << r[2] << " " << r[3];
      if (hog) o << " " << r[4];
      o << "</rect></_>\n";
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
  std::string s;
  if (cc_status st = read_text_file(path, s); st != CC_OK) return st;
  return cc_cascade_load_xml_mem(s.data(), s.size(), out);
}

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
        o << "          <_>\n            <feature>\n";
        write_haar_feature(o, 14, m, m.node_feature[k]);
        o << "</feature>\n            <threshold>" << real_text(m.node_threshold[k]) << "</threshold>\n";
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

}  // extern "C"
