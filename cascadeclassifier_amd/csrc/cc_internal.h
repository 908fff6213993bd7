// Internal declarations shared by the translation units of libcascadeclassifier_amd.so.
#pragma once

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <iosfwd>
#include <string>
#include <vector>

#include "../../include/cascadeclassifier_amd.h"

#include <locale.h>

namespace ccamd {

// Numbers in cascade XML and in generated kernel source are written and parsed with printf / strtod, which follow the
// calling thread's LC_NUMERIC: under a comma-decimal locale (a host program that called setlocale(LC_ALL, "")) "%.8e"
// would print "1,5e+00" and strtod would stop at the '.' of "1.5". Entry points that format or parse numbers hold one
// of these: it switches the calling THREAD to the "C" locale for its lifetime (uselocale; no other thread is affected).
struct CNumericLocale {
  locale_t prev = (locale_t)0;
  CNumericLocale() {
    static locale_t c = newlocale(LC_ALL_MASK, "C", (locale_t)0);
    if (c != (locale_t)0) prev = uselocale(c);
  }
  ~CNumericLocale() {
    if (prev != (locale_t)0) uselocale(prev);
  }
  CNumericLocale(const CNumericLocale&) = delete;
  CNumericLocale& operator=(const CNumericLocale&) = delete;
};

// ---- error plumbing (thread-local message behind cc_last_error) -------------------------------
cc_status set_error(cc_status code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// ---- minimal XML DOM (the subset cv::FileStorage writes) ---------------------------------------
struct XmlNode {
  std::string name;
  std::string text;  // concatenated character data (entities decoded)
  std::vector<std::pair<std::string, std::string>> attrs;
  std::vector<XmlNode> children;
  const XmlNode* child(const char* n) const {
    for (const XmlNode& c : children)
      if (c.name == n) return &c;
    return nullptr;
  }
};
// Returns false and fills err on malformed input.
bool xml_parse(const char* text, size_t len, XmlNode& root, std::string& err);

// ---- parsed cascade ------------------------------------------------
struct HaarFeature {
  int32_t r[3][4];
  float w[3];
  int32_t tilted;
};

struct Cascade {
  int feature_type = 0;
  int win_w = 0, win_h = 0;
  int max_cat_count = 0, subset_size = 0;
  int max_nodes_per_tree = 0;
  bool has_tilted = false;
  // stages
  std::vector<int32_t> stage_first, stage_ntrees;
  std::vector<float> stage_threshold;  // (float)stageThreshold - THRESHOLD_EPS
  // trees (general form)
  std::vector<int32_t> tree_first_node, tree_nnodes, tree_first_leaf;
  std::vector<int32_t> node_left, node_right, node_feature;
  std::vector<float> node_threshold;
  std::vector<int32_t> node_subset;  // subset_size words per node
  std::vector<float> leaves;
  // stump view (max_nodes_per_tree == 1)
  std::vector<int32_t> stump_feature;
  std::vector<float> stump_threshold, stump_left, stump_right;
  // features
  std::vector<int32_t> haar_rects;   // [n][3][4]
  std::vector<float> haar_weights;   // [n][3]
  std::vector<int32_t> haar_tilted;  // [n]
  std::vector<int32_t> lbp_rects;    // [n][4]
  std::vector<int32_t> hog_feats;    // [n][5]: x, y, cell w, cell h of the block's cell 0, component in [0, 36)
  // the training parameters the file carried, when it carried a whole block of them (section 6d of the header)
  bool has_train_params = false;
  cc_train_params train_params = {};
  int n_features() const {
    return feature_type == CC_FEATURE_HAAR ? (int)haar_tilted.size()
           : feature_type == CC_FEATURE_HOG ? (int)(hog_feats.size() / 5)
                                            : (int)(lbp_rects.size() / 4);
  }
};
cc_status cascade_from_xml(const XmlNode& root, Cascade& out);  // cc_cascade_xml.cpp

// ---- text of the files: tokens, numbers, names (cc_cascade.cpp) ----------------------------------
void split_tokens(const std::string& s, std::vector<std::string>& out);
bool to_int(const std::string& t, int32_t& v);  // also integral reals ("6.")
bool to_double(const std::string& t, double& v);
bool node_int(const XmlNode* n, int32_t& v);  // false for a missing node or one that is not a single number
bool node_double(const XmlNode* n, double& v);
std::string trimmed(const std::string& s);
extern const char* const kFeatureNames[3];  // HAAR, LBP, HOG
extern const char* const kBoostNames[4];    // CvBoost's DISCRETE, REAL, LOGIT, GENTLE
extern const char* const kModeNames[3];     // BASIC, CORE, ALL
int name_index(const std::string& s, const char* const* names, int n);  // -1: none
// FileStorage prints float reals with "%.8e", doubles with "%.16e", and integral reals as "2."
std::string real_text(float v);
std::string real_text_d(double v);
cc_status read_text_file(const char* path, std::string& text);
cc_status write_text_file(const char* path, const std::string& text);

// ---- trees: what every reader, writer and builder of them shares (cc_cascade.cpp) -----------------
// The child-reference rule. Node j of a tree of nn nodes names a child > 0 (an internal node of this tree) or <= 0 (leaf
// -child of its nn + 1 leaves). A child lies inside the tree, and an internal child lies behind its parent: the writer
// numbers nodes breadth-first, and insisting on it makes every walk of the tree end (a cycle would hang a kernel).
// nullptr: the references are good; else what is wrong with them, to follow "a child of node j ".
const char* child_ref_fault(int32_t left, int32_t right, int j, int nn);
// n_nodes[t] >= 1 for each of n_trees trees (nullptr: one node each), n_nodes_total their sum: CC_ERR_INVALID_ARG otherwise
cc_status check_node_counts(const char* who, const int32_t* n_nodes, size_t n_trees, int n_nodes_total);
// The <_> of weak classifier t: "left right featureIdx (threshold | subset_words words)" per node of <internalNodes> and
// one more <leafValues> than nodes, appended to nodes (left, right, var_idx, ord_c or subset; the rest 0) and leaves.
// featureIdx lies in [0, feature_bound), feature_bound 0: in [0, inf). CC_ERR_PARSE with messages behind "where: ".
cc_status read_weak_xml(const XmlNode& wn, int subset_words, int feature_bound, const char* where, int t, std::vector<cc_tree_node>& nodes,
                        std::vector<float>& leaves);
// The same <_>, written `indent` spaces deep as FileStorage lays it out.
void write_weak_xml(std::ostream& o, int indent, const cc_tree_node* nodes, int nn, int subset_words, const float* leaves);
// One more tree behind the model's trees; var_map (nullptr: none) renumbers var_idx. The nodes have passed child_ref_fault.
void append_tree(Cascade& c, const cc_tree_node* nodes, int nn, const float* leaves, const int32_t* var_map);
void build_stump_view(Cascade& c);  // once every tree is appended; does nothing unless each has one node

// ---- the parameter block of params.xml and cascade.xml (cc_trainfiles.cpp) -------------------------
cc_status train_params_from_xml(const XmlNode& block, const char* where, cc_train_params& p);
cc_status check_param_names(const char* who, const cc_train_params& p);
void write_params_text(std::ostream& o, int feature_type, int win_w, int win_h, const cc_train_params* p, int max_weak, int max_cat, int feat_size);

// ---- pyramid geometry (host) --------------------------------------------------------------------
struct ScaleGeom {
  float scale;
  int w, h, ystep, nx, ny, win_w, win_h;
};
void scale_plan(int W0, int H0, int imgw, int imgh, const cc_detect_params& p, std::vector<ScaleGeom>& out);

// Per-axis tap table of the fixed-point bilinear resize: left tap and the 8.8 weight of the right tap
// (weight of the left tap is 256 - w1). Border samples have w1 = 0.
struct AxisTaps {
  std::vector<int32_t> ofs;
  std::vector<uint16_t> w1;
};
void linear_exact_taps(int src, int dst, AxisTaps& t);

// levels / level_weights (optional, one per rectangle): the outputRejectLevels overload of cv::groupRectangles
void group_rectangles(std::vector<cc_rect>& rects, int group_threshold, double eps, std::vector<int>* levels = nullptr,
                      std::vector<double>* level_weights = nullptr);

// ---- detector arithmetic that needs no device (cc_pass.hip, cc_tables.hip; tests/cpp/test_detect_host.cpp) ---
// How cc_detector's pass loop cuts a batch of n_frames into passes: sizes in [1, max_batch] that sum to n_frames.
// `pipeline_passes_set`: the pass count was given (CCAMD_PIPELINE_PASSES), so a submitted batch (`defer_last`) keeps it.
std::vector<int> pass_sizes(int n_frames, int max_batch, int pipeline_passes, bool pipeline_passes_set, bool want_results,
                            bool defer_last);

// Stage groups of the cascade kernel (EvalArgs::group_first, EvalArgs::dense_from): consecutive stages from stage `from`
// on share a group while the group stays within `budget` stumps. group_first gets one entry per group plus the stage
// count; dense_from the first group >= 1 that starts at stage `dense_stage` or later (0x7fffffff: none, also for
// dense_stage < 1).
void stage_groups(const std::vector<int32_t>& stage_ntrees, int from, int budget, int dense_stage, std::vector<int>& group_first,
                  int& dense_from);

// Integer form of the stage sums in the Haar wave phase (cc_eval_kernel.inc: wave_phase_haar), per stage of a Haar stump
// cascade whose stage sums are order-independent: where stage_quantum holds (and the threshold is a number), q[s] is the
// stage's quantum, left_q / right_q its leaves in units of q[s] (exact), and thr_q[s] the smallest int32 n with
// n * q[s] >= stage_threshold[s], saturated; the stage sum n * q[s] of any window passes exactly when n >= thr_q[s].
// Elsewhere q[s] = 0 and the stage has no integer form (also everywhere when !enabled, or for any other cascade).
struct WaveIntTables {
  std::vector<double> q;
  std::vector<int32_t> thr_q;
  std::vector<int32_t> left_q, right_q;  // per stump, in the cascade's stump order
};
WaveIntTables wave_int_tables(const Cascade& m, bool enabled);

// ---- catalogs (training side) -------------------------------------------------------------------
void haar_catalog(int W, int H, int mode, std::vector<HaarFeature>& out);
void lbp_catalog(int W, int H, std::vector<int32_t>& rects);
void hog_catalog(int W, int H, std::vector<int32_t>& blocks);  // (x, y, cell w, cell h) per block

// ---- split search, categorical variables: the part after the per-category accumulation (host) ------
// hist: n_cat pairs, regression {sum of response*w, sum of w}, classification {w of class 0, w of class 1}, each
// accumulated in node sample order. Orders the categories and scans them as find_split_cat_reg / find_split_cat_class
// do (o_cvboostree.cpp:466-515, 289-357) with init_quality -1.
struct CatSplit {
  bool found;
  double quality;      // best_val (double, before the cast to float)
  int n_left;          // categories sent left
  int32_t subset[8];
};
void split_categories(const double* hist, int n_cat, bool is_classifier, bool gini, CatSplit& out);

}  // namespace ccamd

struct cc_cascade {
  ccamd::Cascade m;
};
