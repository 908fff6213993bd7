// The trainer's own files (section 6d of include/cascadeclassifier_amd.h): params.xml and the parameter block cascade.xml shares
// with it, stage<i>.xml, and the .vec sample files. Host code only.
#include <algorithm>
#include <cstring>
#include <fstream>
#include <sstream>

#include "cc_internal.h"

namespace ccamd {
namespace {

// a string value: FileStorage quotes one that would not read back as a string otherwise
std::string string_value(const XmlNode* n) {
  std::string s = n ? trimmed(n->text) : std::string();
  if (s.size() >= 2 && s.front() == '"' && s.back() == '"') s = s.substr(1, s.size() - 2);
  return s;
}

}  // namespace

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

cc_status check_param_names(const char* who, const cc_train_params& p) {
  if (p.feature_type < 0 || p.feature_type > 2) return set_error(CC_ERR_INVALID_ARG, "%s: unknown feature type %d", who, p.feature_type);
  if (p.boost_type < 0 || p.boost_type > 3) return set_error(CC_ERR_INVALID_ARG, "%s: unknown boost type %d", who, p.boost_type);
  if (p.feature_type == CC_FEATURE_HAAR && (p.haar_mode < 0 || p.haar_mode > 2)) return set_error(CC_ERR_INVALID_ARG, "%s: unknown Haar mode %d", who, p.haar_mode);
  return CC_OK;
}

// <stageType> .. <featureParams>: CvCascadeParams::write (cascadeclassifier.cpp:33-46) and the two blocks of writeParams (:359-364),
// at the depth params.xml and cascade.xml hold them. p == nullptr: the short blocks cc_cascade_save_xml writes, from the last three arguments.
void write_params_text(std::ostream& o, int feature_type, int win_w, int win_h, const cc_train_params* p, int max_weak, int max_cat, int feat_size) {
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

}  // namespace ccamd

using namespace ccamd;

namespace {

// the object under <opencv_storage> (FileStorage::getFirstTopLevelNode), or the root itself, of the file at path
cc_status first_top_level(const char* path, XmlNode& root, const XmlNode*& top) {
  std::string s, err;
  if (cc_status st = read_text_file(path, s); st != CC_OK) return st;
  if (!xml_parse(s.data(), s.size(), root, err)) return set_error(CC_ERR_PARSE, "%s: %s", path, err.c_str());
  top = root.name != "opencv_storage" ? &root : root.children.empty() ? nullptr : &root.children[0];
  if (!top) return set_error(CC_ERR_PARSE, "%s: <opencv_storage> is empty", path);
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

}  // namespace

extern "C" {

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
  const XmlNode* top = nullptr;
  if (cc_status st = first_top_level(path, root, top); st != CC_OK) return st;
  return train_params_from_xml(*top, path, *out);
}

cc_status cc_stage_save_xml(const char* path, const char* object_name, int max_cat_count, float stage_threshold, int n_weak,
                            const int32_t* n_nodes, int n_nodes_total, const cc_tree_node* nodes, const float* leaves) {
  const CNumericLocale c_numbers;
  const char* who = "cc_stage_save_xml";
  if (!path || !n_nodes || !nodes || !leaves) return set_error(CC_ERR_INVALID_ARG, "%s: null argument", who);
  if (max_cat_count < 0 || max_cat_count > 256) return set_error(CC_ERR_INVALID_ARG, "%s: max_cat_count %d outside [0, 256]", who, max_cat_count);
  if (n_weak < 1) return set_error(CC_ERR_INVALID_ARG, "%s: a stage has at least one weak classifier", who);
  if (cc_status st = check_node_counts(who, n_nodes, (size_t)n_weak, n_nodes_total); st != CC_OK) return st;
  const std::string name = object_name ? object_name : default_object_name(path);
  std::ostringstream o;
  o << "<?xml version=\"1.0\"?>\n<opencv_storage>\n<" << name << ">\n";
  o << "  <maxWeakCount>" << n_weak << "</maxWeakCount>\n  <stageThreshold>" << real_text(stage_threshold) << "</stageThreshold>\n  <weakClassifiers>\n";
  size_t k = 0;
  for (int t = 0; t < n_weak; t++) {
    const int nn = n_nodes[t];
    for (int j = 0; j < nn; j++) {
      const cc_tree_node& nd = nodes[k + (size_t)j];
      if (const char* fault = child_ref_fault(nd.left, nd.right, j, nn))
        return set_error(CC_ERR_OUT_OF_RANGE, "%s: <internalNodes> of weak classifier %d: a child of node %d %s", who, t, j, fault);
      if (nd.var_idx < 0) return set_error(CC_ERR_OUT_OF_RANGE, "%s: variable %d of weak classifier %d", who, nd.var_idx, t);
    }
    write_weak_xml(o, 4, nodes + k, nn, (max_cat_count + 31) / 32, leaves + k + (size_t)t);
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
  const XmlNode* top = nullptr;
  if (cc_status st = first_top_level(path, root, top); st != CC_OK) return st;
  double thr = 0;
  if (!node_double(top->child("stageThreshold"), thr)) return set_error(CC_ERR_PARSE, "%s: bad or missing <stageThreshold>", path);
  const XmlNode* weak = top->child("weakClassifiers");
  if (!weak) return set_error(CC_ERR_PARSE, "%s: <weakClassifiers> is missing", path);
  std::vector<int32_t> counts;
  std::vector<cc_tree_node> all;
  std::vector<float> lv;
  for (const XmlNode& wn : weak->children) {
    if (wn.name != "_") continue;
    const size_t before = all.size();
    if (cc_status st = read_weak_xml(wn, (max_cat_count + 31) / 32, n_variables, path, (int)counts.size(), all, lv); st != CC_OK) return st;
    counts.push_back((int32_t)(all.size() - before));
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

}  // extern "C"
