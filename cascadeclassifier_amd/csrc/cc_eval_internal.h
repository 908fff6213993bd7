// Shared between cc_eval.hip (evaluator, bulk operator(), predict) and cc_split.hip (best-split search): device-side
// feature records, the evaluator handle and the helpers both translation units use.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>
#include <vector>

#include "cc_hip_util.h"
#include "cc_internal.h"

namespace ccamd {

// Haar feature with the reference's fastRect offsets (row stride W+1) — haarfeatures.cpp:266-309.
struct HaarFeatDev {
  int p[3][4];
  float w[3];
  int tilted;
};
struct LbpFeatDev {
  int p[16];
};

cc_status eval_device(cc_evaluator* e);
// Stable sort of every row of [rows][n] with the sample position as the value, one block per row (cc_split.hip); only for
// n <= sort_rows_block_limit(): larger rows take the device-wide segmented sort at the call site.
int sort_rows_block_limit();
hipError_t sort_rows_block(const float* vals, int rows, int n, float* keys_out, int* idx_out, hipStream_t st);

// Launches k_eval_batch over `feats` [fb, fe) for ns samples into d_out_ptr (device). Caller holds e->mu.
cc_status launch_batch(cc_evaluator* e, bool haar, const void* feats, int fb, int fe, const int32_t* d_idx, int ns,
                       float* d_out_ptr, int normalized, size_t out_pitch /* 0 = n_samples */);
// Sends the images queued by cc_eval_set_image to the device (runs of consecutive sample indices, one launch per run).
// Every entry point that reads stored samples on the device calls it first. Caller holds e->mu.
cc_status flush_pending_images(cc_evaluator* e);

// setImage of n windows whose pixels are already on the device (W * H bytes each, readable from e->stream) into the rows
// [first_idx, first_idx + n) of the evaluator's sample tables: the launch cc_eval_set_images makes. Caller holds e->mu.
cc_status launch_set_images(cc_evaluator* e, const uint8_t* d_imgs, int n, int first_idx);
// cc_eval_set_images for device-resident pixels, every sample with one label: pending queue first, generation, host
// mirror, launch, synchronise, labels. Takes e->mu. The range has been checked by the caller.
cc_status eval_set_images_device(cc_evaluator* e, const uint8_t* d_imgs, int n, int first_idx, float label);
// Whether cascade m can be predicted on e's samples (type, window, tilted integrals); `who` names the entry point.
cc_status predict_check(const cc_evaluator* e, const Cascade& m, const char* who);
// CvCascadeClassifier::predict of m on ns stored samples (d_idx: device indices or NULL for 0..ns-1): the flags stay in
// e->d_pred and, if out is set, also go to host out. Synchronises e->stream. Caller holds e->mu, predict_check passed.
cc_status predict_stored(cc_evaluator* e, const Cascade& m, const int32_t* d_idx, int ns, uint8_t* out);

// ---- filling a stage's training set (cc_fill.hip) -----------------------------------------------
// The loop of fillPassedSamples (cascadeclassifier.cpp:329-357) over pass flags that are on the device: where it stops,
// why, and which positions it keeps. FillWork is the caller's workspace; d_keep[0 .. n_filled) holds the kept positions.
struct FillRecord {
  unsigned long long stop;  // position * 4 + reason of the first position at which the loop stops
  int n_filled, pad;
};
struct FillWork {
  DevBuf<long long> d_block;  // per block of the scan: flags set in it, then the count before it
  DevBuf<long long> d_keep;
  DevBuf<FillRecord> d_rec;
  PinnedBuf h_rec;
};
struct FillResult {
  int n_filled = 0, stop = 0;
  long long n_consumed = 0;
};
// Queues the selection over flags [start, n) behind what `st` holds and waits for its record. got_before, consumed_before
// and ratio as cc_negminer_fill takes them.
cc_status fill_select(FillWork& w, const uint8_t* d_flags, long long n, long long start, int want, long long got_before,
                      long long consumed_before, double ratio, hipStream_t st, FillResult* out);

// HOG (cc_hog.hip). Catalog blocks as (x, y, cell w, cell h) (hog_catalog, cc_internal.h); variables are block * 36 + cell * 9 + bin.
// Builds the catalog, sets nfeat to the variable count and allocates the planes. Called by cc_eval_create.
cc_status hog_init(cc_evaluator* e);
// setImage of n images already on the device (e->stream), samples [first_idx, first_idx + n). Caller holds e->mu.
cc_status hog_launch_set_images(cc_evaluator* e, const uint8_t* d_imgs, int n, int first_idx);
// operator() for variables [vb, ve) x ns samples into d_out[(vi - vb) * pitch + s] (pitch 0 = ns). Caller holds e->mu.
cc_status hog_launch_batch(cc_evaluator* e, int vb, int ve, const int32_t* d_idx, int ns, float* d_out, size_t out_pitch);
cc_status hog_launch_list(cc_evaluator* e, const int32_t* d_list, int n, int si, float* d_out);
// CvCascadeClassifier::predict of HOG cascade m (type and window checked by the caller) on ns stored samples (d_idx:
// device indices or NULL for 0..ns-1) into e->d_pred and, if set, host out; synchronous. Caller holds e->mu.
cc_status hog_predict(cc_evaluator* e, const Cascade& m, const int32_t* d_idx, int ns, uint8_t* out);
// Host mirror: the ten planes of one window ([cols][10], the device layout) and one variable's value on them.
void hog_host_planes(const cc_evaluator* e, const uint8_t* px, std::vector<float>& planes);
float hog_host_value(const cc_evaluator* e, const float* planes, int vi);


// ---- the split search (cc_split.hip) as the booster (cc_boost.hip) enters it ---------------------
// per stored sample: weight and (regression) response * weight or (classification) class; w < 0 marks "not in the node"
struct SplitEntry {
  double w, t;
};
// The per-sample table of a node search: where it lives and how wide its entries are. The values are the kernels' TAB.
enum TableForm : int { TABLE_GLOBAL16 = 0, TABLE_LDS16 = 1, TABLE_LDS8 = 2 };
// What a table holds for a stored sample that is not in the node (the values: cc_split.hip).
struct AbsentEntry {
  double e8;
  SplitEntry e16;
};
extern const AbsentEntry ABSENT_ORDERED, ABSENT_CATEGORICAL;
// d_split_out of the ordered search and its pinned copy: best_val [fpad] doubles, then best_i, best_vl and best_vr,
// [fpad] 4-byte values each.
struct OrdResult {
  double* best_val;
  int* best_i;
  float *best_vl, *best_vr;
  OrdResult(void* base, size_t fpad)
      : best_val(static_cast<double*>(base)), best_i(reinterpret_cast<int*>(best_val + fpad)), best_vl(reinterpret_cast<float*>(best_i + fpad)),
        best_vr(best_vl + fpad) {}
  static size_t bytes(size_t fpad) { return fpad * 20; }
};
// The form cc_eval_find_best_split picks for class labels or responses of +-1 over N presorted samples.
TableForm split_table_form_unit(int N);
// Both search the presorted variables over a node table that is already in e->d_split_tab. Caller holds e->mu.
// Ordered: mode 0 regression, 1 GINI, 2 MISCLASS; the per-variable results stay in e->d_split_out (OrdResult).
cc_status split_launch_ordered(cc_evaluator* e, int mode, TableForm form, double w_total0, double w_total1, double rsum0);
// Categorical: node = stored samples in increasing order; the winner as cc_eval_find_best_split reports it.
cc_status split_categorical_from_table(cc_evaluator* e, bool is_classifier, bool gini, TableForm form, cc_split* out);

}  // namespace ccamd

struct cc_evaluator {
  using HaarFeature = ccamd::HaarFeature;
  template <class T>
  using DevBuf = ccamd::DevBuf<T>;
  using HaarFeatDev = ccamd::HaarFeatDev;
  using LbpFeatDev = ccamd::LbpFeatDev;
  int type = 0, mode = 0, W = 0, H = 0, max_samples = 0, device = 0, cols = 0;
  bool use_tilted = false;
  std::vector<HaarFeature> haar;
  std::vector<int32_t> lbp;
  std::vector<float> cls;
  int nfeat = 0;
  hipStream_t stream = nullptr;
  DevBuf<int32_t> d_sum, d_tilted;
  DevBuf<float> d_nf;
  DevBuf<HaarFeatDev> d_haar;
  DevBuf<LbpFeatDev> d_lbp;
  // scratch (guarded by mu: the calc entry points may be called concurrently)
  std::mutex mu;
  DevBuf<uint8_t> d_imgs;
  DevBuf<int32_t> d_idx;
  DevBuf<float> d_out;
  DevBuf<HaarFeatDev> d_custom;
  DevBuf<HaarFeatDev> d_haar_plain;  // catalog with plain fastRect offsets (cc_eval_calc_list), built on first use
  DevBuf<LbpFeatDev> d_lbp_plain;
  DevBuf<uint8_t> d_pred;
  hipEvent_t ev_a = nullptr, ev_b = nullptr;
  hipEvent_t ev_piece[8] = {};  // categorical split search: one per piece of the sums on its way back (cc_split.hip)
  double last_ms = 0;
  int S = 16;
  // resident tables of the split search (cc_eval_presort): per group of 64 features the sorted values and sample
  // indices, interleaved so that lane = feature reads are coalesced: [group][rank][64]
  DevBuf<float> d_sorted_val;
  DevBuf<uint16_t> d_sorted_idx16;
  DevBuf<int32_t> d_sorted_idx32;
  DevBuf<uint8_t> d_codes;  // LBP: [feature][sample] codes
  int cat_sorted_n = 0;          // samples per variable in d_cat_sorted (0: not built)
  DevBuf<uint32_t> d_cat_sorted;  // LBP: (sample << 8 | code) in (code, sample) order, [group][rank][64] (cc_split.hip)
  uint64_t generation = 0;  // bumped by every presort and setImage(s): what a cc_boost was created against
  int presort_n = 0;      // samples covered by the tables (0 = none)
  int presort_f0 = 0, presort_f1 = 0;  // variables covered by the tables
  DevBuf<double> d_split_tab, d_split_out;
  DevBuf<int32_t> d_split_idx;
  ccamd::PinnedBuf pin_in, pin_out;
  // ---- single-image path (cc_eval_set_image / cc_eval_calc / cc_eval_calc_list), see cc_eval.hip ----
  // images set one at a time that the device has not seen yet: pixels (W * H each), sample index, and where a sample's
  // latest image sits in the queue (pend_slot[idx], -1 = not queued); guarded by mu
  std::vector<uint8_t> pend_px;
  std::vector<int32_t> pend_idx;
  std::vector<int32_t> pend_slot;
  std::atomic<int> pend_n{0};
  // host mirror of the sample set LAST by cc_eval_set_image: its integral(s) and norm factor, computed on the host with the
  // device kernels' arithmetic; answers cc_eval_calc / cc_eval_calc_list for that sample without a launch
  int mirror_idx = -1;
  std::vector<int32_t> mirror_sum, mirror_tilted;
  float mirror_nf = 0.f;
  std::once_flag host_catalog_once;
  std::vector<HaarFeatDev> h_haar;  // catalog with plain fastRect offsets (row stride W + 1)
  std::vector<LbpFeatDev> h_lbp;
  // HOG (cc_hog.hip): catalog blocks [n][4] = x, y, cell w, cell h; planes [max_samples][cols][10] (9 bins, then norm);
  // nfeat counts variables (blocks * 36). mirror_hog is the host mirror of the last window, read and written under mu.
  std::vector<int32_t> hog_blocks;
  DevBuf<int32_t> d_hog_blocks;
  DevBuf<float> d_hog;
  int hog_planes_per_pass = 0;
  std::vector<float> mirror_hog;
  // cc_eval_fill_passed (cc_fill.hip): a chunk of candidates is set into these scratch rows, predicted there and the kept
  // rows copied to their slots; guarded by mu
  DevBuf<int32_t> fill_sum, fill_tilted;
  DevBuf<float> fill_nf, fill_hog;
  ccamd::FillWork fill;
  ~cc_evaluator() {
    if (ev_a) (void)hipEventDestroy(ev_a);
    if (ev_b) (void)hipEventDestroy(ev_b);
    for (hipEvent_t& ev : ev_piece)
      if (ev) (void)hipEventDestroy(ev);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

