// Shared by the training-side translation units: cc_eval_store.hip (the evaluator and its samples), cc_eval_calc.hip (bulk
// operator()), cc_eval_predict.hip (cascade predict), cc_hog.hip, cc_fill.hip, cc_presort.hip (the sorted tables and their
// memory), cc_split.hip (best-split search) and cc_boost.hip: device-side feature records, the evaluator handle and the
// helpers more than one of them uses.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
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

// The tables setImage writes for a set of samples, one sample per row: integral and tilted integral [rows][cols], norm
// factor [rows] (Haar, LBP); planes [rows][cols][10] (HOG). The evaluator holds the stored samples and a set of scratch
// rows; what runs on either takes the set as an argument.
struct SampleTables {
  DevBuf<int32_t> sum, tilted;
  DevBuf<float> nf, hog;
};

cc_status eval_device(cc_evaluator* e);

// ---- the evaluator and its samples (cc_eval_store.hip) -------------------------------------------
// Sends the images queued by cc_eval_set_image to the device (runs of consecutive sample indices, one launch per run).
// Every entry point that reads stored samples on the device calls it first. Caller holds e->mu.
cc_status flush_pending_images(cc_evaluator* e);
// setImage of n windows whose pixels are already on the device (W * H bytes each, readable from e->stream) into the rows
// [first_idx, first_idx + n) of t: the launch cc_eval_set_images makes. Caller holds e->mu.
cc_status launch_set_images(cc_evaluator* e, const SampleTables& t, const uint8_t* d_imgs, int n, int first_idx);
// cc_eval_set_images for device-resident pixels, every sample with one label: pending queue first, generation, host
// mirror, launch, synchronise, labels. Takes e->mu. The range has been checked by the caller.
cc_status eval_set_images_device(cc_evaluator* e, const uint8_t* d_imgs, int n, int first_idx, float label);
// operator()(feats[i], si) for i < n from the host mirror, if si is the sample cc_eval_set_image set last (no launch);
// false if it is not. The indices are in range. The public header's contract holds here: cc_eval_calc* are safe for
// concurrent callers only once cc_eval_set_image(s) has returned. HOG reads its mirror under e->mu (cc_eval_set_image
// rewrites it under e->mu); Haar and LBP read theirs without the lock.
bool mirror_answer(cc_evaluator* e, int si, const int32_t* feats, int n, float* out);

// ---- bulk operator() (cc_eval_calc.hip) ----------------------------------------------------------
// Lets the batch kernels ask for `bytes` of dynamic LDS (more than the 64 KB a launch may ask for by default).
cc_status batch_kernels_allow_lds(int bytes);
// Launches k_eval_batch over `feats` [fb, fe) for ns samples into d_out_ptr (device). Caller holds e->mu.
cc_status launch_batch(cc_evaluator* e, bool haar, const void* feats, int fb, int fe, const int32_t* d_idx, int ns,
                       float* d_out_ptr, int normalized, size_t out_pitch /* 0 = n_samples */);
// Checks ns sample indices (NULL: 0 .. ns-1) against max_samples and sends them to e->d_idx; *d_idx is NULL for NULL.
cc_status upload_indices(cc_evaluator* e, const int32_t* sample_idx, int ns, const int32_t** d_idx);

// ---- cascade predict (cc_eval_predict.hip) -------------------------------------------------------
// Whether cascade m can be predicted on e's samples (type, window, tilted integrals); `who` names the entry point.
cc_status predict_check(const cc_evaluator* e, const Cascade& m, const char* who);
// CvCascadeClassifier::predict of m on rows of t (d_idx: ns device indices or NULL for 0..ns-1): the flags stay in
// e->d_pred and, if out is set, also go to host out. Synchronises e->stream. Caller holds e->mu, predict_check passed.
cc_status predict_stored(cc_evaluator* e, const SampleTables& t, const Cascade& m, const int32_t* d_idx, int ns, uint8_t* out);

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
// setImage of n images already on the device (e->stream) into rows [first_idx, first_idx + n) of t. Caller holds e->mu.
cc_status hog_launch_set_images(cc_evaluator* e, const SampleTables& t, const uint8_t* d_imgs, int n, int first_idx);
// operator() for variables [vb, ve) x ns samples into d_out[(vi - vb) * pitch + s] (pitch 0 = ns). Caller holds e->mu.
cc_status hog_launch_batch(cc_evaluator* e, int vb, int ve, const int32_t* d_idx, int ns, float* d_out, size_t out_pitch);
cc_status hog_launch_list(cc_evaluator* e, const int32_t* d_list, int n, int si, float* d_out);
// CvCascadeClassifier::predict of HOG cascade m (type and window checked by the caller) on rows of t (d_idx: ns device
// indices or NULL for 0..ns-1) into e->d_pred and, if set, host out; synchronous. Caller holds e->mu.
cc_status hog_predict(cc_evaluator* e, const SampleTables& t, const Cascade& m, const int32_t* d_idx, int ns, uint8_t* out);
// Host mirror: the ten planes of one window ([cols][10], the device layout) and one variable's value on them.
void hog_host_planes(const cc_evaluator* e, const uint8_t* px, std::vector<float>& planes);
float hog_host_value(const cc_evaluator* e, const float* planes, int vi);

// ---- the sorted tables (cc_presort.hip) as the split search and the booster read them -------------
// Stable sort of every row of [rows][n] with the sample position as the value, one block per row; only for
// n <= sort_rows_block_limit(): larger rows take the device-wide segmented sort at the call site.
int sort_rows_block_limit();
hipError_t sort_rows_block(const float* vals, int rows, int n, float* keys_out, int* idx_out, hipStream_t st);
// Stable sort of the rows of e->d_out (one variable per row of N values, at most FB rows) into keys_out / sorted. Owns
// the scratch of both sorts; that of the device-wide segmented sort is built when a pass first needs it.
struct RowSorter {
  cc_evaluator* e;
  int N, FB;
  DevBuf<float> keys_out;
  DevBuf<int> sorted, iota, offsets;
  DevBuf<char> temp;
  bool segmented_ready = false;

  RowSorter(cc_evaluator* e_, int N_, int FB_) : e(e_), N(N_), FB(FB_) {}
  cc_status init();
  cc_status prepare_segmented();
  cc_status sort(int nf);
  size_t bytes() const { return keys_out.n * 4 + sorted.n * 4 + iota.n * 4 + offsets.n * 4 + temp.n; }
};
// Zeroed ranks behind a table's last group, read ahead into without bounds checks: k_split_ord_lean up to 3 chunks of 16 ranks;
// k_split_cat_sorted, on a trip that starts at rank r0 < n_pre, DEPTH chunks and the DEPTH after them (to r0 + 2 * DEPTH * UNROLL - 1).
constexpr int SPLIT_TABLE_PAD_RANKS = 64;
constexpr int SPLIT_CAT_UNROLL = 16;  // ranks per chunk: four 16-byte loads per lane
constexpr int SPLIT_CAT_DEPTH = 6;    // chunks whose loads are in flight (one wavefront per SIMD: latency is hidden by distance, not by occupancy)
constexpr int SPLIT_CAT_PAD_RANKS = (2 * SPLIT_CAT_DEPTH + 1) * SPLIT_CAT_UNROLL;
// Sample numbers take 16 bits in a table while they fit, 32 otherwise.
inline bool wide_index(size_t n_samples) { return n_samples > 65536; }
// The one place where that width becomes the TI of a kernel launch: f gets a value of the sample-number type.
template <class F>
auto with_index_type(bool wide, F&& f) { return wide ? f(int32_t{}) : f(uint16_t{}); }
// Sorted values and sample numbers of ordered variables, [group][rank][64], with SPLIT_TABLE_PAD_RANKS zeroed ranks behind
// the last group: the resident tables of a presort and the chunk table of a streamed search.
struct SortedTable {
  DevBuf<float> val;
  DevBuf<uint16_t> idx16;
  DevBuf<int32_t> idx32;
  bool wide = false;  // which of the two holds the sample numbers
  static constexpr size_t PAD = (size_t)SPLIT_TABLE_PAD_RANKS * 64;
  // Room for `entries` and the padding, which is zeroed on st. Grows only; the index buffer of the other width stays.
  cc_status alloc(size_t entries, bool wide_, hipStream_t st);
  cc_status zero_padding(size_t entries, hipStream_t st);  // behind `entries`, which may be fewer than alloc was given
  // Gives back every buffer of more than `keep` elements and the index buffer of the other width; all of them by default.
  void release(size_t keep = 0, bool wide_ = false);
  size_t bytes() const { return val.n * 4 + idx16.n * 2 + idx32.n * 4; }
  void* idx() const { return wide ? (void*)idx32.p : (void*)idx16.p; }  // the kernels read it as const TI*; k_interleave writes it
};
// One pass of a presort or of a streamed search, on e->stream: evaluates the ordered variables [fb, fb + nf) on rows.N stored samples
// (launch_batch into e->d_out), sorts the rows and interleaves them into t from group group0 on. `mark`, if set, is called before
// each of the three steps (the streamed search's profiling events). Caller holds e->mu.
cc_status fill_sorted_table(cc_evaluator* e, RowSorter& rows, int fb, int nf, SortedTable& t, size_t group0, cc_status (*mark)(cc_evaluator*));
// LBP's (code, sample)-sorted table is built by a presort and searched by a node, unless CCAMD_SPLIT_CAT_STREAM is set
// (test hook: the streamed codes of k_split_cat only). Read at every call: tests compare the two paths.
bool cat_sorted_table_enabled();

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
// Ordered: mode 0 regression, 1 GINI, 2 MISCLASS; the per-variable results stay in e->d_split_out (OrdResult). After a split
// presort (cc_eval_presort_split) the resident head is searched first, then the tail chunk by chunk: evaluated, sorted,
// interleaved into the chunk table and searched by the same kernel, all queued on e->stream without a host wait. With
// track_winner the best variable so far (k_boost_argmax's rule) is kept in e->d_win_state after the head and after every
// chunk, and a chunk that holds it leaves that variable's sorted row in e->d_win_val / e->d_win_idx.
cc_status split_launch_ordered(cc_evaluator* e, int mode, TableForm form, double w_total0, double w_total1, double rsum0,
                               bool track_winner = false);
// Device time of the last split_launch_ordered (head and streamed chunks); the stream has been synchronised.
double split_search_ms(cc_evaluator* e);
// The best variable so far of a streamed search: k_boost_argmax's (quality, variable), quality 0 and variable -1 for none.
struct StreamBest {
  int var;
  float quality;
};
// Categorical: node = stored samples in increasing order; the winner as cc_eval_find_best_split reports it.
cc_status split_categorical_from_table(cc_evaluator* e, bool is_classifier, bool gini, TableForm form, cc_split* out);

}  // namespace ccamd

struct cc_evaluator {
  // ---- store (cc_eval_store.hip): what the evaluator was created for, its catalog and its stored samples ----
  int type = 0, mode = 0, W = 0, H = 0, max_samples = 0, device = 0, cols = 0;
  bool use_tilted = false;
  int S = 16;  // samples per LDS tile of the batch kernels
  std::vector<ccamd::HaarFeature> haar;
  std::vector<int32_t> lbp;
  std::vector<float> cls;
  int nfeat = 0;
  ccamd::OwnStream stream;
  ccamd::SampleTables samples;
  ccamd::DevBuf<ccamd::HaarFeatDev> d_haar;
  ccamd::DevBuf<ccamd::LbpFeatDev> d_lbp;
  uint64_t generation = 0;  // bumped by every presort and setImage(s): what a cc_boost was created against
  std::mutex mu;  // guards the queue, the scratch and the tables below (the calc entry points may be called concurrently)
  // ---- queue and mirror: the single-image path (cc_eval_set_image / cc_eval_calc / cc_eval_calc_list) ----
  // images set one at a time that the device has not seen yet: pixels (W * H each), sample index, and where a sample's
  // latest image sits in the queue (pend_slot[idx], -1 = not queued)
  std::vector<uint8_t> pend_px;
  std::vector<int32_t> pend_idx;
  std::vector<int32_t> pend_slot;
  // host mirror of the sample set LAST by cc_eval_set_image: its integral(s) and norm factor, computed on the host with the
  // device kernels' arithmetic; answers cc_eval_calc / cc_eval_calc_list for that sample without a launch (mirror_answer)
  int mirror_idx = -1;
  std::vector<int32_t> mirror_sum, mirror_tilted;
  float mirror_nf = 0.f;
  std::once_flag host_catalog_once;
  std::vector<ccamd::HaarFeatDev> h_haar;  // catalog with plain fastRect offsets (row stride W + 1)
  std::vector<ccamd::LbpFeatDev> h_lbp;
  // ---- calc scratch: uploads, outputs and the timing of the last batch launch ----
  ccamd::DevBuf<uint8_t> d_imgs;
  ccamd::DevBuf<int32_t> d_idx;
  ccamd::DevBuf<float> d_out;
  ccamd::DevBuf<ccamd::HaarFeatDev> d_custom;
  ccamd::DevBuf<ccamd::HaarFeatDev> d_haar_plain;  // catalog with plain fastRect offsets (cc_eval_calc_list), built on first use
  ccamd::DevBuf<ccamd::LbpFeatDev> d_lbp_plain;
  ccamd::DevBuf<uint8_t> d_pred;
  ccamd::PinnedBuf pin_in, pin_out;
  ccamd::OwnEvent ev_a, ev_b;
  double last_ms = 0;
  // ---- presort (cc_presort.hip) and split search (cc_split.hip) ----
  // resident tables (cc_eval_presort): per group of 64 features the sorted values and sample indices, interleaved so that
  // lane = feature reads are coalesced: [group][rank][64]
  ccamd::SortedTable head;
  ccamd::DevBuf<uint8_t> d_codes;  // LBP: [feature][sample] codes
  int cat_sorted_n = 0;                  // samples per variable in d_cat_sorted (0: not built)
  ccamd::DevBuf<uint32_t> d_cat_sorted;  // LBP: (sample << 8 | code) in (code, sample) order, [group][rank][64]
  int presort_n = 0;                     // samples covered by the tables (0 = none)
  int presort_f0 = 0, presort_f1 = 0;    // variables covered by the tables
  ccamd::DevBuf<double> d_split_tab, d_split_out;
  ccamd::DevBuf<int32_t> d_split_idx;
  // split presort (cc_eval_presort_split): variables [0, presort_resident) of the range have tables; [presort_resident, F)
  // are evaluated, sorted and searched presort_chunk at a time at every node (0: nothing is streamed). The chunk scratch
  // lives as long as the split: the row sorter (with d_out), one chunk table in the resident layout and the winner row.
  int presort_resident = 0, presort_chunk = 0;
  std::unique_ptr<ccamd::RowSorter> stream_rows;
  ccamd::SortedTable chunk;
  ccamd::DevBuf<float> d_win_val;   // the streamed winner's sorted values, [presort_n] ...
  ccamd::DevBuf<int32_t> d_win_idx;  // ... and sample numbers, in the tables' width (16- or 32-bit)
  ccamd::DevBuf<ccamd::StreamBest> d_win_state;
  ccamd::OwnEvent ev_stream_a;  // start of a streamed search (launch_batch re-records ev_a for every chunk)
  // cc_eval_stream_profile: six events per chunk (before evaluate, after evaluate, sort, interleave, search, winner) and the
  // sums of their distances over the last streamed search, read once the stream has been synchronised (split_search_ms)
  bool stream_profile = false;
  std::vector<ccamd::OwnEvent> stream_ev;
  size_t stream_ev_used = 0;
  double stream_phase_ms[5] = {};
  ccamd::OwnEvent ev_piece[8];  // categorical search: one per piece of the sums on its way back
  // ---- HOG (cc_hog.hip) ----
  // catalog blocks [n][4] = x, y, cell w, cell h; samples.hog holds [max_samples][cols][10] (9 bins, then norm); nfeat counts
  // variables (blocks * 36). mirror_hog is the host mirror of the last window, read and written under mu.
  std::vector<int32_t> hog_blocks;
  ccamd::DevBuf<int32_t> d_hog_blocks;
  int hog_planes_per_pass = 0;  // k_hog_set_images' plan (hog_lds_plan, cc_hog_device.h), fixed by hog_init:
  size_t hog_set_lds = 0;       // planes per LDS pass and the dynamic LDS per workgroup that goes with them
  std::vector<float> mirror_hog;
  // ---- fill (cc_fill.hip) ----
  // cc_eval_fill_passed sets a chunk of candidates into these scratch rows, predicts them there and copies the kept rows
  // to their slots in `samples`
  ccamd::SampleTables fill_rows;
  ccamd::FillWork fill;
};
