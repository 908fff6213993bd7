/*
 * cascadeclassifier_amd.h — C ABI of the MI355X-native cascade-classifier hot path.
 *
 * Drop-in boundary for ONE path of vladiant/CascadeClassifier: integral-image construction and
 * Haar / LBP per-window feature evaluation over the sliding-window / scale pyramid, as used by the
 * detection tool and by CvCascadeBoost stage training. Everything behind these entry points runs as
 * hand-written HIP kernels on gfx950; there is NO CPU fallback: without a usable HIP device every
 * compute entry point fails with CC_ERR_NO_DEVICE.
 *
 * Each group names the reference interface it replaces (paths relative to the reference repo root).
 *
 * Conventions: plain C types; opaque handles; caller-owned buffers; every function returns a
 * cc_status (0 = OK, < 0 = error) unless documented otherwise; cc_last_error() returns a
 * thread-local, human-readable message for the last failing call on the calling thread. No
 * exceptions cross this boundary. Handles are thread-compatible (one thread at a time per handle);
 * cc_eval_calc* are safe for concurrent callers once cc_eval_set_image(s) has returned, as the
 * reference's const operator() is (traincascade/lib/src/o_cvcascadeboosttraindata.cpp:586-594).
 */
#ifndef CASCADECLASSIFIER_AMD_H_
#define CASCADECLASSIFIER_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define CC_API __attribute__((visibility("default")))
#else
#define CC_API
#endif

typedef int cc_status;
enum {
  CC_OK = 0,
  CC_ERR_INVALID_ARG = -1,      /* CV_Assert-class failures in the reference (features.cpp:75,85-87) */
  CC_ERR_NO_DEVICE = -2,        /* HIP runtime / gfx950 device not usable: the product has no CPU path */
  CC_ERR_HIP = -3,              /* a HIP call failed; message carries hipGetErrorString */
  CC_ERR_IO = -4,               /* file cannot be opened / read */
  CC_ERR_PARSE = -5,            /* malformed cascade XML */
  CC_ERR_UNSUPPORTED = -6,      /* valid input the GPU path does not implement yet (message says which) */
  CC_ERR_BUFFER_TOO_SMALL = -7, /* output capacity too small; the required size is reported */
  CC_ERR_OUT_OF_RANGE = -8,
  CC_ERR_NO_TRAIN_PARAMS = -9   /* a cascade file or model without training parameters (section 6d); not a parse error */
};

CC_API const char* cc_last_error(void);
CC_API int cc_version(void);
/* Number of usable HIP devices (0 when there is none or the runtime cannot initialise). */
CC_API int cc_device_count(void);

typedef struct cc_rect {
  int32_t x, y, width, height;
} cc_rect;

/* ============================================================================================
 * 1. Cascade model (cascade.xml, new format).
 *    Replaces: cv::CascadeClassifier(const String&) / load() / empty() as called at
 *    tools/detection/Cpp/main.cpp:42 and tools/detection/Python/detect.py:16; the format is the one
 *    written by CvCascadeClassifier::save (traincascade/lib/src/cascadeclassifier.cpp:439-456,
 *    tags traincascade/lib/include/cascadeclassifier.h:27-73).
 * ============================================================================================ */
typedef struct cc_cascade cc_cascade;

enum { CC_FEATURE_HAAR = 0, CC_FEATURE_LBP = 1, CC_FEATURE_HOG = 2 };

typedef struct cc_cascade_info {
  int32_t feature_type; /* CC_FEATURE_* */
  int32_t win_w, win_h;
  int32_t n_stages, n_weak, n_nodes, n_leaves, n_features;
  int32_t max_cat_count, subset_size;
  int32_t max_nodes_per_tree; /* 1 => stump cascade */
  int32_t has_tilted;
} cc_cascade_info;

CC_API cc_status cc_cascade_load_xml(const char* path, cc_cascade** out);
CC_API cc_status cc_cascade_load_xml_mem(const char* text, size_t len, cc_cascade** out);
CC_API void cc_cascade_destroy(cc_cascade* c);
CC_API cc_status cc_cascade_info_get(const cc_cascade* c, cc_cascade_info* info);
/* Flat views of the parsed model (for inspection / parity tests). Arrays are owned by the cascade. */
CC_API cc_status cc_cascade_stages(const cc_cascade* c, const int32_t** first_weak, const int32_t** n_weak,
                                   const float** threshold /* (float)stageThreshold - 1e-5f */);
/* Stump view (valid when max_nodes_per_tree == 1): per weak classifier feature index, threshold, leaf values and
 * (LBP) subset_size int32 words of category mask. */
CC_API cc_status cc_cascade_stumps(const cc_cascade* c, const int32_t** feature_idx, const float** threshold,
                                   const float** left, const float** right, const int32_t** subsets);
/* Haar: rects as int32[n_features][3][4] (x y w h), weights float[n_features][3], tilted int32[n_features].
 * LBP:  rects as int32[n_features][4]; weights / tilted are NULL.
 * HOG:  rects as int32[n_features][5] = x y w h of the block's cell 0 and the component in [0, 36) (cell comp / 9, bin
 *       comp % 9; HOGfeatures.cpp:155-160); weights / tilted are NULL. A HOG variable's value is the evaluator's
 *       (section 4). */
CC_API cc_status cc_cascade_features(const cc_cascade* c, const int32_t** rects, const float** weights,
                                     const int32_t** tilted);

/* Writes the model back as a new-format cascade.xml (the layout of CvCascadeClassifier::save,
 * traincascade/lib/src/cascadeclassifier.cpp:439-456; stages boost.cpp:520-532, trees o_cvcascadeboosttree.cpp:41-93,
 * features haarfeatures.cpp:311-320 / lbpfeatures.cpp:65-68 / HOGfeatures.cpp:155-160). Reading the written file yields
 * an identical model. */
CC_API cc_status cc_cascade_save_xml(const cc_cascade* c, const char* path);

/* The legacy "baseFormat" layout of CvCascadeClassifier::save(filename, true) (cascadeclassifier.cpp:421-437 tag names,
 * :457-531 writer): <cascade type_id="opencv-haar-classifier"> with <size>, per stage <trees> (nodes breadth-first from
 * the root, inner children numbered as they are queued; <feature> = Feature::write, haarfeatures.cpp:311-320; <threshold>,
 * <left_val>/<left_node>, <right_val>/<right_node>), <stage_threshold>, <parent> = stage - 1, <next> = -1.
 * Haar cascades only: anything else returns CC_ERR_UNSUPPORTED with the reference's message (:461-462). Write-only, as
 * in the reference; cc_cascade_load_xml refuses this layout. */
CC_API cc_status cc_cascade_save_xml_legacy(const cc_cascade* c, const char* path);

/* .vec sample files (positives of the trainer): header int32 count, int32 width*height, 2 x int16 0; per sample one zero
 * byte + width*height int16 pixels. Reader: CvCascadeImageReader::PosReader (traincascade/lib/src/imagestorage.cpp:138-182);
 * writer: icvWriteVecHeader / icvWriteVecSample (tools/createsamples/utility.cpp:128-152). Host-side file IO.
 * cc_vec_read: *count / *vec_size are always set when the header parses; pixels (count * vec_size bytes, may be NULL to
 * query the sizes) receives at most cap_samples samples, each pixel narrowed to 8 bits as the reader does. */
CC_API cc_status cc_vec_read(const char* path, int32_t* count, int32_t* vec_size, uint8_t* pixels, int cap_samples);
CC_API cc_status cc_vec_write(const char* path, const uint8_t* pixels, int count, int width, int height);

/* ============================================================================================
 * 2. Detector.
 *    Replaces: cv::CascadeClassifier::detectMultiScale(gray, objects, scaleFactor, minNeighbors, flags,
 *    minSize, maxSize) as called at tools/detection/Cpp/main.cpp:45 (gray, objects, 4, 50) and
 *    tools/detection/Python/detect.py:22; internally cv::resize(INTER_LINEAR_EXACT), cv::integral and
 *    cv::groupRectangles (OpenCV 4.6.0, external/CMakeLists.txt:11).
 * ============================================================================================ */
typedef struct cc_detector cc_detector;

typedef struct cc_detect_params {
  double scale_factor;   /* > 1 */
  int32_t min_neighbors; /* groupRectangles threshold; <= 0 returns ungrouped candidates */
  int32_t min_w, min_h;  /* 0 = no limit */
  int32_t max_w, max_h;  /* 0 = image size */
} cc_detect_params;

/* device: HIP device ordinal. max_batch: frames processed per pass (workspace is sized for it). Haar and LBP cascades:
 * a HOG cascade returns CC_ERR_UNSUPPORTED (nothing in the reference defines detection with one; OpenCV cannot run them
 * either), as do cc_detector_specialize(_async) and cc_cascade_compile_specialized. */
CC_API cc_status cc_detector_create(const cc_cascade* c, int device, int max_batch, cc_detector** out);
CC_API void cc_detector_destroy(cc_detector* d);
/* Use the caller's HIP stream (hipStream_t) for all work of this detector; NULL = detector's own stream. */
CC_API cc_status cc_detector_set_stream(cc_detector* d, void* hip_stream);

/* One frame, host memory. out receives at most cap rectangles; *n = number found (if *n > cap the call returns
 * CC_ERR_BUFFER_TOO_SMALL and fills the first cap). Rectangle order: class order of cv::groupRectangles for
 * candidates sorted (scale, y, x), i.e. OpenCV's single-threaded order. */
CC_API cc_status cc_detect_multiscale(cc_detector* d, const uint8_t* gray, int width, int height, size_t row_stride,
                                      const cc_detect_params* p, cc_rect* out, int cap, int* n);

/* Pixel formats of the _fmt entry points and cc_to_gray_u8. Colour frames are converted on the device to the gray the
 * detector runs on, as OpenCV's 8-bit COLOR_BGR2GRAY / COLOR_RGB2GRAY (RGB2Gray<uchar>, color_rgb.simd.hpp) compute it:
 *   gray = (B * 1868 + G * 9617 + R * 4899 + 8192) >> 14      (exact integer arithmetic; a 4th channel is ignored)
 * -- which is NOT PIL's convert("L"). Parity with an installed OpenCV is unpinned, like the rest of the detection side
 * (OpenCV is not part of the build). The gray frames are then exactly what a caller converting on the host would pass.
 *   CC_PIX_GRAY8        one byte per pixel (the plain entry points)
 *   CC_PIX_BGR8/BGRA8   interleaved, OpenCV's order (cv::imread, the reference's detection tool)
 *   CC_PIX_RGB8/RGBA8   interleaved, PIL / PPM / torch HWC order
 *   CC_PIX_RGB8_PLANAR  CHW: planes R, G, B of row_stride * height bytes each, back to back (torchvision decoders)
 * row_stride / frame_stride are in BYTES; a row holds width * bytes-per-pixel bytes (width for the planar format). */
enum { CC_PIX_GRAY8 = 0, CC_PIX_BGR8 = 1, CC_PIX_BGRA8 = 2, CC_PIX_RGB8 = 3, CC_PIX_RGBA8 = 4, CC_PIX_RGB8_PLANAR = 5 };

/* Batch of equally sized frames. frames points to HOST memory (on_device = 0) or to DEVICE memory of the detector's
 * device (on_device = 1; e.g. a torch tensor's data_ptr): frame f starts at frames + f * frame_stride.
 * Output: rectangles of frame f are out[offsets[f] .. offsets[f+1]); offsets has n_frames + 1 entries. */
CC_API cc_status cc_detect_batch(cc_detector* d, const uint8_t* frames, int on_device, int n_frames, int width,
                                 int height, size_t row_stride, size_t frame_stride, const cc_detect_params* p,
                                 cc_rect* out, int cap, int32_t* offsets);

/* Same, but only the device pipeline (pyramid, integrals, cascade evaluation, skip-rule filter): candidates stay on
 * the device, nothing is copied back or grouped. For benchmarking the kernels. */
CC_API cc_status cc_detect_batch_device_only(cc_detector* d, const uint8_t* frames, int on_device, int n_frames,
                                             int width, int height, size_t row_stride, size_t frame_stride,
                                             const cc_detect_params* p);

/* cc_detect_batch in two halves, for streams of batches (video): submit launches the batch and returns while its last
 * pass still runs; collect waits for it and returns what cc_detect_batch would have returned (same rectangles, same
 * order, same status codes). Submitting batch k + 1 BEFORE collecting batch k lets the pyramid / integral work of the new
 * batch run under the cascade kernel of the old one and the host side of the old batch's last pass (copy-back, grouping)
 * under the device side of the new one -- the two parts of a synchronous call that nothing overlaps. At most one batch
 * is left unfetched inside the detector: a later submit (or any other detection call) fetches it first; results stay in
 * the ticket until collect. DEVICE frames must stay valid until the batch is collected; HOST frames are copied into the
 * detector's pinned staging area inside submit (three slots; the copy to the device is asynchronous on the front stream and a
 * pass's frames are staged one pass ahead of its kernels) and may be reused as soon as submit returns -- unless they already
 * live in pinned memory (hipHostMalloc / hipHostRegister): those are copied straight from the caller's buffer and must stay valid
 * until the batch is collected. collect frees
 * the ticket, except when it returns CC_ERR_BUFFER_TOO_SMALL (offsets[n_frames] then holds the count: collect again with
 * room for it). cc_detect_batch_discard ends a ticket whose results are not wanted (it waits for the batch's last pass;
 * NULL is accepted); a ticket that is neither collected nor discarded leaks. A ticket is ended only by the detector that
 * issued it: collect / discard with another detector return CC_ERR_INVALID_ARG and leave the ticket valid (collect it
 * with its own detector); after its detector has been destroyed a ticket can only be discarded (with any detector
 * argument, NULL included), collecting it is CC_ERR_INVALID_ARG. No reference counterpart (the reference handles one
 * image per call, tools/detection/Cpp/main.cpp:42-45). */
typedef struct cc_batch_ticket cc_batch_ticket;
CC_API cc_status cc_detect_batch_submit(cc_detector* d, const uint8_t* frames, int on_device, int n_frames, int width,
                                        int height, size_t row_stride, size_t frame_stride, const cc_detect_params* p,
                                        cc_batch_ticket** ticket);
CC_API cc_status cc_detect_batch_collect(cc_detector* d, cc_batch_ticket* ticket, cc_rect* out, int cap, int32_t* offsets);
CC_API cc_status cc_detect_batch_discard(cc_detector* d, cc_batch_ticket* ticket);

/* The _fmt twins take frames in any CC_PIX_* format (after the geometry); the plain calls are these with CC_PIX_GRAY8.
 * CC_ERR_INVALID_ARG for an unknown format, row_stride < width * bytes-per-pixel, or (n_frames > 1) a frame_stride
 * shorter than one frame of the format. Colour frames become gray on the device in the pass's staging slot: host frames
 * are copied as they are (one colour buffer on the device, allocated on first use) and converted by a kernel on the
 * stream that builds the pyramid; device frames are converted straight from the caller's buffer, which must stay valid
 * until the batch is collected, as for gray. A colour single-image call is one hipGraph launch too (one graph per scale
 * plan and pixel format). With profiling on the conversion's time counts under resize_ms (and resize_launches). */
CC_API cc_status cc_detect_multiscale_fmt(cc_detector* d, const uint8_t* img, int width, int height, size_t row_stride,
                                          int pixel_format, const cc_detect_params* p, cc_rect* out, int cap, int* n);
CC_API cc_status cc_detect_batch_fmt(cc_detector* d, const uint8_t* frames, int on_device, int n_frames, int width,
                                     int height, size_t row_stride, size_t frame_stride, int pixel_format,
                                     const cc_detect_params* p, cc_rect* out, int cap, int32_t* offsets);
CC_API cc_status cc_detect_batch_submit_fmt(cc_detector* d, const uint8_t* frames, int on_device, int n_frames, int width,
                                            int height, size_t row_stride, size_t frame_stride, int pixel_format,
                                            const cc_detect_params* p, cc_batch_ticket** ticket);

/* cc_detect_batch_fmt whose out / offsets are DEVICE memory of the detector's device (cap rectangles, n_frames + 1 offsets),
 * for callers whose next stage runs on the same card. No candidate is copied to the host and no host thread sorts or groups:
 * each pass's candidates are ordered and grouped by kernels on the detector's stream (cc_group_rectangles_device below is
 * the grouping on its own), frames of later passes append behind earlier ones, and per pass the host reads back only the pass's two
 * counters (8 bytes: the raw candidate count, which triggers the grow-and-rerun of an overflowing candidate list, and the
 * filtered count). Same rectangles, same order as
 * cc_detect_batch_fmt. The call returns when out / offsets are complete on the detector's stream. *n_total (host) = rectangles
 * over all frames; if it exceeds cap: CC_ERR_BUFFER_TOO_SMALL, offsets still complete, out holds the first cap. A batch
 * submitted earlier and still unfetched is retired first. Work of the caller that still touches out / offsets on another
 * stream must have finished before the call (the detector writes them on its own stream, or the one set with
 * cc_detector_set_stream). The outputRejectLevels variant is cc_detect_batch_to_device_levels below. Out of scope for both:
 * a submit / collect pair and a single-image hipGraph (one frame runs as an ordinary pass). */
CC_API cc_status cc_detect_batch_to_device(cc_detector* d, const uint8_t* frames, int on_device, int n_frames, int width,
                                           int height, size_t row_stride, size_t frame_stride, int pixel_format,
                                           const cc_detect_params* p, cc_rect* d_out, int cap, int32_t* d_offsets,
                                           int* n_total);

/* The outputRejectLevels overload of cv::CascadeClassifier::detectMultiScale (objects, rejectLevels, levelWeights,
 * ..., outputRejectLevels = true; OpenCV 4.6.0 objdetect, no call site in the reference: SURVEY.md 8f-4). Windows that
 * pass every stage are reported with level = number of stages and weight = the stage sum of the last stage; the
 * grouping keeps, per class, the highest level and among its members the largest weight (cv::groupRectangles with
 * weights). Parity unpinned like the rest of the detection side. out / reject_levels / level_weights hold cap entries. */
CC_API cc_status cc_detect_multiscale_levels(cc_detector* d, const uint8_t* gray, int width, int height, size_t row_stride,
                                             const cc_detect_params* p, cc_rect* out, int32_t* reject_levels,
                                             double* level_weights, int cap, int* n);

CC_API cc_status cc_detect_multiscale_levels_fmt(cc_detector* d, const uint8_t* img, int width, int height,
                                                 size_t row_stride, int pixel_format, const cc_detect_params* p,
                                                 cc_rect* out, int32_t* reject_levels, double* level_weights, int cap,
                                                 int* n);

/* cc_detect_batch_fmt with the scores of cc_detect_multiscale_levels_fmt: the same passes, each grouped on the host with
 * levels and weights. reject_levels / level_weights hold cap entries like out; frame f's entries are [offsets[f],
 * offsets[f+1]) of all three arrays, and they are what cc_detect_multiscale_levels_fmt returns for that frame. On
 * CC_ERR_BUFFER_TOO_SMALL the offsets are complete and the three arrays hold their first cap entries. There is no scored
 * submit / collect pair. No reference counterpart (one image per call, tools/detection/Cpp/main.cpp:42-45). */
CC_API cc_status cc_detect_batch_levels_fmt(cc_detector* d, const uint8_t* frames, int on_device, int n_frames, int width,
                                            int height, size_t row_stride, size_t frame_stride, int pixel_format,
                                            const cc_detect_params* p, cc_rect* out, int32_t* reject_levels,
                                            double* level_weights, int cap, int32_t* offsets);

/* cc_detect_batch_to_device with scores: d_levels / d_weights are DEVICE memory of cap entries beside d_out (both required).
 * Same rectangles and offsets as cc_detect_batch_to_device; level = number of stages; weight = the largest last-stage sum
 * among the group's members (cc_group_rectangles_device_levels is this grouping on its own), or with min_neighbors <= 0
 * each candidate's own sum, in (scale, gy, gx) order: what cc_detect_batch_levels_fmt returns. Passes append at the running
 * total, and a pass redone after its candidate list overflowed carries its scores. A detector allocates the scored
 * workspace with its first scored call. Out of scope as for the unscored call: submit / collect, a single-image hipGraph. */
CC_API cc_status cc_detect_batch_to_device_levels(cc_detector* d, const uint8_t* frames, int on_device, int n_frames,
                                                  int width, int height, size_t row_stride, size_t frame_stride,
                                                  int pixel_format, const cc_detect_params* p, cc_rect* d_out,
                                                  int32_t* d_levels, double* d_weights, int cap, int32_t* d_offsets,
                                                  int* n_total);

/* Ungrouped candidates of one frame, as int32[7] = {scale_idx, gx, gy, x, y, w, h}, sorted (scale, gy, gx). */
CC_API cc_status cc_detect_raw(cc_detector* d, const uint8_t* gray, int width, int height, size_t row_stride,
                               const cc_detect_params* p, int32_t* cand, int cap, int* n);

/* Parity instrumentation: per grid window result of runAt for one frame, all scales concatenated scale-major,
 * row-major [gy][gx]: codes: 1 pass, -k rejected at stage k (0 = stage 0), -1 window rejected before stage 0
 * (variance test); sums: stage accumulator (double) at exit; visited: 1 when OpenCV's scan loop visits the window
 * (stage-0 skip rule). Any of the three may be NULL. n_windows = capacity / total count. */
CC_API cc_status cc_detect_debug_windows(cc_detector* d, const uint8_t* gray, int width, int height, size_t row_stride,
                                         const cc_detect_params* p, int32_t* codes, double* sums, uint8_t* visited,
                                         int64_t cap, int64_t* n_windows);

/* Scale pyramid geometry for an image size (host computation only; no device needed). */
typedef struct cc_scale_info {
  float scale;
  int32_t width, height; /* resized image */
  int32_t ystep;
  int32_t nx, ny;        /* grid windows enumerated along x / y */
  int32_t win_w, win_h;  /* emitted rectangle size */
} cc_scale_info;
CC_API cc_status cc_scale_plan(int win_w, int win_h, int width, int height, const cc_detect_params* p,
                               cc_scale_info* out, int cap, int* n);

/* Run-time specialisation of the cascade kernel for THIS detector's cascade (Haar or LBP stump cascades): the first n_stages
 * stages (whole stages, capped by a code-size budget) are compiled with hiprtc into straight-line code whose LDS offsets,
 * weights, thresholds and leaf values are immediates; later stages stay table-driven. Same arithmetic, identical results;
 * the cascade kernel runs about 17 % faster on the bench cascade. Takes a few seconds the first time; code objects are
 * cached per process and on disk ($CCAMD_CACHE_DIR, default ~/.cache/cascadeclassifier_amd; set it empty to disable),
 * keyed by architecture, options and generated source. libhiprtc is loaded on demand and a missing library is CC_ERR_UNSUPPORTED, in which case the detector keeps
 * using the table-driven kernel. n_stages <= 0 switches back. cc_detector_specialized_stages reports the stages in
 * effect (0 = none). cc_cascade_compile_specialized only compiles (no device needed; arch e.g. "gfx950") and returns
 * the code-object size: the build check of the generated source. */
CC_API cc_status cc_detector_specialize(cc_detector* d, int n_stages);
/* Same, without waiting: generation and compilation run on a background host thread while detection continues on the
 * table-driven kernel; the first detection call after the build has finished loads the module and switches over
 * (cc_detector_specialized_stages tells when). CCAMD_AUTO_SPECIALIZE=<stages> in the environment does this for every
 * detector at creation, i.e. without any change to the calling code. */
CC_API cc_status cc_detector_specialize_async(cc_detector* d, int n_stages);
CC_API int cc_detector_specialized_stages(const cc_detector* d);
CC_API cc_status cc_cascade_compile_specialized(const cc_cascade* c, int n_stages, const char* arch, size_t* code_bytes);

/* Per-kernel device time accumulated since the last reset, measured with HIP events on the detector's streams.
 * Profiling is off by default (no events are recorded). A synchronous detection call reads its events before it
 * returns; a submitted batch (cc_detect_batch_submit) does not wait for them: cc_detector_get_timings first waits for the
 * detector's streams and reads what is outstanding. */
typedef struct cc_detector_timings {
  double resize_ms, integral_ms, eval_ms, finalize_ms;
  int64_t resize_launches, integral_launches, eval_launches, finalize_launches;
  int64_t frames;         /* frames processed */
  int64_t grid_windows;   /* grid windows evaluated */
  int64_t integral_elems; /* integral entries per channel produced */
  /* eval_ms spans ALL cascade-kernel launches of a pass (eval_launches counts passes). A run-time specialised Haar kernel is
   * one module per step (k_eval_spec_step2 over the tiles of STEP-2 scales, then k_eval_spec_step1): eval_step1_ms is the
   * part of eval_ms the STEP-1 module's launches took (0 when the pass is a single launch). */
  double eval_step1_ms;
  /* cc_detect_batch_to_device only: the ordering and grouping kernels behind k_filter_candidates (cc_group.hip), one span per
   * pass (group_launches counts passes, a pass redone after a candidate-list overflow twice). Not part of finalize_ms, which
   * stays k_filter_candidates alone. */
  double group_ms;
  int64_t group_launches;
} cc_detector_timings;
CC_API cc_status cc_detector_set_profiling(cc_detector* d, int enabled);
/* Entries of the detector's per-pass candidate lists: 0 until a first pass has sized them (262 144 then), larger after a pass
 * overflowed them and was redone. -1 for a null detector. */
CC_API int cc_detector_candidate_capacity(const cc_detector* d);
CC_API cc_status cc_detector_get_timings(cc_detector* d, cc_detector_timings* t, int reset);
/* Single-image calls (cc_detect_multiscale on a host image; the call shape of tools/detection/Cpp/main.cpp:45) replay
 * the whole device pass from one hipGraph once a first ordinary call has sized the buffers. Returns 1 if the LAST such
 * call was a graph launch, 0 if it used ordinary launches (first call, changed geometry, graphs switched off, or a
 * capture that did not come out: then the detector stays on ordinary launches), negative cc_status on a null handle. */
CC_API int cc_detector_graph_active(const cc_detector* d);
/* Number of hipGraph captures this detector has made (one per scale plan and pixel format while its buffers keep their
 * sizes): a replayed call does not add to it. Negative cc_status on a null handle. */
CC_API int64_t cc_detector_graph_captures(const cc_detector* d);

/* ============================================================================================
 * 3. Building blocks exposed for parity tests and roofline measurement (all run on the device).
 *    Replace: cv::integral (traincascade/lib/src/haarfeatures.cpp:109,112, lbpfeatures.cpp:27),
 *    cv::resize INTER_LINEAR_EXACT (traincascade/lib/src/imagestorage.cpp:86,117), cv::groupRectangles.
 * ============================================================================================ */
/* sum / sqsum / tilted: (height+1) x (width+1) int32, densely packed; sqsum is the detector's CV_32S variant
 * (wrap-around accumulation); any output may be NULL. */
CC_API cc_status cc_integral_u8(int device, const uint8_t* img, int width, int height, size_t row_stride, int32_t* sum,
                                int32_t* sqsum, int32_t* tilted);
CC_API cc_status cc_resize_linear_exact_u8(int device, const uint8_t* src, int sw, int sh, size_t sstride, uint8_t* dst,
                                           int dw, int dh, size_t dstride);
/* cv::resize INTER_AREA of one 8-bit single-channel HOST image to dw x dh (dst: dh rows of dw bytes, dense), with the kernel
 * and the arithmetic of the -info mode (section 8: same-size copy, the integer-ratio fast path, the general float path).
 * 1 <= dw <= w <= 8192, 1 <= dh <= h <= 8192, dw and dh at most 4096; an integer ratio whose block sum could pass 2^31 is
 * CC_ERR_INVALID_ARG. */
CC_API cc_status cc_resize_area_u8(int device, const uint8_t* src, int w, int h, size_t stride, uint8_t* dst, int dw, int dh);
/* cvWarpPerspective of the sample tool (tools/createsamples/utility.cpp:225-417) on one HOST image: the source is mapped
 * into the quadrangle quad[4][2] (x, y per vertex, in order) of the caller-initialised dst; pixels outside the quadrangle's
 * row spans keep their value. Coefficients and spans come from the host arithmetic of cc_sample_plan (section 8), the pixels
 * from the device function the sample renderer uses. A nonconvex or degenerate quadrangle is CC_ERR_INVALID_ARG (the
 * reference throws, :274-276), checked before the device is. Sides 1..16384. */
CC_API cc_status cc_warp_perspective_u8(int device, const uint8_t* src, int sw, int sh, size_t sstride, uint8_t* dst, int dw,
                                        int dh, size_t dstride, const double* quad);
/* The detector's colour conversion (CC_PIX_*, section 2) on one HOST image: dst receives height rows of width gray bytes,
 * dst_stride apart. The device copy of src keeps its byte offset modulo 16 and its row stride, so that odd base addresses
 * and strides reach the kernel as they are. CC_PIX_GRAY8 is copied unchanged (its three weights sum to 2^14). */
CC_API cc_status cc_to_gray_u8(int device, const uint8_t* src, int pixel_format, int width, int height, size_t row_stride,
                               uint8_t* dst, size_t dst_stride);
/* Profiling aid: streams n_bytes of device memory once with the cascade kernel's load shape (one dword per lane,
 * 64 consecutive lanes) so that the FETCH_SIZE counter can be calibrated on a known byte count
 * (MI355X_MICROARCH.md, HBM section). *checksum receives the wrapped 32-bit sum of the words read. */
CC_API cc_status cc_debug_stream_dwords(int device, size_t n_bytes, int repeats, uint32_t* checksum);
/* Parity instrumentation: the bulk evaluator divides by a sample's norm factor with the operand-independent half of the
 * IEEE division hoisted out of the feature loop (cc_eval_calc.hip: div_by_refined). Compares it with the division operator
 * on the device for n_pairs pseudo-random operand pairs of the evaluator's value ranges (x2: arbitrary floats and
 * integer-valued dividends over sqrt-shaped divisors); *mismatches must come back 0. */
CC_API cc_status cc_debug_division_check(int device, uint64_t n_pairs, uint64_t seed, uint64_t* mismatches);
/* Same kind of check for the cascade kernel's variance normalisation: counts values nf = area * valsqsum - valsum^2 (drawn
 * as the kernels form them) for which the refined-rsqrt path differs from (float)(1.0 / sqrt(nf)), the CPU's two correctly
 * rounded operations (cv::CascadeClassifier setWindow). Must report 0. */
CC_API cc_status cc_debug_vnf_check(int device, uint64_t n_values, uint64_t seed, uint64_t* mismatches);
/* Host only, no device: the tables behind the integer form of the Haar cascade kernel's wave phase, as a detector created
 * from `c` now (CCAMD_WAVE_INT is read) builds them. Per stage: q[s] = the quantum 2^k of the stage's leaves, 0 where the
 * stage sums stay in double (no int32 range proof, a NaN threshold, not a Haar stump cascade with order-independent sums,
 * CCAMD_WAVE_INT=0); thr_q[s] = the smallest int32 n with n * q[s] >= the stage threshold as cc_cascade_stages reports it,
 * saturated to the int32 limits. Per weak classifier, in cc_cascade_stumps order: left_q / right_q = the leaves in units of
 * their stage's quantum. Entries of stages without the form are 0. q / thr_q hold n_stages entries, left_q / right_q n_weak;
 * any may be NULL. */
CC_API cc_status cc_debug_wave_int_tables(const cc_cascade* c, double* q, int32_t* thr_q, int32_t* left_q, int32_t* right_q);
/* Host only, no device: what the run-time specialised kernel's module of STEP-1 tiles would be built with for the Haar stump
 * cascade `c` (32-bit tiles, a module per step). rows_wanted > 0: tiles of that many window rows, as CCAMD_SPEC_TILE_Y1
 * would ask for; <= 0: the library's choice, i.e. its default height or, for a window too large for that, the tallest
 * height below it at which four blocks still share a CU (8 rows where none does). Out: *rows = window rows per tile, *lds_bytes = the dynamic LDS
 * request of one block (eval_lds_bytes, lean layout), *blocks_per_cu = blocks that request lets share the 160 KiB of a CU
 * (at most 8) = the wavefronts per SIMD the module's register budget is compiled for, *wave_below = EvalArgs::wave_below of the
 * module's launches given the detector-wide value `wave_below_detector` (24 for such a cascade). Any may be NULL.
 * CC_ERR_UNSUPPORTED for cascades that do not get such a module (LBP, HOG, trees, tilted features). */
CC_API cc_status cc_debug_spec_step1_plan(const cc_cascade* c, int rows_wanted, int wave_below_detector, int* rows, size_t* lds_bytes,
                                          int* blocks_per_cu, int* wave_below);
/* The same for the module of STEP-2 tiles. rows_wanted > 0: any height from 8 to 12, as CCAMD_SPEC_TILE_Y2 would ask for;
 * <= 0: the library's choice, the tallest such height at which as many blocks share a CU as at 8 rows. *blocks_per_cu counts
 * the request in LDS allocation units of 1 280 bytes (lds_blocks_resident). */
CC_API cc_status cc_debug_spec_step2_plan(const cc_cascade* c, int rows_wanted, int wave_below_detector, int* rows, size_t* lds_bytes,
                                          int* blocks_per_cu, int* wave_below);
/* Host-side (tiny, serial in the reference too): cv::groupRectangles(rects, group_threshold, eps). */
CC_API cc_status cc_group_rectangles(const cc_rect* rects, int n, int group_threshold, double eps, cc_rect* out, int cap,
                                     int* n_out);
/* The device twin of cc_group_rectangles, for many frames at once: rects / offsets / out / out_offsets are DEVICE memory of
 * `device`; frame f's input is rects[offsets[f] .. offsets[f+1]) (n_frames + 1 non-decreasing offsets), its result
 * out[out_offsets[f] .. out_offsets[f+1]). Same result, same order as cc_group_rectangles on each frame. *n_total (host) =
 * rectangles over all frames; if it exceeds cap: CC_ERR_BUFFER_TOO_SMALL, out_offsets still complete, out holds the first
 * cap. Blocking, on a stream of its own: work of the caller that still touches the buffers must have finished. Allocates its
 * own workspace (the detector keeps one). */
CC_API cc_status cc_group_rectangles_device(int device, const cc_rect* rects, const int32_t* offsets, int n_frames,
                                            int group_threshold, double eps, cc_rect* out, int cap, int32_t* out_offsets,
                                            int* n_total);
/* Host-side cv::groupRectangles(rects, rejectLevels, levelWeights, group_threshold, eps), the grouping of detectMultiScale's
 * outputRejectLevels overload (OpenCV 4.6.0 objdetect, no call site in the reference: SURVEY.md 8f-4): a kept class has
 * level max(0, highest member level) and the largest weight among its members at that level, counted from DBL_MIN when no
 * member's level exceeded 0. levels / weights: n entries; out / out_levels / out_weights: cap entries. group_threshold <= 0
 * copies all three through. */
CC_API cc_status cc_group_rectangles_levels(const cc_rect* rects, const int32_t* levels, const double* weights, int n,
                                            int group_threshold, double eps, cc_rect* out, int32_t* out_levels,
                                            double* out_weights, int cap, int* n_out);
/* The device twin of cc_group_rectangles_levels, as cc_group_rectangles_device is of cc_group_rectangles: levels / weights lie
 * beside rects, out_levels / out_weights beside out, all in DEVICE memory. Same result, same order as
 * cc_group_rectangles_levels on each frame; on CC_ERR_BUFFER_TOO_SMALL out_offsets are complete and all three outputs hold
 * their first cap entries. Argument checks as for the unscored call. Weights are compared by value: where the best
 * weights of a class are +0.0 and -0.0, either may come out (the host keeps the first it meets, the device +0.0). NaN
 * weights are outside the contract. */
CC_API cc_status cc_group_rectangles_device_levels(int device, const cc_rect* rects, const int32_t* levels,
                                                   const double* weights, const int32_t* offsets, int n_frames,
                                                   int group_threshold, double eps, cc_rect* out, int32_t* out_levels,
                                                   double* out_weights, int cap, int32_t* out_offsets, int* n_total);

/* ============================================================================================
 * 4. Training-side feature evaluator.
 *    Replaces: CvFeatureEvaluator / CvHaarEvaluator / CvLBPEvaluator
 *    (traincascade/lib/include/traincascade_features.h:155-188, haarfeatures.h:61-122, lbpfeatures.h:37-83):
 *    create+init  -> cc_eval_create           (features.cpp:72-81,91-97; haarfeatures.cpp:89-98; lbpfeatures.cpp:15-20)
 *    setImage     -> cc_eval_set_image(s)     (features.cpp:83-89; haarfeatures.cpp:100-114; lbpfeatures.cpp:22-28)
 *    operator()   -> cc_eval_calc / cc_eval_calc_batch (haarfeatures.h:108-122; lbpfeatures.h:44-45,70-83)
 *    getNumFeatures/getMaxCatCount/getFeatureSize/getCls -> cc_eval_* getters
 *    writeFeatures needs only the geometry -> cc_eval_feature_geometry (haarfeatures.cpp:311-320, lbpfeatures.cpp:65-68)
 *    bulk consumer CvCascadeBoostTrainData::precalculate (o_cvcascadeboosttraindata.cpp:490-596) -> cc_eval_calc_batch.
 *
 *    HOG (CvHOGEvaluator, HOGfeatures.h:43-112, HOGfeatures.cpp:16-256): a feature is a block of 2x2 cells and carries
 *    36 variables (4 cells x 9 orientation bins). cc_eval_num_features returns blocks, cc_eval_feature_size 36 and
 *    cc_eval_max_cat_count 0 (every variable ordered). On a HOG evaluator EVERY feature index argument below is a
 *    VARIABLE index vi in [0, num_features * 36): block vi / 36, cell (vi % 36) / 9, bin vi % 9. That covers cc_eval_calc,
 *    cc_eval_calc_list, cc_eval_calc_batch, cc_eval_calc_batch_device, cc_eval_calc_batch_sorted, cc_eval_presort_range
 *    and cc_split.var_idx. cc_eval_feature_geometry, cc_eval_get_sample and cc_eval_calc_custom_haar return
 *    CC_ERR_INVALID_ARG on a HOG evaluator. cc_eval_predict_cascade takes a HOG cascade on a HOG evaluator of the same
 *    window size (the cascade's <rect> names a block's cell 0 and a component, section 1).
 * ============================================================================================ */
typedef struct cc_evaluator cc_evaluator;
enum { CC_HAAR_BASIC = 0, CC_HAAR_CORE = 1, CC_HAAR_ALL = 2 };

CC_API cc_status cc_eval_create(int feature_type, int haar_mode, int win_w, int win_h, int max_samples, int device,
                                cc_evaluator** out);
CC_API void cc_eval_destroy(cc_evaluator* e);
CC_API int cc_eval_num_features(const cc_evaluator* e);
CC_API int cc_eval_max_cat_count(const cc_evaluator* e); /* 0 Haar, 256 LBP, 0 HOG */
CC_API int cc_eval_feature_size(const cc_evaluator* e);  /* 1; HOG: 36 */
/* Haar: rects int32[3][4], weights float[3], *tilted; LBP: rects[0] = one cell (x y w h), weights/tilted untouched. */
CC_API cc_status cc_eval_feature_geometry(const cc_evaluator* e, int fi, int32_t* rects, float* weights, int* tilted);
/* HOG: cells int32[4][4] = x y w h of cell 0 (top-left), 1 (top-right), 2 (bottom-left), 3 (bottom-right) of block
 * feature_idx (HOGfeatures.cpp:120-131). CC_ERR_INVALID_ARG on a Haar / LBP evaluator. */
CC_API cc_status cc_eval_hog_feature_geometry(const cc_evaluator* e, int feature_idx, int32_t* cells);
/* img: win_h rows of win_w bytes, row_stride bytes apart. idx < max_samples.
 * The call does no device work (the trainer makes it per candidate window, cascadeclassifier.cpp:340-347): the pixels are
 * queued -- a later image for the same idx replaces the queued one; the queue reaches the device, runs of consecutive indices
 * per launch, before anything reads stored samples there -- and the integral(s) and norm factor of THIS window are mirrored
 * on the host, from which cc_eval_calc / cc_eval_calc_list answer for idx until the next cc_eval_set_image(s) (SURVEY.md 8b:
 * "scalar, host-mirror fast path"). The mirror's values are bit-identical to the device's for every catalog feature
 * (tests/test_gpu_eval.py::test_host_mirror_of_the_last_set_window_equals_the_device). */
CC_API cc_status cc_eval_set_image(cc_evaluator* e, const uint8_t* img, size_t row_stride, uint8_t cls_label, int idx);
/* n images of win_w x win_h, densely packed, stored at idx first_idx..first_idx+n-1; labels may be NULL (labels kept). */
CC_API cc_status cc_eval_set_images(cc_evaluator* e, const uint8_t* imgs, int n, int first_idx, const uint8_t* labels);
/* Host array of max_samples floats (the reference's `cls` Mat; o_cvcascadeboosttraindata.cpp:238-239 wraps it). */
CC_API const float* cc_eval_labels(const cc_evaluator* e);
/* Scalar operator()(featureIdx, sampleIdx). For the sample set last by cc_eval_set_image: answered from its host mirror, no
 * launch (~20 ns). Any other sample: one device evaluation (slow; prefer the batch / list forms). */
CC_API cc_status cc_eval_calc(cc_evaluator* e, int fi, int si, float* out);
/* out[k] = evaluator(feature_idx[k], si) for an arbitrary list of features and ONE stored sample, in one launch: the call
 * shape of the trainer's stage prediction on a freshly set window (CvCascadeBoostTree::predict ->
 * CvCascadeBoostTrainData::getVarValue, o_cvcascadeboosttree.cpp:16-39, o_cvcascadeboosttraindata.cpp:484-488), which asks
 * for the cascade's features one by one. For the sample set last by cc_eval_set_image the values come from its host mirror;
 * the C++ adaptor batches scalar calls for other samples through this entry point. */
CC_API cc_status cc_eval_calc_list(cc_evaluator* e, const int32_t* feature_idx, int n_feats, int si, float* out);
/* out[(fi - fi_begin) * n_samples + s] = evaluator(fi, sample_idx ? sample_idx[s] : s); out is HOST memory unless
 * out_on_device != 0 (then it is memory of the evaluator's device). */
CC_API cc_status cc_eval_calc_batch(cc_evaluator* e, int fi_begin, int fi_end, const int32_t* sample_idx, int n_samples,
                                    float* out, int out_on_device);
/* The same into DEVICE memory with a row pitch: d_out[(fi - fi_begin) * pitch + s], pitch in elements (0 = n_samples).
 * For consumers that stay on the device (presort, split search, a trainer holding valCache in HBM): the pitch lets rows
 * start on any alignment the consumer likes; measured in round 3, the store rate of the bulk evaluator does not depend
 * on it (profiles/r03_training_kernels.txt). The kernel runs on the evaluator's own non-blocking stream and the call
 * returns when it is done: work of the caller's that writes d_out on another stream (a fill, say) must have finished
 * before the call, or it can land on top of the values. */
CC_API cc_status cc_eval_calc_batch_device(cc_evaluator* e, int fi_begin, int fi_end, const int32_t* sample_idx, int n_samples,
                                           float* d_out, size_t pitch);
/* cc_eval_calc_batch plus, per feature, the argsort of the samples by value: the "sorted index" half of
 * CvCascadeBoostTrainData::precalculate (FeatureValAndIdxPrecalc / FeatureIdxOnlyPrecalc,
 * o_cvcascadeboosttraindata.cpp:490-556: `buf` rows of unsigned short when sample_count < 65536, else int).
 * idx[(fi - fi_begin) * n_samples + k] = index of the sample with the k-th smallest value of feature fi; equal values
 * keep increasing sample order (the reference's std::sort leaves their order unspecified). idx_bytes is 2 or 4
 * (2 requires n_samples <= 65536). vals (float[(fi_end - fi_begin) * n_samples], unsorted, as cc_eval_calc_batch) may be
 * NULL. Host outputs. Samples are 0..n_samples-1. */
CC_API cc_status cc_eval_calc_batch_sorted(cc_evaluator* e, int fi_begin, int fi_end, int n_samples, float* vals, void* idx,
                                           int idx_bytes);
/* Feature::calc (un-normalised) of caller-supplied Haar features on stored samples: the shape of the reference KATs
 * test_features.cpp:462-560. feats: n x {tilted, rects[3][4], weights[3]} as below. */
typedef struct cc_haar_feature {
  int32_t tilted;
  int32_t r[3][4];
  float w[3];
} cc_haar_feature;
CC_API cc_status cc_eval_calc_custom_haar(cc_evaluator* e, const cc_haar_feature* feats, int n_feats, int normalized,
                                          const int32_t* sample_idx, int n_samples, float* out);
/* Feature::calc (haarfeatures.h:114-122) on caller-held flattened integral images: sum / tilted are n_rows rows of
 * row_len int32 (one integral image per row, as the reference's `sum` / `tilted` Mats; either may be NULL if no feature
 * needs it), `step` is the integral's own row stride (window width + 1) used to form the corner offsets exactly as
 * CV_SUM_OFFSETS / CV_TILTED_OFFSETS do. out[f * n_rows + r]. Offsets outside [0, row_len) are rejected. */
CC_API cc_status cc_haar_feature_calc(int device, const cc_haar_feature* feats, int n_feats, int step, const int32_t* sum,
                                      const int32_t* tilted, int n_rows, int row_len, float* out);
/* Cached per-sample data copied back for parity tests: sum / tilted are (win_w+1)*(win_h+1) int32. */
CC_API cc_status cc_eval_get_sample(cc_evaluator* e, int idx, int32_t* sum, int32_t* tilted, float* normfactor);
/* HOG: the integral histograms hist float[9][win_h+1][win_w+1] and the magnitude integral norm float[win_h+1][win_w+1] of
 * stored sample idx (the reference's hist[bin] / normSum rows). Either output may be NULL. */
CC_API cc_status cc_eval_get_hog_sample(cc_evaluator* e, int idx, float* hist, float* norm);
/* Parity instrumentation for HOG: orientation bin and gradient magnitude of every (dx, dy) in [-255, 255]^2 computed on the
 * device with the setImage kernel's per-pixel function; pair (dx, dy) at (dy + 255) * 511 + dx + 255. bin holds 261 121
 * bytes, mag 261 121 floats; *n receives 261 121. */
CC_API cc_status cc_debug_hog_bins(int device, int32_t* n, uint8_t* bin, float* mag);
/* Host only, no device: the LDS plan of a HOG window. *planes_per_pass: how many of the ten integral planes the setImage kernel
 * takes through LDS together, 0 where cc_eval_create refuses the window; *set_budget_kib: the budget that count was chosen
 * under, 64 (no opt-in) or 160; *set_bytes: the setImage kernel's dynamic LDS per workgroup with that count (with one plane per
 * pass where the window is refused); *mine_bytes: the negative miner's dynamic LDS per window, which cc_negminer_create
 * compares with 160 KiB. Any output may be NULL. */
CC_API cc_status cc_debug_hog_lds(int win_w, int win_h, int* planes_per_pass, int* set_budget_kib, int64_t* set_bytes, int64_t* mine_bytes);
/* Training-side cascade predict (CvCascadeClassifier::predict, cascadeclassifier.cpp:297-306 ->
 * boost.cpp:461-477 -> o_cvcascadeboosttree.cpp:16-39) of a stump cascade over stored samples:
 * out[s] = 1 if every stage passes else 0. Feature indices of `c` index the cascade's own <features> list. The cascade's
 * type and window size must be the evaluator's (CC_ERR_INVALID_ARG otherwise). HOG: variable values as operator()
 * computes them on the stored planes, `<=` goes left, stage sums in double over the float leaves. */
CC_API cc_status cc_eval_predict_cascade(cc_evaluator* e, const cc_cascade* c, const int32_t* sample_idx, int n_samples,
                                         uint8_t* out);
CC_API cc_status cc_eval_last_kernel_ms(cc_evaluator* e, double* ms);
/* Test instrumentation: samples per LDS tile of the bulk kernel that cc_eval_create picked from the window (64 = the wide
 * kernel, 32 .. 1 = the narrow one); 0 for a HOG or NULL evaluator. */
CC_API int cc_debug_eval_tile_samples(const cc_evaluator* e);

/* ============================================================================================
 * 5. Batched negative mining over a background image.
 *    Replaces the per-window loop of CvCascadeClassifier::fillPassedSamples for negatives
 *    (traincascade/lib/src/cascadeclassifier.cpp:329-357): NegReader::get (imagestorage.cpp:90-126, one window of
 *    the image's sqrt(2) scale ladder at half-window steps) -> featureEvaluator->setImage (haarfeatures.cpp:100-114)
 *    -> CvCascadeClassifier::predict (cascadeclassifier.cpp:297-306 -> boost.cpp:461-477 ->
 *    o_cvcascadeboosttree.cpp:16-39). One call enumerates the reader's whole window stream for ONE image
 *    (NegReader::nextImg, imagestorage.cpp:57-88, has already chosen the image and the offset), builds each
 *    ladder level and its integral images once, and evaluates the trained stages on every window on the device.
 *    Training-side arithmetic: norm factor sqrt(area*sqsum - sum^2) as float, value = calc / nf (0 if nf == 0),
 *    ordered splits go left on `<=`, a stage passes iff sum >= threshold - 1e-5f.
 *    HOG cascades: no integral images; every window's gradients, bins and ten integral planes are built from the window's
 *    own pixels with replicate borders INSIDE the window (NegReader::get copies the window out and setImage,
 *    HOGfeatures.cpp:163-256, takes its border from that copy), by the device code of the evaluator's setImage, so a mined
 *    window's values are exactly cc_eval_set_image's. cc_negminer_create returns CC_ERR_UNSUPPORTED for a window whose
 *    planes do not fit 160 KiB of LDS (10 * (win_w + 1) * (win_h + 1) floats + 5 bytes per pixel).
 * ============================================================================================ */
typedef struct cc_negminer cc_negminer;
CC_API cc_status cc_negminer_create(const cc_cascade* trained_stages, int device, cc_negminer** out);
CC_API void cc_negminer_destroy(cc_negminer* m);
/* Ladder of one image: level l has size lw[l] x lh[l] and nx[l] x ny[l] window positions (x = ox + i*(win_w/2),
 * y = oy + j*(win_h/2)); the stream visits level 0 first, rows top to bottom, windows left to right. Host only. */
CC_API cc_status cc_negminer_plan(const cc_negminer* m, int width, int height, int ox, int oy, int32_t* lw, int32_t* lh,
                                  int32_t* nx, int32_t* ny, int cap, int* n_levels, int64_t* n_windows);
/* pass[i] = 1 iff stream window i passes every trained stage (i < *n_windows <= cap). If pixels != NULL the first
 * min(max_keep, #passing) passing windows are also copied out, win_w*win_h bytes each, in stream order, with their
 * stream indices in keep_index; *n_keep = how many were written. */
CC_API cc_status cc_negminer_run(cc_negminer* m, const uint8_t* gray, int width, int height, size_t row_stride, int ox, int oy,
                                 uint8_t* pass, int64_t cap, int64_t* n_windows, uint8_t* pixels, int64_t* keep_index,
                                 int max_keep, int* n_keep);
/* The same for n_images (<= 256) images of ONE size consumed with ONE offset -- what NegReader::nextImg hands out between two
 * wraps of its `round` counter over a background set of equal-sized images (imagestorage.cpp:57-88: the offset depends on
 * `round` and the image size only). One copy to the device, one launch of every kernel over all images, one copy back: a call
 * costs about what a single-image call costs. *n_windows = windows PER image; pass[k * *n_windows + i] for image k (cap >=
 * n_images * *n_windows); the kept windows are the first max_keep passing ones in stream order, image 0 first, with
 * keep_index[j] = k * *n_windows + i. A trainer that needs `need` more negatives walks pass[] in this order and stops where
 * the per-window loop would have stopped (cascadeclassifier.cpp:329-357): results behind that point are simply not consumed. */
CC_API cc_status cc_negminer_run_batch(cc_negminer* m, const uint8_t* const* images, int n_images, int width, int height,
                                       size_t row_stride, int ox, int oy, uint8_t* pass, int64_t cap, int64_t* n_windows,
                                       uint8_t* pixels, int64_t* keep_index, int max_keep, int* n_keep);

/* ============================================================================================
 * 6. Best-split search of a boosted-tree node on the device.
 *    Replaces CvDTree::find_best_split (traincascade/lib/src/o_cvdtree.cpp:313-357) and the per-variable searches it
 *    calls, CvBoostTree::find_split_ord_class / find_split_cat_class / find_split_ord_reg / find_split_cat_reg
 *    (o_cvboostree.cpp:151-247, 249-359, 361-426, 428-516), on the variable data CvCascadeBoostTrainData::
 *    get_ord_var_data / get_cat_var_data deliver (o_cvcascadeboosttraindata.cpp:403-482).
 *
 *    cc_eval_presort evaluates EVERY feature on stored samples [0, n_samples) once and keeps the result resident in
 *    HBM: for Haar the per-feature sorted order (values + sample indices; the reference's FeatureValAndIdxPrecalc,
 *    o_cvcascadeboosttraindata.cpp:535-556, limited there to the -precalcValBufSize / -precalcIdxBufSize budgets), for
 *    LBP the category codes (1 byte) and the samples of every feature ordered by (code, sample) (4 bytes). Haar: 6 bytes
 *    per (feature, sample): 19.5 GB for BASIC 24x24 x 20 000 samples; LBP: 5 bytes, 0.85 GB for 8 464 x 20 000. Call it after
 *    the stage's samples are in place (setImage / cc_eval_set_images) and again whenever they change.
 *
 *    cc_eval_find_best_split then searches one node: sample_idx are the node's stored-sample slots in node order (NULL
 *    = 0..n-1; no duplicates; any order is exact, LBP nodes listed in increasing order take the 7x faster kernel), weights the n + 2 "subtree weights" of CvBoostTree::calc_node_value
 *    (o_cvboostree.cpp:657-732: w[i], then the totals w[n], w[n+1]), responses the ordered responses (regression
 *    trees: LOGIT / GENTLE boost) or class_labels the 0/1 labels (DISCRETE / REAL boost), node_value = node->value.
 *    boost_type / split_criteria take CvBoost's values (boost.h: DISCRETE 0, REAL 1, LOGIT 2, GENTLE 3; DEFAULT 0,
 *    GINI 1, MISCLASS 3, SQERR 4) with the reference's defaulting rule (o_cvboostree.cpp:188-190).
 *    The arithmetic is the reference's, operation by operation, in double: one thread walks one variable's samples in
 *    sorted order. Equal feature values are taken in increasing sample-index order (the reference's std::sort leaves
 *    their order unspecified); categories are ordered with the same std::sort call as the reference. The winner over
 *    variables is chosen in variable order with the reference's float comparisons (o_cvdtree.cpp:340-341,351).
 *    out->found = 0 when no split has quality > 0 (find_best_split returns NULL). Optional per-variable results (NULL to
 *    skip): per_var_quality[vi] = best quality of variable vi on its own (-1 if it has no split),
 *    per_var_point[vi] = split_point (ordered) or number of categories sent left - 1 (categorical).
 * ============================================================================================ */
typedef struct cc_split {
  int32_t found;       /* 1 if a split was found */
  int32_t var_idx;     /* feature index (catalog order); HOG: variable index */
  float quality;
  float ord_c;         /* ordered variables: threshold, samples with value <= ord_c go left */
  int32_t split_point; /* ordered variables: position of the last left sample in the node's sorted order */
  int32_t subset[8];   /* categorical variables: bit c set = category c goes left */
} cc_split;
/*    Multi-GPU: variables shard across processes: cc_eval_presort_range keeps only variables
 *    [fi_begin, fi_end) on this device; cc_eval_find_best_split then searches that range (var_idx stays a catalog index,
 *    per_var_* arrays hold fi_end - fi_begin entries). Because the reference's winner is the first variable with the
 *    largest float quality, the global winner is the shard result with the largest quality, lowest shard first.
 */
CC_API cc_status cc_eval_presort(cc_evaluator* e, int n_samples);
CC_API cc_status cc_eval_presort_range(cc_evaluator* e, int fi_begin, int fi_end, int n_samples);
/*    Past the memory limit: a resident head and a streamed tail (ordered variables: Haar, HOG). cc_eval_presort(_range)
 *    refuses with CC_ERR_UNSUPPORTED when the tables of all variables do not fit the device. The reference never does: its
 *    -precalcValBufSize / -precalcIdxBufSize caches hold a head of the catalog, and CvCascadeBoostTrainData::
 *    get_ord_var_data evaluates and sorts every variable beyond them again at every node
 *    (o_cvcascadeboosttraindata.cpp:403-461, the uncached branch :437-458). cc_eval_presort_split does the same on the
 *    device: the first resident_vars variables of [fi_begin, fi_end) keep their tables exactly as cc_eval_presort_range
 *    builds them; the others are evaluated, sorted and searched chunk_vars at a time at every node, through the same
 *    kernels and the same [group][rank][64] layout. Every result -- cc_eval_find_best_split's winner and per-variable
 *    outputs, every record and the whole per-sample state of a cc_boost over it -- is bit-identical to a run with all
 *    tables resident: equal values keep increasing sample order in both (the reference's uncached branch uses an unstable
 *    std::sort; its tie order is not followed).
 *      resident_vars: a multiple of 64 in [0, F], or F = fi_end - fi_begin, which is cc_eval_presort_range itself.
 *      chunk_vars: a multiple of 64, at least 64; ignored when resident_vars == F; cut down to the tail's size and to
 *        2^28 values per pass, as a pass of the full presort.
 *      LBP: only resident_vars == F; anything else is CC_ERR_UNSUPPORTED (categorical variables are not streamed).
 *    The chunk scratch (16 B per value of a chunk, one chunk table, one winner row of 8 B per sample) stays with the
 *    evaluator until the next presort. A cc_boost created over a split presort needs nothing else: per searched node the
 *    head, then the chunks, with no host wait in between.
 *
 *    cc_presort_plan chooses the two numbers for a budget in bytes. Host arithmetic only (no device, unless budget_bytes
 *    is 0 = the calling thread's device's free memory). With N samples, F variables, per = 4 + (N <= 65 536 ? 2 : 4):
 *      everything resident:  ceil64(F) * N * per + min(F, P) * N * 16,  P = max(64, floor64(2^28 / N))   (as cc_eval_presort)
 *      split (R, C):         head(R) + chunk(C) + 8 * N
 *        head(R)  = R == 0 ? 0 : (R * N + 64 * 64) * per        (64 ranks of read-ahead padding)
 *        chunk(C) = C * N * 16 + (C * N + 64 * 64) * per        (values, sorted keys, sorted indices, iota; the chunk table)
 *    If everything fits: *resident_vars = F, *chunk_vars = 0. If all but the last group does, split(Rmax, 64) <= budget
 *    with Rmax = the largest multiple of 64 below F: (Rmax, 64). Otherwise C = the largest multiple of 64 up to
 *    min(ceil64(F), P) with split(0, C) <= budget, and, once C has reached that bound, R = the largest multiple of 64
 *    up to Rmax with split(R, C) <= budget (0 before). *resident_vars never shrinks as the budget grows.
 *    *bytes_needed <= budget is what the plan holds. A budget below split(0, 64) is CC_ERR_UNSUPPORTED; the message names
 *    that minimum. LBP: all resident or CC_ERR_UNSUPPORTED. Beyond 24 576 samples a row is sorted by the device-wide
 *    segmented sort, whose temporary storage comes on top of both sums, as it does for cc_eval_presort.
 *
 *    cc_eval_table_bytes: device bytes the evaluator holds for sorted tables plus streaming scratch.
 *    cc_eval_presort_budget: free device memory now plus cc_eval_table_bytes -- what a presort of this evaluator can use.
 *    cc_eval_stream_profile(e, 1) puts events between the steps of every streamed chunk (no host wait is added);
 *    cc_eval_stream_phase_ms then gives the device time of the last streamed search by step, summed over its chunks:
 *    evaluate, sort, interleave, search, winner (*n_parts = 5; tools/bench_boost_streamed.py).
 */
CC_API cc_status cc_presort_plan(int feature_type, int n_vars, int n_samples, uint64_t budget_bytes, int* resident_vars,
                                 int* chunk_vars, uint64_t* bytes_needed);
CC_API cc_status cc_eval_presort_split(cc_evaluator* e, int fi_begin, int fi_end, int n_samples, int resident_vars,
                                       int chunk_vars);
CC_API cc_status cc_eval_table_bytes(cc_evaluator* e, uint64_t* bytes);
CC_API cc_status cc_eval_presort_budget(cc_evaluator* e, uint64_t* bytes);
CC_API cc_status cc_eval_stream_profile(cc_evaluator* e, int enable);
CC_API cc_status cc_eval_stream_phase_ms(cc_evaluator* e, double* ms, int cap, int* n_parts);
CC_API cc_status cc_eval_find_best_split(cc_evaluator* e, const int32_t* sample_idx, int n, const double* weights,
                                         const float* responses, const int32_t* class_labels, double node_value,
                                         int boost_type, int split_criteria, cc_split* out, double* per_var_quality,
                                         int32_t* per_var_point);

/* ============================================================================================
 * 6b. Boosting a stage: one stage of weak trees trained on the device; cc_boost_create grows stumps (maxDepth 1, the
 *    trainer's default), cc_boost_create_depth trees of up to max_depth levels of splits.
 *    Replaces the loop of CvCascadeBoost::train (traincascade/lib/src/boost.cpp:409-459) with
 *    CvCascadeBoost::update_weights (:160-407) and isErrDesired (:479-518), CvBoost::trim_weights (o_cvboost.cpp:101-139),
 *    CvDTree::try_split_node (o_cvdtree.cpp:122-187), CvBoostTree::calc_node_value (o_cvboostree.cpp:657-732),
 *    calc_node_dir (:87-149) and CvCascadeBoostTree::predict (o_cvcascadeboosttree.cpp:16-39). The split of every node
 *    is section 6's search, one launch per node.
 *
 *    A node stays a leaf when it holds at most 10 samples (min_sample_count), stands at depth max_depth, holds one class
 *    only (DISCRETE / REAL), has sqrt(node_risk) / n < 0.01f (GENTLE; regression_accuracy) or finds no split with
 *    quality > 0. No pruning, no surrogates, no cross-validation folds: what the reference's cascade trainer runs with
 *    (o_cvdtreeparams.cpp:7-13). A child's samples keep increasing sample order (o_cvcascadeboosttree.cpp:300-338), so its
 *    sums are formed in that order. Samples of the subsample reach their leaf by direction (rank in the node's sorted
 *    order <= split_point, ties in increasing sample order; categorical: the subset bit); the samples outside it and the
 *    stage sums of all samples by the predict walk (value <= ord_c / subset bit at every level).
 *
 *    cc_boost_create needs cc_eval_presort(_range) over exactly n_samples; the classes are the evaluator's labels
 *    (getCls == 1.0f positive, 0.0f negative); with a presorted variable range the booster searches that range. Weights
 *    start at 1./n with every sample active (boost.cpp:190-265). A later presort or setImage(s) on the evaluator makes
 *    the next cc_boost_round fail with CC_ERR_INVALID_ARG. Weights, subsample mask, weak_eval and the running stage sums
 *    stay on the device; a round returns one fixed-size record. Every sum the reference forms in a loop is formed in
 *    the reference's order by one lane, so a round is reproducible bit for bit. The scalar log / exp of REAL's leaves and
 *    DISCRETE's C are libm's on the host, as in the reference; the n exponentials of update_weights (the reference:
 *    cvExp) are the device's exp(double), which cc_debug_exp64 exposes.
 * ============================================================================================ */
typedef struct cc_boost cc_boost;
typedef struct cc_boost_params {
  int32_t boost_type;       /* DISCRETE 0, REAL 1, GENTLE 3; LOGIT 2 -> CC_ERR_UNSUPPORTED (its responses change every round) */
  int32_t split_criteria;   /* as cc_eval_find_best_split */
  double weight_trim_rate;  /* 0.95; <= 0 or >= 1 disables trimming (o_cvboost.cpp:109) */
  float min_hit_rate, max_false_alarm; /* 0.995f, 0.5f */
  int32_t max_weak_count;   /* 100 */
} cc_boost_params;
typedef struct cc_weak { /* one round's fixed-size record */
  int32_t trained;       /* 0: the tree could not be trained (boost.cpp:436-440), nothing was added */
  int32_t stop;          /* 0 go on; 1 false alarm reached; 2 max_weak_count; 3 no active sample left (boost.cpp:444); 4 not trained */
  int32_t n_active, var_idx, split_point; /* n_active: samples the tree was trained on */
  float quality, ord_c;
  int32_t subset[8];
  double left_value, right_value; /* node->value of the leaves; after tree->scale(C) for DISCRETE */
  float stage_threshold, hit_rate, false_alarm; /* isErrDesired, boost.cpp:479-518; unchanged when stop == 3 or 4 */
} cc_weak;
/* one internal node of a round's tree, in the order CvCascadeBoostTree::write lists them (o_cvcascadeboosttree.cpp:41-93):
 * breadth-first from the root */
typedef struct cc_tree_node {
  int32_t left, right;          /* > 0: internal node index inside this tree; <= 0: leaf -value */
  int32_t depth, n_samples;     /* node->depth, node->sample_count */
  int32_t var_idx, split_point; /* as cc_weak */
  float quality, ord_c;
  int32_t subset[8];
  double value;                 /* node->value; DISCRETE: after tree->scale(C) */
} cc_tree_node;
/* cc_boost_create(e, n, p, out) is cc_boost_create_depth(e, n, p, 1, out). max_depth < 1: CC_ERR_INVALID_ARG; values above
 * 25 are clamped to 25 (o_cvdtreetraindata.cpp:105). */
CC_API cc_status cc_boost_create(cc_evaluator* e, int n_samples, const cc_boost_params* p, cc_boost** out);
CC_API cc_status cc_boost_create_depth(cc_evaluator* e, int n_samples, const cc_boost_params* p, int max_depth, cc_boost** out);
CC_API void cc_boost_destroy(cc_boost* b);
/* The record describes the tree's root: its split, and in left_value / right_value the node->value of its two children,
 * whether or not they split (for a stump: the leaves). */
CC_API cc_status cc_boost_round(cc_boost* b, cc_weak* out);
/* The tree of the last trained round: n_nodes internal nodes and n_nodes + 1 leaf values in the writer's order; changes
 * nothing. CC_ERR_BUFFER_TOO_SMALL (a cap too small, or a NULL buffer) still sets *n_nodes; CC_ERR_INVALID_ARG before
 * any round has trained a tree. */
CC_API cc_status cc_boost_last_tree(cc_boost* b, cc_tree_node* nodes, int node_cap, double* leaves, int leaf_cap, int* n_nodes);
/* rounds until stop != 0, at most cap of them */
CC_API cc_status cc_boost_train_stage(cc_boost* b, cc_weak* out, int cap, int* n_weak);
/* parity instrumentation: any pointer may be NULL; n_samples values each */
CC_API cc_status cc_boost_get_state(cc_boost* b, double* weights, double* weak_eval, uint8_t* mask, double* stage_sum);
/* device time of the last round's parts in ms: node tables + root value, split search, winner, apply the split, children's
 * values, weight update + stage sums, trimming, stage status (8 values); the first five summed over the tree's nodes */
CC_API cc_status cc_boost_last_round_ms(cc_boost* b, double* ms, int cap, int* n_parts);
/* the device's exp(double), for the witness of update_weights */
CC_API cc_status cc_debug_exp64(int device, const double* x, int n, double* out);
/* Host only, no device needed: the model CvCascadeClassifier::save would write for these stumps
 * (cascadeclassifier.cpp:439-456): the used variables only, renumbered in catalog order (markUsedFeaturesInMap,
 * boost.cpp:566-573; the catalogs are section 4's), stage thresholds and leaves as given. var_idx are catalog indices
 * (HOG: variable indices), one entry per weak classifier in stage order, n_weak_total of them (what n_weak must add up to); ord_c is read for HAAR / HOG, subsets (8 words
 * per weak classifier) for LBP. Callers pass (float)value for the leaves and stage_threshold as isErrDesired left it. */
CC_API cc_status cc_cascade_from_stumps(int feature_type, int haar_mode, int win_w, int win_h, int n_stages, const int32_t* n_weak,
                                        int n_weak_total, const float* stage_threshold, const int32_t* var_idx, const float* ord_c,
                                        const int32_t* subsets, const float* left, const float* right, cc_cascade** out);
/* The same for trees (CvCascadeBoostTree::write, o_cvcascadeboosttree.cpp:41-93): tree t has n_nodes[t] >= 1 internal
 * nodes, as cc_boost_last_tree returns them (left, right, var_idx and ord_c or subset are read), and n_nodes[t] + 1 leaves;
 * nodes and leaves of all trees follow each other in stage order, n_nodes_total and n_nodes_total + n_weak_total of them.
 * The used variables of ALL nodes are renumbered in catalog order (markFeaturesInMap, :349-359). Child references the XML
 * reader refuses (out of range, not larger than the node's own index) are refused here: CC_ERR_OUT_OF_RANGE. When every
 * tree has one node the model equals cc_cascade_from_stumps' model, stump view included. */
CC_API cc_status cc_cascade_from_trees(int feature_type, int haar_mode, int win_w, int win_h, int n_stages, const int32_t* n_weak,
                                       int n_weak_total, const float* stage_threshold, const int32_t* n_nodes, int n_nodes_total,
                                       const cc_tree_node* nodes, const float* leaves, cc_cascade** out);

/* ============================================================================================
 * 6c. Filling a stage's training set.
 *    Replaces CvCascadeClassifier::fillPassedSamples (traincascade/lib/src/cascadeclassifier.cpp:329-357) as
 *    updateTrainingSet (:308-327) calls it: the candidates (windows of the background stream, imagestorage.cpp:90-126, or
 *    the positives) are taken in order, setImage + predict decides each, and the ones that pass fill consecutive sample
 *    slots of the evaluator. Section 5's calls hand every pass flag to the host, which then sends the kept pixels back
 *    through cc_eval_set_images; here the flags, the choice and the kept pixels stay on the device and one small record
 *    comes back.
 *
 *    The loop, with `flags` the pass flag of every stream position (image 0 first, n_images * wins positions):
 *        got = consumed = 0; j = start
 *        loop: if got == want: stop = CC_FILL_FILLED; break                               (:333, the slots are full)
 *              c = consumed_before + consumed; g = got_before + got
 *              if c != 0 and (double)(g + 1) / (double)c <= min_acceptance_ratio: stop = CC_FILL_RATIO; break       (:337)
 *              if j == n_images * wins: stop = CC_FILL_EXHAUSTED; break                   (:342, no further window here)
 *              consumed += 1
 *              if flags[j]: window j -> slot first_idx + got, label 0; keep_index[got] = j; got += 1          (:346-352)
 *              j += 1
 *    On the device: a count of the flags before every position (per block of cc_debug_fill_scan_tile() positions, then a scan
 *    of the block totals), the first position at which one of the three conditions holds (IEEE double division), the
 *    positions kept before it by rank, their pixels gathered out of the ladders, and the evaluator's own setImage code on
 *    those pixels: a filled slot holds bit for bit what cc_eval_set_images stores for the window's pixels. got_before /
 *    consumed_before carry a stage's counts over the calls that fill it; `start` resumes inside image 0's stream.
 *    The evaluator: labels of the filled slots become 0, images queued by cc_eval_set_image are sent first, a host mirror of
 *    an overwritten slot is dropped, boosters and presorted tables made before the call are stale (as after
 *    cc_eval_set_images); slots outside [first_idx, first_idx + *n_filled) keep their contents. A call that fills nothing
 *    leaves the evaluator alone.
 *    Refused, with nothing changed: evaluator and miner of different device, feature type or window, n_images outside
 *    [1, 256], start outside [0, n_images * wins] (CC_ERR_INVALID_ARG); first_idx < 0, want < 0 or first_idx + want >
 *    max_samples (CC_ERR_OUT_OF_RANGE); offsets as cc_negminer_run_batch.
 * ============================================================================================ */
enum { CC_FILL_FILLED = 0, CC_FILL_RATIO = 1, CC_FILL_EXHAUSTED = 2 };
/* A miner with no trained stages, for stage 0 of training: every window passes. (cc_cascade_from_stumps refuses a cascade
 * without stages.) */
CC_API cc_status cc_negminer_create_empty(int feature_type, int win_w, int win_h, int device, cc_negminer** out);
/* n_images (<= 256) images of one size with one offset, as cc_negminer_run_batch takes them. keep_index (NULL, or `want`
 * entries): the stream positions of the filled slots. */
CC_API cc_status cc_negminer_fill(cc_negminer* m, cc_evaluator* e, const uint8_t* const* images, int n_images, int width, int height,
                                  size_t row_stride, int ox, int oy, int64_t start, int first_idx, int want, int64_t got_before,
                                  int64_t consumed_before, double min_acceptance_ratio, int* n_filled, int64_t* n_consumed, int* stop,
                                  int64_t* keep_index);
/* The positive branch (fillPassedSamples(0, numPos, true, 0, consumed)): the candidates are n_imgs packed windows
 * (win_w * win_h bytes each) in order, the ratio is 0 and never stops the loop. The ones that pass `stages` (NULL: all) fill
 * slots first_idx .. in order with `label`; *n_consumed = index of the last one taken + 1, or n_imgs when they run out
 * before `want` are found. Candidates are set into scratch rows a chunk at a time, predicted there by the kernels of
 * cc_eval_predict_cascade, and the kept rows copied to their slots. */
CC_API cc_status cc_eval_fill_passed(cc_evaluator* e, const cc_cascade* stages, const uint8_t* imgs, int n_imgs, int first_idx,
                                     int want, uint8_t label, int* n_filled, int64_t* n_consumed);
/* Test instrumentation: the selection alone (count, first stop, keep list) over n host flags. */
CC_API cc_status cc_debug_fill_select(int device, const uint8_t* flags, int64_t n, int64_t start, int want, int64_t got_before,
                                      int64_t consumed_before, double ratio, int* n_filled, int64_t* n_consumed, int* stop,
                                      int64_t* keep_index);
CC_API int cc_debug_fill_scan_tile(void); /* positions per block of the scan */

/* ============================================================================================
 * 6d. The trainer's files: params.xml, stage<i>.xml and a cascade.xml that carries the training parameters.
 *    Replaces the file side of CvCascadeClassifier::train / load (traincascade/lib/src/cascadeclassifier.cpp:247-275,
 *    :359-364, :534-564): CvCascadeParams::write / read (:33-73), CvCascadeBoostParams::write / read (boost.cpp:58-95),
 *    CvFeatureParams::write / read (features.cpp:47-60), CvHaarFeatureParams::write / read (haarfeatures.cpp:28-52),
 *    CvCascadeBoost::write (boost.cpp:520-532) and CvCascadeBoostTree::write / read (o_cvcascadeboosttree.cpp:41-165).
 *    Host code, no device needed. Tags, their order and their values follow those functions; the byte layout of OpenCV's
 *    FileStorage (indentation, line wrapping, digits of a real) is NOT pinned, as for cascade.xml: there is no OpenCV to
 *    compare with. Floats are written with 9 significant digits and doubles with 17, so every number parses back to
 *    itself; all formatting and parsing runs under the "C" numeric locale.
 * ============================================================================================ */
typedef struct cc_train_params {
  int32_t feature_type, win_w, win_h;  /* CC_FEATURE_*; <width>, <height> */
  int32_t boost_type;                  /* CvBoost: DISCRETE 0 "DAB", REAL 1 "RAB", LOGIT 2 "LB", GENTLE 3 "GAB" */
  float min_hit_rate, max_false_alarm; /* <minHitRate>, <maxFalseAlarm> */
  double weight_trim_rate;             /* <weightTrimRate>: a double in the reference, and kept bit for bit */
  int32_t max_depth, max_weak_count;
  int32_t max_cat_count, feat_size;    /* LBP 256 / 1, HAAR 0 / 1, HOG 0 / 36 */
  int32_t haar_mode;                   /* CC_HAAR_BASIC / CORE / ALL "BASIC|CORE|ALL"; written and read for HAAR only */
} cc_train_params;

/* params.xml: <stageType> <featureType> <height> <width>, <stageParams> { boostType minHitRate maxFalseAlarm weightTrimRate
 * maxDepth maxWeakCount }, <featureParams> { maxCatCount featSize [mode] } inside one top-level element. object_name names
 * that element; NULL: the name FileStorage::getDefaultObjectName derives from the file name ("params" for params.xml). The
 * values are written as given; CC_ERR_INVALID_ARG for a feature type, boost type or Haar mode that has no name. */
CC_API cc_status cc_train_params_save_xml(const cc_train_params* p, const char* path, const char* object_name);
/* Reads the block back from a params.xml or from a cascade.xml (the first element under <opencv_storage>). Tolerated: the
 * historical <featuhreParams>, type_id attributes, comments; a missing <featSize> / <maxCatCount> takes the feature type's
 * default. The range checks of the three read()s fail with CC_ERR_PARSE and name the tag: stageType BOOST, featureType
 * HAAR|LBP|HOG, height > 0, width > 0; boostType DAB|RAB|LB|GAB, minHitRate, maxFalseAlarm and weightTrimRate in (0, 1],
 * maxDepth > 0, maxWeakCount > 0; maxCatCount >= 0, featSize >= 1, and for HAAR mode BASIC|CORE|ALL. A block whose
 * <stageParams> has no <boostType> -- what cc_cascade_save_xml writes -- is CC_ERR_NO_TRAIN_PARAMS, not a parse error. */
CC_API cc_status cc_train_params_load_xml(const char* path, cc_train_params* out);
/* The training parameters a loaded cascade.xml carried: CC_OK, or CC_ERR_NO_TRAIN_PARAMS when the file had none that pass
 * the checks above (loading the model does not depend on them) or the cascade was built by cc_cascade_from_stumps / _trees. */
CC_API cc_status cc_cascade_train_params(const cc_cascade* c, cc_train_params* out);
/* cc_cascade_save_xml with the whole <stageParams> / <featureParams> block of writeParams (cascadeclassifier.cpp:359-364)
 * in place of its short one; every other byte is the same, and the file loads to the same model. feature_type and window
 * of p must be the cascade's: CC_ERR_INVALID_ARG. */
CC_API cc_status cc_cascade_save_xml_params(const cc_cascade* c, const cc_train_params* p, const char* path);

/* stage<i>.xml, as tempStage->write(fs, Mat()) leaves it: <maxWeakCount> (the number of trees), <stageThreshold> (the
 * trained threshold itself, NOT threshold - 1e-5f) and <weakClassifiers>, per tree <internalNodes> = per node "left right
 * featureIdx (threshold | subset words)" and <leafValues>. featureIdx is the CATALOG index of the variable (HOG: the
 * variable index): nothing is renumbered, the feature map is empty. The writer takes one stage of what
 * cc_cascade_from_trees takes: n_weak trees, n_nodes[t] nodes each (left, right, var_idx and ord_c or subset are written),
 * n_nodes_total nodes and n_nodes_total + n_weak leaves. max_cat_count > 0 (LBP: 256) writes (max_cat_count + 31) / 32 <= 8
 * subset words per node, 0 the threshold. object_name as above ("stage3" for stage3.xml). */
CC_API cc_status cc_stage_save_xml(const char* path, const char* object_name, int max_cat_count, float stage_threshold, int n_weak,
                                   const int32_t* n_nodes, int n_nodes_total, const cc_tree_node* nodes, const float* leaves);
/* Reads it back into the same arrays (the fields of a node that the file does not hold are 0). *n_weak and *n_nodes_total are
 * always set when the file parses; with weak_cap < *n_weak, node_cap < *n_nodes_total or a NULL array the call returns
 * CC_ERR_BUFFER_TOO_SMALL and fills nothing else (leaves needs *n_nodes_total + *n_weak entries). Refused with CC_ERR_PARSE,
 * naming the file and the tag: an <internalNodes> length that is no multiple of the node step 3 + (subset words | 1), child
 * references outside the tree or not behind their parent, a <leafValues> count other than nodes + 1, and -- with
 * n_variables > 0, the catalog size -- a featureIdx outside [0, n_variables). */
CC_API cc_status cc_stage_load_xml(const char* path, int max_cat_count, int n_variables, float* stage_threshold, int* n_weak,
                                   int32_t* n_nodes, int weak_cap, int* n_nodes_total, cc_tree_node* nodes, int node_cap, float* leaves);

/* ============================================================================================
 * 7. Multi-GPU: the gather of detections (BASELINE configs[3]).
 *    Detection shards by frame, one process per GPU, and needs no data-path collective: rank r runs cc_detect_batch on
 *    frames [lo, hi) = cc_shard_range(n_frames, r, world). The only exchange is this gather of the per-frame rectangle
 *    lists (a few KB per rank) over RCCL: one ncclAllGather of {frames, rectangles} headers and one padded
 *    ncclAllGather of the payload (per-frame counts, then rectangles), so every rank ends up with all frames'
 *    rectangles in global frame order. librccl is loaded on first use (an RCCL the process has already loaded, e.g.
 *    PyTorch's, is reused); world == 1 needs no RCCL at all.
 *    Bootstrap like any NCCL program: rank 0 calls cc_comm_unique_id and hands the CC_COMM_ID_BYTES bytes to the other
 *    ranks by whatever channel the host program has (MPI_Bcast, a file, a socket, torch.distributed); every rank then
 *    calls cc_comm_create (collective). There is no reference counterpart: the reference is single-process
 *    (tools/detection/Cpp/main.cpp:42-45 handles one image).
 * ============================================================================================ */
typedef struct cc_comm cc_comm;
#define CC_COMM_ID_BYTES 128
CC_API void cc_shard_range(int n_items, int rank, int world, int* lo, int* hi);
/* (An id starts RCCL's bootstrap listener: create one only for a communicator that all ranks then really build.) */
CC_API cc_status cc_comm_unique_id(void* id /* CC_COMM_ID_BYTES bytes */);
CC_API cc_status cc_comm_create(int device, int rank, int world, const void* id /* may be NULL when world == 1 */, cc_comm** out);
CC_API void cc_comm_destroy(cc_comm* c);
CC_API int cc_comm_rank(const cc_comm* c);
CC_API int cc_comm_world(const cc_comm* c);
/* Collective over the communicator. rects / offsets: this rank's frames as cc_detect_batch returns them (offsets has
 * n_frames + 1 entries). On return *n_frames_all / *n_rects_all hold the totals over all ranks. If the caller's buffers
 * (out: cap_rects rectangles, offsets_out: cap_frames + 1 entries) are too small the call returns
 * CC_ERR_BUFFER_TOO_SMALL, but only after the collectives have completed (the ranks stay in step) and with the result
 * kept in the communicator: cc_gather_fetch copies it out later without communicating (never call the gather again on
 * one rank alone). */
CC_API cc_status cc_gather_detections(cc_comm* c, const cc_rect* rects, const int32_t* offsets, int n_frames, cc_rect* out,
                                      int cap_rects, int32_t* offsets_out, int cap_frames, int* n_frames_all, int* n_rects_all);
CC_API cc_status cc_gather_fetch(const cc_comm* c, cc_rect* out, int cap_rects, int32_t* offsets_out, int cap_frames);

/* ============================================================================================
 * 8. Sample synthesis: the positives of the trainer from one object image.
 *    Replaces cvCreateTrainingSamples (tools/createsamples/utility.cpp:952-1027) and what it calls:
 *    icvStartSampleDistortion (:516-578) -> cc_sampler_create; icvRandomQuad (:419-466), cvGetPerspectiveTransform
 *    (:180-223), the scanline walk of cvWarpPerspective (:255-416), the rectangle arithmetic of icvPlaceDistortedSample
 *    (:615-648) and the background reader (:765-886) -> cc_sample_plan (host, serial: every random draw);
 *    the warp's pixels (:351-387), GaussianBlur, the two resizes and the blend (:650-671) -> cc_sampler_render (device).
 *    The random numbers are cv::RNG's (seed 12345 in the tool, createsamples.cpp:88,158): with the tool's image and
 *    options the samples are the tool's, byte for byte.
 *    The tool's other two modes follow below: test images with their info file (cc_testset_plan,
 *    cc_sampler_render_testset) and positives cut from annotated images (-info to .vec: cc_area_tab, cc_samples_from_info;
 *    cc_resize_area_u8 of section 3 is its resize alone).
 * ============================================================================================ */
#define CC_SAMPLE_RANDOM_INVERT 0x7FFFFFFF /* CV_RANDOM_INVERT */
typedef struct cc_sample_params {
  int32_t bgcolor, bgthreshold;
  int32_t invert; /* 0, 1 or CC_SAMPLE_RANDOM_INVERT */
  int32_t maxintensitydev;
  double maxxangle, maxyangle, maxzangle;
  int32_t inscribe; /* cvCreateTrainingSamples passes 0, 0.0, 0.0 for these three (:1000-1002) */
  int32_t reserved;
  double maxshift, maxscale;
} cc_sample_params;

/* One sample, as planned on the host. */
typedef struct cc_sample_record {
  double quad[8];   /* x, y of the four vertices on the canvas */
  double coeffs[9]; /* canvas -> source, row-major 3x3, coeffs[8] = 1 */
  int32_t inverse, forecolordev;
  int32_t roi_x, roi_y, roi_w, roi_h; /* source rectangle of the resize, clipped to the canvas */
  int32_t bg_image, bg_w, bg_h, bg_x, bg_y; /* background window: image (-1: none), the size it is scaled to, origin */
  int32_t reserved;
} cc_sample_record;

/* The tool's background reader (CvBackgroundData + CvBackgroundReader) between calls of cc_sample_plan. The caller sets
 * n_images and sizes (width, height per image) and zeroes the rest before the first call. */
typedef struct cc_sample_bg_reader {
  const int32_t* sizes;
  int32_t n_images;
  int32_t have, round, last, off_x, off_y, pt_x, pt_y, cur_w, cur_h;
  float scale;
} cc_sample_bg_reader;

/* Host only, no device. Makes every random draw and all sequential arithmetic of n samples of an out_w x out_h window from
 * a src_w x src_h object image. Per sample, in the tool's order: the background window (when bg != NULL; a new image is
 * picked with uniform(0, RAND_MAX) % n_images), uniform(0, 2) for `inverse` when invert is random, icvRandomQuad, xshift,
 * yshift, randscale, forecolordev. *rng_state is cv::RNG's state (seed, or 0xffffffff for seed 0) and is carried on: two
 * calls of 37 and 63 samples give what one call of 100 gives. records: n entries. spans (may be NULL): per sample and row
 * of the canvas (src_h + 2 * (src_h / 2) rows of src_w + 2 * (src_w / 2) pixels) ix_min, ix_max of the scanline walk,
 * 0, -1 for a row it does not visit. A nonconvex or degenerate quadrangle, a singular system or a rectangle that misses
 * the canvas is CC_ERR_INVALID_ARG; *rng_state and *bg are then as before the call. Sides: source 2..8192, window 1..4096. */
CC_API cc_status cc_sample_plan(int src_w, int src_h, int out_w, int out_h, const cc_sample_params* params, uint64_t* rng_state,
                                cc_sample_bg_reader* bg, int n, cc_sample_record* records, int32_t* spans);

typedef struct cc_sampler cc_sampler;
/* icvStartSampleDistortion on the device: the mask (0 within bgthreshold of bgcolor, else 255), and the image with its
 * background pixels replaced by the 3x3 minimum / maximum where that differs from bgcolor by more than the threshold
 * (differences taken modulo 256, as the reference's uchar casts do). Both stay in device memory. Sides 2..8192. */
CC_API cc_status cc_sampler_create(int device, const uint8_t* img, int w, int h, size_t stride, int bgcolor, int bgthreshold,
                                   cc_sampler** out);
CC_API void cc_sampler_destroy(cc_sampler* s);
/* The images behind the records' bg_image (the tool's -bg list), kept in device memory; replaces an earlier set. */
CC_API cc_status cc_sampler_set_backgrounds(cc_sampler* s, const uint8_t* const* images, const int32_t* widths,
                                            const int32_t* heights, int n_images);
/* Renders n planned samples into out (n * out_h * out_w bytes, host). records / spans as cc_sample_plan filled them for
 * this sampler's image size and this window. backgrounds: n windows of out_h * out_w bytes (host), or NULL: each sample is
 * then blended onto its record's window of the cc_sampler_set_backgrounds images (scaled by the exact resize, cropped on
 * the device), or onto bgcolor when bg_image is -1 (bgcolor saturated to 0..255 there and where the warp leaves the
 * canvas unwritten, as the reference's Mat = Scalar does; the mask and the border extension use the int). One grid per batch of samples; the batch is sized from free device
 * memory, at most 32768 samples and, when max_batch > 0, at most max_batch. Records whose rectangle or window leaves its
 * image are CC_ERR_INVALID_ARG. */
CC_API cc_status cc_sampler_render(cc_sampler* s, const cc_sample_record* records, const int32_t* spans, int n, int out_w,
                                   int out_h, const uint8_t* backgrounds, int max_batch, uint8_t* out);

/* Test mode of the tool: detection test sets. Replaces cvCreateTestSamples (tools/createsamples/utility.cpp:1031-1123; chosen
 * in createsamples.cpp:193-198 by -img, -bg and -info without -vec): the loop's draws and its rectangle (:1078-1098) ->
 * cc_testset_plan (host, serial), icvPlaceDistortedSample into src(Rect(x, y, width, height)) (:1099-1101, :580-672) ->
 * cc_sampler_render_testset (device). Writing the images and info.dat (:1103-1111) is host file IO (samples.py). */
typedef struct cc_testset_item {
  int32_t iteration;           /* the tool's i + 1, the first field of the file name (:1103) */
  int32_t bg_image;            /* index into the background list */
  int32_t x, y, width, height; /* the object's rectangle in that image: the ground truth of the info line (:1107) */
} cc_testset_item;

/* Host only, no device. Makes every random draw of up to `num` more iterations of the tool's loop for a win_w x win_h
 * window, in the tool's order. The loop runs MIN(num, bg->n_images) times in all (:1078): *iterations_done (0 before the
 * first call) is carried on, and this call makes MIN(num, n_images - *iterations_done) iterations, so that calls of a and b
 * equal one call of a + b. Per iteration: the background image (icvGetNextFromBackgroundData with the reader's window of
 * 10 x 10, :1055, :765-831: uniform(0, RAND_MAX) % n_images, an image with a side under 10 is drawn again, n_images
 * rejections in a row fail); a negative *maxscale becomes MIN(0.7F * cols / win_w, 0.7F * rows / win_h) of THIS image in
 * float and keeps that value from then on (:1082-1085; the tool's default is -1); *maxscale < 1 skips the iteration with
 * its background draw spent (:1087); scale = uniform(1.0F, (float)maxscale), cv::RNG's float overload: one next(),
 * (float)next() * 2.3283064365386962890625e-10f * (b - a) + a in float; width = (int)(scale * win_w), height likewise;
 * x = (int)(uniform(0.1, 0.8) * (cols - width)), y likewise (double); uniform(0, 2) when invert is random; then the
 * placement's plan exactly as cc_sample_plan makes it for a window of width x height with inscribe = 1, maxshift = 0,
 * maxscale = 0 and no background reader (these three fields of *params are ignored here).
 * items / records: room for `num` entries; spans (may be NULL): room for `num` samples' row spans, as cc_sample_plan lays
 * them out. *n_emitted entries are filled. A rectangle that leaves its image (x < 0, y < 0, x + width > cols,
 * y + height > rows; the reference's src(Rect) asserts), a width or height outside 1..4096, no image with both sides of 10
 * or more, and everything cc_sample_plan refuses are CC_ERR_INVALID_ARG naming the iteration; *rng_state, *bg, *maxscale and
 * *iterations_done are then as before the call. bg: as for cc_sample_plan, zeroed before the first call, kept apart from
 * a training-mode reader. */
CC_API cc_status cc_testset_plan(int src_w, int src_h, int win_w, int win_h, const cc_sample_params* params, uint64_t* rng_state,
                                 cc_sample_bg_reader* bg, double* maxscale, int32_t* iterations_done, int num, int32_t* n_emitted,
                                 cc_testset_item* items, cc_sample_record* records, int32_t* spans);

/* Renders n planned test images: for each item a fresh copy of its cc_sampler_set_backgrounds image with the sample blended
 * into Rect(x, y, width, height), the pixel arithmetic being cc_sampler_render's. One grid per batch covers rectangles of
 * different sizes (a table of 256-pixel tiles); the image copies are device to device. out_host (may be NULL): n pointers,
 * item i's image as rows * cols bytes of its background. out_device (may be NULL): device memory that receives the
 * (n, rows, cols) stack, frame i at out_device + i * frame_stride bytes (0: rows * cols); every item's background must then
 * have one size, and frame_stride at least rows * cols. At least one of the two when n > 0. Batches are sized from free
 * device memory over the image bytes, and hold at most max_batch items when max_batch > 0. An item whose image index or
 * rectangle is outside its bounds, a side outside 1..4096, and a record whose source rectangle leaves the canvas are
 * CC_ERR_INVALID_ARG. */
CC_API cc_status cc_sampler_render_testset(cc_sampler* s, const cc_testset_item* items, const cc_sample_record* records,
                                           const int32_t* spans, int n, int max_batch, uint8_t* const* out_host, void* out_device,
                                           size_t frame_stride);

/* The -info mode of the tool: positives from annotated images. Replaces cvCreateTrainingSamplesFromInfo
 * (tools/createsamples/utility.cpp:1125-1232; chosen in createsamples.cpp:201-208 by -info and -vec without -img): every
 * annotated rectangle is cut out of its image and resized to the window,
 *   resize(src(Rect(x, y, width, height)), sample, Size(w, h), 0, 0, width >= w && height >= h ? INTER_AREA : INTER_LINEAR_EXACT).
 * The fscanf walk over the info file and the .vec are host file IO (samples.py); the pixels -> cc_samples_from_info (device).
 * The source of a resize is the rectangle alone (a Mat view): the bilinear branch replicates the border at the rectangle's
 * edge. The INTER_AREA arithmetic is OpenCV's (4.6.0 resize.cpp), restated in DESIGN.md 4.15 from knowledge of that code and
 * not pinned against OpenCV's bytes: same size is a copy; integer ratios on both axes sum the block in an int (2 x 2:
 * (a + b + c + d + 2) >> 2, else cvRound((float)sum * (1.f / area))); every other case weighs whole and partial source pixels
 * per axis with the table cc_area_tab returns, in float, in the table's order. */
typedef struct cc_info_record {
  int32_t image;               /* index into the image list */
  int32_t x, y, width, height; /* the annotated rectangle in that image */
} cc_info_record;

/* Host only, no device: one axis of INTER_AREA from ssize to dsize pixels, 1 <= dsize <= ssize <= 8192.
 * *scale = 1 / ((double)dsize / ssize), *iscale = (int)*scale, *is_integer = |*scale - *iscale| < DBL_EPSILON (both axes
 * integer: the fast path, which does not use the table). The table is computeResizeAreaTab's: entry k adds
 * alpha[k] * source[src_index[k]] to destination dst_index[k]; at most 2 * ssize entries. Any output but n_entries may be
 * NULL (the three arrays only with capacity 0). More than `capacity` entries: CC_ERR_BUFFER_TOO_SMALL with *n_entries set. */
CC_API cc_status cc_area_tab(int ssize, int dsize, double* scale, int32_t* iscale, int32_t* is_integer, int32_t* dst_index,
                             int32_t* src_index, float* alpha, int capacity, int32_t* n_entries);

/* Resizes n annotated rectangles to win_w x win_h windows. images / widths / heights / strides: n_images HOST images (row
 * stride in bytes). Output: out_host (n * win_h * win_w bytes, host), out_device (as many bytes of device memory), or both;
 * at least one when n > 0. One grid per batch covers rectangles of different sizes and both branches (a table of 256-pixel
 * tiles, one thread per window pixel). A batch is a run of consecutive records whose images, each uploaded once per batch,
 * fit a quarter of the free device memory, at most max_batch records when max_batch > 0.
 * Limits: image (and so rectangle) sides 1..8192, window sides 1..4096. CC_ERR_INVALID_ARG, naming the record: an image
 * index outside the list; a rectangle with a side under 1 or not inside its image (the tool's src(Rect) asserts); integer
 * ratios with iscale_x * iscale_y * 255 >= 2^31 (the reference's int sum would overflow). All of this is checked before
 * the device is touched; nothing is written then. */
CC_API cc_status cc_samples_from_info(int device, const uint8_t* const* images, const int32_t* widths, const int32_t* heights,
                                      const size_t* strides, int n_images, const cc_info_record* records, int n, int win_w,
                                      int win_h, int max_batch, uint8_t* out_host, void* out_device);
/* Stream time of the calling thread's last cc_samples_from_info in ms, summed over its batches: image and table upload, the
 * kernel, the copy back to out_host. Any pointer may be NULL. */
CC_API cc_status cc_samples_from_info_last_ms(double* upload_ms, double* kernel_ms, double* download_ms);

#ifdef __cplusplus
}
#endif
#endif /* CASCADECLASSIFIER_AMD_H_ */
