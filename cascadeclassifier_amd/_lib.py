"""ctypes binding of libcascadeclassifier_amd.so (the C ABI declared in include/cascadeclassifier_amd.h).

There is no fallback of any kind: if the shared library has not been built, importing the bindings raises; if no
HIP device is usable, every compute entry point returns CC_ERR_NO_DEVICE and the wrappers raise CascadeError.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CCAMD_LIB selects another build of the same library (tuning experiments); the default is the in-tree build.
LIB_PATH = os.environ.get("CCAMD_LIB") or os.path.join(_HERE, "lib", "libcascadeclassifier_amd.so")

CC_OK = 0
CC_ERR_INVALID_ARG = -1
CC_ERR_NO_DEVICE = -2
CC_ERR_HIP = -3
CC_ERR_IO = -4
CC_ERR_PARSE = -5
CC_ERR_UNSUPPORTED = -6
CC_ERR_BUFFER_TOO_SMALL = -7
CC_ERR_OUT_OF_RANGE = -8
CC_ERR_NO_TRAIN_PARAMS = -9

CC_FEATURE_HAAR, CC_FEATURE_LBP, CC_FEATURE_HOG = 0, 1, 2
CC_PIX_GRAY8, CC_PIX_BGR8, CC_PIX_BGRA8, CC_PIX_RGB8, CC_PIX_RGBA8, CC_PIX_RGB8_PLANAR = 0, 1, 2, 3, 4, 5
CC_HAAR_BASIC, CC_HAAR_CORE, CC_HAAR_ALL = 0, 1, 2


class CascadeError(RuntimeError):
    """A C-ABI call failed; .status is the cc_status code (the reference throws cv::Exception here)."""

    def __init__(self, status: int, message: str):
        super().__init__(f"[cc_status {status}] {message}")
        self.status = status


class Rect(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("width", C.c_int32), ("height", C.c_int32)]


class CascadeInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("feature_type", "win_w", "win_h", "n_stages", "n_weak", "n_nodes", "n_leaves",
                                         "n_features", "max_cat_count", "subset_size", "max_nodes_per_tree", "has_tilted")]


class DetectParams(C.Structure):
    _fields_ = [("scale_factor", C.c_double), ("min_neighbors", C.c_int32), ("min_w", C.c_int32), ("min_h", C.c_int32),
                ("max_w", C.c_int32), ("max_h", C.c_int32)]


class ScaleInfo(C.Structure):
    _fields_ = [("scale", C.c_float), ("width", C.c_int32), ("height", C.c_int32), ("ystep", C.c_int32), ("nx", C.c_int32),
                ("ny", C.c_int32), ("win_w", C.c_int32), ("win_h", C.c_int32)]


class DetectorTimings(C.Structure):
    _fields_ = [("resize_ms", C.c_double), ("integral_ms", C.c_double), ("eval_ms", C.c_double), ("finalize_ms", C.c_double),
                ("resize_launches", C.c_int64), ("integral_launches", C.c_int64), ("eval_launches", C.c_int64),
                ("finalize_launches", C.c_int64), ("frames", C.c_int64), ("grid_windows", C.c_int64),
                ("integral_elems", C.c_int64), ("eval_step1_ms", C.c_double),
                ("group_ms", C.c_double), ("group_launches", C.c_int64)]


class Split(C.Structure):
    _fields_ = [("found", C.c_int32), ("var_idx", C.c_int32), ("quality", C.c_float), ("ord_c", C.c_float),
                ("split_point", C.c_int32), ("subset", C.c_int32 * 8)]


class BoostParams(C.Structure):
    _fields_ = [("boost_type", C.c_int32), ("split_criteria", C.c_int32), ("weight_trim_rate", C.c_double),
                ("min_hit_rate", C.c_float), ("max_false_alarm", C.c_float), ("max_weak_count", C.c_int32)]


class Weak(C.Structure):
    _fields_ = [("trained", C.c_int32), ("stop", C.c_int32), ("n_active", C.c_int32), ("var_idx", C.c_int32),
                ("split_point", C.c_int32), ("quality", C.c_float), ("ord_c", C.c_float), ("subset", C.c_int32 * 8),
                ("left_value", C.c_double), ("right_value", C.c_double), ("stage_threshold", C.c_float),
                ("hit_rate", C.c_float), ("false_alarm", C.c_float)]


class TreeNode(C.Structure):
    _fields_ = [("left", C.c_int32), ("right", C.c_int32), ("depth", C.c_int32), ("n_samples", C.c_int32), ("var_idx", C.c_int32),
                ("split_point", C.c_int32), ("quality", C.c_float), ("ord_c", C.c_float), ("subset", C.c_int32 * 8),
                ("value", C.c_double)]


class TrainParams(C.Structure):
    _fields_ = [("feature_type", C.c_int32), ("win_w", C.c_int32), ("win_h", C.c_int32), ("boost_type", C.c_int32),
                ("min_hit_rate", C.c_float), ("max_false_alarm", C.c_float), ("weight_trim_rate", C.c_double),
                ("max_depth", C.c_int32), ("max_weak_count", C.c_int32), ("max_cat_count", C.c_int32), ("feat_size", C.c_int32),
                ("haar_mode", C.c_int32)]


class HaarFeatureC(C.Structure):
    _fields_ = [("tilted", C.c_int32), ("r", (C.c_int32 * 4) * 3), ("w", C.c_float * 3)]


class SampleParams(C.Structure):
    _fields_ = [("bgcolor", C.c_int32), ("bgthreshold", C.c_int32), ("invert", C.c_int32), ("maxintensitydev", C.c_int32),
                ("maxxangle", C.c_double), ("maxyangle", C.c_double), ("maxzangle", C.c_double), ("inscribe", C.c_int32),
                ("reserved", C.c_int32), ("maxshift", C.c_double), ("maxscale", C.c_double)]


class SampleRecord(C.Structure):
    _fields_ = [("quad", C.c_double * 8), ("coeffs", C.c_double * 9), ("inverse", C.c_int32), ("forecolordev", C.c_int32),
                ("roi_x", C.c_int32), ("roi_y", C.c_int32), ("roi_w", C.c_int32), ("roi_h", C.c_int32),
                ("bg_image", C.c_int32), ("bg_w", C.c_int32), ("bg_h", C.c_int32), ("bg_x", C.c_int32), ("bg_y", C.c_int32),
                ("reserved", C.c_int32)]


class TestsetItem(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("iteration", "bg_image", "x", "y", "width", "height")]


class InfoRecord(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("image", "x", "y", "width", "height")]


class SampleBgReader(C.Structure):
    _fields_ = [("sizes", C.c_void_p), ("n_images", C.c_int32)] + \
               [(n, C.c_int32) for n in ("have", "round", "last", "off_x", "off_y", "pt_x", "pt_y", "cur_w", "cur_h")] + \
               [("scale", C.c_float)]


# every symbol include/cascadeclassifier_amd.h declares: name -> (restype, argtypes)
_vp, _i, _sz, _d = C.c_void_p, C.c_int, C.c_size_t, C.c_double
_pp = C.POINTER(C.c_void_p)
SIGNATURES = {
    "cc_last_error": (C.c_char_p, []),
    "cc_version": (_i, []),
    "cc_device_count": (_i, []),
    "cc_cascade_load_xml": (_i, [C.c_char_p, _pp]),
    "cc_cascade_load_xml_mem": (_i, [C.c_char_p, _sz, _pp]),
    "cc_cascade_destroy": (None, [_vp]),
    "cc_cascade_info_get": (_i, [_vp, C.POINTER(CascadeInfo)]),
    "cc_cascade_stages": (_i, [_vp, _pp, _pp, _pp]),
    "cc_cascade_stumps": (_i, [_vp, _pp, _pp, _pp, _pp, _pp]),
    "cc_cascade_features": (_i, [_vp, _pp, _pp, _pp]),
    "cc_cascade_save_xml": (_i, [_vp, C.c_char_p]),
    "cc_cascade_save_xml_legacy": (_i, [_vp, C.c_char_p]),
    "cc_vec_read": (_i, [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _vp, _i]),
    "cc_vec_write": (_i, [C.c_char_p, _vp, _i, _i, _i]),
    "cc_detector_create": (_i, [_vp, _i, _i, _pp]),
    "cc_detector_destroy": (None, [_vp]),
    "cc_detector_set_stream": (_i, [_vp, _vp]),
    "cc_detect_multiscale": (_i, [_vp, _vp, _i, _i, _sz, C.POINTER(DetectParams), _vp, _i, C.POINTER(_i)]),
    "cc_detect_batch": (_i, [_vp, _vp, _i, _i, _i, _i, _sz, _sz, C.POINTER(DetectParams), _vp, _i, _vp]),
    "cc_detect_batch_submit": (_i, [_vp, _vp, _i, _i, _i, _i, _sz, _sz, C.POINTER(DetectParams), _pp]),
    "cc_detect_batch_collect": (_i, [_vp, _vp, _vp, _i, _vp]),
    "cc_detect_batch_discard": (_i, [_vp, _vp]),
    "cc_detect_batch_device_only": (_i, [_vp, _vp, _i, _i, _i, _i, _sz, _sz, C.POINTER(DetectParams)]),
    "cc_detect_multiscale_fmt": (_i, [_vp, _vp, _i, _i, _sz, _i, C.POINTER(DetectParams), _vp, _i, C.POINTER(_i)]),
    "cc_detect_batch_fmt": (_i, [_vp, _vp, _i, _i, _i, _i, _sz, _sz, _i, C.POINTER(DetectParams), _vp, _i, _vp]),
    "cc_detect_batch_submit_fmt": (_i, [_vp, _vp, _i, _i, _i, _i, _sz, _sz, _i, C.POINTER(DetectParams), _pp]),
    "cc_detect_batch_to_device": (_i, [_vp, _vp, _i, _i, _i, _i, _sz, _sz, _i, C.POINTER(DetectParams), _vp, _i, _vp,
                                       C.POINTER(_i)]),
    "cc_detect_batch_levels_fmt": (_i, [_vp, _vp, _i, _i, _i, _i, _sz, _sz, _i, C.POINTER(DetectParams), _vp, _vp, _vp, _i, _vp]),
    "cc_detect_batch_to_device_levels": (_i, [_vp, _vp, _i, _i, _i, _i, _sz, _sz, _i, C.POINTER(DetectParams), _vp, _vp, _vp, _i,
                                              _vp, C.POINTER(_i)]),
    "cc_detect_multiscale_levels_fmt": (_i, [_vp, _vp, _i, _i, _sz, _i, C.POINTER(DetectParams), _vp, _vp, _vp, _i,
                                             C.POINTER(_i)]),
    "cc_to_gray_u8": (_i, [_i, _vp, _i, _i, _i, _sz, _vp, _sz]),
    "cc_detect_multiscale_levels": (_i, [_vp, _vp, _i, _i, _sz, C.POINTER(DetectParams), _vp, _vp, _vp, _i, C.POINTER(_i)]),
    "cc_detect_raw": (_i, [_vp, _vp, _i, _i, _sz, C.POINTER(DetectParams), _vp, _i, C.POINTER(_i)]),
    "cc_detect_debug_windows": (_i, [_vp, _vp, _i, _i, _sz, C.POINTER(DetectParams), _vp, _vp, _vp, C.c_int64,
                                     C.POINTER(C.c_int64)]),
    "cc_scale_plan": (_i, [_i, _i, _i, _i, C.POINTER(DetectParams), _vp, _i, C.POINTER(_i)]),
    "cc_detector_specialize": (_i, [_vp, _i]),
    "cc_detector_specialize_async": (_i, [_vp, _i]),
    "cc_detector_specialized_stages": (_i, [_vp]),
    "cc_cascade_compile_specialized": (_i, [_vp, _i, C.c_char_p, C.POINTER(C.c_size_t)]),
    "cc_detector_set_profiling": (_i, [_vp, _i]),
    "cc_detector_graph_active": (_i, [_vp]),
    "cc_detector_graph_captures": (C.c_int64, [_vp]),
    "cc_detector_get_timings": (_i, [_vp, C.POINTER(DetectorTimings), _i]),
    "cc_detector_candidate_capacity": (_i, [_vp]),
    "cc_integral_u8": (_i, [_i, _vp, _i, _i, _sz, _vp, _vp, _vp]),
    "cc_resize_linear_exact_u8": (_i, [_i, _vp, _i, _i, _sz, _vp, _i, _i, _sz]),
    "cc_debug_stream_dwords": (_i, [_i, _sz, _i, C.POINTER(C.c_uint32)]),
    "cc_debug_division_check": (_i, [_i, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cc_debug_vnf_check": (_i, [_i, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cc_debug_wave_int_tables": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "cc_debug_spec_step1_plan": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp]),
    "cc_debug_spec_step2_plan": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp]),
    "cc_group_rectangles": (_i, [_vp, _i, _i, _d, _vp, _i, C.POINTER(_i)]),
    "cc_group_rectangles_device": (_i, [_i, _vp, _vp, _i, _i, _d, _vp, _i, _vp, C.POINTER(_i)]),
    "cc_group_rectangles_levels": (_i, [_vp, _vp, _vp, _i, _i, _d, _vp, _vp, _vp, _i, C.POINTER(_i)]),
    "cc_group_rectangles_device_levels": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _d, _vp, _vp, _vp, _i, _vp, C.POINTER(_i)]),
    "cc_eval_create": (_i, [_i, _i, _i, _i, _i, _i, _pp]),
    "cc_eval_destroy": (None, [_vp]),
    "cc_eval_num_features": (_i, [_vp]),
    "cc_eval_max_cat_count": (_i, [_vp]),
    "cc_eval_feature_size": (_i, [_vp]),
    "cc_eval_feature_geometry": (_i, [_vp, _i, _vp, _vp, C.POINTER(_i)]),
    "cc_eval_set_image": (_i, [_vp, _vp, _sz, C.c_uint8, _i]),
    "cc_eval_set_images": (_i, [_vp, _vp, _i, _i, _vp]),
    "cc_eval_labels": (C.POINTER(C.c_float), [_vp]),
    "cc_eval_calc": (_i, [_vp, _i, _i, C.POINTER(C.c_float)]),
    "cc_eval_calc_list": (_i, [_vp, _vp, _i, _i, _vp]),
    "cc_eval_calc_batch": (_i, [_vp, _i, _i, _vp, _i, _vp, _i]),
    "cc_eval_calc_batch_device": (_i, [_vp, _i, _i, _vp, _i, _vp, _sz]),
    "cc_eval_calc_batch_sorted": (_i, [_vp, _i, _i, _i, _vp, _vp, _i]),
    "cc_eval_calc_custom_haar": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp]),
    "cc_haar_feature_calc": (_i, [_i, _vp, _i, _i, _vp, _vp, _i, _i, _vp]),
    "cc_eval_get_sample": (_i, [_vp, _i, _vp, _vp, _vp]),
    "cc_eval_hog_feature_geometry": (_i, [_vp, _i, _vp]),
    "cc_eval_get_hog_sample": (_i, [_vp, _i, _vp, _vp]),
    "cc_debug_hog_bins": (_i, [_i, C.POINTER(C.c_int32), _vp, _vp]),
    "cc_debug_hog_lds": (_i, [_i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "cc_eval_predict_cascade": (_i, [_vp, _vp, _vp, _i, _vp]),
    "cc_eval_last_kernel_ms": (_i, [_vp, C.POINTER(C.c_double)]),
    "cc_debug_eval_tile_samples": (_i, [_vp]),
    "cc_eval_presort": (_i, [_vp, _i]),
    "cc_eval_presort_range": (_i, [_vp, _i, _i, _i]),
    "cc_presort_plan": (_i, [_i, _i, _i, C.c_uint64, C.POINTER(_i), C.POINTER(_i), C.POINTER(C.c_uint64)]),
    "cc_eval_presort_split": (_i, [_vp, _i, _i, _i, _i, _i]),
    "cc_eval_table_bytes": (_i, [_vp, C.POINTER(C.c_uint64)]),
    "cc_eval_presort_budget": (_i, [_vp, C.POINTER(C.c_uint64)]),
    "cc_eval_stream_profile": (_i, [_vp, _i]),
    "cc_eval_stream_phase_ms": (_i, [_vp, _vp, _i, C.POINTER(_i)]),
    "cc_eval_find_best_split": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _d, _i, _i, C.POINTER(Split), _vp, _vp]),
    "cc_boost_create": (_i, [_vp, _i, C.POINTER(BoostParams), _pp]),
    "cc_boost_create_depth": (_i, [_vp, _i, C.POINTER(BoostParams), _i, _pp]),
    "cc_boost_destroy": (None, [_vp]),
    "cc_boost_round": (_i, [_vp, C.POINTER(Weak)]),
    "cc_boost_train_stage": (_i, [_vp, C.POINTER(Weak), _i, C.POINTER(_i)]),
    "cc_boost_last_tree": (_i, [_vp, C.POINTER(TreeNode), _i, _vp, _i, C.POINTER(_i)]),
    "cc_boost_get_state": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "cc_boost_last_round_ms": (_i, [_vp, _vp, _i, C.POINTER(_i)]),
    "cc_debug_exp64": (_i, [_i, _vp, _i, _vp]),
    "cc_cascade_from_stumps": (_i, [_i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _pp]),
    "cc_cascade_from_trees": (_i, [_i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _i, C.POINTER(TreeNode), _vp, _pp]),
    "cc_train_params_save_xml": (_i, [C.POINTER(TrainParams), C.c_char_p, C.c_char_p]),
    "cc_train_params_load_xml": (_i, [C.c_char_p, C.POINTER(TrainParams)]),
    "cc_cascade_train_params": (_i, [_vp, C.POINTER(TrainParams)]),
    "cc_cascade_save_xml_params": (_i, [_vp, C.POINTER(TrainParams), C.c_char_p]),
    "cc_stage_save_xml": (_i, [C.c_char_p, C.c_char_p, _i, C.c_float, _i, _vp, _i, C.POINTER(TreeNode), _vp]),
    "cc_stage_load_xml": (_i, [C.c_char_p, _i, _i, C.POINTER(C.c_float), C.POINTER(_i), _vp, _i, C.POINTER(_i), C.POINTER(TreeNode), _i, _vp]),
    "cc_shard_range": (None, [_i, _i, _i, C.POINTER(_i), C.POINTER(_i)]),
    "cc_comm_unique_id": (_i, [_vp]),
    "cc_comm_create": (_i, [_i, _i, _i, _vp, _pp]),
    "cc_comm_destroy": (None, [_vp]),
    "cc_comm_rank": (_i, [_vp]),
    "cc_comm_world": (_i, [_vp]),
    "cc_gather_detections": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _i, C.POINTER(_i), C.POINTER(_i)]),
    "cc_gather_fetch": (_i, [_vp, _vp, _i, _vp, _i]),
    "cc_negminer_create": (_i, [_vp, _i, _pp]),
    "cc_negminer_destroy": (None, [_vp]),
    "cc_negminer_plan": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, C.POINTER(_i), C.POINTER(C.c_int64)]),
    "cc_negminer_run": (_i, [_vp, _vp, _i, _i, _sz, _i, _i, _vp, C.c_int64, C.POINTER(C.c_int64), _vp, _vp, _i, C.POINTER(_i)]),
    "cc_negminer_run_batch": (_i, [_vp, _vp, _i, _i, _i, _sz, _i, _i, _vp, C.c_int64, C.POINTER(C.c_int64), _vp, _vp, _i, C.POINTER(_i)]),
    "cc_negminer_create_empty": (_i, [_i, _i, _i, _i, _pp]),
    "cc_negminer_fill": (_i, [_vp, _vp, _vp, _i, _i, _i, _sz, _i, _i, C.c_int64, _i, _i, C.c_int64, C.c_int64, _d,
                              C.POINTER(_i), C.POINTER(C.c_int64), C.POINTER(_i), _vp]),
    "cc_eval_fill_passed": (_i, [_vp, _vp, _vp, _i, _i, _i, C.c_uint8, C.POINTER(_i), C.POINTER(C.c_int64)]),
    "cc_debug_fill_select": (_i, [_i, _vp, C.c_int64, C.c_int64, _i, C.c_int64, C.c_int64, _d, C.POINTER(_i), C.POINTER(C.c_int64),
                                  C.POINTER(_i), _vp]),
    "cc_debug_fill_scan_tile": (_i, []),
    "cc_warp_perspective_u8": (_i, [_i, _vp, _i, _i, _sz, _vp, _i, _i, _sz, _vp]),
    "cc_sample_plan": (_i, [_i, _i, _i, _i, C.POINTER(SampleParams), C.POINTER(C.c_uint64), C.POINTER(SampleBgReader), _i, _vp, _vp]),
    "cc_sampler_create": (_i, [_i, _vp, _i, _i, _sz, _i, _i, _pp]),
    "cc_sampler_destroy": (None, [_vp]),
    "cc_sampler_set_backgrounds": (_i, [_vp, _vp, _vp, _vp, _i]),
    "cc_sampler_render": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _i, _vp]),
    "cc_testset_plan": (_i, [_i, _i, _i, _i, C.POINTER(SampleParams), C.POINTER(C.c_uint64), C.POINTER(SampleBgReader),
                             C.POINTER(_d), C.POINTER(C.c_int32), _i, C.POINTER(C.c_int32), _vp, _vp, _vp]),
    "cc_sampler_render_testset": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _sz]),
    "cc_area_tab": (_i, [_i, _i, C.POINTER(_d), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _vp, _vp, _vp, _i, C.POINTER(C.c_int32)]),
    "cc_samples_from_info": (_i, [_i, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _vp, _vp]),
    "cc_samples_from_info_last_ms": (_i, [C.POINTER(_d), C.POINTER(_d), C.POINTER(_d)]),
    "cc_resize_area_u8": (_i, [_i, _vp, _i, _i, _sz, _vp, _i, _i]),
}
CC_FILL_FILLED, CC_FILL_RATIO, CC_FILL_EXHAUSTED = 0, 1, 2
CC_SAMPLE_RANDOM_INVERT = 0x7FFFFFFF

_lib = None


def _share_torch_hip_runtime():
    """One process must hold ONE HIP runtime: PyTorch-ROCm wheels bundle their own libamdhip64.so.7, and a second copy
    (the system one our DT_NEEDED would pick) cannot open the GPU once the first has. Pre-load torch's copy (same
    SONAME) when a torch wheel is installed, so this library and a later `import torch` share it. Without torch the
    system runtime under /opt/rocm is used. CCAMD_HIP_RUNTIME=system forces the latter."""
    if os.environ.get("CCAMD_HIP_RUNTIME", "torch") == "system":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except OSError:
        pass


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
                "or make -C cascadeclassifier_amd/csrc). There is no CPU fallback.")
        _share_torch_hip_runtime()
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)  # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(status: int) -> int:
    if status != CC_OK:
        raise CascadeError(status, lib().cc_last_error().decode("utf-8", "replace"))
    return status


def pack_trees(weak):
    """(n_nodes, TreeNode array, leaves) of weak records, as cc_cascade_from_trees and cc_stage_save_xml take them: a record with
    "nodes" (and "leaves") is a tree, any other the stump left=0, right=-1 of its own fields. Leaves and thresholds are cast to
    float, as the writer does; the caller has dropped the records with trained == False."""
    trees = [(w["nodes"], w["leaves"]) if "nodes" in w else ([dict(w, left=0, right=-1)], [w["left_value"], w["right_value"]]) for w in weak]
    n_nodes = np.array([len(nodes) for nodes, _ in trees], np.int32)
    flat = (TreeNode * max(1, int(n_nodes.sum())))()
    for k, nd in enumerate(nd for nodes, _ in trees for nd in nodes):
        flat[k].left, flat[k].right, flat[k].var_idx = int(nd["left"]), int(nd["right"]), int(nd["var_idx"])
        flat[k].ord_c = float(np.float32(nd.get("ord_c", 0.0)))
        flat[k].subset[:] = [int(v) for v in np.asarray(nd.get("subset", np.zeros(8)), np.int64).astype(np.int32)]
    return n_nodes, flat, np.array([np.float32(v) for _, lv in trees for v in lv], np.float32)
