"""Host side of the device-output entry points (cc_group_rectangles_device, cc_detect_batch_to_device): the symbols exist,
the Python wrappers bind them, the argument checks answer before any device is touched, and without a device both
calls fail with CC_ERR_NO_DEVICE."""
import ctypes as C
import inspect

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L


def test_symbols_and_wrappers_bind():
    lib = L.lib()
    for name in ("cc_group_rectangles_device", "cc_detect_batch_to_device", "cc_detector_candidate_capacity"):
        assert name in L.SIGNATURES and getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert callable(cc.group_rectangles_device)
    assert lib.cc_detector_candidate_capacity(None) == -1
    sig = inspect.signature(cc.CascadeClassifier.detect_batch_to_device)
    for kw in ("out_ptr", "cap", "offsets_ptr", "device_ptr", "shape", "pixel_format"):
        assert kw in sig.parameters


def test_argument_checks_come_first():
    lib = L.lib()
    n = C.c_int(0)
    one = C.c_void_p(64)  # never dereferenced: every call below fails on its arguments
    assert lib.cc_group_rectangles_device(0, one, None, 1, 1, 0.2, one, 4, one, C.byref(n)) == L.CC_ERR_INVALID_ARG
    assert lib.cc_group_rectangles_device(0, one, one, 1, 1, 0.2, one, 4, None, C.byref(n)) == L.CC_ERR_INVALID_ARG
    assert lib.cc_group_rectangles_device(0, one, one, 1, 1, 0.2, one, 4, one, None) == L.CC_ERR_INVALID_ARG
    assert lib.cc_group_rectangles_device(0, one, one, 1, 1, 0.2, one, -1, one, C.byref(n)) == L.CC_ERR_INVALID_ARG
    assert lib.cc_group_rectangles_device(0, one, one, 1, 1, 0.2, None, 4, one, C.byref(n)) == L.CC_ERR_INVALID_ARG
    assert lib.cc_group_rectangles_device(0, one, one, -1, 1, 0.2, one, 4, one, C.byref(n)) == L.CC_ERR_INVALID_ARG
    p = L.DetectParams(1.1, 3, 0, 0, 0, 0)
    assert lib.cc_detect_batch_to_device(None, one, 1, 1, 64, 64, 64, 4096, 0, C.byref(p), one, 4, one,
                                         C.byref(n)) == L.CC_ERR_INVALID_ARG  # null detector


def test_no_device_is_a_loud_error(lbp_xml):
    if L.lib().cc_device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(cc.CascadeError) as ei:
        cc.group_rectangles_device(64, 64, 1, 2, 64, 4, 64)
    assert ei.value.status == L.CC_ERR_NO_DEVICE
    p = cc.CascadeClassifier(lbp_xml)
    with pytest.raises(cc.CascadeError) as ei:
        p.detect_batch_to_device(np.zeros((2, 64, 64), np.uint8), 1.1, 3, out_ptr=64, cap=4, offsets_ptr=64)
    assert ei.value.status == L.CC_ERR_NO_DEVICE
