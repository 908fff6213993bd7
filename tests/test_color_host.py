"""CPU side of colour detection: the integer restatement of COLOR_BGR2GRAY the GPU tests compare with, the Python mapping
from array shapes and pixel_format keywords to the C ABI's formats and byte strides (detector.frame_layout), and the
compat cv::Mat's colour types (tests/cpp/test_color_compat.cpp). No device is touched."""
import os
import subprocess

import numpy as np
import pytest

from cascadeclassifier_amd import _lib as L
from cascadeclassifier_amd.detector import PIXEL_FORMATS, frame_layout

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def restated_gray(b, g, r):
    b, g, r = (np.asarray(x, np.uint32) for x in (b, g, r))
    return ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14).astype(np.uint8)


def test_restatement_known_answers():
    assert restated_gray(255, 0, 0) == 29
    assert restated_gray(0, 255, 0) == 150
    assert restated_gray(0, 0, 255) == 76
    assert restated_gray(255, 255, 255) == 255
    assert restated_gray(0, 0, 0) == 0
    v = np.arange(256)
    assert (restated_gray(v, v, v) == v).all()  # the weights sum to 2^14: gray stays gray
    # 32-bit exact: the largest sum fits easily
    assert 255 * (1868 + 9617 + 4899) + 8192 < 2 ** 31


def test_restatement_is_not_pil():
    rng = np.random.default_rng(0)
    b, g, r = rng.integers(0, 256, (3, 4096), dtype=np.uint32)
    pil = ((r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16).astype(np.uint8)
    assert (restated_gray(b, g, r) != pil).any()


def test_pixel_format_codes_match_the_header():
    assert PIXEL_FORMATS == {"gray": 0, "bgr": 1, "bgra": 2, "rgb": 3, "rgba": 4, "rgb_planar": 5}
    hdr = open(os.path.join(ROOT, "include", "cascadeclassifier_amd.h")).read()
    for name, code in (("GRAY8", 0), ("BGR8", 1), ("BGRA8", 2), ("RGB8", 3), ("RGBA8", 4), ("RGB8_PLANAR", 5)):
        assert f"CC_PIX_{name} = {code}" in hdr
        assert getattr(L, f"CC_PIX_{name}") == code


@pytest.mark.parametrize("shape,fmt,batched,want", [
    ((48, 64), None, False, (1, 48, 64, 0, 64, 64 * 48)),
    ((48, 64), "gray", False, (1, 48, 64, 0, 64, 64 * 48)),
    ((48, 64, 3), None, False, (1, 48, 64, 1, 192, 192 * 48)),
    ((48, 64, 3), "bgr", False, (1, 48, 64, 1, 192, 192 * 48)),
    ((48, 64, 3), "rgb", False, (1, 48, 64, 3, 192, 192 * 48)),
    ((48, 64, 4), None, False, (1, 48, 64, 2, 256, 256 * 48)),
    ((48, 64, 4), "rgba", False, (1, 48, 64, 4, 256, 256 * 48)),
    ((3, 48, 64), "rgb_planar", False, (1, 48, 64, 5, 64, 64 * 48 * 3)),
    ((5, 48, 64), None, True, (5, 48, 64, 0, 64, 64 * 48)),
    ((5, 48, 64, 3), None, True, (5, 48, 64, 1, 192, 192 * 48)),
    ((5, 48, 64, 3), "rgb", True, (5, 48, 64, 3, 192, 192 * 48)),
    ((5, 48, 64, 4), "bgra", True, (5, 48, 64, 2, 256, 256 * 48)),
    ((5, 48, 64, 4), "rgba", True, (5, 48, 64, 4, 256, 256 * 48)),
    ((5, 3, 48, 64), "rgb_planar", True, (5, 48, 64, 5, 64, 64 * 48 * 3)),
    ((1, 1, 1, 3), None, True, (1, 1, 1, 1, 3, 3)),
])
def test_frame_layout(shape, fmt, batched, want):
    assert frame_layout(shape, fmt, batched) == want


@pytest.mark.parametrize("shape,fmt,batched", [
    ((48, 64, 2), None, False),         # two channels
    ((48, 64, 5), None, False),
    ((48, 64), "bgr", False),           # gray array, colour format
    ((48, 64, 3), "rgba", False),       # channel count disagrees
    ((48, 64, 4), "bgr", False),
    ((48, 64, 3), "yuv", False),        # unknown keyword
    ((48, 64, 3), "rgb_planar", False), # planar needs (3, H, W)
    ((4, 48, 64), "rgb_planar", False),
    ((48,), None, False),
    ((2, 48, 64, 3, 1), None, True),
    ((5, 48, 64, 2), None, True),
    ((5, 4, 48, 64), "rgb_planar", True),
    ((0, 0), None, False),
    ((), None, True),                   # a batch without a frame count
    ((), None, False),
])
def test_frame_layout_errors(shape, fmt, batched):
    with pytest.raises(L.CascadeError) as e:
        frame_layout(shape, fmt, batched)
    assert e.value.status == L.CC_ERR_INVALID_ARG


def test_compat_mat_colour_types():
    exe = os.path.join(ROOT, "cascadeclassifier_amd", "lib", "test_color_compat")
    assert os.path.exists(exe), "build() makes it (cascadeclassifier_amd/cpp/Makefile)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
