"""The front-end kernels (cc_front.hip) at their own edges, against the witnesses of tests/front_cases.py with no oracle in
the loop: k_resize at sources narrower than its 16-byte load, at wavefronts that mix both load paths, at tap weights of
256, at the sizes where the operation order of the taps shows, at the quad / block / band boundaries and on upscales;
k_diag_sums / k_tilted_cols at their 64-row segments, 4-diagonal threads and 64-column groups; the training evaluator's
LBP codes on images full of ties. tests/test_front_cases_host.py ties the oracle to the same witnesses and shows that
each case is what its reason says. Then the paths only the detector takes: k_resize feeding the band sums on frames
narrower than 16 columns, and device-resident frames with padded strides. Every comparison is exact."""
import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import detector as det
from cascadeclassifier_amd import evaluator as ev
from oracle import oracle as orc
from tests import front_cases as fc
from tests import haar_windows as hw
from tests.test_gpu_front_totals import _check_detector
from tests.test_gpu_negmine import _truncated
from tests.util import frame_natural

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", fc.resize_cases(), ids=lambda c: c[0])
def test_resize_equals_witness(case):
    _, sw, sh, dw, dh = case
    for name, img in fc.resize_case_images(sw, sh):
        want = fc.resize_witness(img, dw, dh)
        got = det.resize_linear_exact(img, dw, dh)
        assert got.shape == want.shape
        assert (got == want).all(), f"{name}: {(got != want).sum()} of {want.size} pixels differ"


@pytest.mark.parametrize("case", fc.TILTED, ids=lambda c: "%dx%d" % c[:2])
def test_tilted_integral_equals_witness(case):
    w, h, _ = case
    for name, img in fc.tilted_case_images(w, h):
        want = fc.tilted_witness(img)
        g = det.integral(img, sqsum=True, tilted=True)
        assert g["tilted"].shape == want.shape
        assert (g["tilted"] == want).all(), f"{name}: {(g['tilted'] != want).sum()} of {want.size} entries differ"
        assert (g["sum"] == fc.integral_witness(img, False)).all() and (g["sqsum"] == fc.integral_witness(img, True)).all(), name


@pytest.mark.parametrize("W,H", fc.LBP_WINDOWS)
def test_training_lbp_codes_equal_witness(W, H):
    """calc_batch over the whole catalog: on the block images three comparisons in ten are ties."""
    rects = fc.lbp_catalog_witness(W, H)
    e = cc.CvFeatureEvaluator.create(ev.LBP)
    e.init(cc.CvFeatureParams(ev.LBP, 0), fc.LBP_SAMPLES, (W, H))
    assert e.getNumFeatures() == len(rects)
    for fi in range(0, len(rects), 211):
        assert (e.feature_geometry(fi)[0] == rects[fi]).all()
    for name, samples in fc.lbp_samples(W, H):
        e.setImages(samples)
        got = e.calc_batch(0, len(rects))
        want = fc.lbp_witness(samples, rects)
        assert got.shape == want.shape and (got == want).all(), f"{name}: {(got != want).sum()} of {want.size} codes differ"


@pytest.mark.parametrize("tilted", [False, True], ids=["upright", "tilted"])
@pytest.mark.parametrize("w", [15, 16, 17])
def test_detector_on_frames_narrower_than_the_wide_load(tmp_path, w, tilted):
    """k_resize writes the band sums only inside the detector and the miner. A 12x14 window lets frames of 15, 16 and 17
    columns through: at 15 every level is built with byte loads, at 16 and 17 with the 16-byte load clamped to the row's
    last 16 bytes; the levels are 12 to 17 columns wide, most no multiple of 4. The stock Haar cascade, truncated or not,
    has a 24-column window and refuses such frames, so both cascades here are the synthetic 12x14 stump cascades of
    tests/haar_windows.py, one upright and one with tilted features."""
    path = hw.write_xml(tmp_path, hw.stump_xml(12, 14, tilted))
    big = frame_natural(640, 480, 3)
    frames = [np.ascontiguousarray(big[40 + 50 * k:80 + 50 * k, 20 + 30 * w + 7 * k:20 + 30 * w + 7 * k + w]) for k in range(3)]
    assert frames[0].shape == (40, w)
    assert _check_detector(path, frames, True) > 0


@pytest.mark.parametrize("kind", ["haar", "lbp"])
def test_device_batch_with_padded_strides(tmp_path, haar_xml, lbp_xml, kind):
    """Three device-resident frames of 97x211 whose rows are 13 bytes longer than the width and whose frames are 57 bytes
    further apart than their rows need; the padding holds 255."""
    import torch
    path = _truncated(haar_xml, 6, str(tmp_path)) if kind == "haar" else _truncated(lbp_xml, 4, str(tmp_path))
    w, h, n = 97, 211, 3
    rs = w + 13
    fs = h * rs + 57
    frames = [frame_natural(w, h, 90 + i) for i in range(n)]
    buf = np.full(n * fs, 255, np.uint8)
    for i, f in enumerate(frames):
        buf[i * fs:i * fs + h * rs].reshape(h, rs)[:, :w] = f
    t = torch.from_numpy(buf).cuda()
    p = cc.CascadeClassifier(path, max_batch=n)
    o = orc.load_cascade_xml(path)
    for min_neighbors in (0, 2):  # 0: every candidate comes back ungrouped
        got = p.detect_batch(None, 1.1, min_neighbors, device_ptr=t.data_ptr(), shape=(n, h, w), row_stride=rs, frame_stride=fs)
        total = 0
        for i in range(n):
            want = orc.detect_multiscale(o, frames[i], 1.1, min_neighbors, nthreads=8)
            assert got[i].shape == want.shape and (got[i] == want).all(), (min_neighbors, i)
            total += len(want)
        assert total >= 20
