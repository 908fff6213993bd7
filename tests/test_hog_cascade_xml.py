"""HOG cascades in the cascade model (host only): the reference's cascade.xml layout for a CvHOGEvaluator
(featureParams maxCatCount 0 / featSize 36, <rect>x y cw ch comp</rect> per used variable; HOGfeatures.cpp:9-14, 155-160,
cascadeclassifier.cpp:566-578) loads, reports, saves and reloads identically; malformed files are CC_ERR_PARSE; every
consumer that cannot run a HOG cascade refuses it with CC_ERR_UNSUPPORTED before anything reaches a device."""
import ctypes as C
import os

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from tests import hog_cascade_factory as hf
from tests.util import frame_natural


def _windows(W, H, n_side=12, seed=3):
    img = frame_natural(W * 6, H * 5, seed)
    ys = np.linspace(0, img.shape[0] - H, n_side).astype(int)
    xs = np.linspace(0, img.shape[1] - W, n_side).astype(int)
    return np.stack([img[y:y + H, x:x + W] for y in ys for x in xs])


@pytest.fixture(scope="module", params=[(24, 24, 1), (32, 32, 2), (75, 32, 1)], ids=["24x24_stumps", "32x32_trees", "75x32_stumps"])
def hog_case(request):
    W, H, depth = request.param
    xml, feats, stages = hf.hog_cascade(_windows(W, H), seed=W + H, stage_sizes=(3, 4, 6), depth=depth)
    return W, H, depth, xml, feats, stages


def _load(text):
    c = cc.CascadeClassifier()
    ok = c.load_from_string(text)
    return c, ok


def _status(text):
    h = C.c_void_p()
    b = text.encode()
    st = L.lib().cc_cascade_load_xml_mem(b, len(b), C.byref(h))
    if st == L.CC_OK:
        L.lib().cc_cascade_destroy(h)
    return st


def test_load_info_features(hog_case):
    W, H, depth, xml, feats, stages = hog_case
    c, ok = _load(xml)
    assert ok, getattr(c, "load_error", "")
    inf = c.info()
    n_weak = sum(len(w) for _, w in stages)
    per_tree = 1 if depth == 1 else 3
    assert inf["feature_type"] == L.CC_FEATURE_HOG == 2
    assert (inf["win_w"], inf["win_h"]) == (W, H)
    assert inf["n_stages"] == len(stages) and inf["n_weak"] == n_weak
    assert inf["n_nodes"] == n_weak * per_tree and inf["n_leaves"] == n_weak * (per_tree + 1)
    assert inf["n_features"] == len(feats) and inf["max_cat_count"] == 0 and inf["subset_size"] == 0
    assert inf["max_nodes_per_tree"] == per_tree and inf["has_tilted"] == 0
    m = c.model()
    assert m.rects.shape == (len(feats), 5) and m.rects.dtype == np.int32
    assert (m.rects == feats).all()
    assert m.weights is None and m.tilted is None
    want = hf.parsed_model(stages)
    assert np.array_equal(m.stage_threshold, np.array([t for t, _ in want["stages"]], np.float32))
    if depth == 1:  # cc_cascade_stumps keeps working: feature index, threshold, leaves
        nodes = [w[0][0] for _, ws in want["stages"] for w in ws]
        leaves = [w[1] for _, ws in want["stages"] for w in ws]
        assert (m.stump_feature == [n[2] for n in nodes]).all()
        assert np.array_equal(m.stump_threshold, np.array([n[3] for n in nodes], np.float32))
        assert np.array_equal(m.stump_left, np.array([l[0] for l in leaves], np.float32))
        assert np.array_equal(m.stump_right, np.array([l[1] for l in leaves], np.float32))


def test_save_load_roundtrip(hog_case, tmp_path):
    xml = hog_case[3]
    c, ok = _load(xml)
    assert ok
    p1, p2 = str(tmp_path / "a.xml"), str(tmp_path / "b.xml")
    c.save(p1)
    text1 = open(p1).read()
    assert "<featureType>HOG</featureType>" in text1 and "<featSize>36</featSize>" in text1
    c2 = cc.CascadeClassifier(p1)
    assert not c2.empty(), getattr(c2, "load_error", "")
    a, b = c.model(), c2.model()
    assert a.info == b.info
    for f in ("stage_first", "stage_ntrees", "stage_threshold", "rects"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    if a.stump_feature is not None:
        for f in ("stump_feature", "stump_threshold", "stump_left", "stump_right"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
    c2.save(p2)
    assert open(p2, "rb").read() == open(p1, "rb").read()


def _base():
    feats = np.array([[0, 0, 8, 8, 3], [8, 8, 8, 8, 35]], np.int32)
    stages = [(np.float32(-0.5), [([(0, -1, 0, np.float32(0.1))], [np.float32(0.5), np.float32(-0.5)]),
                                  ([(0, -1, 1, np.float32(0.2))], [np.float32(-0.25), np.float32(0.25)])])]
    return feats, stages


def test_minimal_file_loads():
    feats, stages = _base()
    assert _status(hf.hog_xml(feats, stages, 24, 24)) == L.CC_OK


@pytest.mark.parametrize("case", ["comp36", "comp_negative", "block_outside_x", "block_outside_y", "zero_cell", "negative_x",
                                  "missing_rect", "four_numbers", "maxcat256", "featsize1"])
def test_malformed_files_are_parse_errors(case):
    feats, stages = _base()
    kw = {}
    if case == "comp36":
        feats[1, 4] = 36
    elif case == "comp_negative":
        feats[0, 4] = -1
    elif case == "block_outside_x":
        feats[1] = [12, 0, 8, 8, 0]  # 12 + 2 * 8 > 24
    elif case == "block_outside_y":
        feats[1] = [0, 9, 8, 8, 0]  # 9 + 2 * 8 > 24
    elif case == "zero_cell":
        feats[0, 2] = 0
    elif case == "negative_x":
        feats[0, 0] = -4
    elif case == "maxcat256":
        kw["max_cat_count"] = 256
    elif case == "featsize1":
        kw["feat_size"] = 1
    text = hf.hog_xml(feats, stages, 24, 24, **kw)
    if case == "missing_rect":
        text = text.replace("<rect>\n        8 8 8 8 35</rect>", "<rects>\n        8 8 8 8 35</rects>")
    elif case == "four_numbers":
        text = text.replace("8 8 8 8 35</rect>", "8 8 8 8</rect>")
    assert _status(text) == L.CC_ERR_PARSE, L.lib().cc_last_error().decode()


def test_block_on_the_window_edge_is_accepted():
    feats, stages = _base()
    feats[1] = [8, 8, 8, 8, 17]  # 8 + 2 * 8 == 24: the block ends on the window's edge
    assert _status(hf.hog_xml(feats, stages, 24, 24)) == L.CC_OK


def test_legacy_save_refused(tmp_path):
    feats, stages = _base()
    c, ok = _load(hf.hog_xml(feats, stages, 24, 24))
    assert ok
    with pytest.raises(cc.CascadeError) as err:
        c.save(str(tmp_path / "legacy.xml"), baseFormat=True)
    assert err.value.status == L.CC_ERR_UNSUPPORTED
    assert not os.path.exists(str(tmp_path / "legacy.xml"))


def test_detection_consumers_refuse_hog():
    """Checked before any device work, so these hold without a GPU too."""
    feats, stages = _base()
    c, ok = _load(hf.hog_xml(feats, stages, 24, 24))
    assert ok
    d = C.c_void_p()
    assert L.lib().cc_detector_create(c._c, 0, 1, C.byref(d)) == L.CC_ERR_UNSUPPORTED
    assert "HOG" in L.lib().cc_last_error().decode()
    n = C.c_size_t(0)
    assert L.lib().cc_cascade_compile_specialized(c._c, 2, b"gfx950", C.byref(n)) == L.CC_ERR_UNSUPPORTED
    assert "HOG" in L.lib().cc_last_error().decode()
    img = np.zeros((48, 48), np.uint8)
    for call in (lambda: c.detectMultiScale(img), lambda: c.detect_raw(img), lambda: c.specialize(2)):
        with pytest.raises(cc.CascadeError) as err:
            call()
        assert err.value.status == L.CC_ERR_UNSUPPORTED and "HOG" in str(err.value)
