"""GPU parity tests of the HOG evaluator against the numpy restatement (tests/hog_restatement.py) of CvHOGEvaluator
(HOGfeatures.h:84-112, HOGfeatures.cpp:67-256). Every comparison is bitwise (uint32 views, tolerance 0)."""
import os

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from cascadeclassifier_amd import evaluator as ev
from oracle import oracle as orc
from tests import hog_lds_cases as lds
from tests import hog_restatement as hog
from tests.util import read_vec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _u(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _make(win, n):
    e = cc.CvFeatureEvaluator.create(ev.HOG)
    e.init(cc.CvFeatureParams.create(ev.HOG), n, win)
    return e


def _windows(win, n, seed):
    """Random, constant and step-edge windows, and smooth ramps with noise."""
    W, H = win
    rng = np.random.default_rng(seed)
    imgs = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(0, n, 4):
        kind = (i // 4) % 4
        if kind == 0:
            imgs[i] = (i * 37) % 256
        elif kind == 1:
            imgs[i] = np.where(xx >= (i % W), 200, 10)
        elif kind == 2:
            imgs[i] = np.where(yy >= (i % H), 30, 240)
        else:
            imgs[i] = np.clip(xx * 3 + yy * 2 + rng.integers(-4, 5, (H, W)), 0, 255)
    return imgs


def _barcode():
    return read_vec(os.path.join(ROOT, "tests", "golden", "barcode.vec"))


def test_factory_and_getters():
    p = cc.CvFeatureParams.create(ev.HOG)
    assert p is not None and p.featSize == 36 and p.maxCatCount == 0
    e = _make((32, 32), 4)
    assert e.getNumFeatures() == 36
    assert e.getFeatureSize() == 36
    assert e.getMaxCatCount() == 0
    assert e.getNumVariables() == 1296
    for fi in (0, 7, 35):
        assert (e.feature_geometry(fi) == hog.cells(hog.catalog(32, 32)[fi])).all()
    import ctypes as C
    rects = np.zeros(12, np.int32)
    assert L.lib().cc_eval_feature_geometry(e._e, 0, rects.ctypes.data_as(C.c_void_p), None, None) == L.CC_ERR_INVALID_ARG
    s = np.zeros(33 * 33, np.int32)
    assert L.lib().cc_eval_get_sample(e._e, 0, s.ctypes.data_as(C.c_void_p), None, None) == L.CC_ERR_INVALID_ARG
    with pytest.raises(cc.CascadeError):
        e.calc_custom_haar([(False, [(0, 0, 2, 2, 1.0)])])


@pytest.mark.parametrize("win,blocks", [((16, 16), 1), ((24, 24), 9), ((75, 32), 159), ((64, 64), 528), ((12, 12), 0)])
def test_num_features(win, blocks):
    assert _make(win, 2).getNumFeatures() == blocks


def test_reference_cases():
    """test_features.cpp:394-440: constant image -> every variable 0; vertical edge -> some variable > 0."""
    e = _make((32, 32), 2)
    flat = np.full((32, 32), 90, np.uint8)
    edge = np.zeros((32, 32), np.uint8)
    edge[:, 16:] = 255
    e.setImages(np.stack([flat, edge]))
    v = e.calc_batch(0, e.getNumVariables())
    assert not v[:, 0].any()
    assert (v[:, 1] > 0).any()


def test_bins_all_pairs():
    import ctypes as C
    n = C.c_int32(0)
    b = np.empty(511 * 511, np.uint8)
    m = np.empty(511 * 511, np.float32)
    L.check(L.lib().cc_debug_hog_bins(0, C.byref(n), b.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p)))
    assert n.value == 261121
    wb, wm = hog.bin_table()
    assert (b == wb).all(), f"{int((b != wb).sum())} bins differ"
    assert (_u(m) == _u(wm)).all()


def _assert_planes(e, imgs, where):
    for i in range(len(imgs)):
        h, nrm = e.get_sample(i)
        wh, wn = hog.set_image(imgs[i])
        assert (_u(h) == _u(wh)).all(), (where, i)
        assert (_u(nrm) == _u(wn)).all(), (where, i)


# the windows at the edges of the setImage kernel's LDS plan (tests/hog_lds_cases.py, held to the library's own plan in
# tests/test_hog_lds_host.py): ten and nine planes per pass, tall windows, one plane per pass inside 64 KiB, the first window
# of the 160 KiB branch, the last windows accepted at all
@pytest.mark.parametrize("win", [(16, 16), (24, 24), (32, 32), (75, 32), (70, 40)] + lds.EVAL_WINDOWS)
def test_planes(win):
    imgs = _windows(win, 6 if win in lds.EVAL_WINDOWS else 12, sum(win))
    e = _make(win, len(imgs))
    e.setImages(imgs)
    _assert_planes(e, imgs, win)


@pytest.mark.parametrize("order", ["large_first", "small_first"])
def test_evaluators_of_two_sizes_share_the_kernel(order):
    """k_hog_set_images' LDS opt-in belongs to the kernel, not to an evaluator: a 134x135 evaluator (163 350 B) and an 86x85
    one (154 870 B), created and filled in either order; then the large one takes new windows and still gives the
    restatement's planes, and so does the small one."""
    large, small = (134, 135), (86, 85)
    assert lds.eval_opts_in(large) and lds.eval_opts_in(small) and lds.TABLE[large][2] > lds.TABLE[small][2]
    made = {}
    for win in ((large, small) if order == "large_first" else (small, large)):
        imgs = _windows(win, 4, sum(win))
        made[win] = _make(win, len(imgs))
        made[win].setImages(imgs)
        _assert_planes(made[win], imgs, (order, win, "first"))
    for win in (large, small):
        again = _windows(win, 4, sum(win) + 1)
        made[win].setImages(again)
        _assert_planes(made[win], again, (order, win, "again"))


def test_all_variables_barcode():
    imgs = _barcode()
    assert imgs.shape == (100, 32, 75)
    e = _make((75, 32), len(imgs))
    e.setImages(imgs)
    nv = e.getNumVariables()
    assert nv == 5724
    hist, norm = hog.set_images(imgs)
    want = hog.eval_vars(hog.catalog(75, 32), hist, norm)
    got = e.calc_batch(0, nv)
    assert (_u(got) == _u(want)).all(), f"{int((_u(got) != _u(want)).sum())} values differ"


def test_all_variables_20000_at_32x32():
    n = 20000
    rng = np.random.default_rng(5)
    imgs = rng.integers(0, 256, (n, 32, 32), dtype=np.uint8)
    imgs[::7] = np.clip(np.mgrid[0:32, 0:32][1] * 8, 0, 255).astype(np.uint8)  # repeated structured windows
    e = _make((32, 32), n)
    e.setImages(imgs)
    got = e.calc_batch(0, e.getNumVariables())
    # the restatement on a subset of samples (it is slow in numpy); every sample is compared through the planes' values
    sub = np.r_[0:300, n - 300:n, rng.choice(n, 400, replace=False)]
    hist, norm = hog.set_images(imgs[sub])
    want = hog.eval_vars(hog.catalog(32, 32), hist, norm)
    assert (_u(got[:, sub]) == _u(want)).all()
    # and the gathered form of the same call over all samples
    again = e.calc_batch(0, e.getNumVariables(), sample_idx=np.arange(n, dtype=np.int32))
    assert (_u(again) == _u(got)).all()


@pytest.fixture(scope="module")
def ev32():
    win, n = (32, 32), 300
    imgs = _windows(win, n, 9)
    e = _make(win, n)
    e.setImages(imgs, labels=(np.arange(n) % 2).astype(np.uint8))
    full = e.calc_batch(0, e.getNumVariables())
    hist, norm = hog.set_images(imgs)
    want = hog.eval_vars(hog.catalog(32, 32), hist, norm)
    assert (_u(full) == _u(want)).all()
    return e, imgs, full


def test_gather_ranges_pitched_list_scalar(ev32):
    import torch
    e, imgs, full = ev32
    n = len(imgs)
    idx = np.random.default_rng(3).permutation(n)[:123].astype(np.int32)
    g = e.calc_batch(0, e.getNumVariables(), sample_idx=idx)
    assert (_u(g) == _u(full[:, idx])).all()
    r = e.calc_batch(17, 1000)  # starts and ends inside a block
    assert (_u(r) == _u(full[17:1000])).all()
    r = e.calc_batch(40, 41, sample_idx=idx[:5])
    assert (_u(r) == _u(full[40:41, idx[:5]])).all()
    pitch = n + 37
    d = torch.full((1000 - 17, pitch), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()  # the fill runs on torch's stream, the evaluator on its own: unordered, the fill can land last
    e.calc_batch_device(17, 1000, d.data_ptr(), pitch=pitch)
    torch.cuda.synchronize()
    dd = d.cpu().numpy()
    assert (_u(dd[:, :n]) == _u(full[17:1000])).all() and (dd[:, n:] == -7.0).all()
    vl = np.array([0, 35, 36, 500, 1295, 17, 17], np.int32)
    assert (_u(e.calc_list(vl, 11)) == _u(full[vl, 11])).all()
    # scalar operator() on the window set last by setImage (host mirror) and on a stored sample (device)
    e.setImage(imgs[5], 1, 5)
    mir = np.array([e(vi, 5) for vi in range(e.getNumVariables())], np.float32)
    assert (_u(mir) == _u(full[:, 5])).all()
    assert (_u(e.calc_list(np.arange(1296, dtype=np.int32), 5)) == _u(full[:, 5])).all()
    assert np.float32(e(700, 9)).view(np.uint32) == full[700, 9].view(np.uint32)
    # a new window through the pending queue: the mirror and the device agree with the restatement
    new = _windows((32, 32), 8, 77)[3]
    e.setImage(new, 0, 7)
    hist, norm = hog.set_images(new[None])
    want = hog.eval_vars(hog.catalog(32, 32), hist, norm)[:, 0]
    assert (_u(np.array([e(vi, 7) for vi in range(0, 1296, 7)], np.float32)) == _u(want[::7])).all()
    assert (_u(e.calc_batch(0, 1296, sample_idx=np.array([7], np.int32))[:, 0]) == _u(want)).all()
    e.setImage(imgs[7], 1, 7)  # restore for the tests below


@pytest.mark.parametrize("idx_bytes", [2, 4])
def test_sorted(ev32, idx_bytes):
    e, imgs, full = ev32
    vals, idx = e.calc_batch_sorted(0, e.getNumVariables(), idx_bytes=idx_bytes)
    assert (_u(vals) == _u(full)).all()
    want = np.argsort(full, axis=1, kind="stable")
    assert (idx.astype(np.int64) == want).all()


def _weights(n, lab, seed, classifier):
    rng = np.random.default_rng(seed)
    w = rng.random(n) ** 3 + 1e-3
    w /= w.sum()
    if classifier:
        r = [0.0, 0.0]
        for i in range(n):
            r[int(lab[i])] += w[i]
        return np.concatenate([w, r])
    tot = 0.0
    for i in range(n):
        tot += w[i]
    return np.concatenate([w, [tot, 0.0]])


@pytest.mark.parametrize("boost_type", [ev.BOOST_GENTLE, ev.BOOST_DISCRETE])
@pytest.mark.parametrize("subset", [False, True])
def test_presort_find_best_split(ev32, boost_type, subset):
    e, imgs, full = ev32
    n_all = len(imgs)
    labels = (np.arange(n_all) % 2).astype(np.int32)
    e.presort()
    idx = np.sort(np.random.default_rng(4).choice(n_all, 170, replace=False)).astype(np.int32) if subset else None
    lab = labels if idx is None else labels[idx]
    n = len(lab)
    classifier = boost_type == ev.BOOST_DISCRETE
    w = _weights(n, lab, 8, classifier)
    kw, node_value = {}, 0.0
    if classifier:
        kw["class_labels"] = lab
    else:
        resp = (lab * 2 - 1).astype(np.float32)
        kw["responses"] = resp
        s = r = 0.0
        for i in range(n):
            r += w[i]
            s += float(resp[i]) * w[i]
        node_value = s * (1.0 / r)
    got, gq, gpt = e.find_best_split(w, sample_idx=idx, node_value=node_value, boost_type=boost_type, per_var=True, **kw)
    vals = full if idx is None else full[:, idx]
    want, wq, wpt = orc.find_best_split(vals, w, node_value=node_value, boost_type=boost_type, tie_key=idx, per_feature=True, **kw)
    gqf = np.where(gpt >= 0, gq.astype(np.float32), np.float32(-1))
    assert (gpt == wpt).all()
    assert (_u(gqf) == _u(wq)).all()
    assert bool(want["found"]) == got["found"] and got["found"]
    assert got["var_idx"] == want["var_idx"] and got["quality"] == want["quality"]
    assert got["ord_c"] == want["ord_c"] and got["split_point"] == want["split_point"]
