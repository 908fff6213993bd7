"""The training side past its size thresholds, compared exactly with the oracle (oracle/oracle.py) or, for HOG, with the
restatement (tests/hog_restatement.py). Each test goes past one point where the device code changes path:

* more than 65 536 presorted samples: 32-bit sorted indices (`wide_index`, cc_eval_internal.h), and presort in several
  passes of FB = 2^28 / N variables;
* LBP sample numbers >= 2^16 in the packed (sample << 8 | code) entries of the categorical tables, and the default number
  of parts per variable at N = 100 000 (97 on 256 CUs; CCAMD_SPLIT_CAT_PARTS cannot go past 64);
* calc_batch_sorted with 4-byte indices (2-byte indices refused past 65 536);
* negative-mining batches of several 8 MiB pieces (cc_negmine.hip mine_images);
* HOG windows whose setImage kernel needs more than 64 KB of LDS, and the windows at the edges of its LDS plan
  (tests/hog_lds_cases.py);
* more than 4 096 queued setImage windows (the queue is flushed while calls still arrive).

Samples j < N - 65 536 are copied to j + 65 536 with the opposite label and a very different weight: an index truncated
to 16 bits then reads the wrong sample, and the ties between the two copies are ordered by sample index."""
import os

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from cascadeclassifier_amd import evaluator as ev
from oracle import oracle as orc
from tests import cascade_factory as cf
from tests import hog_lds_cases as lds
from tests import hog_mine_cases as mc
from tests import hog_restatement as hog
from tests.test_gpu_negmine import _truncated
from tests.test_gpu_split import _samples
from tests.util import frame_natural

pytestmark = pytest.mark.gpu

SHIFT = 65536  # sample j's copy lives at j + SHIFT
SPLIT_CASES = [(ev.BOOST_GENTLE, 0), (ev.BOOST_LOGIT, 0), (ev.BOOST_REAL, 0), (ev.BOOST_DISCRETE, 0),
               (ev.BOOST_REAL, ev.SPLIT_MISCLASS), (ev.BOOST_DISCRETE, ev.SPLIT_GINI)]


def _u(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _copies(n):
    return np.arange(0, max(n - SHIFT, 0), 3)


def _with_copies(imgs, labels, seed):
    """Copies j -> j + SHIFT (opposite label), and per-sample weights where a copy weighs 1000 times more or less."""
    n = len(imgs)
    src = _copies(n)
    imgs[src + SHIFT] = imgs[src]
    labels[src + SHIFT] = 1 - labels[src]
    gw = np.random.default_rng(seed).random(n) ** 3 + 1e-3
    gw[src + SHIFT] = np.where(src % 2 == 0, gw[src] * 1000.0, gw[src] / 1000.0)
    return imgs, labels, gw


def _radix_argsort(vals):
    """Stable argsort in the device's radix order of float keys: like a stable argsort, but -0.0 before +0.0."""
    u = _u(vals)
    key = np.where(u >> 31 == 1, ~u, u | np.uint32(0x80000000))
    return np.argsort(key, axis=1, kind="stable")


def _node(gw, labels, idx, boost_type, seed, real_responses=False):
    """Weights (n + 2 doubles as CvBoostTree::calc_node_value leaves them, totals accumulated in node order), labels or
    responses, and the node value of the node listing stored samples `idx` in that order."""
    lab = labels[idx].astype(np.int32)
    w = gw[idx] / gw[idx].sum()
    classifier = boost_type in (ev.BOOST_DISCRETE, ev.BOOST_REAL)
    if classifier:
        tot = [np.cumsum(w[lab == c])[-1] if (lab == c).any() else 0.0 for c in (0, 1)]
        return np.concatenate([w, tot]), {"class_labels": lab}, 0.0
    resp = (lab * 2 - 1).astype(np.float32)
    if real_responses:  # LOGIT boost hands arbitrary working responses to the tree
        resp = (resp * np.random.default_rng(seed).random(len(idx)) * 3).astype(np.float32)
    r = np.cumsum(w)[-1]
    s = np.cumsum(resp.astype(np.float64) * w)[-1]
    return np.concatenate([w, [r, 0.0]]), {"responses": resp}, s * (1.0 / r)


def _oracle_split(slices, w, tie, **kw):
    """orc.find_best_split over slices (first variable, values in node order) of the variables, combined the way the
    device combines variables: the first of the variables with the largest float quality wins."""
    best, qs, pts = None, [], []
    for f0, vals in slices:
        want, q, pt = orc.find_best_split(vals, w, tie_key=tie, per_feature=True, **kw)
        qs.append(q)
        pts.append(pt)
        if want["found"] and (best is None or want["quality"] > best["quality"]):
            best = {k: want[k] for k in want.dtype.names}
            best["var_idx"] = int(want["var_idx"]) + f0
    if best is None:
        best = {"found": 0}
    return best, np.concatenate(qs), np.concatenate(pts)


def _check(e, slices, gw, labels, idx, *, boost_type, criteria=0, categorical=False, seed=0, real_responses=False, root=False):
    """Device search of the node `idx` (root=True: the whole presorted set, no index list) against the oracle: every
    variable's split point and float quality, and the winner (variable, quality, threshold / subset, split point)."""
    idx = np.asarray(idx, np.int32)
    w, kw, nv = _node(gw, labels, idx, boost_type, seed, real_responses)
    got, gq, gpt = e.find_best_split(w, sample_idx=None if root else idx, node_value=nv, boost_type=boost_type, split_criteria=criteria,
                                     per_var=True, **kw)
    want, wq, wpt = _oracle_split(slices(idx), w, idx, categorical=categorical, node_value=nv, boost_type=boost_type, split_criteria=criteria, **kw)
    gqf = np.where(gpt >= 0, gq.astype(np.float32), np.float32(-1))
    assert (gpt == wpt).all(), f"split points differ for {int((gpt != wpt).sum())} of {len(gpt)} variables (n = {len(idx)})"
    assert (_u(gqf) == _u(wq)).all(), f"qualities differ for {int((_u(gqf) != _u(wq)).sum())} of {len(gq)} variables (n = {len(idx)})"
    assert bool(want["found"]) == got["found"]
    if got["found"]:
        assert got["var_idx"] == want["var_idx"] and got["quality"] == want["quality"]
        if categorical:
            assert (got["subset"] == want["subset"]).all()
        else:
            assert got["ord_c"] == want["ord_c"] and got["split_point"] == want["split_point"]
    return got, gq, gpt


def _nodes(n, seed):
    """The root, a sorted subset with members on both sides of SHIFT (both copies of some samples among them), the same
    subset in permuted order, and a two-sample node."""
    rng = np.random.default_rng(seed)
    src = _copies(n)
    pick = src[::11]
    sub = np.unique(np.concatenate([rng.choice(n, n // 5, replace=False), pick, pick + SHIFT, [3, n - 1]]))
    pair = [3, 3 + SHIFT] if n > 3 + SHIFT else [3, n - 1]
    return [("root", np.arange(n)), ("sorted", sub), ("permuted", rng.permutation(sub)), ("pair", np.array(pair))]


# ---- 1. ordered split with 32-bit sorted indices (Haar) ------------------------------------------------------------
HAAR_RANGE = (900, 1092)  # 192 variables of the 8x8 BASIC catalog (2 056): one presort pass at every size below


@pytest.fixture(scope="module", params=[65536, 65537, 100000])
def haar_big(request):
    n, win = request.param, (8, 8)
    imgs, labels = _samples(n, win, 17)
    imgs, labels, gw = _with_copies(imgs, labels, 18)
    e = cc.CvFeatureEvaluator.create(ev.HAAR)
    e.init(cc.CvFeatureParams(ev.HAAR, ev.BASIC), n, win)
    e.setImages(imgs, labels)
    e.presort(n, *HAAR_RANGE)
    s, t, nf = orc.set_images(imgs)
    vals = orc.haar_eval_batch(orc.haar_catalog(8, 8, ev.BASIC), *HAAR_RANGE, s, t, nf, 8, 8)
    return n, e, labels, gw, vals


@pytest.mark.parametrize("boost_type,criteria", SPLIT_CASES)
def test_haar_ordered_split_past_65536_samples(haar_big, boost_type, criteria):
    """Sizes 65 536 (the last with 16-bit indices), 65 537 and 100 000; all three MODEs of k_split_ord (regression,
    GINI, MISCLASS) with the per-sample table in global memory; root, sorted, permuted and two-sample nodes."""
    n, e, labels, gw, vals = haar_big
    slices = lambda idx: [(HAAR_RANGE[0], vals[:, idx])]  # noqa: E731
    for k, (name, idx) in enumerate(_nodes(n, 5 + boost_type)):
        got, _, _ = _check(e, slices, gw, labels, idx, boost_type=boost_type, criteria=criteria, seed=k, root=name == "root",
                           real_responses=boost_type == ev.BOOST_LOGIT)
        if name != "pair":
            assert got["found"], name


def test_haar_presort_in_two_passes():
    """At N = 100 000 a presort pass holds 2 624 variables: [0, 2 700) of the 10x10 catalog takes two passes, the second
    writing the 32-bit index tables of the groups behind the first pass's. The oracle runs on slices of 300 variables."""
    n, win, f0, f1 = 100000, (10, 10), 0, 2700
    assert f0 + ((1 << 28) // n) // 64 * 64 < f1 < orc.haar_catalog_size(10, 10, ev.BASIC)
    imgs, labels = _samples(n, win, 27)
    imgs, labels, gw = _with_copies(imgs, labels, 28)
    e = cc.CvFeatureEvaluator.create(ev.HAAR)
    e.init(cc.CvFeatureParams(ev.HAAR, ev.BASIC), n, win)
    e.setImages(imgs, labels)
    e.presort(n, f0, f1)
    s, t, nf = orc.set_images(imgs)
    cat = orc.haar_catalog(10, 10, ev.BASIC)

    def slices(idx):
        for a in range(f0, f1, 300):
            yield a, orc.haar_eval_batch(cat, a, min(a + 300, f1), s, t, nf, 10, 10, idx)

    got, _, _ = _check(e, slices, gw, labels, np.arange(n), boost_type=ev.BOOST_GENTLE, seed=1, root=True)
    assert got["found"]
    sub = np.unique(np.concatenate([np.random.default_rng(3).choice(n, 6000, replace=False), _copies(n)[::40] + SHIFT]))
    _check(e, slices, gw, labels, sub, boost_type=ev.BOOST_DISCRETE, seed=2)


# ---- 2. calc_batch_sorted, gathers and cascade prediction past 65 536 samples --------------------------------------
SORT_RANGE = (700, 956)


@pytest.fixture(scope="module")
def haar_65537():
    n, win = 65537, (8, 8)
    imgs, labels = _samples(n, win, 37)
    imgs, labels, _ = _with_copies(imgs, labels, 38)
    imgs[100:110] = imgs[20000]  # whole columns of ties
    e = cc.CvFeatureEvaluator.create(ev.HAAR)
    e.init(cc.CvFeatureParams(ev.HAAR, ev.BASIC), n, win)
    e.setImages(imgs, labels)
    s, t, nf = orc.set_images(imgs)
    return e, imgs, (s, t, nf)


def test_sorted_indices_past_65536(haar_65537):
    e, imgs, (s, t, nf) = haar_65537
    n = len(imgs)
    want = orc.haar_eval_batch(orc.haar_catalog(8, 8, ev.BASIC), *SORT_RANGE, s, t, nf, 8, 8)
    vals, idx = e.calc_batch_sorted(*SORT_RANGE)  # the default past 65 535 samples: 4-byte indices
    assert idx.dtype == np.int32 and vals.shape == idx.shape == (SORT_RANGE[1] - SORT_RANGE[0], n)
    assert (_u(vals) == _u(want)).all()
    assert (idx == _radix_argsort(want)).all()
    with pytest.raises(cc.CascadeError):
        e.calc_batch_sorted(SORT_RANGE[0], SORT_RANGE[0] + 4, idx_bytes=2)
    # 65 536 samples: 16-bit indices still hold every sample number (0 ... 65 535)
    v16, i16 = e.calc_batch_sorted(*SORT_RANGE, n_samples=SHIFT, idx_bytes=2)
    assert i16.dtype == np.uint16 and i16.shape == (SORT_RANGE[1] - SORT_RANGE[0], SHIFT)
    assert (_u(v16) == _u(want[:, :SHIFT])).all()
    ref16 = _radix_argsort(want[:, :SHIFT])
    assert ref16.max() == SHIFT - 1 and (i16.astype(np.int64) == ref16).all()
    # like the reference (is_buf_16u: sample_count < 65536), the Python default takes 4-byte indices at 65 536
    v32, i32 = e.calc_batch_sorted(*SORT_RANGE, n_samples=SHIFT)
    assert i32.dtype == np.int32 and (i32 == ref16).all() and (_u(v32) == _u(v16)).all()


def test_gathers_and_cascade_prediction_past_65536(tmp_path):
    n, win = 100000, (8, 8)
    imgs, labels = _samples(n, win, 47)
    imgs, labels, _ = _with_copies(imgs, labels, 48)
    e = cc.CvFeatureEvaluator.create(ev.HAAR)
    e.init(cc.CvFeatureParams(ev.HAAR, ev.BASIC), n, win)
    e.setImages(imgs, labels)
    s, t, nf = orc.set_images(imgs)
    cat = orc.haar_catalog(8, 8, ev.BASIC)
    rng = np.random.default_rng(49)
    sel = np.concatenate([[SHIFT, SHIFT - 1, n - 1, 3, 3 + SHIFT], rng.integers(SHIFT, n, 3000), rng.integers(0, SHIFT, 1000)])
    rng.shuffle(sel)
    got = e.calc_batch(0, len(cat), sample_idx=sel)
    want = orc.haar_eval_batch(cat, 0, len(cat), s, t, nf, 8, 8, sel)
    assert (_u(got) == _u(want)).all(), f"{int((_u(got) != _u(want)).sum())} values differ"
    # a stump cascade on the 8x8 window, thresholds at the medians: predict on stored samples beyond 65 536
    fi = rng.choice(len(cat), 12, replace=False)
    feats = cat[fi].copy()
    v = orc.haar_eval_batch(feats, 0, len(feats), s, t, nf, 8, 8, np.arange(0, n, 7))
    thr = np.median(v, axis=1).astype(np.float32)
    stages, k = [], 0
    for nw in (3, 4, 5):
        weaks = [([(0, -1, k + i, thr[k + i])], [1.0 if (k + i) % 2 else -1.0, -1.0 if (k + i) % 2 else 1.0]) for i in range(nw)]
        stages.append((np.float32(-0.5), weaks))
        k += nw
    path = os.path.join(str(tmp_path), "stumps8.xml")
    open(path, "w").write(cf.haar_xml(feats, stages, mode="BASIC", W=8, H=8))
    c = cc.CascadeClassifier(path)
    o = orc.load_cascade_xml(path)
    want_p = np.array([orc.train_predict(o, s, t, nf, int(i), 8, 8) for i in sel], np.uint8)
    assert 0 < want_p.sum() < len(sel)
    assert (e.predict_cascade(c, sample_idx=sel) == want_p).all()
    every = e.predict_cascade(c)
    assert every.shape == (n,) and (every[sel] == want_p).all()


# ---- 3. LBP categorical split at N = 100 000 -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lbp_big():
    n, win = 100000, (8, 8)
    imgs, labels = _samples(n, win, 57)
    imgs, labels, gw = _with_copies(imgs, labels, 58)
    e = cc.CvFeatureEvaluator.create(ev.LBP)
    e.init(cc.CvFeatureParams(ev.LBP, 0), n, win)
    e.setImages(imgs, labels)
    e.presort()
    assert e.getNumVariables() == 81
    s, _, _ = orc.set_images(imgs, want_norm=False)
    vals = orc.lbp_eval_batch(orc.lbp_catalog(8, 8), 0, 81, s, 8, 8)
    return n, e, labels, gw, vals


@pytest.mark.parametrize("boost_type", [ev.BOOST_GENTLE, ev.BOOST_LOGIT, ev.BOOST_REAL, ev.BOOST_DISCRETE])
def test_lbp_categorical_split_at_100000(lbp_big, boost_type, monkeypatch):
    """Sorted nodes search the (code, sample)-sorted table (k_split_cat_sorted, sample numbers >= 2^16 in the packed
    entries), permuted ones stream the codes (k_split_cat); the default 97 parts per variable on 256 CUs. Then the same
    nodes with the sorted table switched off (CCAMD_SPLIT_CAT_STREAM=1) give the same results bit for bit."""
    n, e, labels, gw, vals = lbp_big
    slices = lambda idx: [(0, vals[:, idx])]  # noqa: E731
    nodes = _nodes(n, 65 + boost_type)
    runs = []
    for k, (name, idx) in enumerate(nodes):
        runs.append(_check(e, slices, gw, labels, idx, boost_type=boost_type, categorical=True, seed=k, root=name == "root",
                           real_responses=boost_type == ev.BOOST_LOGIT))
        if name != "pair":
            assert runs[-1][0]["found"], name
    monkeypatch.setenv("CCAMD_SPLIT_CAT_STREAM", "1")
    try:
        e.presort()
        for k, (name, idx) in enumerate(nodes):
            w, kw, nv = _node(gw, labels, np.asarray(idx, np.int32), boost_type, k, boost_type == ev.BOOST_LOGIT)
            got, gq, gpt = e.find_best_split(w, sample_idx=None if name == "root" else np.asarray(idx, np.int32), node_value=nv,
                                             boost_type=boost_type, per_var=True, **kw)
            ref = runs[k]
            assert all(np.array_equal(got[key], ref[0][key]) for key in ref[0]), name
            assert (gq.view(np.uint64) == ref[1].view(np.uint64)).all() and (gpt == ref[2]).all(), name
    finally:
        monkeypatch.delenv("CCAMD_SPLIT_CAT_STREAM")
        e.presort()


# ---- 4. HOG variables at N = 70 000 ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hog_70000():
    n, win = 70000, (16, 16)
    rng = np.random.default_rng(67)
    imgs = rng.integers(0, 256, (n, 16, 16), dtype=np.uint8)
    yy, xx = np.mgrid[0:16, 0:16]
    imgs[1::5] = np.clip(xx * 9 + yy * 4 + rng.integers(-6, 7, (len(imgs[1::5]), 16, 16)), 0, 255)  # structured windows
    imgs[2::97] = 50  # flat windows: every variable 0
    labels = (rng.random(n) < 0.5).astype(np.uint8)
    imgs, labels, gw = _with_copies(imgs, labels, 68)
    e = cc.CvFeatureEvaluator.create(ev.HOG)
    e.init(cc.CvFeatureParams.create(ev.HOG), n, win)
    e.setImages(imgs, labels)
    assert e.getNumVariables() == 36
    vals = e.calc_batch(0, 36)
    return n, e, imgs, labels, gw, vals


def test_hog_values_and_sorted_indices_at_70000(hog_70000):
    n, e, imgs, labels, gw, vals = hog_70000
    rng = np.random.default_rng(69)
    sub = np.concatenate([np.arange(0, 200), np.arange(SHIFT - 200, SHIFT + 200), np.arange(n - 200, n), rng.choice(n, 200, replace=False)])
    hist, norm = hog.set_images(imgs[sub])
    want = hog.eval_vars(hog.catalog(16, 16), hist, norm)
    assert (_u(vals[:, sub]) == _u(want)).all(), f"{int((_u(vals[:, sub]) != _u(want)).sum())} values differ"
    sv, si = e.calc_batch_sorted(0, 36)
    assert si.dtype == np.int32 and (_u(sv) == _u(vals)).all()
    assert (si == _radix_argsort(vals)).all()


@pytest.mark.parametrize("boost_type", [ev.BOOST_GENTLE, ev.BOOST_REAL, ev.BOOST_DISCRETE])
def test_hog_split_at_70000(hog_70000, boost_type):
    """HOG's ordered variables go through the Haar tables with 32-bit indices; the oracle searches the device's values."""
    n, e, imgs, labels, gw, vals = hog_70000
    e.presort()
    slices = lambda idx: [(0, vals[:, idx])]  # noqa: E731
    for k, (name, idx) in enumerate(_nodes(n, 75 + boost_type)):
        got, _, _ = _check(e, slices, gw, labels, idx, boost_type=boost_type, seed=k, root=name == "root")
        if name != "pair":
            assert got["found"], name


# ---- 5. negative-mining batches of several pieces --------------------------------------------------------------------
def _mining_cascade(kind, tmp, haar_xml, lbp_xml):
    if kind == "haar3":
        return _truncated(haar_xml, 3, tmp)
    if kind == "lbp4":
        return _truncated(lbp_xml, 4, tmp)
    calib = frame_natural(320, 240, 3)
    wins = np.stack([calib[y:y + 24, x:x + 24] for y in range(0, 200, 9) for x in range(0, 280, 11)])
    path = os.path.join(tmp, kind + ".xml")
    open(path, "w").write(cf.haar_tree_cascade(wins, with_tilted=True))
    return path


@pytest.mark.parametrize("width", [1918, 1920])
@pytest.mark.parametrize("kind", ["haar3", "lbp4", "haar_trees"])
def test_negative_mining_batch_in_several_pieces(tmp_path, haar_xml, lbp_xml, kind, width):
    """Full-HD images: 4 per 8 MiB piece, so batches of 9 and 10 images take three pieces (staged by several threads).
    Width 1918 is staged row by row into a pitch of 1920, width 1920 with one copy per image. One miner runs 1, 3, 2 and
    3 pieces in turn (the per-piece event list grows on the second call). Every image's flags equal the oracle's reader
    loop and a per-image run; the kept windows, some of them from the third piece, equal the per-image runs'."""
    path = _mining_cascade(kind, str(tmp_path), haar_xml, lbp_xml)
    o = orc.load_cascade_xml(path)
    c = cc.CascadeClassifier(path)
    assert not c.empty(), getattr(c, "load_error", "")
    m = cc.NegativeMiner(c)
    imgs = [frame_natural(width, 1080, 300 + k) for k in range(10)]
    single = []
    for im in imgs:
        want_f, want_p, want_i = orc.negmine_image(o, im, max_keep=64)
        f, p, i = m.run(im, max_keep=int(want_f.sum()))
        assert f.shape == want_f.shape and (f == want_f).all(), f"{int((f != want_f).sum())} of {len(want_f)} windows differ"
        assert (i[:64] == want_i).all() and (p[:64] == want_p).all()
        single.append((f, p, i))
    wins = len(single[0][0])
    passes = [int(f.sum()) for f, _, _ in single]
    assert passes[8] > 0 and passes[9] > 0, passes
    for k in (3, 10, 6, 9):
        keep = sum(passes[:k - 1]) + (passes[k - 1] + 1) // 2  # ends in the middle of the last image's kept windows
        flags, pix, idx = m.run_batch(imgs[:k], max_keep=keep)
        assert flags.shape == (k, wins)
        for j in range(k):
            assert (flags[j] == single[j][0]).all(), f"batch of {k}, image {j}: {int((flags[j] != single[j][0]).sum())} windows differ"
        want_idx = np.concatenate([i + j * wins for j, (_, _, i) in enumerate(single[:k])])[:keep]
        want_pix = np.concatenate([p for _, p, _ in single[:k]])[:keep]
        assert len(idx) == keep and (idx == want_idx).all() and (pix == want_pix).all()
        if k >= 9:
            assert idx[-1] // wins >= 8  # kept windows of the third piece (k_negmine_gather's image offset)


def test_negative_mining_batch_limits(tmp_path, haar_xml):
    """256 small images take two pieces (204 per piece at 256x160) and equal one run per image; 257 are refused."""
    path = _truncated(haar_xml, 3, str(tmp_path))
    o = orc.load_cascade_xml(path)
    m = cc.NegativeMiner(cc.CascadeClassifier(path))
    big = frame_natural(256 * 16, 160 * 16, 91)
    imgs = [np.ascontiguousarray(big[(k // 16) * 160:(k // 16 + 1) * 160, (k % 16) * 256:(k % 16 + 1) * 256]) for k in range(256)]
    single = [m.run(im, max_keep=0)[0] for im in imgs]
    flags, pix, idx = m.run_batch(imgs, max_keep=10 ** 5)
    wins = flags.shape[1]
    for j in range(256):
        assert (flags[j] == single[j]).all(), f"image {j}: {int((flags[j] != single[j]).sum())} windows differ"
    for j in (0, 203, 204, 255):  # either side of the piece boundary
        assert (flags[j] == orc.negmine_image(o, imgs[j], max_keep=1)[0]).all(), j
    assert (idx == np.nonzero(flags.ravel())[0][:10 ** 5]).all() and flags[204:].any()
    assert len(pix) == len(idx)
    with pytest.raises(cc.CascadeError):
        m.run_batch(imgs + imgs[:1], max_keep=0)
    assert wins == m.plan(256, 160)["n_windows"]


# ---- 6. HOG windows beyond 64 KB of LDS ------------------------------------------------------------------------------
def _hog_windows(win, n, seed):
    W, H = win
    rng = np.random.default_rng(seed)
    imgs = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    imgs[1] = np.where(xx >= W // 3, 200, 10)
    imgs[2] = np.clip(xx * 2 + yy + rng.integers(-4, 5, (H, W)), 0, 255)
    imgs[3] = frame_natural(W, H, seed + 1)
    return imgs


@pytest.mark.parametrize("win", [(128, 64), (96, 96), (128, 128)])
def test_hog_windows_beyond_64k_of_lds(win):
    """128x64 and 96x96 take three planes per LDS pass (140 032 and 157 824 B), 128x128 one (147 968 B)."""
    want_plan = {(128, 64): (3, 160, 140032), (96, 96): (3, 160, 157824), (128, 128): (1, 160, 147968)}[win]
    assert lds.exported(*win)[:3] == want_plan == lds.TABLE[win][:3]
    imgs = _hog_windows(win, 4, sum(win))
    e = cc.CvFeatureEvaluator.create(ev.HOG)
    e.init(cc.CvFeatureParams.create(ev.HOG), len(imgs), win)
    e.setImages(imgs)
    hist, norm = hog.set_images(imgs)
    for i in range(len(imgs)):
        h, nrm = e.get_sample(i)
        assert (_u(h) == _u(hist[i])).all() and (_u(nrm) == _u(norm[i])).all(), (win, i)
    nv = e.getNumVariables()
    assert nv == 36 * len(hog.catalog(*win))
    got = e.calc_batch(0, nv)
    want = hog.eval_vars(hog.catalog(*win), hist, norm)
    assert (_u(got) == _u(want)).all(), f"{int((_u(got) != _u(want)).sum())} values differ"


def _var_ranges(n_blocks, seed):
    """Variable ranges for windows whose every variable is too much for the numpy loop: the first 20 blocks, the last 20, and
    8 runs of 5 blocks at seeded places (40 blocks). Each range starts and ends inside a block."""
    rng = np.random.default_rng(seed)
    starts = [0, n_blocks - 20] + sorted(int(b) for b in rng.choice(np.arange(20, n_blocks - 25), 8, replace=False))
    return [(b * 36 + 5 + 3 * k, (b + (20 if k < 2 else 5)) * 36 - 7 - k) for k, b in enumerate(starts)]


@pytest.mark.parametrize("win", lds.EVAL_WINDOWS, ids=lambda w: "%dx%d" % w)
def test_hog_windows_at_the_edges_of_the_lds_plan(win):
    """The setImage plan at each budget's edge (tests/hog_lds_cases.py; the classes are asserted in tests/test_hog_lds_host.py):
    37x37 ten planes per pass, 38x38 and 24x60 nine, 32x75 five, 85x85 one inside 64 KiB, 86x85 four of 160 KiB, 134x135 and
    135x134 one of 160 KiB and the last windows accepted. Planes bitwise; every variable up to 86x85, ranges beyond."""
    assert lds.exported(*win) == lds.TABLE[win] and lds.eval_accepts(win)
    imgs = _hog_windows(win, 5, sum(win))
    e = cc.CvFeatureEvaluator.create(ev.HOG)
    e.init(cc.CvFeatureParams.create(ev.HOG), len(imgs), win)
    e.setImages(imgs)
    hist, norm = hog.set_images(imgs)
    for i in range(len(imgs)):
        h, nrm = e.get_sample(i)
        assert (_u(h) == _u(hist[i])).all() and (_u(nrm) == _u(norm[i])).all(), (win, i)
    cat = hog.catalog(*win)
    nv = e.getNumVariables()
    assert nv == 36 * len(cat)
    if win not in lds.EVAL_LAST_ACCEPTED:
        assert nv <= 47952  # 86x85: 1 332 blocks
        got = e.calc_batch(0, nv)
        want = hog.eval_vars(cat, hist, norm)
        assert (_u(got) == _u(want)).all(), f"{int((_u(got) != _u(want)).sum())} values differ"
        return
    assert len(cat) == 5728 and nv == 206208
    new = _hog_windows(win, 4, sum(win) + 9)[3]
    e.setImage(new, 0, 2)  # the host mirror of a window set through setImage
    h_new, n_new = hog.set_images(new[None])
    rng = np.random.default_rng(sum(win))
    for vb, ve in _var_ranges(len(cat), sum(win)):
        assert vb % 36 != 0 and ve % 36 != 0
        want = hog.eval_vars(cat, hist, norm, vb, ve)
        got = e.calc_batch(vb, ve, sample_idx=np.array([0, 1, 3, 4], np.int32))
        assert (_u(got) == _u(want[:, [0, 1, 3, 4]])).all(), (vb, ve)
        vis = np.sort(rng.choice(np.arange(vb, ve), 40, replace=False))
        mirror = np.array([e(int(vi), 2) for vi in vis], np.float32)
        assert (_u(mirror) == _u(hog.eval_vars(cat, h_new, n_new, vb, ve)[vis - vb, 0])).all(), (vb, ve)
    h, nrm = e.get_sample(2)  # and the device's copy of that window
    assert (_u(h) == _u(h_new[0])).all() and (_u(nrm) == _u(n_new[0])).all()


def test_hog_predict_at_the_first_window_of_the_160k_branch(tmp_path):
    """predict_cascade with a HOG stump cascade at 86x85 (planes of 299 280 B per sample) against the restatement's walk.
    The case and its 10-90 % pass share: tests/hog_mine_cases.py, tests/test_hog_mine_cases_host.py."""
    win = (86, 85)
    samples, xml, _, _, want = mc.predict_case_86x85()
    assert 0 < want.sum() < len(samples)
    path = str(tmp_path / "hog.xml")
    open(path, "w").write(xml)
    c = cc.CascadeClassifier(path)
    assert not c.empty(), getattr(c, "load_error", "")
    e = cc.CvFeatureEvaluator.create(ev.HOG)
    e.init(cc.CvFeatureParams.create(ev.HOG), len(samples), win)
    e.setImages(samples)
    assert (e.predict_cascade(c) == want).all()


def test_hog_window_too_large_for_lds():
    e = cc.CvFeatureEvaluator.create(ev.HOG)
    for win in [(160, 160)] + lds.EVAL_FIRST_REFUSED:  # 135x135 and 136x134: the first windows past 134x135
        assert not lds.eval_accepts(win)
        with pytest.raises(cc.CascadeError) as err:
            e.init(cc.CvFeatureParams.create(ev.HOG), 2, win)
        assert err.value.status == L.CC_ERR_UNSUPPORTED and "LDS" in str(err.value), win
    for win in lds.EVAL_LAST_ACCEPTED:
        assert lds.eval_accepts(win)
        e.init(cc.CvFeatureParams.create(ev.HOG), 2, win)
    imgs = _hog_windows((24, 24), 4, 3)  # and after a refusal an evaluator still works
    e.init(cc.CvFeatureParams.create(ev.HOG), len(imgs), (24, 24))
    e.setImages(imgs)
    hist, norm = hog.set_images(imgs)
    assert (_u(e.calc_batch(0, e.getNumVariables())) == _u(hog.eval_vars(hog.catalog(24, 24), hist, norm))).all()


# ---- 7. the setImage queue past 4 096 windows ------------------------------------------------------------------------
@pytest.mark.parametrize("ftype", [ev.HAAR, ev.HOG])
def test_set_image_queue_past_4096(ftype):
    """About 5 400 setImage calls into 5 000 distinct odd slots in random order, with no read in between: the queue
    (kMaxQueued = 4 096) is flushed while calls still arrive. Some slots are written twice, inside one queue and across
    the flush. calc_batch over all samples then equals setImages of the same windows, and the oracle / restatement."""
    n, win = 12000, ((8, 8) if ftype == ev.HAAR else (16, 16))
    W, H = win
    rng = np.random.default_rng(81 + ftype)
    base = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    lab = (rng.random(n) < 0.5).astype(np.uint8)
    params = cc.CvFeatureParams.create(ftype) if ftype == ev.HOG else cc.CvFeatureParams(ev.HAAR, ev.BASIC)
    e = cc.CvFeatureEvaluator.create(ftype)
    e.init(params, n, win)
    e.setImages(base, lab)
    slots = rng.permutation(np.arange(1, n, 2))[:5000]
    new = rng.integers(0, 256, (len(slots), H, W), dtype=np.uint8)
    new[::3] = np.clip(np.mgrid[0:H, 0:W][1] * 13, 0, 255).astype(np.uint8)
    new_lab = 1 - lab[slots]
    decoy = rng.integers(0, 256, (H, W), dtype=np.uint8)
    final, final_lab = base.copy(), lab.copy()
    final[slots], final_lab[slots] = new, new_lab
    calls = [(int(s), decoy, 0) for s in slots[:200]]                                  # replaced inside the first queue
    calls += [(int(s), new[k], int(new_lab[k])) for k, s in enumerate(slots)]           # the 4 097th distinct slot flushes
    for ks in (range(0, 50), range(4100, 4150)):                                        # already on the device / still queued
        calls += [(int(slots[k]), decoy, 1) for k in ks] + [(int(slots[k]), new[k], int(new_lab[k])) for k in ks]
    for s, img, c in calls:
        e.setImage(img, c, s)
    got = e.calc_batch(0, e.getNumVariables())
    assert (e.getCls() == final_lab).all()
    fresh = cc.CvFeatureEvaluator.create(ftype)
    fresh.init(params, n, win)
    fresh.setImages(final, final_lab)
    ref = fresh.calc_batch(0, fresh.getNumVariables())
    assert (_u(got) == _u(ref)).all(), f"{int((_u(got) != _u(ref)).sum())} values differ"
    if ftype == ev.HAAR:
        s, t, nf = orc.set_images(final)
        want = orc.haar_eval_batch(orc.haar_catalog(W, H, ev.BASIC), 0, e.getNumVariables(), s, t, nf, W, H)
        assert (_u(got) == _u(want)).all()
    else:
        sub = np.unique(np.concatenate([slots[:100], slots[4090:4200], slots[-100:], np.arange(0, 100)]))
        hist, norm = hog.set_images(final[sub])
        want = hog.eval_vars(hog.catalog(W, H), hist, norm)
        assert (_u(got[:, sub]) == _u(want)).all()
