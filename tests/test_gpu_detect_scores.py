"""Detection scores on batches: detect_batch3 (cc_detect_batch_levels_fmt) against per-frame detectMultiScale3 and the oracle,
and detect_batch_to_device with levels_ptr / weights_ptr (cc_detect_batch_to_device_levels) against both -- the rectangles and
offsets of the unscored call, the levels and weights of detect_batch3 -- over several passes, host, device and colour frames,
the specialised kernel, the candidate-list regrow, a short buffer, and frames whose candidate counts lie on both sides of the
scored grouping kernel's LDS limit. Everything is compared exactly, the float64 weights with ==."""
import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from tests import score_cases as sc
from tests.util import frame_natural

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["haar", "lbp", "haar_specialised"])
def make(request, haar_xml, lbp_xml):
    """-> (xml, a function that makes a fresh detector for it)"""
    xml = lbp_xml if request.param == "lbp" else haar_xml

    def factory(max_batch=2):
        p = cc.CascadeClassifier(xml, max_batch=max_batch)
        if request.param == "haar_specialised":
            assert p.specialize(4) > 0
        return p
    return xml, factory


@pytest.fixture(scope="module")
def frames():
    return np.array(sc.detector_frames())  # a writable copy: torch.from_numpy wants one


def _same(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = (a,) if isinstance(a, np.ndarray) else a, (b,) if isinstance(b, np.ndarray) else b
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all(), (i, x, y)


def _to_device(p, frames, mn, cap=4096, scored=True, **kw):
    """-> per frame (rects, levels, weights), or the rectangles alone of the unscored call; the rows behind cap are checked."""
    import torch
    d_out = torch.full((cap + 1, 4), -7, dtype=torch.int32, device="cuda")
    d_lv = torch.full((cap + 1,), -7, dtype=torch.int32, device="cuda")
    d_wt = torch.full((cap + 1,), -7.0, dtype=torch.float64, device="cuda")
    d_off = torch.full((len(frames) + 1,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # the fills run on torch's stream, the detector on its own
    host = kw.pop("host", None)
    if scored:
        kw.update(levels_ptr=d_lv.data_ptr(), weights_ptr=d_wt.data_ptr())
    total = p.detect_batch_to_device(host, 1.1, mn, out_ptr=d_out.data_ptr(), cap=cap, offsets_ptr=d_off.data_ptr(), **kw)
    out, lv, wt, off = d_out.cpu().numpy(), d_lv.cpu().numpy(), d_wt.cpu().numpy(), d_off.cpu().numpy()
    assert (out[cap:] == -7).all() and off[0] == 0 and off[-1] == total
    if not scored:
        assert (lv == -7).all() and (wt == -7.0).all()
        return [out[off[i]:off[i + 1]] for i in range(len(frames))]
    assert (lv[total:] == -7).all() and (wt[total:] == -7.0).all()
    return [(out[off[i]:off[i + 1]], lv[off[i]:off[i + 1]], wt[off[i]:off[i + 1]]) for i in range(len(frames))]


@pytest.mark.parametrize("mn", [0, 2, 3])
def test_detect_batch3(make, frames, mn):
    xml, factory = make
    p = factory()  # 5 frames: passes of 2, 2 and 1
    got = p.detect_batch3(frames, 1.1, mn)
    _same(got, [p.detectMultiScale3(f, 1.1, mn) for f in frames])  # same order
    _same(got, sc.oracle_scores(xml, mn))  # the oracle's candidates in (scale, gy, gx) order, grouped by the oracle
    _same([sc.sorted_scores(*g) for g in got], [sc.sorted_scores(*w) for w in sc.oracle_detect_levels(xml, mn)])
    _same([g[0] for g in got], p.detect_batch(frames, 1.1, mn))
    if mn == 2:
        assert max(len(g[0]) for g in got) >= 2 and len(got[1][0]) == 0


@pytest.mark.parametrize("mn", [0, 2, 3])
def test_to_device_with_scores(make, frames, mn):
    import torch
    xml, factory = make
    p = factory()
    want = p.detect_batch3(frames, 1.1, mn)
    plain = _to_device(p, frames, mn, scored=False, host=frames)  # before the detector's first scored call
    _same(plain, [w[0] for w in want])
    _same(_to_device(p, frames, mn, host=frames), want)
    t = torch.from_numpy(frames).cuda()
    _same(_to_device(p, frames, mn, device_ptr=t.data_ptr(), shape=t.shape), want)
    _same(_to_device(p, frames, mn, scored=False, host=frames), plain)  # and after it
    _same(_to_device(p, frames[:1], mn, host=frames[:1]), want[:1])  # one frame alone
    _same(p.detect_batch3(frames, 1.1, mn), want)


def test_colour_frames(make, frames):
    xml, factory = make
    bgr = np.stack([frames, np.roll(frames, 3, 2), 255 - frames], -1)
    p = factory()
    want = p.detect_batch3(bgr, 1.1, 2)
    _same(want, [p.detectMultiScale3(f, 1.1, 2) for f in bgr])
    _same(_to_device(p, bgr, 2, host=bgr), want)
    _same([w[0] for w in want], _to_device(p, bgr, 2, scored=False, host=bgr))


def test_regrow_carries_the_scores(make, frames, monkeypatch):
    """Frames in sc.ORDER under lists of 16 candidates. max_batch 1: pass 0 (flat) fits, pass 1 overflows, the pass launched
    behind it is dead on the device and redone. max_batch 2: the first pass overflows and the second is dead behind it. None of
    them may leave a rectangle, level or weight behind, and the redone passes must."""
    xml, factory = make
    perm = np.ascontiguousarray(frames[sc.ORDER])
    ref = factory()
    want, want_plain = ref.detect_batch3(perm, 1.1, 2), ref.detect_batch(perm, 1.1, 2)
    _same(want, [sc.oracle_scores(xml, 2)[i] for i in sc.ORDER])
    monkeypatch.setenv("CCAMD_CAND_CAP", "16")
    for mb in (1, 2):
        q = factory(mb)
        assert q.candidate_capacity() == 16
        _same(_to_device(q, perm, 2, host=perm), want)
        grown = q.candidate_capacity()
        assert grown > 16
        _same(_to_device(q, perm, 2, host=perm), want)
        assert q.candidate_capacity() == grown  # grown once, then it stays
        _same(q.detect_batch(perm, 1.1, 2), want_plain)
        _same(q.detect_batch3(perm, 1.1, 2), want)


def test_cap_too_small(make, frames):
    import torch
    xml, factory = make
    p = factory()
    want = p.detect_batch3(frames, 1.1, 0)
    n = sum(len(w[0]) for w in want)
    assert n > 16
    cap = n - 1
    d_out = torch.full((cap + 1, 4), -7, dtype=torch.int32, device="cuda")
    d_lv = torch.full((cap + 1,), -7, dtype=torch.int32, device="cuda")
    d_wt = torch.full((cap + 1,), -7.0, dtype=torch.float64, device="cuda")
    d_off = torch.zeros(len(frames) + 1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(cc.CascadeError) as err:
        p.detect_batch_to_device(frames, 1.1, 0, out_ptr=d_out.data_ptr(), cap=cap, offsets_ptr=d_off.data_ptr(),
                                 levels_ptr=d_lv.data_ptr(), weights_ptr=d_wt.data_ptr())
    assert err.value.status == L.CC_ERR_BUFFER_TOO_SMALL and err.value.needed == n
    assert d_off.cpu().numpy().tolist() == np.concatenate([[0], np.cumsum([len(w[0]) for w in want])]).tolist()
    for got, k in ((d_out, 0), (d_lv, 1), (d_wt, 2)):
        got = got.cpu().numpy()
        assert (got[:cap] == np.concatenate([w[k] for w in want])[:cap]).all() and (got[cap] == -7).all()
    _same(_to_device(p, frames, 0, host=frames), want)  # the failed call left no pass pending
    with pytest.raises(cc.CascadeError) as err:  # both score buffers are required
        p.detect_batch_to_device(frames, 1.1, 0, out_ptr=d_out.data_ptr(), cap=cap, offsets_ptr=d_off.data_ptr(),
                                 levels_ptr=0, weights_ptr=d_wt.data_ptr())
    assert err.value.status == L.CC_ERR_INVALID_ARG


@pytest.mark.parametrize("mn", [0, 2])
def test_many_candidates_on_both_sides_of_the_lds_limit(mn, monkeypatch):
    """The cascade of score_cases that passes almost every window with one of several weights, on a textured 160x120 frame
    (many more candidates than T: the global workspace) and one with two small patches (fewer: LDS), in one pass. minNeighbors
    0: every candidate's own sum in the oracle's (scale, gy, gx) order; 2: grouped by the oracle."""
    monkeypatch.setenv("CCAMD_PIPELINE_PASSES", "1")
    path = sc.score_cascade()
    frames = np.asarray(sc.score_frames())
    want = sc.oracle_scores(path, mn, "many")
    if mn == 0:
        assert len(want[0][0]) > sc.T + 400 and 16 < len(want[1][0]) < sc.T
        assert len(np.unique(np.concatenate([w[2] for w in want]))) >= 3
    p = cc.CascadeClassifier(path, max_batch=2)
    _same(_to_device(p, frames, mn, cap=32768, host=frames), want)
    _same(p.detect_batch3(frames, 1.1, mn), want)
    _same(_to_device(p, frames, mn, cap=32768, scored=False, host=frames), [w[0] for w in want])


def test_hog_is_refused(tmp_path):
    import torch
    from tests import hog_cascade_factory as hf
    text, _, _ = hf.hog_cascade(np.stack([frame_natural(24, 24, k) for k in range(50)]), seed=2, stage_sizes=(2,))
    path = str(tmp_path / "hog.xml")
    open(path, "w").write(text)
    c = cc.CascadeClassifier(path)
    img = frame_natural(64, 48, 1)
    d = torch.zeros((64, 4), dtype=torch.int32, device="cuda")
    w = torch.zeros(64, dtype=torch.float64, device="cuda")
    for call in (lambda: c.detect_batch3(img[None]),
                 lambda: c.detect_batch_to_device(img[None], out_ptr=d.data_ptr(), cap=64, offsets_ptr=d.data_ptr(),
                                                  levels_ptr=d.data_ptr(), weights_ptr=w.data_ptr())):
        with pytest.raises(cc.CascadeError) as err:
            call()
        assert err.value.status == L.CC_ERR_UNSUPPORTED and "HOG" in str(err.value)
