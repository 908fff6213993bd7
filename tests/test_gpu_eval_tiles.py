"""The training evaluator (cc_eval_*.hip) at every tile size cc_eval_create can pick and at its window limits, against the
oracle with tolerance 0 on uint32 views. The cases, their expected tile and the inputs come from tests/eval_tiles.py;
tests/test_eval_tiles_host.py checks the table and shows the oracle exact at these shapes. cc_debug_eval_tile_samples
proves that a case ran on the kernel configuration it names."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from oracle import oracle as orc
from tests import eval_tiles as et

pytestmark = pytest.mark.gpu

PAIRS = [(c, n) for c in et.EVAL_CASES for n in c.sample_counts()]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _make(ftype, mode, n, win):
    e = cc.CvFeatureEvaluator.create(ftype)
    e.init(cc.CvFeatureParams(ftype, mode), n, win)
    return e


def _tile(e):
    return L.lib().cc_debug_eval_tile_samples(e._e)


# ---- per case: one oracle reference (shared, never written to) and one live evaluator -------------------------------
class Reference:
    """The oracle's integrals and values of every range of a case for the largest sample count and a few images more: the
    last one (a noise image, index `extra`) is what the scalar test puts into a slot with setImage."""

    def __init__(self, case):
        W, H = case.W, case.H
        self.n_max = max(case.sample_counts())
        self.extra = (self.n_max + 3) // 4 * 4  # et.images: every fourth image is noise
        self.imgs = et.images(W, H, self.extra + 1)
        haar = case.ftype == et.HAAR
        self.s, self.t, self.nf = orc.set_images(self.imgs, want_tilted=case.tilted, want_norm=haar)
        self.cat = orc.haar_catalog(W, H, case.mode) if haar else orc.lbp_catalog(W, H)
        assert len(self.cat) == case.nfeat
        self.vals = {}
        for a, b in case.ranges():
            v = (orc.haar_eval_batch(self.cat, a, b, self.s, self.t, self.nf, W, H) if haar
                 else orc.lbp_eval_batch(self.cat, a, b, self.s, W, H))
            v.setflags(write=False)
            self.vals[(a, b)] = v
        for arr in (self.s, self.t, self.nf):
            if arr is not None:
                arr.setflags(write=False)


@functools.lru_cache(maxsize=1)
def _reference(case):
    return Reference(case)


_live = {"case": None, "e": None, "n": None}


def _evaluator(case):
    """One evaluator alive at a time (159x127 LBP keeps 715 MB of feature records on the device)."""
    if _live["case"] != case.id:
        if _live["e"] is not None:
            _live["e"]._release()
        _live.update(case=None, e=None, n=None)
        _live.update(case=case.id, e=_make(case.ftype, case.mode, max(case.sample_counts()), (case.W, case.H)), n=None)
    return _live["e"]


def _store(case, n):
    e, ref = _evaluator(case), _reference(case)
    if _live["n"] != n:
        e.setImages(ref.imgs[:n], np.arange(n) % 2)
        _live["n"] = n
    return e, ref


@pytest.fixture(scope="module", params=PAIRS, ids=lambda p: "%s-n%d" % (p[0].id, p[1]))
def rig(request):
    """(case, n stored samples, evaluator, reference); module scope makes pytest run the tests of one pair together."""
    case, n = request.param
    e, ref = _store(case, n)
    return case, n, e, ref


@pytest.fixture(scope="module", autouse=True)
def _release_at_the_end():
    yield
    if _live["e"] is not None:
        _live["e"]._release()
    _live.update(case=None, e=None, n=None)
    _reference.cache_clear()


def _gather(n, length):
    """Reverse order with repeats, `length` indices into the n stored samples."""
    base = np.concatenate([np.arange(n)[::-1], [0, n - 1, n // 2, n // 2]])
    return np.resize(base, length).astype(np.int32)


# ---- every case, every sample count ---------------------------------------------------------------------------------------
def test_tile_and_integrals(rig):
    case, n, e, ref = rig
    assert _tile(e) == case.S == et.tile_samples(case.W, case.H, case.tilted)
    assert e.getNumFeatures() == case.nfeat
    for i in sorted({0, n // 2, n - 1}):
        s, t, nf = e.get_sample(i)
        assert (s == ref.s[i]).all()
        if case.tilted:
            assert (t == ref.t[i]).all()
        if case.ftype == et.HAAR:
            assert np.float32(nf).view(np.uint32) == ref.nf[i].view(np.uint32)
    if case.ftype == et.HAAR and n > 1:
        assert ref.nf[1] == 0  # the flat sample


def test_bulk_values(rig):
    case, n, e, ref = rig
    for a, b in case.ranges():
        got, want = e.calc_batch(a, b, n_samples=n), ref.vals[(a, b)][:, :n]
        assert got.shape == want.shape
        bad = _bits(got) != _bits(want)
        assert not bad.any(), "features [%d, %d): %d of %d values differ" % (a, b, bad.sum(), bad.size)
    if case.ftype == et.HAAR and n > 1:
        a, b = case.ranges()[0]
        v = ref.vals[(a, b)][:, :n]
        assert not v[:, 1].any() and v[:, 0].any()  # the flat sample's values are 0, the others' are not


def test_bulk_values_through_a_gather(rig):
    """sample_idx in reverse order with repeats, longer than max_samples."""
    case, n, e, ref = rig
    idx = _gather(n, e.maxSampleCount + 5)
    assert len(idx) > e.maxSampleCount and idx.max() == n - 1
    for a, b in case.ranges():
        got, want = e.calc_batch(a, b, sample_idx=idx), ref.vals[(a, b)][:, idx]
        bad = _bits(got) != _bits(want)
        assert not bad.any(), "features [%d, %d): %d of %d values differ" % (a, b, bad.sum(), bad.size)


def test_bulk_values_into_pitched_device_memory(rig):
    import torch
    case, n, e, ref = rig
    pitch = n + 37
    for a, b in case.ranges():
        out = torch.full((b - a, pitch), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # the fill runs on torch's stream, the evaluator on its own: unordered, the fill can land last
        e.calc_batch_device(a, b, out.data_ptr(), n_samples=n, pitch=pitch)
        got = out.cpu().numpy()
        bad = _bits(got[:, :n]) != _bits(ref.vals[(a, b)][:, :n])
        assert not bad.any(), "features [%d, %d): %d of %d values differ" % (a, b, bad.sum(), bad.size)
        assert (got[:, n:] == -7.0).all()


def test_feature_list_and_scalar_call(rig):
    """calc_list and e(fi, si) on a stored sample (k_eval_list on the device) and on the window set last by setImage (the
    host mirror) give the bulk values. Runs last for its pair: it replaces a stored sample, and puts it back."""
    case, n, e, ref = rig
    rng = np.random.default_rng(n)
    (a, b), (a2, b2) = case.ranges()[0], case.ranges()[2]
    lst = np.concatenate([rng.integers(a, b, 500), rng.integers(a2, b2, 500), [a, b2 - 1, a + 7, a + 7]]).astype(np.int32)

    def want(col):
        return np.where(lst < b, ref.vals[(a, b)][np.minimum(lst, b - 1) - a, col], ref.vals[(a2, b2)][np.maximum(lst, a2) - a2, col])

    assert a2 >= b  # head and tail do not overlap
    for si in sorted({0, n - 1}):
        assert (_bits(e.calc_list(lst, si)) == _bits(want(si))).all()
        for fi in (a, b2 - 1):
            assert np.float32(e(int(fi), si)).view(np.uint32) == _bits(want(si))[list(lst).index(fi)]
    slot, extra = n - 1, ref.extra  # an image that is not among the stored ones goes into the last slot
    assert extra >= n and len(np.unique(ref.imgs[extra])) > 50
    try:
        e.setImage(ref.imgs[extra], 1, slot)
        assert (_bits(e.calc_list(lst, slot)) == _bits(want(extra))).all()  # host mirror
        for fi in (a, b2 - 1):
            assert np.float32(e(int(fi), slot)).view(np.uint32) == _bits(want(extra))[list(lst).index(fi)]
        got = e.calc_batch(a, a + 50, n_samples=n)  # flushes the queued image: the device has it too
        assert (_bits(got[:, slot]) == _bits(ref.vals[(a, b)][:50, extra])).all()
        assert (e.get_sample(slot)[0] == ref.s[extra]).all()
    finally:
        e.setImages(ref.imgs[slot:slot + 1], first_idx=slot)
    assert (e.get_sample(slot)[0] == ref.s[slot]).all()


# ---- k_set_images alone -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", et.SET_IMAGE_WINDOWS, ids=lambda w: "%dx%d" % w)
@pytest.mark.parametrize("ftype", [et.HAAR, et.LBP], ids=["ALL", "LBP"])
def test_set_images_at_windows_around_the_block_size(win, ftype):
    """64 threads walk the rows (y += 64), the columns (x += 64) and the tilted entries: windows with fewer and with more
    than 64 of each, every sample compared."""
    W, H = win
    haar = ftype == et.HAAR
    imgs = et.images(W, H, 6)
    e = _make(ftype, et.ALL if haar else 0, 6, win)
    assert _tile(e) == et.tile_samples(W, H, haar)
    e.setImages(imgs)
    s, t, nf = orc.set_images(imgs, want_tilted=haar, want_norm=haar)
    for i in range(6):
        gs, gt, gnf = e.get_sample(i)
        assert (gs == s[i]).all()
        if haar:
            assert (gt == t[i]).all()
            assert np.float32(gnf).view(np.uint32) == nf[i].view(np.uint32)
    if haar and win == (3, 3):  # the norm rectangle is one pixel: norm factor 0, every value +0.0
        assert (nf == 0).all() and e.getNumFeatures() == 43
        assert not _bits(e.calc_batch(0, 43)).any()
    e._release()


# ---- the wide kernel without the XCD layout ------------------------------------------------------------------------------
_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import cascadeclassifier_amd as cc
from tests import eval_tiles as et
case = next(c for c in et.CASES if c.id == sys.argv[2])
n = int(sys.argv[3])
e = cc.CvFeatureEvaluator.create(case.ftype)
e.init(cc.CvFeatureParams(case.ftype, case.mode), n, (case.W, case.H))
e.setImages(et.images(case.W, case.H, n))
np.savez(sys.argv[4], **{"%d_%d" % r: e.calc_batch(r[0], r[1]) for r in case.ranges()})
"""


def test_wide_kernel_without_xcd_tiles_in_a_child_process(repo_root, tmp_path):
    """CCAMD_EVAL_NO_XCD_TILES is read at launch: a fresh process keeps the two layouts apart. Same bits either way."""
    case = next(c for c in et.EVAL_CASES if c.id == "31x19-BASIC")
    n = 64 * 17 + 5
    out = os.path.join(str(tmp_path), "plain.npz")
    assert "CCAMD_EVAL_NO_XCD_TILES" not in os.environ
    r = subprocess.run([sys.executable, "-c", _CHILD, repo_root, case.id, str(n), out],
                       env=dict(os.environ, CCAMD_EVAL_NO_XCD_TILES="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    plain = np.load(out)
    e, ref = _store(case, n)
    for a, b in case.ranges():
        got = plain["%d_%d" % (a, b)]
        assert (_bits(got) == _bits(ref.vals[(a, b)][:, :n])).all()
        assert (_bits(got) == _bits(e.calc_batch(a, b, n_samples=n))).all()


# ---- window limits ----------------------------------------------------------------------------------------------------------
def test_set_images_kernel_past_64_kb_of_lds():
    """128x128 LBP: k_set_images keeps 128 * 129 * 4 = 66 048 bytes of row sums in LDS. Batched setImages and a queued
    setImage (flush_pending_images) both launch it."""
    case = next(c for c in et.EVAL_CASES if c.id == "128x128-LBP")
    e, ref = _evaluator(case), _reference(case)
    _live["n"] = None
    assert _tile(e) == 1
    e.setImages(ref.imgs[:2])
    e.setImage(ref.imgs[2], 1, 1)  # queued; the next call that reads stored samples sends it to the device
    assert (e.get_sample(1)[0] == ref.s[2]).all() and (e.get_sample(0)[0] == ref.s[0]).all()
    for a, b in (case.ranges()[0], case.ranges()[2]):
        got = e.calc_batch(a, b, n_samples=2)
        assert (_bits(got) == _bits(ref.vals[(a, b)][:, [0, 2]])).all()


@pytest.mark.parametrize("case", et.REFUSED, ids=et.case_id)
def test_window_too_large_for_one_sample_is_refused(case):
    with pytest.raises(cc.CascadeError) as err:
        _make(case.ftype, case.mode, 1, (case.W, case.H))
    assert err.value.status == L.CC_ERR_UNSUPPORTED


def test_longest_window_side():
    """256x3 has 1028 entries: accepted, 16 samples per tile. One pixel more a side, or fewer than 3, is an invalid argument."""
    assert et.tile_samples(256, 3, False) == 16
    imgs = et.images(256, 3, 17)
    e = _make(et.LBP, 0, 17, (256, 3))
    assert _tile(e) == 16 and e.getNumFeatures() == et.lbp_count(256, 3) == 10880
    e.setImages(imgs)
    s, _, _ = orc.set_images(imgs, want_norm=False)
    assert (e.calc_batch(0, 10880) == orc.lbp_eval_batch(orc.lbp_catalog(256, 3), 0, 10880, s, 256, 3)).all()
    e._release()
    for win in ((257, 3), (2, 24), (3, 257), (24, 2)):
        for ftype in (et.HAAR, et.LBP):
            with pytest.raises(cc.CascadeError) as err:
                _make(ftype, 0, 1, win)
            assert err.value.status == L.CC_ERR_INVALID_ARG
