"""CPU checks of tests/eval_tiles.py: the case table against the restated tile rule, and the oracle against the plain
definitions at every shape the GPU tests of the training evaluator use (tests/test_gpu_eval_tiles.py judges the kernels
by the oracle, so the oracle alone must be exact there first)."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import eval_tiles as et


# ---- the table ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", et.CASES, ids=et.case_id)
def test_rule_gives_each_case_its_tile(case):
    assert et.tile_samples(case.W, case.H, case.tilted) == case.S
    if case.exact:
        assert case.exact == (et.WIDE_BUDGET if case.wide else et.NARROW_BUDGET)
        assert case.S * et.bytes_per_sample(case.W, case.H, case.tilted) == case.exact


def test_table_covers_every_tile_size_and_the_refusal():
    assert {c.S for c in et.CASES} == {64, 32, 16, 8, 4, 2, 1, None}
    have = {(c.id, c.S) for c in et.CASES}
    want = {("31x19-BASIC", 64), ("31x19-LBP", 64), ("19x31-LBP", 64), ("25x24-BASIC", 16), ("39x31-BASIC", 16),
            ("15x19-ALL", 32), ("16x16-ALL", 32), ("31x19-ALL", 16), ("39x31-ALL", 8), ("47x39-ALL", 4), ("79x63-LBP", 4),
            ("127x79-LBP", 2), ("101x101-LBP", 1), ("128x128-LBP", 1), ("159x127-LBP", 1), ("160x127-LBP", None)}
    assert want <= have
    exact = {c.id for c in et.CASES if c.exact}
    assert exact >= {"31x19-BASIC", "31x19-LBP", "19x31-LBP", "39x31-BASIC", "15x19-ALL", "31x19-ALL", "39x31-ALL",
                     "79x63-LBP", "127x79-LBP", "159x127-LBP"}
    assert et.SET_IMAGE_WINDOWS == [(3, 3), (3, 70), (70, 3), (65, 66)]


def test_window_edges_named_in_the_table():
    assert et.entries(31, 19) == 640 and et.entries(25, 24) == 650 and et.entries(39, 31) == 1280
    assert et.entries(15, 19) == 320 and et.entries(47, 39) == 1920 and et.entries(79, 63) == 5120
    assert et.entries(127, 79) == 10240 and et.entries(101, 101) == 10404 and et.entries(128, 128) == 16641
    assert et.entries(160, 127) == 20608 and et.entries(159, 127) == 20480
    assert et.tile_samples(100, 100, False) == 2 and et.tile_samples(101, 101, False) == 1  # first square window with S = 1
    assert et.tile_samples(159, 127, False) == 1 and et.tile_samples(160, 127, False) is None
    assert et.tile_samples(256, 3, False) == 16 and et.entries(256, 3) == 1028
    assert 128 * 129 * 4 == 66048 > 64 * 1024  # k_set_images' row prefix sums at 128x128


def test_no_window_without_a_tilted_tile_gets_32_samples():
    """64 samples fit in 160 KB exactly when 32 fit in 80 KB: without a tilted tile the wide kernel takes every window
    that S = 32 could have."""
    sides = range(3, et.MAX_SIDE + 1)
    got = {et.tile_samples(W, H, False) for W in sides for H in sides}
    assert got == {64, 16, 8, 4, 2, 1, None}
    assert 32 in {et.tile_samples(W, H, True) for W in sides for H in sides}


def test_ranges_and_sample_counts_of_a_case():
    for c in et.EVAL_CASES:
        r = c.ranges()
        assert len(r) == 6 and r[0][0] == 0 and r[2][1] == c.nfeat
        assert sorted(b - a for a, b in r)[:2] == sorted([1, max(1, 1024 // c.S - 3)])
        assert 2049 in [b - a for a, b in r]
        ns = c.sample_counts()
        assert 1 in ns and c.S + 1 in ns and (c.S == 1 or c.S - 1 in ns)
        if c.wide:
            assert 64 * 8 + 1 in ns and 64 * 17 + 5 in ns
    c = next(c for c in et.CASES if c.id == "47x39-ALL")
    assert [b - a for a, b in c.ranges()[:3]] == [20000] * 3


def test_images_keep_their_prefix_and_hold_every_kind():
    a, b = et.images(31, 19, 5), et.images(31, 19, 70)
    assert (a == b[:5]).all()
    assert (b[1] == b[1, 0, 0]).all() and len(np.unique(b[2])) == 2 and len(np.unique(b[0])) > 100


# ---- catalogue counts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", et.CASES, ids=et.case_id)
def test_catalogue_counts(case):
    if case.ftype == et.HAAR:
        assert orc.haar_catalog_size(case.W, case.H, case.mode) == case.nfeat
    else:
        assert et.lbp_count(case.W, case.H) == case.nfeat
        if case.S is not None:
            assert len(_catalog(case.ftype, case.mode, case.W, case.H)) == case.nfeat
    assert {c.id: c.nfeat for c in et.CASES}["127x79-LBP"] == 2739009
    assert {c.id: c.nfeat for c in et.CASES}["101x101-LBP"] == 2832489
    assert {c.id: c.nfeat for c in et.CASES}["128x128-LBP"] == 7338681
    assert {c.id: c.nfeat for c in et.CASES}["159x127-LBP"] == 11166729


# ---- the oracle against the definitions -------------------------------------------------------------------------------
def _catalog(ftype, mode, W, H):
    return orc.haar_catalog(W, H, mode) if ftype == et.HAAR else orc.lbp_catalog(W, H)


def _check_oracle(ftype, mode, W, H, n_feats):
    """A few samples (noise, flat, step edge, gradient) and n_feats features spread over the catalogue."""
    tilted = ftype == et.HAAR and mode == et.ALL
    imgs = np.array(et.images(W, H, 4))
    s, t, nf = orc.set_images(imgs, want_tilted=tilted, want_norm=(ftype == et.HAAR))
    S = [et.sum_def(im) for im in imgs]
    T = [et.tilted_def(im) for im in imgs] if tilted else [None] * len(imgs)
    for i, im in enumerate(imgs):
        assert (s[i].astype(np.int64) == S[i].ravel()).all()
        if tilted:
            assert (t[i].astype(np.int64) == T[i].ravel()).all()
        if ftype == et.HAAR:
            assert nf[i].view(np.uint32) == et.norm_factor_def(im).view(np.uint32)
    if ftype == et.HAAR:
        assert nf[1] == 0 and (nf[0] > 0 or (W, H) == (3, 3))  # the flat sample; at 3x3 the norm rectangle is one pixel
    cat = _catalog(ftype, mode, W, H)
    F = len(cat)
    picks = np.unique(np.concatenate([np.linspace(0, F - 1, min(F, n_feats)).astype(np.int64), [0, F - 1]]))
    for fi in picks:
        fi = int(fi)
        if ftype == et.HAAR:
            got = orc.haar_eval_batch(cat, fi, fi + 1, s, t, nf, W, H)[0]
            f = (int(cat["tilted"][fi]), cat["r"][fi], cat["wt"][fi])
            want = np.array([et.haar_value_def(f, S[i], T[i], nf[i]) for i in range(len(imgs))], np.float32)
        else:
            got = orc.lbp_eval_batch(cat, fi, fi + 1, s, W, H)[0]
            want = np.array([et.lbp_code_def(cat[fi], S[i]) for i in range(len(imgs))], np.float32)
        assert (got.view(np.uint32) == want.view(np.uint32)).all(), (fi, got, want)
    return cat, picks


@pytest.mark.parametrize("case", et.EVAL_CASES, ids=et.case_id)
def test_oracle_equals_the_definitions_at_each_case(case):
    cat, picks = _check_oracle(case.ftype, case.mode, case.W, case.H, 300)
    if case.tilted:  # both kinds of feature were among the picks, and are in the middle and tail ranges the GPU tests evaluate
        assert 0 < cat["tilted"][picks].sum() < len(picks)
        for a, b in case.ranges()[1:3]:
            assert 0 < cat["tilted"][a:b].sum() < b - a
        a, b = case.ranges()[4]
        assert cat["tilted"][a:b].any()


@pytest.mark.parametrize("win", et.SET_IMAGE_WINDOWS, ids=lambda w: "%dx%d" % w)
@pytest.mark.parametrize("ftype", [et.HAAR, et.LBP], ids=["ALL", "LBP"])
def test_oracle_equals_the_definitions_at_the_set_image_windows(win, ftype):
    W, H = win
    cat, _ = _check_oracle(ftype, et.ALL if ftype == et.HAAR else 0, W, H, 200)
    if (W, H) == (3, 3):  # the norm rectangle is one pixel: norm factor 0 for every image, every Haar value 0
        imgs = np.array(et.images(3, 3, 4))
        s, t, nf = orc.set_images(imgs, want_tilted=True)
        assert (nf == 0).all() and all(et.norm_factor_def(im) == 0 for im in imgs)
        if ftype == et.HAAR:
            assert not orc.haar_eval_batch(cat, 0, len(cat), s, t, nf, 3, 3).any()
        else:
            assert len(cat) == 1
