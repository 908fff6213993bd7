"""CPU side of tests/front_cases.py: the oracle equals every witness on every case (resize, sum and wrapped squared sum,
tilted integral, LBP codes), the fast tilted witness equals its four-loop form, and a census computed from the witness
taps alone shows that every case is what its reason says. The GPU tests (tests/test_gpu_front_edges.py) then compare the
kernels with the witnesses directly."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import front_cases as fc


# ------------------------------------------------------------------------------------------------ oracle == witnesses
@pytest.mark.parametrize("case", fc.resize_cases(), ids=lambda c: c[0])
def test_oracle_resize_equals_witness(case):
    _, sw, sh, dw, dh = case
    for name, img in fc.resize_case_images(sw, sh):
        want = fc.resize_witness(img, dw, dh)
        got = orc.resize_linear_exact(img, dw, dh)
        assert (got == want).all(), f"{name}: {(got != want).sum()} of {want.size} pixels differ"


@pytest.mark.parametrize("w,h", fc.TILTED_LITERAL_SIZES)
def test_fast_tilted_witness_equals_the_four_loops(w, h):
    for name, img in fc.images(w, h, 50 + w):
        assert (fc.tilted_witness(img) == fc.tilted_literal(img)).all(), name


@pytest.mark.parametrize("case", fc.TILTED, ids=lambda c: "%dx%d" % c[:2])
def test_oracle_integrals_equal_witnesses(case):
    w, h, _ = case
    for name, img in fc.tilted_case_images(w, h):
        o = orc.integral(img, sqsum_i32=True, tilted=True)
        assert (o["sum"] == fc.integral_witness(img, False)).all(), name
        assert (o["sqsum_i32"] == fc.integral_witness(img, True)).all(), name
        assert (o["tilted"] == fc.tilted_witness(img)).all(), name


def test_oracle_squared_sum_wraps_like_the_witness():
    img = np.full((200, 400), 255, np.uint8)
    assert 255 * 255 * img.size > 2 ** 32
    assert (orc.integral(img, sqsum_i32=True)["sqsum_i32"] == fc.integral_witness(img, True)).all()


@pytest.mark.parametrize("W,H", fc.LBP_WINDOWS)
def test_oracle_lbp_codes_equal_witness(W, H):
    rects = orc.lbp_catalog(W, H)
    assert (rects == fc.lbp_catalog_witness(W, H)).all()
    assert (W, H) != (24, 24) or len(rects) == 8464
    for name, samples in fc.lbp_samples(W, H):
        s, _, _ = orc.set_images(samples, want_norm=False)
        got = orc.lbp_eval_batch(rects, 0, len(rects), s, W, H)
        want = fc.lbp_witness(samples, rects)
        assert (got == want).all(), f"{name}: {(got != want).sum()} of {want.size} codes differ"
    # the single-feature entry point, on a flattened integral built by the witness
    img = fc.lbp_samples(W, H)[1][1][0]
    flat = fc.integral_witness(img, False).ravel()
    for fi in range(0, len(rects), 97):
        assert orc.lbp_feature_calc(rects[fi], flat, W + 1) == fc.lbp_witness(img[None], rects[fi:fi + 1])[0, 0]


# ------------------------------------------------------------------------------------------------ census: LBP
@pytest.mark.parametrize("W,H", fc.LBP_WINDOWS)
def test_lbp_block_images_tie_and_split(W, H, capsys):
    """On the block images at least a tenth of the neighbour-to-centre comparisons are exact ties (`>=` against `>`
    decides the bit) and each outcome of the others occurs in at least a tenth of them (a kernel that compares the wrong
    way round cannot hide). Measured: ties 27-30 % on the block images (0.15 % on noise), the rest splits 49 / 51 or closer."""
    rects = fc.lbp_catalog_witness(W, H)
    for name, samples in fc.lbp_samples(W, H):
        tie, gt, lt = fc.lbp_comparison_shares(samples, rects)
        with capsys.disabled():
            print(f"\n  LBP {W}x{H} {name}: ties {tie:.4f}, greater {gt:.4f}, less {lt:.4f} of the rest")
        assert gt >= 0.1 and lt >= 0.1, name
        if name != "noise":
            assert tie >= 0.1, name


# ------------------------------------------------------------------------------------------------ census: resize
def test_order_sensitive_cases_change_a_pixel():
    """scale = src / dst instead of 1 / (dst / src) changes at least one pixel of the case's own noise image."""
    sh, dh = fc.RESIZE_H_ROWS
    for s, d, why in fc.RESIZE_H:
        if why != "order-sensitive":
            continue
        c = fc.tap_census(s, d)
        assert c["differs"].any()
        name, img = fc.resize_case_images(s, sh)[0]
        assert name == "noise"
        a, b = fc.resize_witness(img, d, dh), fc.resize_witness(img, d, dh, order="ratio")
        assert (a != b).any(), (s, d)


def test_order_sensitivity_is_rare_and_mostly_invisible(capsys):
    """Where the two orderings differ it is almost always at an integral f: offset i - 1 with weight 256 against offset i
    with weight 0, the same pixel. The census separates those from the taps that move a pixel: among the downscales of
    24 to 199 columns 684 of 15 400 pairs differ in a tap and none in a pixel, which is why the order-sensitive cases
    have 256 destination columns."""
    pairs = differing = visible_taps = 0
    for src in range(24, 200):
        for dst in range(24, src):
            pairs += 1
            o0, w0 = fc.axis_taps(src, dst)
            o1, w1 = fc.axis_taps(src, dst, "ratio")
            diff = (o0 != o1) | (w0 != w1)
            if diff.any():
                differing += 1
                same_pixel = ((o0 == o1 - 1) & (w0 == 256) & (w1 == 0)) | ((o1 == o0 - 1) & (w1 == 256) & (w0 == 0))
                visible_taps += int((diff & ~same_pixel).sum())
    with capsys.disabled():
        print(f"\n  {differing} of {pairs} pairs differ in a tap, {visible_taps} taps could move a pixel")
    assert (pairs, differing, visible_taps) == (15400, 684, 0)


def test_weight_256_cases_contain_one():
    n = 0
    for s, d, why in fc.RESIZE_H:
        if why == "weight 256":
            c = fc.tap_census(s, d)
            assert c["weight256"].any() and int(c["w1"].max()) == 256, (s, d)
            assert not (c["weight256"] & c["border"]).any()
            n += 1
    assert n >= 3


def test_exact_taps_agree_with_the_float_taps_away_from_ties():
    """The float64 taps are the exact rational ones wherever the exact value is not on a rounding tie or an integer: there
    the published order's rounding errors decide, which is what the order-sensitive cases are about."""
    from fractions import Fraction
    for s, d, _ in fc.RESIZE_H:
        c = fc.tap_census(s, d)
        for k in np.nonzero(~(c["tie"] | c["f_integral"] | c["border"]))[0]:
            f = Fraction(s, d) * Fraction(2 * int(k) + 1, 2) - Fraction(1, 2)
            i = f.numerator // f.denominator
            assert c["ofs"][k] == i and c["w1"][k] == round((f - i) * 256), (s, d, k)


def test_load_path_census():
    for s, d, why in fc.RESIZE_H:
        lp = fc.load_path(s, d)
        if why.startswith("narrow"):
            assert s < 16 and not lp.any(), (s, d)
        if why.startswith("mixed"):
            assert fc.mixed_in_one_wavefront(s, d), (s, d)
            assert (fc.load_span(s, d) == 16).any() and (fc.load_span(s, d) == 15).any(), (s, d)  # both sides of the limit
        if why.startswith("all wide"):
            assert lp.all(), (s, d)
        if why.startswith("all byte loads"):
            assert s >= 16 and not lp.any(), (s, d)
    assert sum(why.startswith("mixed") for _, _, why in fc.RESIZE_H) >= 2
    assert fc.load_path(16, 4).all() and fc.load_path(17, 4).all() and fc.load_path(16, 3).all()
    assert fc.load_path(16, 16).all() and fc.load_path(3, 1025).size == 257
    assert fc.load_path(1920, 417).all()


def test_row_census():
    for s, d, _, label in fc.RESIZE_V:
        c = fc.row_census(s, d)
        inner = ~c["first"]
        if label == "reuse":
            assert c["reuse"][inner].all() and not c["clamped"].any(), (s, d)
        elif label == "no reuse":
            assert not c["reuse"].any() and not c["repeat"].any(), (s, d)
        elif label == "clamped bottom":
            assert c["repeat"].any() and c["clamped"][-1] and not c["clamped"][0], (s, d)
            assert (c["repeat"] & ~c["reuse"]).any()  # a repeated upper row that the cached-row test must NOT take for cached
    assert {label for _, _, _, label in fc.RESIZE_V} >= {"reuse", "no reuse", "clamped bottom"}


def test_case_lists_hold_what_the_plan_names():
    """The minimum lists: nothing dropped."""
    h = {(s, d) for s, d, _ in fc.RESIZE_H}
    for pair in [(1, 1), (1, 5), (2, 98), (3, 17), (15, 4), (15, 15), (16, 3), (16, 4), (17, 4), (640, 140), (640, 137), (640, 130),
                 (1000, 200), (333, 70), (11, 9), (13, 5), (18, 10), (391, 256), (393, 256), (415, 256), (417, 256), (16, 64), (17, 40),
                 (24, 97), (64, 65), (100, 257), (3, 1025)] + [(1100, d) for d in (1, 2, 3, 4, 5, 255, 256, 257, 1021, 1024, 1025)]:
        assert pair in h, pair
    v = {(s, d) for s, d, _, _ in fc.RESIZE_V}
    for pair in [(1, 1), (1, 9), (2, 17), (9, 7), (9, 8), (9, 9), (33, 31), (33, 32), (33, 33), (100, 7), (100, 8), (100, 9), (48, 47),
                 (70, 33), (64, 200)]:
        assert pair in v, pair
    assert {c[:4] for c in fc.RESIZE_BOTH} >= {(101, 57, 33, 19), (17, 9, 40, 31), (1920, 1080, 417, 235)}
    t = {(w, h) for w, h, _ in fc.TILTED}
    assert t >= {(w, h) for w in (1, 2, 3, 4, 5, 62, 63, 64, 65) for h in (1, 2, 63, 64, 65)}
    assert t >= {(61, 127), (61, 128), (61, 129), (61, 200), (1000, 37)}
    for n in (255, 256, 257, 511, 512, 513):
        assert any(w + h - 1 == n and h > w for w, h in t) and any(w + h - 1 == n and w > h for w, h in t), n
