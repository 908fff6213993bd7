"""CPU checks of the HOG restatement (tests/hog_restatement.py): catalog sizes and order, the reference's own HOG cases
(traincascade/test/test_features.cpp:394-440) and the exactness of the float32 FMA emulation."""
from fractions import Fraction

import numpy as np
import pytest

from tests import hog_restatement as hog


@pytest.mark.parametrize("win,blocks", [((16, 16), 1), ((20, 20), 4), ((24, 24), 9), ((32, 32), 36), ((75, 32), 159),
                                        ((64, 64), 528), ((15, 40), 0), ((8, 8), 0)])
def test_catalog_sizes(win, blocks):
    cat = hog.catalog(*win)
    assert len(cat) == blocks
    assert len(cat) * hog.FEATURE_SIZE == blocks * 36


def test_catalog_order_x_outer():
    cat = hog.catalog(32, 32)
    # t = 8, cells 8x8 (16x16 blocks): x outer, y inner
    assert [tuple(r) for r in cat[:6]] == [(0, 0, 8, 8), (0, 4, 8, 8), (0, 8, 8, 8), (0, 12, 8, 8), (0, 16, 8, 8), (4, 0, 8, 8)]
    # then cells 8x16 (16 wide, 32 tall: y = 0 only), cells 16x8, then t = 16
    assert [tuple(r) for r in cat[25:30]] == [(0, 0, 8, 16), (4, 0, 8, 16), (8, 0, 8, 16), (12, 0, 8, 16), (16, 0, 8, 16)]
    assert [tuple(r) for r in cat[30:35]] == [(0, 0, 16, 8), (0, 4, 16, 8), (0, 8, 16, 8), (0, 12, 16, 8), (0, 16, 16, 8)]
    assert tuple(cat[35]) == (0, 0, 16, 16)
    c = hog.cells(cat[7])
    assert c.tolist() == [[4, 8, 8, 8], [12, 8, 8, 8], [4, 16, 8, 8], [12, 16, 8, 8]]


def test_reference_case_constant_image_is_zero():
    """test_features.cpp: every HOG variable of a constant image is 0."""
    cat = hog.catalog(32, 32)
    hist, norm = hog.set_images(np.full((1, 32, 32), 77, np.uint8))
    assert not hist.any() and not norm.any()
    assert not hog.eval_vars(cat, hist, norm).any()


def test_reference_case_vertical_edge_is_positive():
    """test_features.cpp: some variable is > 0 on a vertical step edge, and it sits in the horizontal-gradient bins."""
    img = np.zeros((32, 32), np.uint8)
    img[:, 16:] = 200
    cat = hog.catalog(32, 32)
    hist, norm = hog.set_images(img[None])
    v = hog.eval_vars(cat, hist, norm)
    assert (v > 0).any()
    # a horizontal gradient (dy = 0, dx > 0) has angle 0: bin floor(-0.5) + 9 = 8
    assert hist[0, 8, -1, -1] == norm[0, -1, -1] > 0


def test_bin_table_edges():
    b, mag = hog.bin_table()
    at = lambda dx, dy: (dy + 255) * 511 + dx + 255  # noqa: E731
    assert b[at(0, 0)] == 8 and mag[at(0, 0)] == 0  # angle 0
    assert b[at(3, 4)] in range(9) and mag[at(3, 4)] == 5
    assert b.max() < 9
    # the signed angle folds onto 9 bins of 20 degrees: opposite gradients share a bin (angle + 180 degrees -> bin + 9)
    assert (b[at(10, 0)] == b[at(-10, 0)]) and (b[at(0, 10)] == b[at(0, -10)])


def _round_f32_exact(q: Fraction) -> np.float32:
    """Round a rational to the nearest float32, ties to even, by comparing the neighbours of a close candidate."""
    c = np.float32(float(q))
    cands = {c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))}
    best = sorted(cands, key=lambda v: (abs(Fraction(float(v)) - q), int(np.array(v).view(np.uint32)) & 1))
    return best[0]


def _fma_triples():
    rng = np.random.default_rng(11)
    n = 3000
    a = rng.standard_normal(n).astype(np.float32) * np.float32(50)
    b = rng.standard_normal(n).astype(np.float32)
    c = (rng.standard_normal(n) * rng.choice([1e-6, 1e-2, 1.0, 1e3], n)).astype(np.float32)
    # the polynomial's own operands
    cc = rng.random(n // 3).astype(np.float32) ** 2
    a = np.concatenate([a, cc, cc, cc])
    b = np.concatenate([b, np.full(n // 3, hog.P7), np.full(n // 3, hog.P5), np.full(n // 3, hog.P3)])
    c = np.concatenate([c, np.full(n // 3, hog.P5), np.full(n // 3, hog.P3), np.full(n // 3, hog.P1)])
    # products that land exactly on a float32 tie, nudged by tiny addends of both signs (and none)
    u = np.float32(1 + 2.0 ** -12)
    tie_a = np.full(9, u)
    tie_b = np.full(9, u)
    tie_c = np.array([0, 2.0 ** -60, -2.0 ** -60, 2.0 ** -40, -2.0 ** -40, 2.0 ** -24, -2.0 ** -24, 2.0 ** -23, -2.0 ** -23], np.float32)
    return np.concatenate([a, tie_a]), np.concatenate([b, tie_b]), np.concatenate([c, tie_c])


def test_fma32_is_exactly_rounded():
    a, b, c = _fma_triples()
    got = hog.fma32(a, b, c)
    bad = 0
    for x, y, z, g in zip(a, b, c, got):
        want = _round_f32_exact(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))
        bad += int(np.array(g).view(np.uint32) != np.array(want).view(np.uint32))
    assert bad == 0


def test_fma32_tie_cases_differ_from_double_rounding():
    """At a tie the naive float64-then-float32 rounding is wrong; the emulation must round by the sign of the addend."""
    u = np.float32(1 + 2.0 ** -12)  # u * u = 1 + 2^-11 + 2^-24: exactly halfway between two float32 values
    lo, hi = np.float32(1 + 2.0 ** -11), np.nextafter(np.float32(1 + 2.0 ** -11), np.float32(2))
    assert hog.fma32(u, u, np.float32(0)) == lo  # tie to even
    assert hog.fma32(u, u, np.float32(2.0 ** -60)) == hi
    assert hog.fma32(u, u, np.float32(-2.0 ** -60)) == lo
