"""The witness of the -info mode (tests/area_witness.py) against exact rational area means, cc_area_tab (host, no device)
against the witness bit for bit, and what each crafted input of tests/info_cases.py is there for, asserted on the witness."""
import math
from fractions import Fraction

import numpy as np
import pytest

from cascadeclassifier_amd import _lib as L
from cascadeclassifier_amd.samples import area_tab  # the witness is tested as the yardstick of this entry point and its kernel
from tests import area_witness as AW
from tests import sample_witness as W
from tests.info_cases import (AXIS_SIZES, BILINEAR_RECTS, EXACT_SHAPES, INFO_CASES, NO_OVERFLOW_SIDES, OVERFLOW_SIDES, RESIZE_CASES,
                              bilinear_with_image_as_source, info_case, info_want, mode_of, random_image, resize_input, resize_want)


def _exact_weights(ssize, dsize, d):
    """The share of every source pixel in destination cell d of an exact area resize: [(index, Fraction)], summing to 1."""
    lo, hi = Fraction(d * ssize, dsize), Fraction((d + 1) * ssize, dsize)
    out = []
    for s in range(math.floor(lo), math.ceil(hi)):
        out.append((s, (min(hi, s + 1) - max(lo, s)) / (hi - lo)))
    assert sum(w for _, w in out) == 1
    return out


@pytest.mark.parametrize("sw,sh,dw,dh", EXACT_SHAPES)
def test_witness_against_exact_area_means(sw, sh, dw, dh):
    """|witness - exact mean| <= 0.5 + 255 (lost_x + lost_y) + slack.
    0.5: the final rounding to an integer. lost: the weight of the partial source pixels the table leaves out (narrower than
    1e-3 of a pixel, at most two per cell and axis, a cell being at least one pixel wide: lost <= 2e-3 per axis, so the term is
    at most 255 * 4e-3); the remaining weights are not renormalised, so a pixel of 255 loses at most 255 * lost. It is taken
    from the witness's own table, and is 0 (up to the rounding of d * scale) where no sliver occurs. slack: every float32
    operation has a relative error of at most 2^-24 on a partial sum of at most 255 (1 + lost); a pixel takes one rounding
    of each weight, one product and one sum per entry, (nx + 3) and (ny + 3) operations deep per axis, doubled for room."""
    img = random_image(sw, sh, 7 * sw + sh)
    got = AW.resize_area(img, dw, dh).astype(np.int64)
    lost_x, lost_y, n_x, n_y = [], [], 1, 1
    if not AW.is_fast(sw, sh, dw, dh) and (sw, sh) != (dw, dh):
        tx = AW.area_tab(sw, dw, dropped=lost_x)
        ty = AW.area_tab(sh, dh, dropped=lost_y)
        n_x = max(sum(1 for e in tx if e[0] == d) for d in range(dw))
        n_y = max(sum(1 for e in ty if e[0] == d) for d in range(dh))
    else:  # the fast path sums a block exactly and rounds once or twice: (float)sum, the product with 1.f / area
        n_x, n_y = 1, 1
    lost = max(lost_x, default=0.0) + max(lost_y, default=0.0)
    assert lost <= 4e-3
    slack = 2 * 255.0 * (n_x + n_y + 6) * 2.0 ** -24
    bound = 0.5 + 255.0 * lost + slack
    assert bound < 0.5 + 255 * 4e-3 + 0.01
    worst = 0.0
    wx = [_exact_weights(sw, dw, d) for d in range(dw)]
    for dy in range(dh):
        rows = _exact_weights(sh, dh, dy)
        for dx in range(dw):
            mean = sum(b * a * int(img[sy, sx]) for sy, b in rows for sx, a in wx[dx])
            worst = max(worst, abs(float(got[dy, dx] - mean)))
    print(f"{sw}x{sh}->{dw}x{dh}: worst {worst:.6f}, bound {bound:.6f}, lost {lost:.3e}")
    assert worst <= bound
    if (sw, dw) != (1001, 1000):  # the one shape with partial pixels at the threshold; elsewhere only the rounding of
        assert lost < 1e-9        # d * scale looks like a sliver, and the bound is 0.5 and the float slack
        assert bound < 0.505


@pytest.mark.parametrize("sw,sh,dw,dh", [(25, 25, 24, 24), (27, 29, 5, 7), (31, 24, 24, 24), (49, 49, 1, 1), (72, 48, 24, 24),
                                         (48, 48, 24, 24), (96, 48, 24, 24), (24, 24, 24, 24), (301, 3, 300, 1)])
def test_vector_form_equals_the_scalar_definition(sw, sh, dw, dh):
    img = random_image(sw, sh, 31 * sw + dh)
    whole = AW.resize_area(img, dw, dh)
    for dy in range(dh):
        for dx in range(0, dw, 1 if dw <= 24 else 37):
            assert whole[dy, dx] == AW.area_pixel(img, dw, dh, dx, dy), (dx, dy)


@pytest.mark.parametrize("ssize,dsize", AXIS_SIZES)
def test_area_tab_equals_witness(ssize, dsize):
    scale, iscale, integer, di, si, al = area_tab(ssize, dsize)
    w_scale, w_iscale, w_integer = AW.axis(ssize, dsize)
    margins = []
    want = AW.area_tab(ssize, dsize, margins=margins)
    assert np.float64(scale).view(np.uint64) == np.float64(w_scale).view(np.uint64)
    assert (iscale, integer) == (w_iscale, w_integer)
    assert len(di) == len(want) <= 2 * ssize
    assert di.tolist() == [e[0] for e in want] and si.tolist() == [e[1] for e in want]
    assert (al.view(np.uint32) == np.array([e[2] for e in want], np.float32).view(np.uint32)).all()
    assert 0 <= si.min() and si.max() <= ssize - 1 and sorted(set(di.tolist())) == list(range(dsize))
    if (ssize, dsize) == (49, 1):  # 1 / (1. / 49) is not 49.0: the general path despite the integer ratio
        assert not integer and iscale in (48, 49) and scale != 49.0
    if (ssize, dsize) in ((72, 24), (48, 24), (24, 24), (1, 1), (8192, 1), (8192, 4096), (600, 75)):
        assert integer and iscale * dsize == ssize
    if (ssize, dsize) in ((25, 24), (47, 24), (280, 32), (1001, 1000)):
        assert not integer
    if (ssize, dsize) == (1001, 1000):  # the comparison with 1e-3 is decided in the last bits here
        assert min(abs(m) for m in margins) < 1e-9
        assert any(0 < -m < 1e-9 for m in margins) or any(0 < m < 1e-9 for m in margins)


def test_area_tab_refusals_and_capacity():
    lib = L.lib()
    n = L.C.c_int32(0)
    for ssize, dsize in ((0, 1), (5, 0), (5, 6), (8193, 1), (-1, -1)):
        assert lib.cc_area_tab(ssize, dsize, None, None, None, None, None, None, 0, L.C.byref(n)) == L.CC_ERR_INVALID_ARG
    assert lib.cc_area_tab(25, 24, None, None, None, None, None, None, 0, None) == L.CC_ERR_INVALID_ARG
    assert lib.cc_area_tab(25, 24, None, None, None, None, None, None, 4, L.C.byref(n)) == L.CC_ERR_INVALID_ARG  # room without arrays
    assert lib.cc_area_tab(25, 24, None, None, None, None, None, None, 0, L.C.byref(n)) == L.CC_ERR_BUFFER_TOO_SMALL
    assert n.value == len(AW.area_tab(25, 24))
    assert len(area_tab(25, 24)[3]) == n.value  # and the next call works


def test_crafted_2x2_sums_round_half_up():
    img = resize_input("2x2_fast")
    sums = img.astype(np.int64).reshape(24, 2, 24, 2).sum(axis=(1, 3))
    assert (sums % 4 == 2).all()
    want = resize_want("2x2_fast")
    assert (want == (sums + 2) >> 2).all()
    half_even = np.rint(sums / 4.0).astype(np.int64)
    assert (want != half_even).any() and (want == half_even).any()  # even k differ, odd k do not


def test_crafted_4x2_sums_round_half_to_even():
    img = resize_input("4x2_fast_ties")
    sums = img.astype(np.int64).reshape(24, 2, 24, 4).sum(axis=(1, 3))
    assert (sums % 8 == 4).all()
    k = sums // 8
    assert (k % 2 == 0).any() and (k % 2 == 1).any()
    want = resize_want("4x2_fast_ties").astype(np.int64)
    assert (want == k + (k % 2)).all()  # to the even neighbour
    half_up = np.floor(sums / 8.0 + 0.5).astype(np.int64)
    assert (want != half_up).any() and (want[k % 2 == 1] == half_up[k % 2 == 1]).all()


def test_bilinear_branch_reads_the_rectangle_alone():
    images, records, (dw, dh) = info_case("bilinear")
    want = info_want("bilinear")
    for k, (i, x, y, w, h) in enumerate(records):
        assert not AW.uses_area(w, h, dw, dh)
        assert (want[k] == W.resize_linear_exact(images[i][y:y + h, x:x + w], dw, dh)).all()
        other = bilinear_with_image_as_source(images[i], (x, y, w, h), dw, dh)
        assert (other != want[k]).any()  # the 255 around the rectangle would show at its edges
        inner = (slice(3, dh - 3), slice(3, dw - 3))
        assert (other[inner] == want[k][inner]).all()  # and only there
    assert [tuple(r[3:]) for r in records] == [(20, 30), (30, 20), (10, 10)] == [r[2:] for r in BILINEAR_RECTS]


def test_cases_reach_every_mode():
    modes = {name: [mode_of(r[1:], info_case(name)[2]) for r in info_case(name)[1]] for name in INFO_CASES}
    assert set(modes["mixed"]) == {"copy", "linear", "fast", "area"} == set(modes["window_5x7"])
    assert set(modes["bilinear"]) == {"linear"} and set(modes["copy"]) == {"copy"}
    assert modes["window_1x1"] == ["area", "fast", "copy"]  # 49 -> 1: the general path; 1 / (1. / 7) and 1 / (1. / 5) are whole
    images, records, _ = info_case("mixed")
    used = [r[0] for r in records]
    assert len({im.shape for im in images}) >= 4 and used.count(0) >= 4 and used[0] == used[-1] == 0
    assert any(a != b for a, b in zip(used, used[1:]))
    images, records, _ = info_case("corners")
    h, w = images[0].shape
    assert {(x, y) for _, x, y, _, _ in records[:4]} == {(0, 0), (w - 30, 0), (0, h - 26), (w - 30, h - 26)}
    assert records[4][1:] == (0, 0, w, h) and records[5][1:] == (0, 0) + images[1].shape[::-1]
    assert {name: mode_of((0, 0) + c[:2], c[2:]) for name, c in RESIZE_CASES.items()} == {
        "2x2_fast": "fast", "3x2_fast": "fast", "4x2_fast_ties": "fast", "49_to_1": "area", "25_to_24": "area", "47_to_24": "area",
        "y_scale_1": "area", "27x29_to_5x7": "area", "7x5_to_1x1": "fast", "1x1": "copy", "row_301": "area", "row_1001": "area",
        "8192_to_1": "fast", "barcode": "area"}


def test_overflow_threshold():
    (w, h), (w2, h2) = OVERFLOW_SIDES, NO_OVERFLOW_SIDES
    assert AW.is_fast(w, h, 1, 1) and w * h * 255 >= 2 ** 31 > w * (h - 1) * 255 and (w2, h2) == (w, h - 1)
    with pytest.raises(ValueError):
        AW.resize_area(np.zeros((h, w), np.uint8), 1, 1)
    assert AW.resize_area(np.full((h2, w2), 255, np.uint8), 1, 1)[0, 0] == 255
