"""cc_presort_plan (host arithmetic, no device): how a presort fits a budget of device memory. The sums are restated here
from the header (include/cascadeclassifier_amd.h, section 6): with N samples, F variables, per = 4 + (2 or 4) bytes of a
table entry, P = max(64, floor64(2^28 / N)) variables per pass and 64 ranks of read-ahead padding,
    everything resident:  ceil64(F) * N * per + min(F, P) * N * 16        (PresortCosts of cc_presort.hip)
    split (R, C):         head(R) + chunk(C) + 8 * N
      head(R)  = R == 0 ? 0 : (R * N + 64 * 64) * per
      chunk(C) = C * N * 16 + (C * N + 64 * 64) * per
The plan: everything resident if that fits; all but the last group beside a chunk of 64 if that fits; otherwise the chunk
first, up to min(ceil64(F), P), and a head only beside a chunk of that size."""
import re

import pytest

from cascadeclassifier_amd import _lib as L
from cascadeclassifier_amd import evaluator as ev

PAD = 64 * 64  # SPLIT_TABLE_PAD_RANKS ranks of 64 lanes


def _per(n):
    return 4 + (2 if n <= 65536 else 4)


def _pass_rule(n):
    return max(64, ((1 << 28) // n) // 64 * 64)


def _resident(f, n):
    return (f + 63) // 64 * 64 * n * _per(n) + min(f, _pass_rule(n)) * n * 16


def _head(r, n):
    return 0 if r == 0 else (r * n + PAD) * _per(n)


def _chunk(c, n):
    return c * n * 16 + (c * n + PAD) * _per(n)


def _split(r, c, n):
    return _head(r, n) + _chunk(c, n) + 8 * n


def _want(f, n, budget):
    """The plan the header describes, by search over the multiples of 64 instead of by division."""
    if _resident(f, n) <= budget:
        return f, 0, _resident(f, n)
    r_max = (f - 1) // 64 * 64
    if _split(r_max, 64, n) <= budget:
        return r_max, 64, _split(r_max, 64, n)
    bound = min((f + 63) // 64 * 64, _pass_rule(n))
    c = max(x for x in range(64, bound + 1, 64) if _split(0, x, n) <= budget)
    r = 0
    if c == bound:
        r = max(x for x in range(0, r_max + 1, 64) if _split(x, c, n) <= budget)
    return r, c, _split(r, c, n)


CASES = [(1, 300), (64, 300), (65, 300), (200, 300), (2056, 20000), (192, 65536), (192, 65537), (162336, 20000), (2790554, 20000)]


@pytest.mark.parametrize("f,n", CASES)
@pytest.mark.parametrize("ftype", [ev.HAAR, ev.HOG])
def test_resident_formula_and_one_byte_less(ftype, f, n):
    full = _resident(f, n)
    for budget in (full, full + 1, 10 * full):
        assert ev.presort_plan(ftype, f, n, budget) == (f, 0, full)
    if full - 1 < _split(0, 64, n):
        # up to 64 variables or so the chunk scratch (a chunk table beside the pass scratch, and the winner row) outweighs the
        # resident tables: there is no split plan below them
        assert f <= 64
        with pytest.raises(L.CascadeError) as ei:
            ev.presort_plan(ftype, f, n, full - 1)
        assert ei.value.status == L.CC_ERR_UNSUPPORTED
        return
    r, c, need = ev.presort_plan(ftype, f, n, full - 1)
    assert r % 64 == 0 and 0 <= r < f and c % 64 == 0 and c >= 64 and need <= full - 1
    assert (r, c, need) == _want(f, n, full - 1)


def test_index_width_changes_at_65537_samples():
    """16-bit sample numbers up to 65 536 samples, 32-bit beyond: 6 and 8 bytes per table entry."""
    f = 192
    a, b = _resident(f, 65536), _resident(f, 65537)
    assert a == 192 * 65536 * 6 + 192 * 65536 * 16 and b == 192 * 65537 * 8 + 192 * 65537 * 16
    assert ev.presort_plan(ev.HAAR, f, 65536, a) == (f, 0, a)
    assert ev.presort_plan(ev.HAAR, f, 65537, b) == (f, 0, b)
    # a head of 128 beside a chunk of 64: the table entries are 6 and 8 bytes wide
    for n in (65536, 65537):
        budget = _split(128, 64, n)
        assert budget == (128 * n + PAD) * _per(n) + 64 * n * 16 + (64 * n + PAD) * _per(n) + 8 * n
        assert ev.presort_plan(ev.HAAR, f, n, budget) == (128, 64, budget)
        assert ev.presort_plan(ev.HAAR, f, n, budget - 1) == _want(f, n, budget - 1)
        assert ev.presort_plan(ev.HAAR, f, n, budget - 1)[0] < 128


@pytest.mark.parametrize("f,n", [(1, 300), (64, 300), (65, 300), (200, 300), (200, 65537), (5000, 20000), (70000, 20000)])
def test_plan_is_monotone_and_within_the_budget(f, n):
    least, hi = _split(0, 64, n), _resident(f, n)
    lo = min(least, hi) // 2
    steps = 400
    last = (0, 0)
    seen = set()
    for k in range(steps + 1):
        budget = lo + (hi - lo) * k // steps
        if budget < min(least, hi):
            with pytest.raises(L.CascadeError):
                ev.presort_plan(ev.HAAR, f, n, budget)
            continue
        r, c, need = ev.presort_plan(ev.HAAR, f, n, budget)
        assert need <= budget, (budget, r, c, need)
        assert (r, c, need) == _want(f, n, budget), budget
        if c:  # streaming: the head never shrinks as the budget grows, nor the chunk while there is no head
            assert r >= last[0] and (c >= last[1] or r > 0), (budget, (r, c), last)
            last = (r, c)
        else:
            assert r == f and budget >= hi
        seen.add((r, c))
    assert (f, 0) in seen
    if f >= 200:  # (at 65 variables a head of 64 beside a chunk of 64 already costs more than everything resident)
        assert len(seen) >= 3
        assert any(r > 0 and c > 0 for r, c in seen)  # a head beside a chunk occurs
    if f > 4 * _pass_rule(n):  # the tables of all but the last group outweigh the scratch of a full pass
        assert sum(1 for r, c in seen if r > 0 and c == _pass_rule(n)) > 3  # ... and grows beside a chunk of a full pass


@pytest.mark.parametrize("f,n", [(1, 300), (65, 300), (200, 65537), (162336, 20000)])
def test_too_small_a_budget_names_its_minimum(f, n):
    least = _split(0, 64, n)
    if _resident(f, n) < least:  # F = 1: the resident tables with their one-variable pass are smaller than a chunk of 64
        assert ev.presort_plan(ev.HAAR, f, n, least - 1)[:2] == (f, 0)
        least = _resident(f, n)
    with pytest.raises(L.CascadeError) as ei:
        ev.presort_plan(ev.HAAR, f, n, least - 1)
    assert ei.value.status == L.CC_ERR_UNSUPPORTED
    named = [int(x) for x in re.findall(r"\d+", str(ei.value))]
    assert least in named, str(ei.value)
    assert ev.presort_plan(ev.HAAR, f, n, least) == _want(f, n, least)
    assert ev.presort_plan(ev.HAAR, f, n, least)[2] == least


def test_the_example_window_of_the_reference_fits_with_a_tail():
    """75x32 Haar BASIC, 2 790 554 variables, at 20 000 samples: 335 GB of tables against 288 GB of HBM."""
    f, n = 2790554, 20000
    assert f * n * 6 > 288e9
    r, c, need = ev.presort_plan(ev.HAAR, f, n, 256 * 10**9)
    assert 0 < r < f and r % 64 == 0 and c == _pass_rule(n) and need <= 256 * 10**9
    assert (r, c, need) == _want(f, n, 256 * 10**9)


def test_lbp_is_resident_or_refused():
    f, n = 8464, 20000
    cat_pad = (2 * 6 + 1) * 16  # SPLIT_CAT_PAD_RANKS
    need = f * n + (f + 63) // 64 * 64 * (n + 3 + cat_pad) * 4 + min(f, _pass_rule(n)) * n * 16
    assert ev.presort_plan(ev.LBP, f, n, need) == (f, 0, need)
    with pytest.raises(L.CascadeError) as ei:
        ev.presort_plan(ev.LBP, f, n, need - 1)
    assert ei.value.status == L.CC_ERR_UNSUPPORTED and "categorical variables are not streamed" in str(ei.value)


def test_bad_arguments():
    for args in ((ev.HAAR, 0, 10, 1 << 30), (ev.HAAR, 10, 0, 1 << 30)):
        with pytest.raises(L.CascadeError) as ei:
            ev.presort_plan(*args)
        assert ei.value.status == L.CC_ERR_OUT_OF_RANGE
    with pytest.raises(L.CascadeError) as ei:
        ev.presort_plan(7, 10, 10, 1 << 30)
    assert ei.value.status == L.CC_ERR_INVALID_ARG
