"""The host tables of the wave phase's integer stage sums (cc_debug_wave_int_tables: per stage the quantum q_s and the
integer threshold T_s, per stump the leaves in quanta) against the same construction in exact arithmetic (Python integers
and fractions.Fraction, tests/wave_int_cases.py: expected_tables), on the headline cascade, the cascades on either side of
the stage_quantum bound, and cascades whose stage thresholds are a reachable sum, negative, and beyond the reachable range
in both directions. No device.

The threshold property is checked for every n in [T_s - 2, T_s + 2] that a stage sum can be: |n| <= 2^31 - 2 quanta
(stage_quantum). T_s saturates to INT32_MAX / INT32_MIN for a threshold beyond that range, and the two int32 values outside
it are the only ones for which `n >= T_s` would not be `n * q_s >= threshold`."""
from fractions import Fraction

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from tests import cascade_edges as ce
from tests import wave_int_cases as wi

NAMES = ["headline", "b_below", "b_at", "b_above", "chunks", "thresholds"]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("wave_int_host")


@pytest.fixture(scope="module")
def tables(tmp):
    """name -> (oracle cascade, expected tables, the library's tables): built once, never modified."""
    cache = {}

    def get(name):
        if name not in cache:
            o = wi.oracle_cascade(tmp, name)
            p = cc.CascadeClassifier()
            assert p.load_from_string(wi.xml_text(name)), getattr(p, "load_error", "")
            cache[name] = (o, wi.expected_tables(o), p.wave_int_tables())
        return cache[name]
    return get


@pytest.mark.parametrize("name", NAMES)
def test_integer_form_exactly_where_the_proofs_hold(tables, name):
    o, (q, T, _, _), (got_q, _, _, _) = tables(name)
    assert ce.order_independent(o, 1)
    for s in range(o.nstages):
        want = ce.quantum_ok(o, s)
        assert (q[s] is not None) == want
        assert (got_q[s] != 0) == want, f"{name}: stage {s}"
        if want:
            assert Fraction(float(got_q[s])) == q[s], f"{name}: stage {s}"
    assert any(q[s] is not None for s in range(o.nstages))


def test_headline_stages_on_both_sides(tables):
    """Stages 0-10 of the headline cascade have the integer form and stages 11-24 do not: a launch on it runs both."""
    o, _, (got_q, _, _, _) = tables("headline")
    assert o.nstages == 25
    assert [bool(v != 0) for v in got_q] == [s <= 10 for s in range(25)]


@pytest.mark.parametrize("name,without", [("b_below", []), ("b_at", [2, 3]), ("b_above", [2, 3])])
def test_quantum_bound_pair(tables, name, without):
    o, _, (got_q, _, _, _) = tables(name)
    assert [s for s in range(o.nstages) if got_q[s] == 0] == without
    if without:
        assert ce.stage_ratio(o, 2) >= 2 ** 31 - 1
    else:
        assert ce.stage_ratio(o, 2) == 2 ** 31 - 2


@pytest.mark.parametrize("name", NAMES)
def test_integer_threshold_is_the_double_comparison(tables, name):
    o, (q, T, _, _), (got_q, got_T, _, _) = tables(name)
    for s in range(o.nstages):
        if q[s] is None:
            assert got_T[s] == 0
            continue
        assert int(got_T[s]) == T[s], f"{name}: stage {s}"
        thr = ce.exact(ce.effective_threshold(o.stage_threshold[s]))
        ns = [n for n in range(T[s] - 2, T[s] + 3) if abs(n) <= wi.REACH]
        assert ns, f"{name}: stage {s}"
        for n in ns:
            assert (n * q[s] < thr) == (n < T[s]), f"{name}: stage {s}, n = {n}"
            # ... and the kernel's two expressions on these very numbers: (double)n * q is exact, the comparison is in double
            assert (np.float64(n) * np.float64(got_q[s]) < np.float64(ce.effective_threshold(o.stage_threshold[s]))) == (n < int(got_T[s]))


def test_threshold_cases_are_what_they_claim(tables):
    """'thresholds': stage 1 sits on a reachable sum, stage 2 is negative, stages 3 / 4 saturate; 'chunks': the tie stage."""
    o, (q, T, lq, rq), _ = tables("thresholds")
    assert all(v is not None for v in q)
    sl = ce.stage_slices(o)
    thr1 = ce.exact(ce.effective_threshold(o.stage_threshold[1])) / q[1]
    assert thr1.denominator == 1 and T[1] == thr1
    # reachable: a subset-sum over (left or right per stump) hits it -- by dynamic programming over the integer leaves
    reach = {0}
    for k in range(sl[1].start, sl[1].stop):
        reach = {v + int(lq[k]) for v in reach} | {v + int(rq[k]) for v in reach}
    assert int(thr1) in reach
    assert T[2] < 0 and abs(T[2]) < wi.REACH
    assert T[3] == wi.INT32_MIN and T[4] == wi.INT32_MAX
    o, (q, T, _, _), _ = tables("chunks")
    assert [int(v) for v in o.stage_ntrees] == list(wi.CHUNK_SIZES) and all(v is not None for v in q)
    t = ce.exact(ce.effective_threshold(o.stage_threshold[wi.CHUNK_TIE_STAGE])) / q[wi.CHUNK_TIE_STAGE]
    assert t.denominator == 1


@pytest.mark.parametrize("name", NAMES)
def test_integer_leaves_are_exact(tables, name):
    o, (q, _, lq, rq), (got_q, _, got_l, got_r) = tables(name)
    sl = ce.stage_slices(o)
    for s in range(o.nstages):
        for k in range(sl[s].start, sl[s].stop):
            if q[s] is None:
                assert got_l[k] == 0 and got_r[k] == 0
                continue
            assert lq[k].denominator == 1 and rq[k].denominator == 1
            assert int(got_l[k]) == lq[k] and int(got_r[k]) == rq[k]
            assert int(got_l[k]) * Fraction(float(got_q[s])) == ce.exact(o.stump_left[k])
            assert int(got_r[k]) * Fraction(float(got_q[s])) == ce.exact(o.stump_right[k])


def test_switch_and_other_cascades(tables, monkeypatch, repo_root):
    """CCAMD_WAVE_INT=0: no stage has the form. LBP cascades never have one."""
    import os
    p = cc.CascadeClassifier(os.path.join(repo_root, "data", "lbpcascade_frontalface.xml"))
    assert not any(np.any(a != 0) for a in p.wave_int_tables())
    p = cc.CascadeClassifier(wi.HEADLINE)
    assert np.count_nonzero(p.wave_int_tables()[0]) == 11
    monkeypatch.setenv("CCAMD_WAVE_INT", "0")
    assert not any(np.any(a != 0) for a in p.wave_int_tables())
