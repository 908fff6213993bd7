"""The LDS classes of HOG windows (tests/hog_lds_cases.py) against the library's own report (cc_debug_hog_lds, host only) and
against the formulas restated in plain Python. The GPU tests pick their windows from that table's lists: if a budget, a formula
or the plan loop changes, a window moves to another class here, on the CPU, and not silently on the device."""
import ctypes as C

import pytest

from cascadeclassifier_amd import _lib as L
from tests import hog_lds_cases as lds


@pytest.mark.parametrize("win", sorted(lds.TABLE), ids=lambda w: "%dx%d" % w)
def test_table_equals_export_and_restatement(win):
    assert lds.exported(*win) == lds.TABLE[win]
    assert lds.restated(*win) == lds.TABLE[win]


def test_export_equals_restatement_on_a_grid():
    """Every window of a coarse grid and every window around the four edges of the two budgets."""
    wins = {(w, h) for w in range(8, 200, 7) for h in range(8, 200, 11)}
    for w0, h0 in lds.TABLE:
        wins |= {(w0 + dw, h0 + dh) for dw in (-1, 0, 1) for dh in (-1, 0, 1)}
    for w, h in sorted(wins):
        assert lds.exported(w, h) == lds.restated(w, h), (w, h)


def test_window_classes():
    """What each list of windows is in the GPU tests for."""
    T = lds.TABLE
    limit, default = lds.MAX_KIB * lds.KIB, lds.DEFAULT_KIB * lds.KIB
    assert (limit, default) == (163840, 65536)
    # the miner: either side of the opt-in, the last accepted and the first refused windows
    assert T[(37, 37)][3] <= default < T[(38, 38)][3]
    assert not lds.miner_opts_in((37, 37)) and lds.miner_opts_in((38, 38))
    for win in lds.MINER_WINDOWS:
        assert lds.miner_accepts(win) and lds.eval_accepts(win), win
    for win in lds.MINER_LARGE:
        assert T[win][3] > 0.97 * limit, win
    for (w, h), (w1, h1) in zip(lds.MINER_LAST_ACCEPTED, [(60, 59), (89, 40), (40, 89)]):
        assert lds.miner_accepts((w, h)) and lds.restated(w1, h1)[3] > limit, (w, h)
    for win in lds.MINER_FIRST_REFUSED:
        assert not lds.miner_accepts(win) and lds.eval_accepts(win), win  # refused for the miner's LDS, nothing else
    assert any(h > w for w, h in lds.MINER_WINDOWS) and any(h > w for w, h in lds.MINER_LARGE)
    # the evaluator: planes per pass at each budget's edges
    assert [T[w][:2] for w in lds.EVAL_WINDOWS] == [(10, 64), (9, 64), (9, 64), (5, 64), (1, 64), (4, 160), (1, 160), (1, 160)]
    assert T[(85, 85)][2] <= default and not lds.eval_opts_in((85, 85))       # ten passes of one plane, no opt-in
    assert lds.restated(86, 85)[1] == 160 and lds.restated(85, 86)[1] == 160  # one more column or row: the 160 KiB branch
    assert lds.eval_opts_in((86, 85))
    for win in lds.EVAL_LAST_ACCEPTED:
        assert lds.eval_accepts(win) and T[win][2] > 0.99 * limit, win
    for win in lds.EVAL_FIRST_REFUSED:
        assert not lds.eval_accepts(win) and T[win][2] > limit, win
    assert any(h > w for w, h in lds.EVAL_WINDOWS)
    # windows of tests that predate the table (tests/test_gpu_training_sizes.py, section 6; tests/test_gpu_hog_cascade.py)
    assert [T[w][0] for w in [(128, 64), (96, 96), (128, 128)]] == [3, 3, 1]
    assert not lds.eval_accepts((160, 160)) and not lds.miner_accepts((128, 96))


def test_export_arguments():
    p = C.c_int(-1)
    assert L.lib().cc_debug_hog_lds(24, 24, C.byref(p), None, None, None) == L.CC_OK and p.value == 10
    assert L.lib().cc_debug_hog_lds(0, 24, C.byref(p), None, None, None) == L.CC_ERR_INVALID_ARG
    assert L.lib().cc_debug_hog_lds(24, 4097, None, None, None, None) == L.CC_ERR_INVALID_ARG
