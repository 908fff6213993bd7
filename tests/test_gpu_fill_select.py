"""The selection kernels of section 6c (cc_fill.hip: count of the flags before every position, first stop, keep list)
through cc_debug_fill_select against the loop of tests/fill_witness.py, at tolerance 0: n_filled, n_consumed, the reason
and every kept position. Lengths sit at the edges of a wavefront's ballot (64) and of a block's tile (T), and one is long
enough for the scan of the block totals to take more than one block's worth of totals per step."""
import ctypes as C

import numpy as np
import pytest

from cascadeclassifier_amd import _lib as L
from tests import fill_witness as fw

pytestmark = pytest.mark.gpu


def _tile():
    return L.lib().cc_debug_fill_scan_tile()


def _select(flags, start, want, g0, c0, ratio):
    flags = np.ascontiguousarray(flags, np.uint8)
    keep = np.full(max(want, 1), -1, np.int64)
    nf, nc, stop = C.c_int(-1), C.c_int64(-1), C.c_int(-1)
    L.check(L.lib().cc_debug_fill_select(0, flags.ctypes.data_as(C.c_void_p) if len(flags) else None, len(flags), start, want, g0, c0,
                                         ratio, C.byref(nf), C.byref(nc), C.byref(stop), keep.ctypes.data_as(C.c_void_p)))
    return nf.value, nc.value, stop.value, keep[:max(nf.value, 0)].tolist()


LENGTHS = ["0", "1", "63", "64", "65", "T-1", "T", "T+1", "3*T+5"]


@pytest.mark.parametrize("length", LENGTHS)
def test_selection_equals_the_loop(length):
    T = _tile()
    n = eval(length, {"T": T})
    reasons = set()
    cases = 0
    for density, flags in fw.flag_arrays(n).items():
        for start, want, g0, c0, ratio, name in fw.select_cases(flags):
            want_out = fw.fill_select(flags, start, want, g0, c0, ratio)
            got = _select(flags, start, want, g0, c0, ratio)
            assert got == want_out, (density, start, want, name, got[:3], want_out[:3])
            reasons.add(want_out[2])
            cases += 1
    assert cases >= 4 * 2 * 7  # densities, wants, ratio cases at the least
    if n >= 63:
        assert reasons == {fw.FILLED, fw.RATIO, fw.EXHAUSTED}


def test_selection_over_more_blocks_than_a_tile_has_positions():
    """T * T + 1 positions: T + 1 block totals and a stop in the last block."""
    T = _tile()
    n = T * T + 1
    if n > 4 * 1024 * 1024:
        pytest.skip("T * T + 1 = %d positions: more than this test is meant to run" % n)
    reasons = set()
    for density, flags in fw.flag_arrays(n).items():
        count = int(flags.sum(dtype=np.int64))
        for start, want, g0, c0, ratio, name in fw.select_cases(flags, starts=[0, n // 2 + 1], ratios=("zero", "tie64", "below64")):
            if want == 0:
                continue
            want_out = fw.fill_select_np(flags, start, want, g0, c0, ratio)
            got = _select(flags, start, want, g0, c0, ratio)
            assert got[:3] == want_out[:3] and got[3] == want_out[3], (density, start, want, name, got[:3], want_out[:3])
            reasons.add(want_out[2])
        assert _select(flags, n, 1, 0, 0, 0.0) == (0, 0, fw.EXHAUSTED, [])
        if count:  # the last flag of the stream is the last one kept
            last = int(np.nonzero(flags)[0][-1])
            out = _select(flags, 0, count, 0, 0, 0.0)
            assert out[:3] == (count, last + 1, fw.FILLED) and out[3][-1] == last
    assert reasons == {fw.FILLED, fw.RATIO, fw.EXHAUSTED}


def test_hand_cases_and_refusals():
    zeros = np.zeros(8, np.uint8)
    assert _select(zeros, 0, 3, 0, 0, 0.25) == (0, 4, fw.RATIO, [])  # (0 + 1) / 4 == 0.25 stops
    assert _select(zeros, 0, 3, 0, 0, float(np.nextafter(0.25, 0))) == (0, 5, fw.RATIO, [])
    assert _select(np.ones(2, np.uint8), 0, 2, 0, 0, 10.0) == (1, 1, fw.RATIO, [0])  # not at consumed == 0
    assert _select(np.ones(1, np.uint8), 0, 1, 0, 0, 10.0) == (1, 1, fw.FILLED, [0])
    assert _select(zeros, 8, 1, 0, 0, 0.0) == (0, 0, fw.EXHAUSTED, [])
    lib = L.lib()
    nf, nc, stop = C.c_int(0), C.c_int64(0), C.c_int(0)
    for n, start, want in ((8, 9, 1), (8, -1, 1), (8, 0, -1), (-1, 0, 1)):
        st = lib.cc_debug_fill_select(0, zeros.ctypes.data_as(C.c_void_p), n, start, want, 0, 0, 0.0, C.byref(nf), C.byref(nc), C.byref(stop), None)
        assert st == L.CC_ERR_INVALID_ARG, (n, start, want)
