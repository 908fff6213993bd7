"""Cascades and frames for the integer form of the Haar wave phase's stage sums, shared by tests/test_wave_int_host.py (the
host tables against exact arithmetic) and tests/test_gpu_wave_int.py (the kernels against the oracle).

The wave phase (cc_eval_kernel.inc: wave_phase_haar) sums a stage's votes as int32 multiples of the stage's quantum where
the host proves that every subset sum is one (order_independent and quantum_ok of tests/cascade_edges.py), and in double
elsewhere. The cascades here put stages on both sides of that proof inside one launch, stage sizes on the edges of the 64-stump
chunks, and stage thresholds on a reachable sum, below zero and beyond both ends of the reachable range."""
import functools
import os
from fractions import Fraction

import numpy as np

from oracle import oracle as orc
from tests import cascade_edges as ce
from tests.util import frame_natural

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = os.path.join(ROOT, "data", "haarcascade_frontalface_synthetic.xml")
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
REACH = 2 ** 31 - 2  # quantum_ok: sum max(|l|,|r|) / q < 2^31 - 1, so no vote sum exceeds this many quanta in magnitude

CHUNK_SIZES = (8, 12, 63, 64, 65, 128, 129)  # late stages on the edges of one and two chunks of 64 lanes
CHUNK_TIE_STAGE = 3                          # its threshold is the most frequent sum of the windows that reach it


@functools.lru_cache(maxsize=None)
def built(name):
    """name -> tests.cascade_edges.Built. 'chunks': leaves are multiples of 1/8 of one binary exponent, every stage has an
    integer form, the stage of 64 stumps has a threshold that windows hit exactly. 'thresholds': stage 1 a reachable sum, stage 2 negative, stage 3 below
    every reachable sum, stage 4 above every reachable sum (in quanta: beyond int32 in both directions)."""
    if name in ce.B_NAMES:
        return ce.built(name)
    if name == "chunks":
        # Leaves of +-{4, 5, 6, 7} / 8: one binary exponent, so q = 2^-24 and 129 stumps stay below 2^31 - 1 quanta
        # (129 * 7/8 * 2^24 = 0.88 * 2^31); multiples of 1/8 anywhere in [-1, 1] would put q at 2^-26 and lose the form.
        rng = np.random.default_rng(301)
        stages = []
        for s, nt in enumerate(CHUNK_SIZES):
            stumps = []
            for _ in range(nt):
                a, b = 0, 0
                while a == b:
                    a, b = (int(rng.integers(4, 8)) * int(rng.choice([-1, 1])) for _ in range(2))
                stumps.append(ce.cal(a / 8, b / 8))
            stages.append(((("mode",) if s == CHUNK_TIE_STAGE else ("q", 0.5, 0)), stumps))
        return ce.haar_cascade(stages, 311, critical=CHUNK_TIE_STAGE)
    if name == "thresholds":
        rng = np.random.default_rng(302)
        mk = lambda n: [ce.cal(l, r) for l, r in ce._random_leaves(rng, n, 0.125)]
        stages = [ce._cal_stage(rng, 6, 0.5, 0.125), (("mode",), mk(9)), (("eff", -0.375), mk(10)), (("eff", -1e6), mk(12)), (("eff", 1e6), mk(14))]
        return ce.haar_cascade(stages, 312, critical=1)
    raise KeyError(name)


def xml_text(name):
    return open(HEADLINE).read() if name == "headline" else built(name).xml


def oracle_cascade(tmp, name):
    if name == "headline":
        return orc.load_cascade_xml(HEADLINE)
    from tests import haar_windows as hw
    return hw.oracle_cascade(tmp, built(name).xml, "wave_int_" + name + ".xml")


# ------------------------------------------------------------------ the tables in exact arithmetic
def expected_tables(o):
    """Per stage (q, T) with q a Fraction or None (no integer form) and T the saturated integer threshold; per stump the
    leaves in quanta (Fractions; 0 where the stage has no form). From the oracle's own parse of the cascade."""
    ns = o.nstages
    sl = ce.stage_slices(o)
    stumps_only = o.feature_type == 0 and int(np.max(o.tree_nnodes)) == 1
    oi = stumps_only and ce.order_independent(o, 1)
    q, T = [None] * ns, [0] * ns
    lq, rq = [Fraction(0)] * len(o.stump_left), [Fraction(0)] * len(o.stump_left)
    for s in range(ns):
        thr = ce.effective_threshold(o.stage_threshold[s])
        if not oi or not ce.quantum_ok(o, s) or np.isnan(thr):
            continue
        q[s] = ce.stage_magnitude(o, s)[1]
        if np.isinf(thr):
            T[s] = INT32_MAX if thr > 0 else INT32_MIN
        else:
            x = ce.exact(thr) / q[s]
            n = -((-x.numerator) // x.denominator)  # ceil
            T[s] = min(max(n, INT32_MIN), INT32_MAX)
        for k in range(sl[s].start, sl[s].stop):
            lq[k], rq[k] = ce.exact(o.stump_left[k]) / q[s], ce.exact(o.stump_right[k]) / q[s]
    return q, T, lq, rq


# ------------------------------------------------------------------ frames and what the oracle says about them
@functools.lru_cache(maxsize=None)
def frames():
    """Two frames of 384 x 288, natural content with the face template pasted at 24, 38 and 65 pixels."""
    tm = np.load(os.path.join(ROOT, "data", "face_template_24x24.npy"))
    out = []
    for seed, spots in ((41, ((30, 40, 24), (200, 60, 38), (110, 170, 65))), (42, ((300, 20, 24), (60, 200, 38), (220, 150, 65)))):
        img = frame_natural(384, 288, seed)
        for x, y, s in spots:
            img[y:y + s, x:x + s] = orc.resize_linear_exact(tm, s, s)
        out.append(img)
    return out


SCALE_FACTOR = 1.1
SUPER_ROWS = 24  # whole tiles of 8 and of 12 window rows (the table-driven kernel; the specialised STEP-2 / STEP-1 modules)


def wave_phase_windows(o, img, codes, wave_below, form):
    """From the oracle's result codes alone: (rejected, passed) = windows that some stage r >= 2 WITH an integer form
    (form[r]) rejected / passed while their tile was provably in the wave phase. A tile goes over to the wave phase at the
    first stage that fewer than wave_below of its windows enter; a block of 64 x 24 window origins holds whole tiles of every
    kernel, so a window in a block with fewer than wave_below windows entering stage r is evaluated there by the wave phase."""
    h, w = img.shape
    rej = np.zeros(len(codes), bool)
    pas = np.zeros(len(codes), bool)
    first = 0
    for sc in orc.scales(o.win_w, o.win_h, w, h, SCALE_FACTOR):
        nx, ny = int(sc["nx"]), int(sc["ny"])
        c = codes[first:first + nx * ny].reshape(ny, nx)
        for r in range(2, o.nstages):
            if not form[r]:
                continue
            entered = ce.reached(c, r)
            for ty in range(0, ny, SUPER_ROWS):
                for tx in range(0, nx, 64):
                    e = entered[ty:ty + SUPER_ROWS, tx:tx + 64]
                    if 0 < e.sum() < wave_below:
                        cc_ = c[ty:ty + SUPER_ROWS, tx:tx + 64]
                        idx = first + (np.arange(ty, min(ty + SUPER_ROWS, ny))[:, None] * nx + np.arange(tx, min(tx + 64, nx))[None, :])
                        rej[idx[e & (cc_ == -r)]] = True
                        pas[idx[e & (cc_ != -r)]] = True
        first += nx * ny
    return rej, pas
