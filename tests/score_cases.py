"""Inputs for the tests of detection scores (rejectLevels / levelWeights) on batches and on results that stay on the device,
shared by tests/test_score_cases_host.py (CPU: cc_group_rectangles_levels against the oracle, and checks that these inputs
reach what they aim at) and the GPU tests tests/test_gpu_group_device_scores.py / tests/test_gpu_detect_scores.py: the
rectangle lists of tests/group_cases.py with levels and weights, the five detector frames of
tests/test_gpu_detect_device_out.py, and a one-stage cascade that passes almost every window with several weights."""
import functools
import os
import sys
import tempfile

import numpy as np

from oracle import oracle as orc
from tests import cascade_factory as cf
from tests import group_cases as gc
from tests.util import frame_natural

T = 1536  # rectangles of a frame up to which k_group_frames_scored keeps its workspace in LDS (GROUP_LDS_RECTS_SCORED)
DBL_MIN = sys.float_info.min
LEVELS = (-1, 0, 1, 2, 3)
SEED = 23


# ------------------------------------------------------------------ levels and weights for rectangle lists
def random_scores(n, rng):
    """n levels from LEVELS and n weights: normal values of both signs over many magnitudes, values below DBL_MIN in
    magnitude (subnormals of both signs, +0.0), DBL_MIN itself, and -- about a third -- exact repeats of an earlier weight of
    the same list. No -0.0 (its tie with +0.0 may come out either way) and no NaN."""
    levels = rng.choice(np.array(LEVELS, np.int32), n).astype(np.int32)
    w = np.zeros(n, np.float64)
    for i in range(n):
        kind = int(rng.integers(0, 6))
        if kind == 0 and i > 0:
            w[i] = w[int(rng.integers(0, i))]
        elif kind == 1 and i > 0:
            w[i] = w[i - 1]
        elif kind == 2:
            w[i] = DBL_MIN
        elif kind == 3:
            w[i] = (0.0, 5e-324, -5e-324, 1e-310, -1e-310, DBL_MIN / 2, -DBL_MIN / 2)[int(rng.integers(0, 7))]
        else:
            w[i] = rng.standard_normal() * 10.0 ** int(rng.integers(-3, 4))
    return levels, w


def _cluster(x, y, n):
    return [[x + k % 2, y, 40, 40] for k in range(n)]


def hand_made_lists():
    """-> [(rects, levels, weights)]: a list with a class whose members all have level <= 0 (weights below and above DBL_MIN
    beside a class of level 2), and one with a class of level 3 whose weights are all negative (beside members of lower
    levels with positive weights)."""
    a = (np.array(_cluster(100, 100, 4) + _cluster(400, 100, 3) + _cluster(700, 100, 3), np.int32),
         np.array([0, -1, 0, -1] + [0, 0, -1] + [2, 1, 2], np.int32),
         np.array([-3.0, 7.0, 1e-310, 9.0] + [0.25, 0.5, 4.0] + [-1.0, 5.0, -2.0], np.float64))
    b = (np.array(_cluster(100, 100, 5) + _cluster(400, 100, 3), np.int32),
         np.array([3, 1, 3, 0, 3] + [1, 1, 1], np.int32),
         np.array([-4.0, 6.0, -0.5, 8.0, -2.5] + [1.0, 3.0, 2.0], np.float64))
    return [a, b]


HAND_MADE_WANT = [  # at threshold 1, eps 0.2: (levels, weights) of the classes in order
    ([0, 0, 2], [DBL_MIN, 0.5, -1.0]),
    ([3, 1], [-0.5, 3.0]),
]


@functools.lru_cache(maxsize=None)
def scored_lists():
    """The 100 lists of group_cases.random_lists() with random_scores, then hand_made_lists(): (rects, levels, weights)."""
    rng = np.random.default_rng(SEED)
    out = [(r,) + random_scores(len(r), rng) for r in gc.random_lists()]
    return tuple(out + hand_made_lists())


def with_scores(rects, seed):
    rects = np.ascontiguousarray(rects, np.int32).reshape(-1, 4)
    return (rects,) + random_scores(len(rects), np.random.default_rng(seed))


def oracle_group(rects, levels, weights, thr, eps=0.2, cap=None):
    """orc_group_rectangles_levels -> (count, rects, levels, weights), the arrays `cap` long (default: all)."""
    import ctypes as C
    n = len(rects)
    cap = max(n, 1) if cap is None else cap
    out, ol, ow = np.zeros((max(cap, 1), 4), np.int32), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.float64)
    p = orc._p
    m = orc.lib().orc_group_rectangles_levels(p(np.ascontiguousarray(rects, np.int32)), p(np.ascontiguousarray(levels, np.int32)),
                                              p(np.ascontiguousarray(weights, np.float64)), n, int(thr), C.c_double(eps), p(out),
                                              p(ol), p(ow), cap)
    k = min(m, cap)
    return m, out[:k], ol[:k], ow[:k]


# ------------------------------------------------------------------ detector frames (tests/test_gpu_detect_device_out.py's recipe)
W, H, N = 320, 240, 5
ORDER = [1, 3, 0, 2, 4]  # a pass that fits (the flat frame), one that overflows 16 candidates, a dead pass behind it


def _paste(img, seed, ks):
    tm = np.load(os.path.join(os.path.dirname(__file__), "..", "data", "face_template_24x24.npy"))
    rng = np.random.default_rng(seed)
    out = img.copy()
    for k in ks:
        s = int(24 * k)
        y, x = int(rng.integers(0, H - s)), int(rng.integers(0, W - s))
        out[y:y + s, x:x + s] = orc.resize_linear_exact(tm, s, s)
    return out


@functools.lru_cache(maxsize=None)
def detector_frames():
    """Smooth noise plus pasted templates; frame 1 is flat (no window passes the variance test)."""
    f = [_paste(frame_natural(W, H, 300 + i), 40 + i, ks) for i, ks in enumerate([(1.0, 1.7, 2.6), (), (1.3, 3.0), (2.0,), (1.0, 1.5, 4.0)])]
    f[1] = np.full((H, W), 77, np.uint8)
    out = np.stack(f)
    out.setflags(write=False)
    return out


def ordered_candidates(o, frame, sf=1.1):
    """The oracle's candidates of one frame in (scale, gy, gx) order -> (rects (n, 4), last-stage sums (n,))."""
    det = orc.detect_raw(o, frame, sf, nthreads=8, full=True)
    raw = det.candidates[np.lexsort((det.candidates[:, 1], det.candidates[:, 2], det.candidates[:, 0]))]
    sc = orc.scales(o.win_w, o.win_h, frame.shape[1], frame.shape[0], sf)
    first = np.concatenate([[0], np.cumsum(sc["nx"].astype(np.int64) * sc["ny"])])  # a window's place in det.sums, as
    at = first[raw[:, 0]] + raw[:, 2].astype(np.int64) * sc["nx"][raw[:, 0]] + raw[:, 1]  # orc.detect_multiscale_levels finds it
    return np.ascontiguousarray(raw[:, 3:7], np.int32), np.ascontiguousarray(det.sums[at], np.float64)


@functools.lru_cache(maxsize=None)
def oracle_scores(xml, mn, which="frames"):
    """Per frame of detector_frames() ("frames") or score_frames() ("many") at scaleFactor 1.1: (rects, levels, weights), the
    oracle's candidates in (scale, gy, gx) order grouped with levels and weights at threshold mn."""
    o = orc.load_cascade_xml(xml)
    out = []
    for f in (detector_frames() if which == "frames" else score_frames()):
        r, w = ordered_candidates(o, f)
        out.append(oracle_group(r, np.full(len(r), o.nstages, np.int32), w, mn)[1:])
    return out


@functools.lru_cache(maxsize=None)
def oracle_detect_levels(xml, mn):
    """orc.detect_multiscale_levels of every frame of detector_frames() at scaleFactor 1.1 (its own candidate order)."""
    o = orc.load_cascade_xml(xml)
    return [orc.detect_multiscale_levels(o, f, 1.1, mn, nthreads=8) for f in detector_frames()]


def sorted_scores(rects, levels, weights):
    """A frame's result in an order that does not depend on the order of the candidates it was grouped from."""
    k = np.lexsort((weights, rects[:, 3], rects[:, 2], rects[:, 1], rects[:, 0])) if len(rects) else np.zeros(0, int)
    return rects[k], levels[k], weights[k]


def clusters(n_clusters, per, seed, cols=25):
    """n_clusters x per rectangles in tight clusters 100 apart, shuffled: one class per cluster at eps 0.2."""
    rng = np.random.default_rng(seed)
    c = np.arange(n_clusters)
    centres = np.stack([100 * (c % cols), 100 * (c // cols), np.full(n_clusters, 40), np.full(n_clusters, 40)], 1)
    r = np.repeat(centres, per, 0) + rng.integers(-2, 3, (n_clusters * per, 4))
    return r[rng.permutation(len(r))].astype(np.int32)


# ------------------------------------------------------------------ a cascade that passes almost every window, with several weights
def score_cascade_text():
    """One stage of three Haar stumps with unequal leaves (all multiples of 1/8: their sums are exact in any order) and a
    threshold below every sum: every window with some variance is a candidate, and its weight is one of up to eight sums."""
    feats = orc.haar_catalog(24, 24, 0)[[1234, 4321, 777]].copy()
    weak = [([(0, -1, 0, np.float32(0.0))], [0.5, -0.25]), ([(0, -1, 1, np.float32(0.01))], [1.0, 0.125]),
            ([(0, -1, 2, np.float32(-0.01))], [-0.75, 2.0])]
    return cf.haar_xml(feats, [(np.float32(-10.0), weak)], mode="BASIC")


@functools.lru_cache(maxsize=None)
def score_cascade():
    """-> path of score_cascade_text(), written once per process to a temporary directory."""
    path = os.path.join(tempfile.mkdtemp(prefix="ccamd_score_"), "score.xml")
    with open(path, "w") as f:
        f.write(score_cascade_text())
    return path


@functools.lru_cache(maxsize=None)
def score_frames():
    """The textured 160x120 frame of group_cases.many_candidate_frames() (far more than T candidates) and its frame of two
    small patches (a few hundred)."""
    f = np.asarray(gc.many_candidate_frames())[[0, 3]].copy()
    f.setflags(write=False)
    return f
