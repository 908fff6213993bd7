"""Inputs for the tests of the device ordering and grouping (cc_group.hip), shared by tests/test_group_cases_host.py (CPU:
the host grouping against the oracle, and checks that these inputs reach what they aim at) and the GPU tests
tests/test_gpu_group_device.py / tests/test_gpu_detect_device_out.py: random rectangle lists over an eps and threshold
grid, hand-made lists for the rounding in the inside-a-bigger-class filter, frame lists past one block scan, chains and a
single class for the union-find, and frames for a one-stage cascade that passes almost every window."""
import functools
import os
import tempfile

import numpy as np

from oracle import oracle as orc
from tests import cascade_factory as cf
from tests.util import frame_natural

EPS_GRID = (0.0, 0.05, 0.1, 0.2, 0.25, 0.5, 1.0, 1.5)
THRESHOLDS = (1, 2, 3, 5)
N_LISTS = 100
SEED = 11


# ------------------------------------------------------------------ random lists
def random_list(rng):
    """0..199 rectangles around max(n // u, 1) centres, u in 2..11: centres in [-50, 700)^2, a base (w, h) per cluster
    from [8, 120)^2 (not square), one jitter j in 0..11 per list on all four fields, sides at least 1."""
    n = int(rng.integers(0, 200))
    k = max(n // int(rng.integers(2, 12)), 1)
    centres = np.concatenate([rng.integers(-50, 700, (k, 2)), rng.integers(8, 120, (k, 2))], 1)
    j = int(rng.integers(0, 12))
    r = centres[rng.integers(0, k, n)] + rng.integers(-j, j + 1, (n, 4))
    r[:, 2:] = np.maximum(r[:, 2:], 1)
    return np.ascontiguousarray(r, np.int32).reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def random_lists(count=N_LISTS, seed=SEED):
    rng = np.random.default_rng(seed)
    return tuple(random_list(rng) for _ in range(count))


def similar_matrix(r, eps):
    """-> (similar[i, j], at_delta[i, j]): cv::SimilarRects of every pair with the kernel's double expression, and whether
    one of the pair's four distances equals delta exactly."""
    r = np.asarray(r, np.int64).reshape(-1, 4)
    x, y, w, h = (r[:, k] for k in range(4))
    delta = np.float64(eps) * (np.minimum(w[:, None], w[None, :]) + np.minimum(h[:, None], h[None, :])) * 0.5
    d = np.stack([np.abs(x[:, None] - x[None, :]), np.abs(y[:, None] - y[None, :]),
                  np.abs((x + w)[:, None] - (x + w)[None, :]), np.abs((y + h)[:, None] - (y + h)[None, :])])
    sim = (d <= delta).all(0)
    return sim, sim & (d == delta).any(0)


def has_pair_at_delta(r, eps):
    sim, at = similar_matrix(r, eps)
    return bool(np.triu(at, 1).any())


def class_sizes(r, eps):
    """Sizes of the connected components of the similarity graph (plain union-find over all pairs)."""
    sim, _ = similar_matrix(r, eps)
    n = len(sim)
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for i, j in zip(*np.nonzero(np.triu(sim, 1))):
        a, b = find(int(i)), find(int(j))
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.bincount([find(i) for i in range(n)], minlength=n)[[i for i in range(n) if parent[i] == i]]


# ------------------------------------------------------------------ the filter's cvRound
def round_half_even(v):
    return int(np.rint(v))


def round_half_up(v):  # a truncation of v + 0.5
    return int(v + 0.5)


def round_down(v):
    return int(v)


def filter_count(classes, threshold, eps, rnd):
    """Length of groupRectangles' output for classes [(rect, count)] of identical rectangles (their average is the
    rectangle itself), with `rnd` as the filter's cvRound: the filter restated, for the hand-made cases only."""
    kept = 0
    for i, (r1, n1) in enumerate(classes):
        if n1 <= threshold:
            continue
        inside = False
        for j, (r2, n2) in enumerate(classes):
            if j == i or n2 <= threshold:
                continue
            dx, dy = rnd(r2[2] * eps), rnd(r2[3] * eps)
            if (r1[0] >= r2[0] - dx and r1[1] >= r2[1] - dy and r1[0] + r1[2] <= r2[0] + r2[2] + dx and
                    r1[1] + r1[3] <= r2[1] + r2[3] + dy and (n2 > max(3, n1) or n1 < 3)):
                inside = True
        kept += not inside
    return kept


# eps 0.5, threshold 1. A class of four with width 5 (5 * 0.5 = 2.5 -> 2) or 7 (3.5 -> 4) and a class of two whose left
# edge is 3 (4) to the left of it, far enough in y not to be similar: kept at dx = 2, dropped at dx = 3 (4).
ROUNDING_EPS, ROUNDING_THRESHOLD = 0.5, 1
ROUNDING_CASES = {
    "2.5": [([100, 100, 5, 40], 4), ([97, 85, 3, 20], 2)],   # half to even keeps both; v + 0.5 truncated drops the small one
    "3.5": [([100, 100, 7, 40], 4), ([96, 85, 3, 20], 2)],   # half to even drops the small one; rounding down keeps both
}
ROUNDING_WANT = {"2.5": 2, "3.5": 1}


def rounding_rects(name):
    return np.array([r for r, n in ROUNDING_CASES[name] for _ in range(n)], np.int32)


# ------------------------------------------------------------------ many small frames
def small_frames(n_frames, seed):
    """n_frames lists of 0..12 rectangles, about a third of them empty: up to three tight clusters of side 40 per frame."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_frames):
        n = 0 if rng.integers(0, 3) == 0 else int(rng.integers(1, 13))
        k = int(rng.integers(1, 4))
        centres = np.stack([150 * np.arange(k), rng.integers(0, 300, k), np.full(k, 40), np.full(k, 40)], 1)
        r = centres[rng.integers(0, k, n)] + rng.integers(-2, 3, (n, 4))
        out.append(np.ascontiguousarray(r, np.int32).reshape(-1, 4))
    return out


# ------------------------------------------------------------------ union-find under load
def one_class(n, seed=1):
    """n rectangles within 1 of (100, 100, 40, 40): every pair is similar."""
    return (np.array([100, 100, 40, 40]) + np.random.default_rng(seed).integers(-1, 2, (n, 4))).astype(np.int32)


def chain(n):  # r_k ~ r_k+1 only: w = h = 40 -> delta 8, neighbours 5 apart, next-but-one 10 apart
    return np.array([[5 * k, 7, 40, 40] for k in range(n)], np.int32)


def two_chains(n):
    """Two chains taking turns in the list, 2 apart in x and 1000 apart in y."""
    k = np.arange(n)
    return np.stack([5 * (k // 2) + 2 * (k % 2), 7 + 1000 * (k % 2), np.full(n, 40), np.full(n, 40)], 1).astype(np.int32)


# ------------------------------------------------------------------ a cascade that passes almost every window
def weak_cascade_text():
    """One stage of one Haar stump whose two leaves both pass: every window with some variance is a candidate."""
    feats = orc.haar_catalog(24, 24, 0)[[1234]].copy()
    return cf.haar_xml(feats, [(np.float32(-1.0), [([(0, -1, 0, np.float32(0.0))], [1.0, 1.0])])], mode="BASIC")


@functools.lru_cache(maxsize=None)
def weak_cascade():
    """-> (path, oracle cascade) of weak_cascade_text(), written once per process to a temporary directory."""
    path = os.path.join(tempfile.mkdtemp(prefix="ccamd_weak_"), "weak.xml")
    with open(path, "w") as f:
        f.write(weak_cascade_text())
    return path, orc.load_cascade_xml(path)


FLAT = 77
MANY_W, MANY_H = 160, 120
# (x, y, w, h) of the textured patches in frames 1 and 3 of many_candidate_frames: one in each of two opposite corners
PATCHES_MID, PATCHES_FEW = ((0, 0, 48, 34), (150, 110, 10, 10)), ((0, 0, 16, 16), (150, 110, 10, 10))


@functools.lru_cache(maxsize=None)
def many_candidate_frames():
    """Four 160x120 frames for scaleFactor 1.1: all texture (18 913 raw candidates), two patches of texture on a flat ground
    (2 997), flat (none), two smaller patches (349). A window is a candidate as soon as it touches texture."""
    tex = frame_natural(MANY_W, MANY_H, 5)
    out = [tex]
    for patches in (PATCHES_MID, (), PATCHES_FEW):
        f = np.full((MANY_H, MANY_W), FLAT, np.uint8)
        for x, y, w, h in patches:
            f[y:y + h, x:x + w] = tex[y:y + h, x:x + w]
        out.append(f)
    out = np.stack(out)
    out.setflags(write=False)
    return out


SMALL_N, SMALL_SIDE = 300, 40


def small_flat(i):
    return i in (0, SMALL_N - 1) or i % 5 == 3


@functools.lru_cache(maxsize=None)
def many_small_frames():
    """300 frames of 40x40, a fifth of them flat (frames 0 and 299 among them), the others textured."""
    out = np.stack([np.full((SMALL_SIDE, SMALL_SIDE), FLAT, np.uint8) if small_flat(i) else frame_natural(SMALL_SIDE, SMALL_SIDE, 700 + i)
                    for i in range(SMALL_N)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_results(which):
    """Per frame of many_candidate_frames ("many") or many_small_frames ("small"), at scaleFactor 1.1: (the raw candidates'
    rectangles in (scale, gy, gx) order, detect_multiscale at minNeighbors 2)."""
    _, o = weak_cascade()
    frames = many_candidate_frames() if which == "many" else many_small_frames()
    out = []
    for f in frames:
        c = orc.detect_raw(o, f, 1.1, nthreads=8).candidates
        ordered = np.ascontiguousarray(c[np.lexsort((c[:, 1], c[:, 2], c[:, 0]))][:, 3:7])
        out.append((ordered, orc.detect_multiscale(o, f, 1.1, 2, nthreads=8)))
    return out
