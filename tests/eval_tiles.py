"""The training evaluator's tile sizes and window limits, shared by tests/test_eval_tiles_host.py and
tests/test_gpu_eval_tiles.py: the tile rule restated from DESIGN.md's LDS budgets, one case per kernel configuration and
budget edge, and plain definitions of what the evaluator computes (numpy int64 / Python integers and single float32
operations, written from the reference's formulas: features.cpp:13-25, haarfeatures.h:108-122, lbpfeatures.h:70-83,
traincascade_features.h:40-63). Nothing here imports the library or the oracle."""
import functools
from dataclasses import dataclass

import numpy as np

HAAR, LBP = 0, 1
BASIC, CORE, ALL = 0, 1, 2

# ---- the tile rule (k_eval_batch / k_eval_batch_wide) ------------------------------------------------
NARROW_BUDGET = 80 * 1024   # two blocks of the narrow kernel per CU
WIDE_BUDGET = 160 * 1024    # the wide kernel's tile of 64 samples: the whole LDS of a CU
MAX_SIDE = 256              # cc_eval_create takes windows of 3 .. 256 pixels a side


def entries(W, H):
    return (W + 1) * (H + 1)


def bytes_per_sample(W, H, tilted):
    """One int32 per integral entry; Haar ALL stages a tilted tile behind the sum tile."""
    return entries(W, H) * 4 * (2 if tilted else 1)


def tile_samples(W, H, tilted):
    """Samples per tile: 64 (wide kernel) where no tilted tile is needed and 64 samples fit in 160 KB, else the largest
    of 32 .. 1 that fits in 80 KB, else None (the window is refused)."""
    per = bytes_per_sample(W, H, tilted)
    if not tilted and per * 64 <= WIDE_BUDGET:
        return 64
    for S in (32, 16, 8, 4, 2, 1):
        if per * S <= NARROW_BUDGET:
            return S
    return None


def lbp_count(W, H):
    """lbpfeatures.cpp:35-45: every 3w x 3h block inside the window."""
    def c(n):
        return sum(n - 3 * w + 1 for w in range(1, n // 3 + 1))
    return c(W) * c(H)


# ---- cases -----------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    ftype: int
    mode: int
    W: int
    H: int
    S: object        # expected samples per tile; None: cc_eval_create refuses the window
    nfeat: int       # catalogue size (checked against the oracle's catalogue on the host)
    edge: str        # why the window is here
    exact: int = 0   # != 0: S * bytes_per_sample is exactly this budget
    span: int = 3000 # features of the head and tail ranges

    @property
    def tilted(self):
        return self.ftype == HAAR and self.mode == ALL

    @property
    def id(self):
        kind = "LBP" if self.ftype == LBP else ("BASIC", "CORE", "ALL")[self.mode]
        return "%dx%d-%s" % (self.W, self.H, kind)

    @property
    def wide(self):
        return self.S == 64

    def ranges(self):
        """Feature ranges [a, b): head, a middle piece and tail of the catalogue, exactly one feature, 2049 features
        (launch_batch cuts them into two chunks of 1025 and 1024) and fewer features than the 1024 / S a block of the
        narrow kernel takes per trip. A Haar ALL catalogue interleaves upright and tilted features from x = 1 on:
        the head has no tilted feature, the middle, the tail and the short range hold both kinds."""
        n, k = self.nfeat, min(self.span, self.nfeat)
        mid = n // 2
        out = [(0, k), (mid - k // 2, mid - k // 2 + k), (n - k, n), (mid, mid + 1), (n // 3, n // 3 + 2049),
               (mid + 7, mid + 7 + max(1, 1024 // self.S - 3))]
        return [(a, b) for (a, b) in out if 0 <= a < b <= n]

    def sample_counts(self):
        """Stored samples: 1, S - 1, S + 1; the wide kernel also 9 and 18 tiles (more than one tile per XCD, a grid padded
        to a multiple of 8)."""
        ns = {1, self.S - 1, self.S + 1}
        if self.wide:
            ns |= {64 * 8 + 1, 64 * 17 + 5}
        return sorted(v for v in ns if v > 0)


CASES = [
    Case(HAAR, BASIC, 31, 19, 64, 169562, "wide tile of exactly 160 KB, the whole LDS of a CU", exact=WIDE_BUDGET),
    Case(LBP, 0, 31, 19, 64, 8835, "wide tile of exactly 160 KB, the whole LDS of a CU", exact=WIDE_BUDGET),
    Case(LBP, 0, 19, 31, 64, 8835, "the same tile with the transposed row stride", exact=WIDE_BUDGET),
    Case(HAAR, BASIC, 25, 24, 16, 175964, "650 entries: first window past the wide tile (no S = 32 without a tilted tile)"),
    Case(HAAR, BASIC, 39, 31, 16, 710292, "1280 entries: 16 samples are exactly 80 KB", exact=NARROW_BUDGET),
    Case(HAAR, ALL, 15, 19, 32, 62381, "320 entries: 32 samples with the tilted tile are exactly 80 KB", exact=NARROW_BUDGET),
    Case(HAAR, ALL, 16, 16, 32, 50878, "S = 32 below its budget: only a tilted tile reaches S = 32"),
    Case(HAAR, ALL, 31, 19, 16, 264333, "640 entries: 16 samples with the tilted tile are exactly 80 KB", exact=NARROW_BUDGET),
    Case(HAAR, ALL, 39, 31, 8, 1151839, "1280 entries: 8 samples with the tilted tile are exactly 80 KB", exact=NARROW_BUDGET),
    Case(HAAR, ALL, 47, 39, 4, 2666088, "1920 entries: the deepest tilted case that stays cheap", span=20000),
    Case(LBP, 0, 79, 63, 4, 668577, "5120 entries: 4 samples are exactly 80 KB", exact=NARROW_BUDGET),
    Case(LBP, 0, 127, 79, 2, 2739009, "10 240 entries: 2 samples are exactly 80 KB", exact=NARROW_BUDGET),
    Case(LBP, 0, 101, 101, 1, 2832489, "10 404 entries: the first square window with S = 1"),
    Case(LBP, 0, 128, 128, 1, 7338681, "16 641 entries: k_set_images needs 66 048 bytes of LDS, more than 64 KB"),
    Case(LBP, 0, 159, 127, 1, 11166729, "20 480 entries: one sample is exactly 80 KB, the largest window taken", exact=NARROW_BUDGET),
    Case(LBP, 0, 160, 127, None, lbp_count(160, 127), "20 608 entries: one sample does not fit in 80 KB"),
]
# Not covered: tilted S = 2 and S = 1 as tiles of the bulk kernel (Haar ALL catalogues of many millions of records; 65x66 ALL
# below is created for k_set_images alone).
EVAL_CASES = [c for c in CASES if c.S is not None]
REFUSED = [c for c in CASES if c.S is None]

# k_set_images alone: the smallest window, one side past the 64 threads of a block each way, and both sides past them
SET_IMAGE_WINDOWS = [(3, 3), (3, 70), (70, 3), (65, 66)]


def case_id(c):
    return c.id


# ---- inputs -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def images(W, H, n, seed=20261019):
    """n samples that do not depend on n beyond their count: noise, a flat image (norm factor 0), a step edge, a noisy
    gradient, in turn."""
    rng = np.random.default_rng(seed + 1000 * W + H)
    out = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    for i in range(n):
        if i % 4 == 1:
            out[i] = (37 * i + 11) % 256
        elif i % 4 == 2:
            out[i] = 0
            if i % 8 == 2:
                out[i, :, W // 2:] = 255 - (i % 5)
            else:
                out[i, H // 2:, :] = 200 + (i % 50)
        elif i % 4 == 3:
            ramp = np.add.outer(np.arange(H) * (200.0 / H), np.arange(W) * (50.0 / W))
            out[i] = np.clip(ramp + (out[i] % 16), 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


# ---- definitions ------------------------------------------------------------------------------------------------------
def sum_def(img):
    """sum(Y, X) = the pixels of rows y < Y and columns x < X; (H + 1) x (W + 1) int64."""
    H, W = img.shape
    out = np.zeros((H + 1, W + 1), np.int64)
    out[1:, 1:] = img.astype(np.int64).cumsum(0).cumsum(1)
    return out


def tilted_def(img):
    """tilted(Y, X) = the pixels of rows y < Y with |x - (X - 1)| <= Y - y - 1; (H + 1) x (W + 1) int64."""
    H, W = img.shape
    px = img.astype(np.int64)
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    out = np.zeros((H + 1, W + 1), np.int64)
    for Y in range(H + 1):
        for X in range(W + 1):
            out[Y, X] = px[(ys < Y) & (np.abs(xs - (X - 1)) <= Y - ys - 1)].sum()
    return out


def norm_factor_def(img):
    """calcNormFactor: sqrt(area * sum(p^2) - sum(p)^2) over the rectangle (1, 1, W - 2, H - 2). The radicand is an exact
    integer below 2^53, so the float64 the reference forms is that integer: one float64 square root, rounded to float32."""
    import math
    H, W = img.shape
    inner = [int(v) for v in img[1:H - 1, 1:W - 1].ravel()]
    area, sm, sq = (W - 2) * (H - 2), sum(inner), sum(v * v for v in inner)
    rad = area * sq - sm * sm
    assert 0 <= rad < 2 ** 53
    return np.float32(math.sqrt(float(rad)))


def _upright(S, x, y, w, h):
    return int(S[y, x] - S[y, x + w] - S[y + h, x] + S[y + h, x + w])


def _tilted(T, x, y, w, h):
    return int(T[y, x] - T[y + h, x - h] - T[y + w, x + w] + T[y + w + h, x + w - h])


def haar_value_def(feature, S, T, nf):
    """operator(): w0 * r0 + w1 * r1 (+ w2 * r2 when w2 != 0) in float32, one operation at a time, divided by the norm
    factor; 0 when the norm factor is 0. feature = (tilted, rects[3][4] as x y w h, weights[3]); rects after the first
    zero weight are not read."""
    tilted, rects, wts = feature
    f32 = np.float32
    r = []
    for j in range(3):
        if f32(wts[j]) == 0:
            break
        x, y, w, h = (int(v) for v in rects[j])
        r.append(f32(_tilted(T, x, y, w, h) if tilted else _upright(S, x, y, w, h)))
    r += [f32(0)] * (3 - len(r))
    ret = f32(f32(wts[0]) * r[0]) + f32(f32(wts[1]) * r[1])
    if f32(wts[2]) != 0:
        ret = f32(ret + f32(f32(wts[2]) * r[2]))
    return f32(0) if nf == 0 else f32(f32(ret) / f32(nf))


def lbp_code_def(rect, S):
    """The 3 x 3 grid of w x h cells at (x, y): a neighbour cell sets its bit when its sum is >= the centre's; bits from
    128 down: top-left, top, top-right, right, bottom-right, bottom, bottom-left, left."""
    x, y, w, h = (int(v) for v in rect)
    cell = [[_upright(S, x + c * w, y + r * h, w, h) for c in range(3)] for r in range(3)]
    ring = [cell[0][0], cell[0][1], cell[0][2], cell[1][2], cell[2][2], cell[2][1], cell[2][0], cell[1][0]]
    return sum(128 >> k for k, v in enumerate(ring) if v >= cell[1][1])
