"""Witnesses and case lists for the front end (cc_front.hip: k_resize, the band integrals, k_diag_sums / k_tilted_cols)
and for the LBP code, shared by tests/test_front_cases_host.py (the oracle against the witnesses, and a census that shows
each case is what its reason says) and tests/test_gpu_front_edges.py (the kernels against the witnesses, no oracle).

Pure numpy and `fractions`: this module imports neither the oracle nor the package.

What each witness is, and is not:
* integral_witness, tilted_witness, lbp_witness are written from the DEFINITIONS (a sum over a rectangle, over a
  45-degree triangle, over nine cells of pixels). They share no recurrence, no integral image and no source line with
  cc_oracle.cpp or the kernels.
* resize_witness is NOT an independent source. It is a second statement of the same published INTER_LINEAR_EXACT formula
  that oracle/cc_oracle.cpp (linear_exact_axis) and the library (linear_exact_taps) transcribe, in another language and in
  array form. A misreading of the formula would be shared. What this module adds is tap_census: the taps in exact rational
  arithmetic, which names the inputs on which a slip in the operation order or in the width of a weight becomes visible.
  Only the hand-computed cases of tests/test_oracle_detect.py pin resize to OpenCV.
"""
import functools
from fractions import Fraction

import numpy as np


# ------------------------------------------------------------------------------------------------ images
def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def checker(w, h):
    """0 / 255 alternating along both axes: a tap offset off by one inverts a pixel, a weight off by one moves it."""
    y, x = np.mgrid[0:h, 0:w]
    return (((x + y) & 1) * 255).astype(np.uint8)


def images(w, h, seed):
    """The contents every resize and tilted case runs on: (name, image)."""
    return [("noise", noise(w, h, seed)), ("checker", checker(w, h)), ("all255", np.full((h, w), 255, np.uint8))]


# ------------------------------------------------------------------------------------------------ integrals
def integral_witness(img, square):
    """sum (or sum of squares) over [0, y) x [0, x) modulo 2^32, as int32: numpy's cumsum in 64 bits, reduced."""
    v = img.astype(np.uint64)
    if square:
        v = v * v
    out = np.zeros((img.shape[0] + 1, img.shape[1] + 1), np.uint64)
    out[1:, 1:] = v.cumsum(0).cumsum(1)  # < 2^64 for any image here; reduced modulo 2^32 below
    return (out & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


# ------------------------------------------------------------------------------------------------ resize
def axis_taps(src, dst, order="published"):
    """Left tap index and 8.8 weight of the right tap for every destination index, in float64 in the published operation
    order: inv = dst / src; scale = 1.0 / inv; f = scale * (d + 0.5) - 0.5; i = floor(f); w1 = rint((f - i) * 256).
    Outside [0, src - 1) the border pixel is replicated (weight 0). order="ratio" computes scale = src / dst instead:
    the slip the order-sensitive cases are there to catch."""
    if order == "published":
        inv = np.float64(dst) / np.float64(src)
        scale = np.float64(1.0) / inv
    else:
        scale = np.float64(src) / np.float64(dst)
    f = scale * (np.arange(dst, dtype=np.float64) + 0.5) - 0.5
    i = np.floor(f)
    w1 = np.rint((f - i) * 256.0).astype(np.int64)  # rint: half to even, as cvRound
    i = i.astype(np.int64)
    inside = (i >= 0) & (src > 1) & (i < src - 1)
    ofs = np.where(inside, i, np.where((i >= 0) & (src > 1), src - 1, 0))
    return ofs, np.where(inside, w1, 0)


def resize_witness(img, dw, dh, order="published"):
    """INTER_LINEAR_EXACT of an 8-bit image: horizontal pass in 8.8 (fits 16 bits), vertical pass (fits 32 bits),
    (v + 2^15) >> 16. See the module docstring: a restatement, not an independent source."""
    h, w = img.shape
    p = img.astype(np.int64)
    x0, wx1 = axis_taps(w, dw, order)
    y0, wy1 = axis_taps(h, dh, order)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    hor = (256 - wx1)[None, :] * p[:, x0] + wx1[None, :] * p[:, x1]
    assert hor.max() < 1 << 16
    v = (256 - wy1)[:, None] * hor[y0] + wy1[:, None] * hor[y1]
    assert v.max() + (1 << 15) < 1 << 32
    return ((v + (1 << 15)) >> 16).astype(np.uint8)


def tap_census(src, dst):
    """Every destination index of one axis classified in exact rational arithmetic, f = (src / dst)(d + 1/2) - 1/2:
      f_integral  f is an integer (the two orderings may then pick offset i - 1 with weight 256 or i with weight 0: same pixel)
      tie         (f - floor f) * 256 lies exactly between two integers (the rounding direction matters)
      border      the border pixel is replicated (floor f < 0, or >= src - 1, or a one-pixel source)
      weight256   the float64 tap (published order) has weight 256, which needs 9 bits
      differs     the float64 taps of the published order and of scale = src / dst differ (offset or weight)
    plus the taps themselves ("ofs", "w1": published order; "ofs_ratio", "w1_ratio")."""
    ofs, w1 = axis_taps(src, dst)
    ofs_r, w1_r = axis_taps(src, dst, "ratio")
    f_integral, tie, border = (np.zeros(dst, bool) for _ in range(3))
    for d in range(dst):
        f = Fraction(src, dst) * Fraction(2 * d + 1, 2) - Fraction(1, 2)
        i = f.numerator // f.denominator
        f_integral[d] = f.denominator == 1
        tie[d] = ((f - i) * 512).denominator == 1 and ((f - i) * 512).numerator % 2 == 1
        border[d] = i < 0 or src <= 1 or i >= src - 1
    return {"f_integral": f_integral, "tie": tie, "border": border, "weight256": w1 == 256,
            "differs": (ofs != ofs_r) | (w1 != w1_r), "ofs": ofs, "w1": w1, "ofs_ratio": ofs_r, "w1_ratio": w1_r}


def load_path(src_w, dst_w):
    """k_resize's per-thread choice between one 16-byte load with byte permutes (True) and eight single-byte loads (False),
    restated from the witness taps: a thread owns 4 adjacent output columns (the tap table is padded with copies of the
    last tap); it takes the wide path when the source has at least 16 columns and the 8 source bytes of its columns lie
    within 16 bytes from min(x0 of its first column, src_w - 16). One entry per thread of a row; a wavefront is 64 of them."""
    return (src_w >= 16) & (load_span(src_w, dst_w) <= 15)


def load_span(src_w, dst_w):
    """Per thread: the offset of its last source byte from the start of its 16-byte load (15 is the last that fits)."""
    x0, _ = axis_taps(src_w, dst_w)
    x0 = np.concatenate([x0, np.repeat(x0[-1:], -dst_w % 4)]).reshape(-1, 4)
    x1 = np.minimum(x0 + 1, src_w - 1)
    return x1[:, 3] - np.minimum(x0[:, 0], src_w - 16)


def mixed_in_one_wavefront(src_w, dst_w):
    lp = load_path(src_w, dst_w)
    return any(lp[k:k + 64].any() and not lp[k:k + 64].all() for k in range(0, len(lp), 64))


RESIZE_ROWS = 8  # output rows a k_resize thread walks, keeping the horizontally interpolated lower source row


def row_census(src_h, dst_h):
    """What k_resize's walk down a band of 8 output rows meets, from the witness taps: per output row, whether its upper
    source row is the one kept from the row before ("reuse"; never the first row of a band), whether it is the same upper
    row as the row before ("repeat": an upscale) and whether both taps are the last source row ("clamped")."""
    y0, _ = axis_taps(src_h, dst_h)
    y1 = np.minimum(y0 + 1, src_h - 1)
    first = np.arange(dst_h) % RESIZE_ROWS == 0
    prev0, prev1 = np.concatenate([[-1], y0[:-1]]), np.concatenate([[-1], y1[:-1]])
    return {"reuse": ~first & (y0 == prev1), "repeat": ~first & (y0 == prev0), "clamped": (y1 == y0) & (y0 == src_h - 1),
            "first": first}


# (src, dst, reason). Horizontal cases run on a 9-row source resized to 7 rows.
RESIZE_H_ROWS = (9, 7)
RESIZE_H = [
    # narrow sources: below 16 columns there is no 16-byte load to take
    (1, 1, "narrow: one pixel"), (1, 5, "narrow: one pixel, replicated"), (2, 98, "narrow: two pixels, upscale by 49"),
    (3, 17, "narrow: upscale"), (15, 4, "narrow: widest source below 16, one thread"), (15, 15, "narrow: identity"),
    (15, 14, "narrow: the detector's second level of a 15-column frame"),
    (16, 3, "first width with the 16-byte load: start clamps to column 0, three columns and a padded one"), (16, 4, "16 columns, start clamps to 0"),
    (17, 4, "start = min(x0, 1)"), (16, 16, "16 columns, identity: every thread loads from column 0"),
    # around ratio 4.6, where the 8 bytes of a thread stop fitting 16: one wavefront holds threads of both load paths
    (640, 140, "all wide: ratio 4.57, the largest spans that still fit 16 bytes"), (640, 137, "mixed load paths, ratio 4.67: one thread of 35 not wide"),
    (640, 135, "mixed load paths, ratio 4.74"), (640, 130, "mixed load paths, ratio 4.92: 8 threads of 33 wide"),
    (1000, 200, "all byte loads in a wide source: ratio 5, every span is 17 bytes"), (333, 70, "mixed load paths, ratio 4.76"),
    # a tap weight of exactly 256
    (11, 9, "weight 256"), (13, 5, "weight 256"), (18, 10, "weight 256"), (15, 13, "weight 256"),
    # scale = src / dst instead of 1 / (dst / src) changes a pixel
    (391, 256, "order-sensitive"), (393, 256, "order-sensitive"), (415, 256, "order-sensitive"), (417, 256, "order-sensitive"),
    # destination widths around the quad (4 columns per thread) and the 256-column block
    (1100, 1, "one column"), (1100, 2, "half a quad"), (1100, 3, "quad minus one"), (1100, 4, "one quad"), (1100, 5, "quad plus one"),
    (1100, 255, "block minus one"), (1100, 256, "one block"), (1100, 257, "block plus one"), (1100, 1021, "four blocks minus three"),
    (1100, 1024, "four blocks"), (1100, 1025, "four blocks plus one"),
    # upscales: the C ABI accepts them, no pyramid produces them
    (16, 64, "upscale by 4"), (17, 40, "upscale"), (24, 97, "upscale, odd width"), (64, 65, "upscale by one column"),
    (100, 257, "upscale over a block edge"), (3, 1025, "upscale by 342: every thread of four blocks reads the same 3 bytes"),
]

# (src, dst, reason, expected row census). Vertical cases run on a 40-column source resized to 33 columns.
RESIZE_V_COLS = (40, 33)
RESIZE_V = [
    (1, 1, "one row", None), (1, 9, "one row, replicated over two bands", None), (2, 17, "two rows over three bands", None),
    (9, 7, "one band, short", None), (9, 8, "exactly one band", None), (9, 9, "one row into the second band", None),
    (33, 31, "4-band block minus one row", None), (33, 32, "exactly one block of 4 bands", None), (33, 33, "one row into the next block", None),
    (100, 7, "ratio 14, short band", None), (100, 8, "ratio 12.5, one band", None), (100, 9, "ratio 11, second band", None),
    (48, 47, "every row reuses the cached source row", "reuse"),
    (70, 33, "no row reuses it", "no reuse"),
    (64, 200, "upscale: the upper row repeats, the bottom rows clamp", "clamped bottom"),
]

# (src_w, src_h, dst_w, dst_h, reason)
RESIZE_BOTH = [
    (101, 57, 33, 19, "both axes, odd sizes"), (17, 9, 40, 31, "both axes, upscale"),
    (1920, 1080, 417, 235, "Full-HD at ratio 4.6: many blocks along both axes, every thread on the 16-byte load"),
]


def resize_cases():
    """Every resize case as (id, src_w, src_h, dst_w, dst_h)."""
    out = [("h_%d_to_%d" % (s, d), s, RESIZE_H_ROWS[0], d, RESIZE_H_ROWS[1]) for s, d, _ in RESIZE_H]
    out += [("v_%d_to_%d" % (s, d), RESIZE_V_COLS[0], s, RESIZE_V_COLS[1], d) for s, d, _, _ in RESIZE_V]
    out += [("%dx%d_to_%dx%d" % c[:4],) + c[:4] for c in RESIZE_BOTH]
    return out


@functools.lru_cache(maxsize=None)
def resize_case_images(sw, sh):
    return images(sw, sh, 1000 * sw + sh)


# ------------------------------------------------------------------------------------------------ tilted integral
def tilted_witness(img):
    """OpenCV's tilted integral from its definition: tilted(Y, X) = sum of p(y, x) over y < Y, |x - X + 1| <= Y - y - 1.
    Row y contributes the pixels of columns [X - Y + y, X + Y - y - 2] clipped to the image: a difference of that row's
    plain prefix sums. No recurrence, no diagonals."""
    h, w = img.shape
    pre = np.zeros((h, w + 1), np.int64)
    pre[:, 1:] = img.astype(np.int64).cumsum(1)
    X = np.arange(w + 1)[None, :]
    out = np.zeros((h + 1, w + 1), np.int64)
    for Y in range(1, h + 1):
        y = np.arange(Y)[:, None]
        lo = np.clip(X - Y + y, 0, w)
        hi = np.clip(X + Y - y - 1, 0, w)  # one past the last column
        rows = np.broadcast_to(y, lo.shape)
        out[Y] = np.where(hi > lo, pre[rows, hi] - pre[rows, lo], 0).sum(0)
    return (out & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def tilted_literal(img):
    """The same definition as four loops over single pixels (only for small images: it checks the fast form)."""
    h, w = img.shape
    out = np.zeros((h + 1, w + 1), np.int64)
    for Y in range(h + 1):
        for X in range(w + 1):
            acc = 0
            for y in range(Y):
                for x in range(w):
                    if abs(x - X + 1) <= Y - y - 1:
                        acc += int(img[y, x])
            out[Y, X] = acc
    return out.astype(np.int32)


TILTED_LITERAL_SIZES = [(1, 1), (3, 5), (7, 2), (13, 9), (20, 17), (5, 1), (1, 6), (2, 2)]  # (w, h)

TSEG = 64  # rows per segment of the tilted kernels; a k_diag_sums thread walks 4 diagonals, a group 256; k_tilted_cols: 64 columns


def _tilted_cases():
    out = [(w, h, "width %d (4-diagonal thread, 64-column group) x height %d (64-row segment)" % (w, h))
           for w in (1, 2, 3, 4, 5, 62, 63, 64, 65) for h in (1, 2, 63, 64, 65, 66)]
    out += [(61, h, "segments above the second: %d rows" % h) for h in (127, 128, 129, 200)]
    for n in (255, 256, 257, 511, 512, 513):
        out.append((6, n + 1 - 6, "%d diagonals (256 per group), tall" % n))
        out.append((n + 1 - 3, 3, "%d diagonals (256 per group), wide" % n))
    out.append((1000, 37, "wide: 16 column groups, one segment"))
    return out


TILTED = _tilted_cases()  # (w, h, reason)


@functools.lru_cache(maxsize=None)
def tilted_case_images(w, h):
    return images(w, h, 7000 + 1000 * w + h)


# ------------------------------------------------------------------------------------------------ LBP code
def _box_sums(samples, w, h):
    """[n, H - h + 1, W - w + 1]: the sum of the h x w pixels whose top-left corner is (y, x), by adding shifted slices."""
    n, H, W = samples.shape
    s = samples.astype(np.int64)
    out = np.zeros((n, H - h + 1, W - w + 1), np.int64)
    for dy in range(h):
        for dx in range(w):
            out += s[:, dy:dy + H - h + 1, dx:dx + W - w + 1]
    return out


# bit value -> (cell row, cell column) of the 3x3 block: 128, 64, 32 the top row left to right, 16 middle right,
# 8, 4, 2 the bottom row right to left, 1 middle left
LBP_BITS = [(128, 0, 0), (64, 0, 1), (32, 0, 2), (16, 1, 2), (8, 2, 2), (4, 2, 1), (2, 2, 0), (1, 1, 0)]


def lbp_cells(samples, rects):
    """centre [F, n] and neighbours [8, F, n] (in LBP_BITS order): sums of the pixels of each cell, no integral image.
    rects: (x, y, w, h) of the top-left cell of every feature."""
    rects = np.asarray(rects, np.int64)
    F, n = len(rects), len(samples)
    centre = np.zeros((F, n), np.int64)
    neigh = np.zeros((8, F, n), np.int64)
    for (w, h) in sorted({(int(r[2]), int(r[3])) for r in rects}):
        sel = np.nonzero((rects[:, 2] == w) & (rects[:, 3] == h))[0]
        box = _box_sums(samples, w, h)
        x, y = rects[sel, 0], rects[sel, 1]
        centre[sel] = box[:, y + h, x + w].T
        for b, (_, r, c) in enumerate(LBP_BITS):
            neigh[b, sel] = box[:, y + r * h, x + c * w].T
    return centre, neigh


def lbp_witness(samples, rects):
    """[F, n] LBP codes: a bit is set where the neighbour cell's sum >= the centre cell's."""
    centre, neigh = lbp_cells(samples, rects)
    code = np.zeros(centre.shape, np.int64)
    for b, (bit, _, _) in enumerate(LBP_BITS):
        code += bit * (neigh[b] >= centre)
    return code


def lbp_comparison_shares(samples, rects):
    """(ties, greater, less) as shares: ties of all neighbour-to-centre comparisons, the other two of the non-tied ones."""
    centre, neigh = lbp_cells(samples, rects)
    tie, gt = (neigh == centre[None]).sum(), (neigh > centre[None]).sum()
    lt = neigh.size - tie - gt
    return tie / neigh.size, gt / max(gt + lt, 1), lt / max(gt + lt, 1)


def lbp_catalog_witness(W, H):
    """Every 3x3-cell block that fits a W x H window, in the trainer's order (x, then y, then cell width, then height)."""
    return np.array([(x, y, w, h) for x in range(W) for y in range(H) for w in range(1, W // 3 + 1) for h in range(1, H // 3 + 1)
                     if x + 3 * w <= W and y + 3 * h <= H], np.int32)


LBP_WINDOWS = [(24, 24), (20, 34)]  # (W, H)
LBP_SAMPLES = 16


def _blocks(W, H, n, side, levels, seed):
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, len(levels), (n, (H + side - 1) // side, (W + side - 1) // side))
    return np.asarray(levels, np.uint8)[np.kron(coarse, np.ones((side, side), np.int64))[:, :H, :W]]


@functools.lru_cache(maxsize=None)
def lbp_samples(W, H):
    """(name, [16, H, W] samples): uniform noise (ties are rare), 4x4 blocks at three gray levels and 2x2 blocks at two
    (about three in ten comparisons tie: `>=` against `>` decides the bit)."""
    return [("noise", np.random.default_rng(300 + W).integers(0, 256, (LBP_SAMPLES, H, W), dtype=np.uint8)),
            ("blocks4x4_3levels", _blocks(W, H, LBP_SAMPLES, 4, (40, 128, 215), 301 + W)),
            ("blocks2x2_2levels", _blocks(W, H, LBP_SAMPLES, 2, (60, 190), 302 + W))]
