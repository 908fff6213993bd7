"""numpy restatement of the reference's HOG evaluator (CvHOGEvaluator), the yardstick of the HOG tests.

Sources: traincascade/lib/include/HOGfeatures.h:84-112 (operator(), Feature::calc), traincascade/lib/src/HOGfeatures.cpp
:67-106 (catalog), :115-131 (cells), :163-256 (integralHistogram), and OpenCV 4.6.0's cv::cartToPolar (hal::magnitude32f,
hal::fastAtan32f in core/src/mathfuncs_core.simd.hpp) and cv::integral for float input, restated (OpenCV is not part of
the reference tree; see DESIGN.md, "HOG").

Every value is float32 and every operation is rounded where the reference rounds it: numpy's float32 +, -, *, / and
sqrt are the correctly rounded IEEE operations, np.add.accumulate adds strictly in order (unlike np.sum, which is
pairwise), and the polynomial's fused multiply-adds go through fma32, an exact emulation (no math.fma on Python 3.10).
"""
from __future__ import annotations

import math
import sys

import numpy as np

f32 = np.float32
N_BINS, N_CELLS = 9, 4
FEATURE_SIZE = N_BINS * N_CELLS  # HOGfeatures.cpp:13

# hal::fastAtan32f (mathfuncs_core.simd.hpp): atan2_p1..p7 = coefficient * (float)(180 / CV_PI), products in float
_DEG = f32(180 / math.pi)
P1 = f32(f32(0.9997878412794807) * _DEG)
P3 = f32(f32(-0.3258083974640975) * _DEG)
P5 = f32(f32(0.1555786518463281) * _DEG)
P7 = f32(f32(-0.04432655554792128) * _DEG)
EPS = f32(sys.float_info.epsilon)      # (float)DBL_EPSILON
RAD = f32(math.pi / 180)               # fastAtan32f's scale when angleInDegrees is false
ANGLE_SCALE = f32(N_BINS / math.pi)    # HOGfeatures.cpp:204: (float)(nbins / CV_PI)


def fma32(a, b, c):
    """Correctly rounded float32 a * b + c, elementwise. The float64 product of two float32 values is exact (48 bits);
    s = fl64(p + c) with TwoSum's exact error e. Rounding s to float32 is correct unless s lies exactly on a float32
    rounding boundary (a tie) while e != 0: then the exact sum lies on the side of the tie that e points to."""
    a, b, c = (np.asarray(v, np.float32) for v in (a, b, c))
    p = a.astype(np.float64) * b.astype(np.float64)
    cd = c.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        s = p + cd
        bb = s - p
        err = (p - (s - bb)) + (cd - bb)
        r = s.astype(np.float32)
        up = np.nextafter(s, np.inf).astype(np.float32)
        dn = np.nextafter(s, -np.inf).astype(np.float32)
    tie = up != dn
    r = np.where(tie & (err > 0), up, r)
    r = np.where(tie & (err < 0), dn, r)
    return r.astype(np.float32)


def fma32_unfused(a, b, c):
    """a * b + c with the product rounded first (the SSE2-only build and the scalar tail)."""
    a, b, c = (np.asarray(v, np.float32) for v in (a, b, c))
    return (a * b + c).astype(np.float32)


def grad_bin(dx, dy, fused=True):
    """(magnitude, bin) of integer central differences dx, dy (HOGfeatures.cpp:209-231)."""
    fma = fma32 if fused else fma32_unfused
    fx = np.asarray(dx).astype(np.float32)
    fy = np.asarray(dy).astype(np.float32)
    mag = np.sqrt(fx * fx + fy * fy)  # hal::magnitude32f; the sum is exact in float
    ax, ay = np.abs(fx), np.abs(fy)
    c = np.minimum(ax, ay) / (np.maximum(ax, ay) + EPS)
    cc = c * c
    a = fma(fma(fma(cc, P7, P5), cc, P3), cc, P1) * c
    a = np.where(ax < ay, f32(90) - a, a)
    a = np.where(fx < 0, f32(180) - a, a)
    a = np.where(fy < 0, f32(360) - a, a)
    angle = (a * RAD).astype(np.float32)
    t = angle * ANGLE_SCALE - f32(0.5)
    b = np.floor(t).astype(np.int32)  # cvFloor
    b = np.where(b < 0, b + N_BINS, np.where(b >= N_BINS, b - N_BINS, b))
    return mag.astype(np.float32), b.astype(np.uint8)


def bin_table(fused=True):
    """Bin and magnitude of every (dx, dy) in [-255, 255]^2, pair (dx, dy) at (dy + 255) * 511 + dx + 255."""
    dy, dx = np.mgrid[-255:256, -255:256]
    mag, b = grad_bin(dx.ravel(), dy.ravel(), fused)
    return b, mag


def catalog(W, H):
    """Blocks as rows (x, y, cell w, cell h) in the reference's order (HOGfeatures.cpp:67-106): t = 8, 16, ... while
    t <= W / 2; shapes (cells t x t, t x 2t, 2t x t); x outer, y inner, step 4."""
    out = []
    t = 8
    while t <= W // 2:
        for cw, ch in ((t, t), (t, 2 * t), (2 * t, t)):
            for x in range(0, W - 2 * cw + 1, 4):
                for y in range(0, H - 2 * ch + 1, 4):
                    out.append((x, y, cw, ch))
        t += 8
    return np.array(out, np.int32).reshape(-1, 4)


def cells(block):
    """Cells 0..3 (top-left, top-right, bottom-left, bottom-right) of a block as (x, y, w, h) (HOGfeatures.cpp:120-131)."""
    x, y, cw, ch = (int(v) for v in block)
    return np.array([(x, y, cw, ch), (x + cw, y, cw, ch), (x, y + ch, cw, ch), (x + cw, y + ch, cw, ch)], np.int32)


def set_image(img):
    """(hist[9][H+1][W+1], norm[H+1][W+1]) of one window (HOGfeatures.cpp:163-256)."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    xs = np.arange(W)
    ys = np.arange(H)
    xl, xr = np.maximum(xs - 1, 0), np.minimum(xs + 1, W - 1)  # BORDER_REPLICATE
    yu, yd = np.maximum(ys - 1, 0), np.minimum(ys + 1, H - 1)
    im = img.astype(np.int32)
    dx = im[:, xr] - im[:, xl]
    dy = im[yd, :] - im[yu, :]
    mag, b = grad_bin(dx, dy)
    planes = np.zeros((10, H + 1, W + 1), np.float32)
    for c in range(10):
        m = mag if c == 9 else np.where(b == c, mag, f32(0))
        rows = np.add.accumulate(m, axis=1, dtype=np.float32)             # s += mag[x], left to right
        planes[c, 1:, 1:] = np.add.accumulate(rows, axis=0, dtype=np.float32)  # sum[y+1][x+1] = sum[y][x+1] + s
    return planes[:9], planes[9]


def set_images(imgs):
    """Stacked set_image: (hist[n][9][H+1][W+1], norm[n][H+1][W+1])."""
    hs, ns = zip(*(set_image(im) for im in imgs))
    return np.stack(hs), np.stack(ns)


def eval_vars(blocks, hist, norm, vi_begin=0, vi_end=None):
    """values[vi - vi_begin][s] for variables [vi_begin, vi_end) (HOGfeatures.h:84-112); hist [n][9][H+1][W+1]."""
    nb = len(blocks)
    vi_end = nb * FEATURE_SIZE if vi_end is None else vi_end
    n = hist.shape[0]
    out = np.empty((vi_end - vi_begin, n), np.float32)
    for vi in range(vi_begin, vi_end):
        x, y, cw, ch = (int(v) for v in blocks[vi // FEATURE_SIZE])
        comp = vi % FEATURE_SIZE
        cell, b = comp // N_BINS, comp % N_BINS
        cx, cy = x + (cell & 1) * cw, y + (cell >> 1) * ch
        h = hist[:, b]
        res = ((h[:, cy, cx] - h[:, cy, cx + cw]) - h[:, cy + ch, cx]) + h[:, cy + ch, cx + cw]
        nf = ((norm[:, y, x] - norm[:, y, x + 2 * cw]) - norm[:, y + 2 * ch, x]) + norm[:, y + 2 * ch, x + 2 * cw]
        with np.errstate(divide="ignore", invalid="ignore"):
            out[vi - vi_begin] = np.where(res > f32(0.001), res / (nf + f32(0.001)), f32(0))
    return out
