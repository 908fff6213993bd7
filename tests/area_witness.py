"""numpy restatement of the createsamples tool's -info mode (tools/createsamples/utility.cpp:1125-1232): every annotated
rectangle cut out of its image and resized to the window, INTER_AREA when the rectangle is at least the window on both axes
and INTER_LINEAR_EXACT otherwise. Written from the arithmetic DESIGN.md 4.15 lists (cv::resize of OpenCV 4.6.0 for 8-bit
single-channel images), not from the product's code: the table in Python floats (doubles, one rounding per operation), the
sums in np.float32 in the stated order. The bilinear branch is tests/sample_witness.py's exact resize on the rectangle alone.

area_pixel is the definition, one window pixel with np.float32 scalars; resize_area computes the same sums for a whole window
with float32 vectors over the rows (the rows of a window column are independent until they are combined) and is what the
tests compare against. That the two agree is itself tested on the host."""
import math

import numpy as np

from tests import sample_witness as W

F = np.float32
DBL_EPSILON = 2.220446049250313e-16
SLIVER = 1e-3  # a partial source pixel narrower than this is left out of the table


def axis(ssize, dsize):
    """(scale, iscale, integer) of one axis: scale = 1 / (dsize / ssize), the ratio is integer iff |scale - iscale| < DBL_EPSILON."""
    scale = 1.0 / (float(dsize) / float(ssize))
    iscale = int(scale)
    return scale, iscale, abs(scale - iscale) < DBL_EPSILON


def area_tab(ssize, dsize, scale=None, margins=None, dropped=None):
    """computeResizeAreaTab: [(d, source index, float32 alpha)] in table order. margins (a list) receives how far each of the
    two `> 1e-3` comparisons of every d is from its threshold; dropped (a list) per d the weight of the partial pixels left out."""
    scale = axis(ssize, dsize)[0] if scale is None else scale
    tab = []
    for d in range(dsize):
        fsx1 = d * scale
        fsx2 = fsx1 + scale
        cell = min(scale, ssize - fsx1)
        sx1, sx2 = math.ceil(fsx1), math.floor(fsx2)
        sx2 = min(sx2, ssize - 1)
        sx1 = min(sx1, sx2)
        lost = 0.0
        if sx1 - fsx1 > SLIVER:
            tab.append((d, sx1 - 1, F((sx1 - fsx1) / cell)))
        else:
            lost += max(sx1 - fsx1, 0.0) / cell
        for sx in range(sx1, sx2):
            tab.append((d, sx, F(1.0 / cell)))
        if fsx2 - sx2 > SLIVER:
            tab.append((d, sx2, F(min(min(fsx2 - sx2, 1.0), cell) / cell)))
        else:
            lost += max(fsx2 - sx2, 0.0) / cell
        if margins is not None:
            margins += [sx1 - fsx1 - SLIVER, fsx2 - sx2 - SLIVER]
        if dropped is not None:
            dropped.append(lost)
    assert len(tab) <= 2 * ssize
    return tab


def _saturate_round(v):
    """saturate_cast<uchar>(cvRound(v)) of float32 values: half to even, then clamped."""
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def is_fast(sw, sh, dw, dh):
    return axis(sw, dw)[2] and axis(sh, dh)[2]


def check_fast_sum(kx, ky):
    if kx * ky * 255 >= 2 ** 31:
        raise ValueError("the integer-ratio block sum passes 2^31")


def area_pixel(S, dw, dh, dx, dy):
    """One pixel of resize(S, Size(dw, dh), INTER_AREA), sh >= dh and sw >= dw, with np.float32 scalars in the stated order."""
    sh, sw = S.shape
    if (sw, sh) == (dw, dh):
        return int(S[dy, dx])
    (scale_x, kx, int_x), (scale_y, ky, int_y) = axis(sw, dw), axis(sh, dh)
    if int_x and int_y:
        check_fast_sum(kx, ky)
        block = S[dy * ky:(dy + 1) * ky, dx * kx:(dx + 1) * kx]
        assert block.shape == (ky, kx)
        total = int(block.astype(np.int64).sum())
        if kx == 2 and ky == 2:
            return (total + 2) >> 2
        return int(_saturate_round(F(total) * (F(1.0) / F(kx * ky))))
    xs = [(s, a) for d, s, a in area_tab(sw, dw, scale_x) if d == dx]
    ys = [(s, b) for d, s, b in area_tab(sh, dh, scale_y) if d == dy]
    total = None
    for sy, beta in ys:
        buf = F(0.0)
        for sx, alpha in xs:
            buf = buf + F(S[sy, sx]) * alpha
        total = beta * buf if total is None else total + beta * buf
    assert total.dtype == np.float32
    return int(_saturate_round(total))


def resize_area(S, dw, dh):
    """resize(S, Size(dw, dh), INTER_AREA) of an (sh, sw) uint8 image with sh >= dh and sw >= dw."""
    S = np.asarray(S)
    sh, sw = S.shape
    assert S.dtype == np.uint8 and 1 <= dw <= sw and 1 <= dh <= sh
    if (sw, sh) == (dw, dh):
        return S.copy()
    (scale_x, kx, int_x), (scale_y, ky, int_y) = axis(sw, dw), axis(sh, dh)
    if int_x and int_y:
        check_fast_sum(kx, ky)
        assert (sw, sh) == (kx * dw, ky * dh)
        sums = S.astype(np.int64).reshape(dh, ky, dw, kx).sum(axis=(1, 3))
        if kx == 2 and ky == 2:
            return ((sums + 2) >> 2).astype(np.uint8)
        return _saturate_round(sums.astype(np.float32) * (F(1.0) / F(kx * ky)))
    Sf = S.astype(np.float32)
    buf = np.zeros((sh, dw), np.float32)  # buf[sy, dx]: the left-to-right sum over dx's entries, for every source row
    for d, s, alpha in area_tab(sw, dw, scale_x):
        buf[:, d] = buf[:, d] + Sf[:, s] * alpha
    out = np.zeros((dh, dw), np.float32)
    started = [False] * dh
    for d, s, beta in area_tab(sh, dh, scale_y):
        out[d] = out[d] + beta * buf[s] if started[d] else beta * buf[s]
        started[d] = True
    assert all(started) and out.dtype == np.float32
    return _saturate_round(out)


def uses_area(w, h, dw, dh):
    """The tool's choice (utility.cpp:1207): width >= winwidth && height >= winheight ? INTER_AREA : INTER_LINEAR_EXACT."""
    return w >= dw and h >= dh


def sample(img, rect, dw, dh):
    """resize(src(Rect(x, y, w, h)), sample, Size(dw, dh), ...): the rectangle alone is the source."""
    x, y, w, h = (int(v) for v in rect)
    ih, iw = img.shape
    if w < 1 or h < 1 or x < 0 or y < 0 or x + w > iw or y + h > ih:
        raise ValueError(f"rectangle {w} x {h} at ({x}, {y}) leaves its {iw} x {ih} image")
    crop = img[y:y + h, x:x + w]
    if uses_area(w, h, dw, dh):
        return resize_area(crop, dw, dh)
    return W.resize_linear_exact(crop, dw, dh)


def samples(images, records, dw, dh):
    """records: (image, x, y, w, h). The (n, dh, dw) stack cc_samples_from_info must give."""
    out = np.zeros((len(records), dh, dw), np.uint8)
    for k, (i, x, y, w, h) in enumerate(records):
        if not 0 <= i < len(images):
            raise ValueError(f"record {k}: image {i} of {len(images)}")
        out[k] = sample(images[i], (x, y, w, h), dw, dh)
    return out
