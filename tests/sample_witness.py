"""numpy restatement of the reference's sample synthesis (tools/createsamples/utility.cpp: icvStartSampleDistortion,
icvRandomQuad, cvGetPerspectiveTransform, cvWarpPerspective, icvPlaceDistortedSample, the background reader), written
from the arithmetic DESIGN.md lists, not from the product's code. Everything is double precision with one rounding per
operation (numpy never fuses a multiply with an add); the roi arithmetic is float32 where the reference's is.

Two forms of one sample:
  dense   builds the (w + 2 (w/2)) x (h + 2 (h/2)) canvas, blurs the whole mask and resizes the roi, as the reference does;
  sparse  evaluates the warp only at the canvas pixels the resize reads (and, for the mask, their 3x3 blur support).
"""
import math

import numpy as np

RANDOM_INVERT = 0x7FFFFFFF
RAND_MAX = 2147483647
INT_MIN = -2 ** 31


class RNG:
    """cv::RNG: multiply-with-carry, doubles from two draws."""

    def __init__(self, seed=12345):
        self.state = (seed & 0xFFFFFFFFFFFFFFFF) or 0xFFFFFFFF

    def next(self):
        self.state = ((self.state & 0xFFFFFFFF) * 4164903690 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        return self.state & 0xFFFFFFFF

    def uniform_int(self, a, b):
        if a == b:
            return a
        v = (self.next() % ((b - a) & 0xFFFFFFFF) + a) & 0xFFFFFFFF
        return v - (1 << 32) if v >= 1 << 31 else v

    def uniform(self, a, b):
        t = self.next()
        d = float((t << 32) | self.next()) * 5.4210108624275221700372640043497e-20
        return d * (b - a) + a


def cv_round(v):
    """cvRound of a double: half to even; what does not fit an int32 converts to INT_MIN (cvtsd2si)."""
    if not math.isfinite(v):
        return INT_MIN
    r = round(v)
    return r if -2 ** 31 <= r < 2 ** 31 else INT_MIN


def rodrigues(r):
    x, y, z = r
    theta = math.sqrt(x * x + y * y + z * z)
    if theta < 2.220446049250313e-16:
        return [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    c, s = math.cos(theta), math.sin(theta)
    c1 = 1.0 - c
    it = 1.0 / theta
    v = [x * it, y * it, z * it]
    rx = [[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]]
    return [[(c * (1.0 if i == j else 0.0) + c1 * (v[i] * v[j])) + s * rx[i][j] for j in range(3)] for i in range(3)]


def random_quad(rng, w, h, maxx, maxy, maxz):
    rx = rng.uniform(-maxx, maxx)
    ry = (maxy - abs(rx)) * rng.uniform(-1.0, 1.0)
    rz = rng.uniform(-maxz, maxz)
    d = (3.0 + 1.0 * rng.uniform(-1.0, 1.0)) * w
    R = rodrigues((rx, ry, rz))
    hw, hh = 0.5 * w, 0.5 * h
    quad = []
    for px, py in ((-hw, -hh), (hw, -hh), (hw, hh), (-hw, hh)):
        v = [(R[i][0] * px + R[i][1] * py) + R[i][2] * 0.0 for i in range(3)]
        quad.append([v[0] * d / (d + v[2]) + hw, v[1] * d / (d + v[2]) + hh])
    return quad


def perspective_coeffs(w, h, quad):
    """cvGetPerspectiveTransform: the 8x8 system solved by partial-pivot LU (cv::hal::LU64f)."""
    a = [[0.0] * 8 for _ in range(8)]
    b = [0.0] * 8
    for i in range(4):
        a[i][0], a[i][1], a[i][2] = quad[i][0], quad[i][1], 1.0
        a[i + 4][3], a[i + 4][4], a[i + 4][5] = quad[i][0], quad[i][1], 1.0
    u, v = w - 1, h - 1
    for i in (1, 2):
        a[i][6], a[i][7], b[i] = -quad[i][0] * u, -quad[i][1] * u, float(u)
    for i in (2, 3):
        a[i + 4][6], a[i + 4][7], b[i + 4] = -quad[i][0] * v, -quad[i][1] * v, float(v)
    m = 8
    for i in range(m):
        k = i
        for j in range(i + 1, m):
            if abs(a[j][i]) > abs(a[k][i]):
                k = j
        if abs(a[k][i]) < 2.220446049250313e-16 * 100:
            raise ValueError("singular system")
        if k != i:
            a[i], a[k] = a[k], a[i]
            b[i], b[k] = b[k], b[i]
        d = -1.0 / a[i][i]
        for j in range(i + 1, m):
            alpha = a[j][i] * d
            for kk in range(i + 1, m):
                a[j][kk] += alpha * a[i][kk]
            b[j] += alpha * b[i]
    for i in range(m - 1, -1, -1):
        s = b[i]
        for k in range(i + 1, m):
            s -= a[i][k] * b[k]
        b[i] = s / a[i][i]
    return b + [1.0]


def row_spans(quad, cols, rows):
    """The scanline walk of cvWarpPerspective: (rows, 2) int32 of ix_min, ix_max per destination row, (0, -1) where the
    walk never comes. Raises ValueError for a nonconvex or degenerate quad."""
    f64 = np.float64
    direction = 0
    for i in range(4):
        ni, pi = (i + 1) % 4, (i + 3) % 4
        d = (quad[i][0] - quad[pi][0]) * (quad[ni][1] - quad[i][1]) - (quad[i][1] - quad[pi][1]) * (quad[ni][0] - quad[i][0])
        cur = 1 if d > 0 else -1 if d < 0 else 0
        if direction == 0:
            direction = cur
        elif direction * cur < 0:
            direction = 0
            break
    if direction == 0:
        raise ValueError("Quadrangle is nonconvex or degenerated.")
    left = 0
    for i in range(1, 4):
        if quad[i][1] < quad[left][1] or (quad[i][1] == quad[left][1] and quad[i][0] < quad[left][0]):
            left = i
    if direction > 0:
        q = [quad[i] for i in range(left, 4)] + [quad[i] for i in range(left)]
    else:
        q = [quad[i] for i in range(left, -1, -1)] + [quad[i] for i in range(3, left, -1)]
    q = [[f64(p[0]), f64(p[1])] for p in q]
    spans = np.zeros((rows, 2), np.int32)
    spans[:, 1] = -1
    left = 0
    right = 1 if q[0][1] == q[1][1] else 0
    next_left, next_right = 3, right + 1
    y_min = q[left][1] - 1

    def edge(a, b):
        with np.errstate(all="ignore"):
            return ((q[a][0] - q[b][0]) / (q[a][1] - q[b][1]),
                    (q[a][1] * q[b][0] - q[a][0] * q[b][1]) / (q[a][1] - q[b][1]))

    k_left, b_left = edge(left, next_left)
    k_right, b_right = edge(right, next_right)
    while True:
        y_max = min(q[next_left][1], q[next_right][1])
        iy_min = max(cv_round(float(y_min)), 0) + 1
        iy_max = min(cv_round(float(y_max)), rows - 1)
        with np.errstate(all="ignore"):
            x_min = k_left * iy_min + b_left
            x_max = k_right * iy_min + b_right
            for y in range(iy_min, iy_max + 1):
                spans[y, 0] = max(cv_round(float(x_min)), 0)
                spans[y, 1] = min(cv_round(float(x_max)), cols - 1)
                x_min = x_min + k_left
                x_max = x_max + k_right
        if next_left == next_right or (next_left + 1 == next_right and q[next_left][1] == q[next_right][1]):
            break
        if y_max == q[next_left][1]:
            left = next_left
            next_left = left - 1
            k_left, b_left = edge(left, next_left)
        if y_max == q[next_right][1]:
            right = next_right
            next_right = right + 1
            k_right, b_right = edge(right, next_right)
        y_min = y_max
    return spans


def warp_at(src, c, X, Y):
    """The warped value at destination pixels (X, Y) (integer arrays of one shape) that lie inside their row's span."""
    sh, sw = src.shape
    x, y = X.astype(np.float64), Y.astype(np.float64)
    with np.errstate(all="ignore"):
        div = (c[6] * x + c[7] * y) + c[8]
        sx = ((c[0] * x + c[1] * y) + c[2]) / div
        sy = ((c[3] * x + c[4] * y) + c[5]) / div
    ix, iy = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    dx, dy = sx - ix, sy - iy

    def tap(ok, yy, xx):
        return np.where(ok, src[np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)].astype(np.int64), 0)

    x_in, x1_in = (ix >= 0) & (ix < sw), (ix >= -1) & (ix + 1 < sw)
    y_in, y1_in = (iy >= 0) & (iy < sh), (iy >= -1) & (iy + 1 < sh)
    i00, i10 = tap(x_in & y_in, iy, ix), tap(x1_in & y_in, iy, ix + 1)
    i01, i11 = tap(x_in & y1_in, iy + 1, ix), tap(x1_in & y1_in, iy + 1, ix + 1)
    i0 = i00 + (i10 - i00) * dx
    i1 = i01 + (i11 - i01) * dx
    return (i0 + (i1 - i0) * dy).astype(np.int64).astype(np.uint8)


def warp_perspective(src, dst, quad):
    """cvWarpPerspective into the caller's canvas (dense: row by row over the spans)."""
    c = perspective_coeffs(src.shape[1], src.shape[0], quad)
    spans = row_spans(quad, dst.shape[1], dst.shape[0])
    for y in range(dst.shape[0]):
        a, b = int(spans[y, 0]), int(spans[y, 1])
        if a <= b:
            X = np.arange(a, b + 1)
            dst[y, a:b + 1] = warp_at(src, c, X, np.full_like(X, y))
    return dst


def start_distortion(img, bgcolor, bgthreshold):
    """icvStartSampleDistortion: (border-extended source, mask)."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    s = img.astype(np.int64)
    mask = np.where((bgcolor - bgthreshold <= s) & (s <= bgcolor + bgthreshold), 0, 255).astype(np.uint8)
    lo = np.pad(img, 1, constant_values=255)   # a 3x3 minimum / maximum that leaves pixels outside the image out
    hi = np.pad(img, 1, constant_values=0)
    er = np.min([lo[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], axis=0).astype(np.int64)
    di = np.max([hi[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], axis=0).astype(np.int64)
    de, dd = (bgcolor - er) & 0xFF, (di - bgcolor) & 0xFF
    out = s.copy()
    bg = mask == 0
    t1 = bg & (de >= dd) & (de > bgthreshold)
    out[t1] = er[t1]
    t2 = bg & (dd > de) & (dd > bgthreshold)
    out[t2] = di[t2]
    return out.astype(np.uint8), mask


def linear_exact_taps(src, dst):
    """INTER_LINEAR_EXACT taps of one axis: left tap and the 8.8 weight of the right one."""
    scale = 1.0 / (float(dst) / float(src))
    ofs, w1 = np.zeros(dst, np.int64), np.zeros(dst, np.int64)
    for d in range(dst):
        f = scale * (d + 0.5) - 0.5
        i = math.floor(f)
        if 0 <= i < src - 1:
            ofs[d], w1[d] = i, round((f - i) * 256.0)
        else:
            ofs[d] = src - 1 if (i >= 0 and src > 1) else 0
    return ofs, w1


def _resize_from(fetch, rw, rh, out_w, out_h):
    """The exact bilinear resize of an rw x rh image given by fetch(rows, cols) -> 2-D values."""
    xo, xw = linear_exact_taps(rw, out_w)
    yo, yw = linear_exact_taps(rh, out_h)
    x1, y1 = np.minimum(xo + 1, rw - 1), np.minimum(yo + 1, rh - 1)
    rows, cols = np.concatenate([yo, y1]), np.concatenate([xo, x1])
    v = fetch(rows, cols).astype(np.int64)
    hz = (256 - xw)[None, :] * v[:, :out_w] + xw[None, :] * v[:, out_w:]
    return (((256 - yw)[:, None] * hz[:out_h] + yw[:, None] * hz[out_h:] + (1 << 15)) >> 16).astype(np.uint8)


def resize_linear_exact(img, out_w, out_h):
    return _resize_from(lambda r, c: img[np.ix_(r, c)], img.shape[1], img.shape[0], out_w, out_h)


def gaussian3(img):
    """cv::GaussianBlur 3x3 of 8-bit pixels: 1-2-1 both ways in fixed point, (S + 8) >> 4, BORDER_REFLECT_101."""
    p = np.pad(img.astype(np.int64), 1, mode="reflect")
    hz = p[:, :-2] + 2 * p[:, 1:-1] + p[:, 2:]
    return ((hz[:-2] + 2 * hz[1:-1] + hz[2:] + 8) >> 4).astype(np.uint8)


def _reflect(i, n):
    i = np.where(i < 0, -i, i)
    return np.clip(np.where(i >= n, 2 * n - 2 - i, i), 0, n - 1)


class Params:
    def __init__(self, bgcolor=0, bgthreshold=80, invert=0, maxintensitydev=40, maxxangle=1.1, maxyangle=1.1, maxzangle=0.5,
                 inscribe=0, maxshift=0.0, maxscale=0.0):
        self.bgcolor, self.bgthreshold, self.invert, self.maxintensitydev = bgcolor, bgthreshold, invert, maxintensitydev
        self.maxxangle, self.maxyangle, self.maxzangle = maxxangle, maxyangle, maxzangle
        self.inscribe, self.maxshift, self.maxscale = inscribe, maxshift, maxscale


class BgReader:
    """The tool's background reader (icvGetNextFromBackgroundData / icvGetBackgroundImage) over image SIZES: per window
    which image, at which size, from which origin."""

    def __init__(self, sizes, win_w, win_h):
        self.sizes, self.win_w, self.win_h = [(int(w), int(h)) for w, h in sizes], win_w, win_h
        self.round = 0
        self.have = False

    def _next_image(self, rng):
        f32 = np.float32
        found = False
        for _ in range(len(self.sizes)):
            rnd = self.round
            self.last = rng.uniform_int(0, RAND_MAX) % len(self.sizes)
            w, h = self.sizes[self.last]
            self.round = (self.round + self.last // len(self.sizes)) % (self.win_w * self.win_h)
            ox, oy = min(rnd % self.win_w, w - self.win_w), min(rnd // self.win_w, h - self.win_h)
            if ox >= 0 and oy >= 0:
                found = True
                break
        if not found:
            raise ValueError("no background image holds a window")
        self.off = self.pt = (ox, oy)
        self.scale = max(f32(f32(self.win_w) + f32(ox)) / f32(w), f32(f32(self.win_h) + f32(oy)) / f32(h))
        self.cur = (int(self.scale * f32(w) + f32(0.5)), int(self.scale * f32(h) + f32(0.5)))
        self.have = True

    def take(self, rng):
        """(image, width, height, x, y) of the next window; draws from rng when a new image is opened."""
        f32 = np.float32
        if not self.have:
            self._next_image(rng)
        res = (self.last, self.cur[0], self.cur[1], self.pt[0], self.pt[1])
        step = f32(0.5)
        if int(f32(self.pt[0]) + (f32(1.0) + step) * f32(self.win_w)) < self.cur[0]:
            self.pt = (self.pt[0] + int(step * f32(self.win_w)), self.pt[1])
        else:
            self.pt = (self.off[0], self.pt[1])
            if int(f32(self.pt[1]) + (f32(1.0) + step) * f32(self.win_h)) < self.cur[1]:
                self.pt = (self.pt[0], self.pt[1] + int(step * f32(self.win_h)))
            else:
                self.pt = (self.pt[0], self.off[1])
                self.scale = f32(self.scale * f32(1.4142135623730950488))
                if self.scale <= f32(1.0):
                    w, h = self.sizes[self.last]
                    self.cur = (int(self.scale * f32(w)), int(self.scale * f32(h)))
                else:
                    self._next_image(rng)
        return res


def plan(src_w, src_h, out_w, out_h, p, rng, n, bg=None):
    """Every draw and all sequential arithmetic of n samples: a list of dicts (quad, coeffs, spans, inverse, forecolordev,
    roi, bg)."""
    f32 = np.float32
    dx, dy = src_w // 2, src_h // 2
    cw, ch = src_w + 2 * dx, src_h + 2 * dy
    recs = []
    for _ in range(n):
        r = {}
        r["bg"] = bg.take(rng) if bg is not None else (-1, 0, 0, 0, 0)
        inverse = p.invert
        if p.invert == RANDOM_INVERT:
            inverse = rng.uniform_int(0, 2)
        quad = random_quad(rng, src_w, src_h, p.maxxangle, p.maxyangle, p.maxzangle)
        quad = [[q[0] + float(dx), q[1] + float(dy)] for q in quad]
        r["quad"] = quad
        r["coeffs"] = perspective_coeffs(src_w, src_h, quad)
        r["spans"] = row_spans(quad, cw, ch)
        cx, cy, cwid, chei = dx, dy, src_w, src_h
        if p.inscribe:
            cx = int(min(quad[0][0], quad[3][0]))
            cy = int(min(quad[0][1], quad[1][1]))
            cwid = int(max(quad[1][0], quad[2][0]) + 0.5) - cx
            chei = int(max(quad[2][1], quad[3][1]) + 0.5) - cy
        xshift = rng.uniform(0.0, p.maxshift)
        yshift = rng.uniform(0.0, p.maxshift)
        cx -= int(xshift * cwid)
        cy -= int(yshift * chei)
        cwid = int((1.0 + p.maxshift) * cwid)
        chei = int((1.0 + p.maxshift) * chei)
        randscale = rng.uniform(0.0, p.maxscale)
        cx -= int(0.5 * randscale * cwid)
        cy -= int(0.5 * randscale * chei)
        cwid = int((1.0 + randscale) * cwid)
        chei = int((1.0 + randscale) * chei)
        scale = max(f32(cwid) / f32(out_w), f32(chei) / f32(out_h))
        rx = int(f32(-0.5) * (scale * f32(out_w) - f32(cwid)) + f32(cx))
        ry = int(f32(-0.5) * (scale * f32(out_h) - f32(chei)) + f32(cy))
        rw, rh = int(scale * f32(out_w)), int(scale * f32(out_h))
        x0, y0, x1, y1 = max(rx, 0), max(ry, 0), min(rx + rw, cw), min(ry + rh, ch)
        if x1 <= x0 or y1 <= y0:
            raise ValueError("the sample's source rectangle misses the canvas")
        r["roi"] = (x0, y0, x1 - x0, y1 - y0)
        r["inverse"] = int(inverse)
        r["forecolordev"] = rng.uniform_int(-p.maxintensitydev, p.maxintensitydev)
        recs.append(r)
    return recs


def fill_byte(bgcolor):
    """The byte `Mat = Scalar(bgcolor)` stores (utility.cpp:607, :992): saturated, 300 -> 255 and -5 -> 0. The mask test and
    de / dd of start_distortion use the int itself."""
    return min(max(int(bgcolor), 0), 255)


def _blend(img, alpha, bg, forecolordev, inverse):
    t = np.clip(forecolordev + img.astype(np.int64), 0, 255)
    if inverse:
        t = t ^ 0xFF
    a = alpha.astype(np.int64)
    return ((t * a + (255 - a) * bg.astype(np.int64)) // 255).astype(np.uint8)


def render_dense(src, mask, bgcolor, rec, out_w, out_h, bg=None):
    h, w = src.shape
    cw, ch = w + 2 * (w // 2), h + 2 * (h // 2)
    img = np.full((ch, cw), fill_byte(bgcolor), np.uint8)
    mimg = np.zeros((ch, cw), np.uint8)
    for s, d in ((src, img), (mask, mimg)):
        for y in range(ch):
            a, b = int(rec["spans"][y, 0]), int(rec["spans"][y, 1])
            if a <= b:
                X = np.arange(a, b + 1)
                d[y, a:b + 1] = warp_at(s, rec["coeffs"], X, np.full_like(X, y))
    mimg = gaussian3(mimg)
    x, y, rw, rh = rec["roi"]
    bgw = np.full((out_h, out_w), fill_byte(bgcolor), np.uint8) if bg is None else bg
    return _blend(resize_linear_exact(img[y:y + rh, x:x + rw], out_w, out_h),
                  resize_linear_exact(mimg[y:y + rh, x:x + rw], out_w, out_h), bgw, rec["forecolordev"], rec["inverse"])


def render_sparse(src, mask, bgcolor, rec, out_w, out_h, bg=None):
    h, w = src.shape
    cw, ch = w + 2 * (w // 2), h + 2 * (h // 2)
    spans, c = rec["spans"], rec["coeffs"]
    x0, y0, rw, rh = rec["roi"]

    def canvas(s, fill, rows, cols):  # canvas values at the outer product of canvas rows and columns
        Y, X = np.meshgrid(rows, cols, indexing="ij")
        inside = (X >= spans[Y, 0]) & (X <= spans[Y, 1])
        return np.where(inside, warp_at(s, c, X, Y), np.uint8(fill))

    def fetch_img(rows, cols):
        return canvas(src, fill_byte(bgcolor), rows + y0, cols + x0)

    def fetch_mask(rows, cols):
        rows, cols = rows + y0, cols + x0
        acc = np.zeros((len(rows), len(cols)), np.int64)
        for dy, wy in ((-1, 1), (0, 2), (1, 1)):
            for dx, wx in ((-1, 1), (0, 2), (1, 1)):
                acc += wy * wx * canvas(mask, 0, _reflect(rows + dy, ch), _reflect(cols + dx, cw)).astype(np.int64)
        return (acc + 8) >> 4

    bgw = np.full((out_h, out_w), fill_byte(bgcolor), np.uint8) if bg is None else bg
    return _blend(_resize_from(fetch_img, rw, rh, out_w, out_h), _resize_from(fetch_mask, rw, rh, out_w, out_h), bgw,
                  rec["forecolordev"], rec["inverse"])


def background_window(images, bgrec, out_w, out_h):
    """The window the reader's record names: the image at the record's size, cropped at its origin."""
    i, w, h, x, y = bgrec
    img = np.asarray(images[i], np.uint8)
    scaled = img if (w, h) == (img.shape[1], img.shape[0]) else resize_linear_exact(img, w, h)
    return scaled[y:y + out_h, x:x + out_w]


def generate(image, n, out_w, out_h, p, rng, backgrounds=None, bg_images=None, dense=False):
    """n samples as (n, out_h, out_w) uint8. backgrounds: (n, out_h, out_w) caller windows; bg_images: the tool's -bg list."""
    src, mask = start_distortion(image, p.bgcolor, p.bgthreshold)
    reader = BgReader([(b.shape[1], b.shape[0]) for b in bg_images], out_w, out_h) if bg_images is not None else None
    recs = plan(src.shape[1], src.shape[0], out_w, out_h, p, rng, n, reader)
    out = np.empty((n, out_h, out_w), np.uint8)
    for i, r in enumerate(recs):
        bg = None
        if bg_images is not None:
            bg = background_window(bg_images, r["bg"], out_w, out_h)
        elif backgrounds is not None:
            bg = backgrounds[i]
        out[i] = (render_dense if dense else render_sparse)(src, mask, p.bgcolor, r, out_w, out_h, bg)
    return out
