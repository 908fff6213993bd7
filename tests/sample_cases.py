"""Inputs shared by the sample-synthesis tests: the fixture image, small synthetic objects and backgrounds, and the
parameter sets of the cases (tests/test_sample_plan_host.py, tests/test_sample_witness_host.py, tests/test_gpu_samples.py,
tests/test_gpu_sample_edges.py)."""
import hashlib
import os

import numpy as np

from tests import sample_witness as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BARCODE_SHA256 = "550ea662f0a99d46ad00ed21e8774d349b85c9328e36241040ae71b0a7ccf382"
BARCODE = dict(maxxangle=0.0, maxyangle=0.0, maxzangle=1.6)  # the README's command: -w 75 -h 32 -num 100


def barcode_image():
    g = np.load(os.path.join(GOLDEN, "ean13_5012345678900.npz"))["gray"]
    assert g.shape == (280, 600) and g.dtype == np.uint8
    assert hashlib.sha256(g.tobytes()).hexdigest() == BARCODE_SHA256
    return g


def barcode_vec_samples():
    raw = open(os.path.join(GOLDEN, "barcode.vec"), "rb").read()
    body = np.frombuffer(raw[12:], np.uint8).reshape(100, 1 + 2 * 75 * 32)[:, 1:]
    return np.ascontiguousarray(body).view("<i2").astype(np.uint8).reshape(100, 32, 75)


def obj_image(w, h, seed, bgcolor=0):
    """A bright blob with texture on a background of bgcolor +- a few levels (so mask and border extension both matter)."""
    r = np.random.RandomState(seed)
    img = np.clip(bgcolor + r.randint(-6, 7, (h, w)), 0, 255)
    yy, xx = np.mgrid[:h, :w]
    inside = ((xx - w / 2) / (w * 0.38)) ** 2 + ((yy - h / 2) / (h * 0.42)) ** 2 < 1
    fg = r.randint(100, 200, (h, w)) if bgcolor < 128 else r.randint(20, 120, (h, w))
    return np.where(inside, fg, img).astype(np.uint8)


def bg_images():
    """Three small backgrounds: one that holds several scales of a 24 x 24 window ladder, one barely larger than the window,
    one between."""
    r = np.random.RandomState(77)
    return [r.randint(0, 256, (h, w)).astype(np.uint8) for w, h in ((70, 52), (30, 26), (45, 61))]


# name -> (source w, h, window w, h, Params kwargs)
CASES = {
    "default_24": (40, 24, 24, 24, {}),
    "default_20x13": (40, 24, 20, 13, {}),
    "upscale": (10, 8, 24, 24, {}),
    "angles_0": (40, 24, 24, 24, dict(maxxangle=0.0, maxyangle=0.0, maxzangle=0.0)),
    "bg255_inv": (40, 24, 24, 24, dict(bgcolor=255, invert=1)),
    "randinv": (40, 24, 24, 24, dict(invert=W.RANDOM_INVERT)),
    "inscribe_clipped": (40, 24, 24, 24, dict(inscribe=1, maxshift=0.3, maxscale=0.5)),
    "odd_source": (41, 23, 24, 24, {}),
}

ZERO_ANGLES = dict(maxxangle=0.0, maxyangle=0.0, maxzangle=0.0)
_CLIP = dict(maxshift=0.6, maxscale=1.0)

# name -> (source w, h, window w, h, Params kwargs, samples, seed): the sizes at which the kernels and the plan take another
# path or meet a limit. What each row is for is a condition tests/test_sample_witness_host.py asserts on the witness's plan
# (test_edge_case_meets_its_condition), so a row cannot silently stop covering its edge.
#   source_8192x2: a 24 x 3 window with default angles is a flat picture in the witness; 512 x 2 with zero angles keeps 16
#   source columns per output pixel and the textured row of obj_image, which gives more than 8 distinct values (asserted).
EDGE_CASES = {
    "clipped_all_edges": (40, 24, 24, 24, _CLIP, 24, 12345),        # the rectangle reaches every canvas edge
    "canvas_5": (3, 3, 5, 7, _CLIP, 16, 12345),                     # canvas 5 x 5, every edge touched
    "canvas_4": (2, 2, 5, 3, dict(_CLIP, bgthreshold=10), 16, 7),   # canvas 4 x 4, the rectangle is the whole canvas
    "min_source_1x1": (2, 2, 1, 1, {}, 16, 12345),                  # window side 1 on both axes
    "narrow_source": (2, 9, 7, 3, {}, 16, 12345),                   # side-2 source, not square
    "wide_row": (130, 9, 300, 2, {}, 8, 12345),                     # a window row crosses a 256-thread block
    "deep_downscale": (200, 120, 5, 3, {}, 8, 12345),               # ratio 80:1, taps far apart
    "flipped_quads": (40, 24, 24, 24, dict(maxxangle=3.0, maxyangle=3.0, maxzangle=3.14), 48, 12345),  # reversed vertex order
    "idev_clamps": (40, 24, 24, 24, dict(maxintensitydev=255), 24, 12345),  # the blend's clamp engages on both sides
    "idev_zero": (40, 24, 24, 24, dict(ZERO_ANGLES, maxintensitydev=0), 4, 12345),  # uniform(a, a) draws nothing
    "window_4096x1": (40, 24, 4096, 1, {}, 2, 12345),               # window limit, 16 blocks per sample
    "window_1x4096": (40, 24, 1, 4096, {}, 2, 12345),
    "source_2x8192": (2, 8192, 3, 24, ZERO_ANGLES, 2, 12345),       # source limit, 16384 span rows per sample
    "source_8192x2": (8192, 2, 512, 2, ZERO_ANGLES, 2, 12345),      # source limit the other way
}
# rows whose canvas or window is too large for the dense witness (it builds the canvas and resizes row by row)
EDGE_SPARSE_ONLY = ("window_4096x1", "window_1x4096", "source_2x8192", "source_8192x2")
# rows that must give more than 8 distinct output values on a constant background; the two left out have a 2 x 2 source
# (four source pixels) and are there for the index arithmetic, not the picture
EDGE_TEXTURED = ("clipped_all_edges", "canvas_5", "narrow_source", "wide_row", "deep_downscale", "flipped_quads", "idev_clamps",
                 "idev_zero", "window_4096x1", "window_1x4096", "source_2x8192", "source_8192x2")

BG_LIST_SIZES = [(24, 24), (24, 40), (150, 70), (23, 100), (25, 24)]  # for a 24 x 24 window: exact fit, as wide but taller,
#                                                                      a four-step scale ladder, too narrow (skipped), one wider


def bg_list_images():
    r = np.random.RandomState(78)
    return [r.randint(0, 256, (h, w)).astype(np.uint8) for w, h in BG_LIST_SIZES]


def edge_inputs(name):
    """(image, caller backgrounds of random bytes) of an EDGE_CASES row."""
    sw, sh, ow, oh, kw, n, _ = EDGE_CASES[name]
    img = obj_image(sw, sh, 5, kw.get("bgcolor", 0))
    bg = np.random.RandomState(31).randint(0, 256, (n, oh, ow)).astype(np.uint8)
    return img, bg


_edge_witness_cache = {}


def edge_witness(name):
    """The sparse witness's samples of a row on its caller backgrounds (computed once per process; do not modify)."""
    if name not in _edge_witness_cache:
        sw, sh, ow, oh, kw, n, seed = EDGE_CASES[name]
        img, bg = edge_inputs(name)
        out = W.generate(img, n, ow, oh, W.Params(**kw), W.RNG(seed), backgrounds=bg)
        out.setflags(write=False)
        _edge_witness_cache[name] = out
    return _edge_witness_cache[name]


def quad_walk(quad):
    """(direction, topmost vertex) of a quad as the scanline walk sees it: the sign of the vertex order and the index of the
    topmost (leftmost of two) vertex."""
    d = 0
    for i in range(4):
        n, p = (i + 1) % 4, (i + 3) % 4
        c = (quad[i][0] - quad[p][0]) * (quad[n][1] - quad[i][1]) - (quad[i][1] - quad[p][1]) * (quad[n][0] - quad[i][0])
        d = d or (1 if c > 0 else -1 if c < 0 else 0)
    top = min(range(4), key=lambda i: (quad[i][1], quad[i][0]))
    return d, top


def edge_touches(recs, cw, ch):
    """How many records' rectangles lie on the left, top, right and bottom canvas edge."""
    rois = [r["roi"] for r in recs]
    return (sum(x == 0 for x, y, w, h in rois), sum(y == 0 for x, y, w, h in rois),
            sum(x + w == cw for x, y, w, h in rois), sum(y + h == ch for x, y, w, h in rois))


def rec_dict(r, spans):
    """One planned cc_sample_record (a ctypes structure) and its (canvas rows, 2) spans as the witness's record."""
    q = list(r.quad)
    return dict(quad=[[q[2 * i], q[2 * i + 1]] for i in range(4)], coeffs=list(r.coeffs), spans=np.asarray(spans, np.int32),
                roi=(r.roi_x, r.roi_y, r.roi_w, r.roi_h), inverse=r.inverse, forecolordev=r.forecolordev,
                bg=(r.bg_image, r.bg_w, r.bg_h, r.bg_x, r.bg_y))


def render_records(src, mask, bgcolor, recs, out_w, out_h, backgrounds=None, bg_images=None):
    """The sparse witness over witness records. backgrounds: (n, h, w) caller windows; bg_images: the list the records'
    bg fields index (a record with image -1 gets the background-less window)."""
    out = np.empty((len(recs), out_h, out_w), np.uint8)
    for i, r in enumerate(recs):
        bg = None
        if backgrounds is not None:
            bg = backgrounds[i]
        elif bg_images is not None and r["bg"][0] != -1:
            bg = W.background_window(bg_images, r["bg"], out_w, out_h)
        out[i] = W.render_sparse(src, mask, bgcolor, r, out_w, out_h, bg)
    return out


# k_sampler_prepare past one block column (64) and one block row (4), at the ends of its colour arithmetic
PREPARE_SOURCES = ((65, 5), (129, 9), (130, 9))
PREPARE_PARAMS = ((250, 20), (3, 10), (0, 0), (0, 255), (300, 80), (-5, 80))  # (bgcolor, bgthreshold)


def prepare_case(w, h, bgcolor, bgthreshold):
    """A noisy-background object at zero angles, window = source size, 2 samples on random-byte backgrounds:
    (image, Params kwargs, backgrounds, witness output, witness output had the border extension been skipped)."""
    kw = dict(ZERO_ANGLES, bgcolor=bgcolor, bgthreshold=bgthreshold)
    img = obj_image(w, h, 9, W.fill_byte(bgcolor))
    bg = np.random.RandomState(41).randint(0, 256, (2, h, w)).astype(np.uint8)
    src, mask = W.start_distortion(img, bgcolor, bgthreshold)
    recs = W.plan(w, h, w, h, W.Params(**kw), W.RNG(12345), 2)
    return img, kw, bg, render_records(src, mask, bgcolor, recs, w, h, bg), render_records(img, mask, bgcolor, recs, w, h, bg)


def stride_image(w, h, pad):
    """(h, w + pad) bytes: a background of 0..6 with a bright column at w - 2, so that the background pixels of column
    w - 1 take their 3x3 maximum from it and sit under a nonzero blurred mask; the padding is 255. A prepare kernel that
    read past w would extend those pixels with 255."""
    r = np.random.RandomState(13)
    full = np.full((h, w + pad), 255, np.uint8)
    full[:, :w] = r.randint(0, 7, (h, w))
    full[:, w - 2] = r.randint(100, 200, h)
    full[1:h - 1, w // 3:w // 2] = r.randint(100, 200, (h - 2, w // 2 - w // 3))
    return full


# coefficient sets whose source coordinates leave the source, the int range or the numbers: cc_sampler_render takes caller
# records, so the fold in warp_coord is reachable through the C ABI. Rendered over roi (0, 0, 80, 48) with every span
# [0, 79] on the 40 x 24 object.
_N = float("nan")
COORD_CASES = {
    "horizon": [1, 0, -20, 0, 1, -12, 0.125, 0, -5],       # div is 0 at column 40: both infinities and NaN around it
    "huge": [1e300, 0, 0, 0, 1e300, 0, 0, 0, 1e-300],
    "neg_huge": [-1e18, 0, -1e18, 0, -1e18, -1e18, 0, 0, 1],
    "nan": [_N] * 9,
    "just_out": [1, 0, -20, 0, 1, -12, 0, 0, 1],           # a translation: taps at -1 and at sw - 1 on both axes
}
COORD_DRAWS = ("horizon", "just_out")  # the sets with taps inside the source; the others leave the background as it is


def coord_record(rec, name):
    """The planned witness record with the rectangle, spans and coefficients of a COORD_CASES row."""
    r = dict(rec)
    r["roi"] = (0, 0, 80, 48)
    r["spans"] = np.tile(np.array([0, 79], np.int32), (48, 1))
    r["coeffs"] = [float(v) for v in COORD_CASES[name]]
    return r
