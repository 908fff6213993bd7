"""Inputs shared by the sample-synthesis tests: the fixture image, small synthetic objects and backgrounds, and the
parameter sets of the cases (tests/test_sample_plan_host.py, tests/test_gpu_samples.py)."""
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
