"""Shapes and inputs shared by the tests of the -info mode (tests/test_area_witness_host.py, tests/test_info_samples_host.py,
tests/test_gpu_info_samples.py). What each crafted input is there for is asserted on the witness on the host."""
import functools
import math

import numpy as np

from tests import area_witness as AW

# one axis, source -> destination: the sizes cc_area_tab is compared on
AXIS_SIZES = [(25, 24), (47, 24), (49, 1), (72, 24), (48, 24), (24, 24), (280, 32), (600, 75), (1001, 1000), (8192, 1), (8192, 4096),
              (1, 1)]

# the witness against exact rational area means: (sw, sh, dw, dh)
EXACT_SHAPES = [(25, 25, 24, 24), (47, 47, 24, 24), (49, 49, 1, 1), (100, 37, 24, 24), (31, 24, 24, 24), (27, 29, 5, 7),
                (98, 49, 2, 1), (48, 48, 24, 24), (72, 48, 24, 24), (1001, 2, 1000, 1)]

# resize_area alone: name -> (sw, sh, dw, dh)
RESIZE_CASES = {
    "2x2_fast": (48, 48, 24, 24),
    "3x2_fast": (72, 48, 24, 24),
    "4x2_fast_ties": (96, 48, 24, 24),
    "49_to_1": (49, 49, 1, 1),
    "25_to_24": (25, 25, 24, 24),
    "47_to_24": (47, 47, 24, 24),
    "y_scale_1": (31, 24, 24, 24),
    "27x29_to_5x7": (27, 29, 5, 7),
    "7x5_to_1x1": (7, 5, 1, 1),
    "1x1": (1, 1, 1, 1),
    "row_301": (301, 3, 300, 1),
    "row_1001": (1001, 2, 1000, 1),
    "8192_to_1": (8192, 1, 1, 1),
    "barcode": (600, 280, 75, 32),
}


def random_image(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def block_sum_image(w, h, kx, ky, modulus, residue, seed):
    """Random bytes whose kx x ky block sums are all `residue` modulo `modulus`: the last pixel of each block is chosen for it."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    for by in range(h // ky):
        for bx in range(w // kx):
            blk = img[by * ky:(by + 1) * ky, bx * kx:(bx + 1) * kx]
            rest = int(blk.sum()) - int(blk[-1, -1])
            blk[-1, -1] = (residue - rest) % modulus + modulus * int(rng.integers(0, 256 // modulus - 1))
    return img


@functools.lru_cache(maxsize=None)
def resize_input(name):
    sw, sh, dw, dh = RESIZE_CASES[name]
    if name == "2x2_fast":  # sums of 4k + 2: (s + 2) >> 2 rounds the half up, half-to-even would not for even k
        return block_sum_image(sw, sh, 2, 2, 4, 2, 11)
    if name == "4x2_fast_ties":  # sums of 8k + 4: sum / 8 lands on k + .5, cvRound goes to the even neighbour
        return block_sum_image(sw, sh, 4, 2, 8, 4, 12)
    if name == "barcode":
        from tests.sample_cases import GOLDEN
        import os
        return np.load(os.path.join(GOLDEN, "ean13_5012345678900.npz"))["gray"]
    return random_image(sw, sh, 100 + sorted(RESIZE_CASES).index(name))


@functools.lru_cache(maxsize=None)
def resize_want(name):
    _, _, dw, dh = RESIZE_CASES[name]
    return AW.resize_area(resize_input(name), dw, dh)


def surrounded(w, h, rects, seed):
    """A w x h image of 255 with random bytes of 0..199 inside each rectangle: what lies around a rectangle must not be read."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 255, np.uint8)
    for x, y, rw, rh in rects:
        img[y:y + rh, x:x + rw] = rng.integers(0, 200, (rh, rw), dtype=np.uint8)
    return img


def bilinear_with_image_as_source(img, rect, dw, dh):
    """What the bilinear branch would give if the image, not the rectangle, were the source: the same taps in the
    rectangle's coordinates, but a tap outside the rectangle reads the image's pixel there and is not replicated."""
    x, y, w, h = rect

    def taps(src, dst):
        scale = 1.0 / (float(dst) / float(src))
        f = [scale * (d + 0.5) - 0.5 for d in range(dst)]
        i = np.array([math.floor(v) for v in f], np.int64)
        return i, np.array([round((v - math.floor(v)) * 256.0) for v in f], np.int64)

    xo, xw = taps(w, dw)
    yo, yw = taps(h, dh)
    v = img.astype(np.int64)
    r0, r1, c0, c1 = y + yo, y + yo + 1, x + xo, x + xo + 1
    hz0 = (256 - xw)[None, :] * v[np.ix_(r0, c0)] + xw[None, :] * v[np.ix_(r0, c1)]
    hz1 = (256 - xw)[None, :] * v[np.ix_(r1, c0)] + xw[None, :] * v[np.ix_(r1, c1)]
    return (((256 - yw)[:, None] * hz0 + yw[:, None] * hz1 + (1 << 15)) >> 16).astype(np.uint8)


BILINEAR_RECTS = [(15, 12, 20, 30), (14, 20, 30, 20), (25, 25, 10, 10)]  # 20 x 30, 30 x 20 and 10 x 10 to 24 x 24


@functools.lru_cache(maxsize=None)
def info_case(name):
    """(images, records, (dw, dh)): records are (image, x, y, w, h)."""
    if name == "corners":  # all four corners of an image and the whole of it; a second image that is one rectangle
        a, b = random_image(64, 48, 1), random_image(100, 37, 2)
        return [a, b], [(0, 0, 0, 30, 26), (0, 34, 0, 30, 26), (0, 0, 22, 30, 26), (0, 34, 22, 30, 26), (0, 0, 0, 64, 48),
                        (1, 0, 0, 100, 37)], (24, 24)
    if name == "bilinear":  # one axis or both grow: INTER_LINEAR_EXACT on the rectangle, 255 all around it
        return [surrounded(60, 60, BILINEAR_RECTS, 3)], [(0,) + r for r in BILINEAR_RECTS], (24, 24)
    if name == "copy":  # same size: a whole image and a rectangle inside another
        a, b = random_image(24, 24, 4), random_image(64, 48, 5)
        return [a, b], [(0, 0, 0, 24, 24), (1, 17, 9, 24, 24)], (24, 24)
    if name == "mixed":  # every mode and several image sizes in one launch; image 0 comes back after others were used
        a, b = random_image(64, 48, 6), random_image(100, 37, 7)
        c = surrounded(60, 60, BILINEAR_RECTS, 8)
        d = random_image(24, 24, 9)
        e = block_sum_image(96, 48, 4, 2, 8, 4, 10)
        recs = [(0, 3, 4, 25, 25), (0, 1, 1, 47, 47), (1, 10, 5, 72, 24), (2,) + BILINEAR_RECTS[0], (3, 0, 0, 24, 24),
                (4, 0, 0, 96, 48), (0, 7, 9, 49, 30), (0, 0, 0, 48, 48), (2,) + BILINEAR_RECTS[1], (1, 0, 0, 100, 37),
                (4, 48, 0, 48, 48), (2,) + BILINEAR_RECTS[2], (0, 40, 24, 24, 24), (1, 69, 6, 31, 24), (0, 0, 0, 64, 48)]
        return [a, b, c, d, e], recs, (24, 24)
    if name == "window_5x7":  # a window that is not square, with a record of every mode
        a = surrounded(40, 40, [(4, 4, 4, 6), (20, 5, 3, 9)], 13)
        b = random_image(33, 31, 14)
        return [a, b], [(1, 2, 1, 27, 29), (0, 4, 4, 4, 6), (1, 9, 9, 5, 7), (1, 0, 20, 10, 7), (0, 20, 5, 3, 9), (1, 0, 0, 33, 31)], (5, 7)
    if name == "window_1x1":
        a = random_image(50, 49, 15)
        return [a], [(0, 1, 0, 49, 49), (0, 3, 3, 7, 5), (0, 49, 48, 1, 1)], (1, 1)
    if name == "window_row_300":  # a window row longer than a block, from a rectangle inside a larger image
        a = random_image(320, 8, 16)
        return [a], [(0, 19, 5, 301, 3), (0, 0, 0, 320, 8)], (300, 1)
    raise KeyError(name)


INFO_CASES = ["corners", "bilinear", "copy", "mixed", "window_5x7", "window_1x1", "window_row_300"]


@functools.lru_cache(maxsize=None)
def info_want(name):
    images, records, (dw, dh) = info_case(name)
    return AW.samples(images, records, dw, dh)


def mode_of(rect, win):
    """copy / linear / fast / area of one record, from the witness's own choices."""
    w, h = rect[2], rect[3]
    if (w, h) == tuple(win):
        return "copy"
    if not AW.uses_area(w, h, *win):
        return "linear"
    return "fast" if AW.is_fast(w, h, *win) else "area"


# The smallest integer-ratio rectangle for a 1 x 1 window whose block sum could pass 2^31, and the largest that cannot.
OVERFLOW_SIDES, NO_OVERFLOW_SIDES = (4096, 2057), (4096, 2056)

# cc_samples_from_info's refusals on a valid call of three records over two images (64 x 48 and 100 x 37), one field changed
# in record 1 = (image 0, x 34, y 0, 30 x 26): name -> (field index in (image, x, y, w, h), value)
RECORD_REFUSALS = {
    "image_minus_1": (0, -1),
    "image_count": (0, 2),
    "x_negative": (1, -1),
    "y_negative": (2, -1),
    "x_past_the_edge": (1, 35),
    "y_past_the_edge": (2, 23),
    "width_zero": (3, 0),
    "height_zero": (4, 0),
    "width_negative": (3, -5),
    "width_past_the_edge": (3, 31),
    "height_past_the_edge": (4, 49),
}
