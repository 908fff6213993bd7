"""Haar cascades at windows other than 24x24, shared by tests/test_haar_windows_host.py and tests/test_gpu_haar_windows.py:
the window list, the calibration windows (cut at the cascade's own size) and one cached cascade per (window, kind)."""
import functools
import os

import numpy as np

from oracle import oracle as orc
from tests import cascade_factory as cf
from tests.util import frame_natural

# (W, H): why this window is here (cc_tables.hip / cc_pass.hip / cc_eval_common.h / cc_spec.hip select code by it)
WINDOWS = [
    (20, 20),    # the stock frontal-face size: even / even, smaller than 24x24
    (19, 23),    # odd / odd: no compact squared-sum integral at step 2
    (25, 24),    # one odd side each: the && of the compact-integral condition, row-stride rounding
    (24, 25),
    (14, 28),    # far from square, both ways
    (44, 12),
    (75, 32),    # the reference's barcode window; not eligible for the 16-bit tile; tilted: more than 64 KiB of LDS
    (128, 40),   # widest tile row; upright just under 64 KiB
    (96, 96),    # upright: more than 64 KiB; tilted: more than 160 KiB, refused by the detector
]
PAIRS = [(W, H, tilted) for (W, H) in WINDOWS for tilted in (False, True)]


def pair_id(p):
    return "%dx%d-%s" % (p[0], p[1], "tilted" if p[2] else "upright")


def calibration_positions(W, H):
    """(x, y) of the calibration windows in frame_natural(640, 480, 3), in the order of calibration_windows."""
    return [(x, y) for y in range(0, 480 - H + 1, 13) for x in range(0, 640 - W + 1, 17)]


@functools.lru_cache(maxsize=None)
def calibration_windows(W, H):
    img = frame_natural(640, 480, 3)
    return np.stack([img[y:y + H, x:x + W] for (x, y) in calibration_positions(W, H)])


@functools.lru_cache(maxsize=None)
def stump_xml(W, H, tilted, min_area=16):
    """Stump cascade of stages (6, 10, 14, 20), each calibrated to pass half of the calibration windows that reach it."""
    return cf.tilted_stump_cascade(calibration_windows(W, H), tilted=tilted, min_area=min_area, W=W, H=H)


@functools.lru_cache(maxsize=None)
def tree_xml(W, H, tilted):
    return cf.haar_tree_cascade(calibration_windows(W, H), with_tilted=tilted, W=W, H=H)


def write_xml(tmp, text, name="cascade.xml"):
    path = os.path.join(str(tmp), name)
    with open(path, "w") as f:
        f.write(text)
    return path


def oracle_cascade(tmp, text, name="cascade.xml"):
    return orc.load_cascade_xml(write_xml(tmp, text, name))


def exit_stage_counts(codes, nstages):
    """Windows per exit: index k < nstages = rejected by stage k, index nstages = passed every stage. Code -1 is both
    'rejected by stage 1' and 'failed the variance test' in the oracle's result codes; it is counted for stage 1."""
    return np.array([(codes == -k).sum() for k in range(nstages)] + [(codes == 1).sum()])


def pasted_frame(W, H, seed, w=400, h=300, scales=(1.0, 1.3, 1.7)):
    """A natural frame with calibration windows of the cascade pasted back at a few scales: the cascade was calibrated
    to pass half of them per stage, so windows survive into the late stages and the per-tile queues stay long."""
    img = frame_natural(w, h, seed)
    wins = calibration_windows(W, H)
    rng = np.random.default_rng(seed)
    for k in range(24):
        s = scales[k % len(scales)]
        pw, ph = int(round(W * s)), int(round(H * s))
        if pw >= w or ph >= h:
            continue
        x, y = int(rng.integers(0, w - pw)), int(rng.integers(0, h - ph))
        img[y:y + ph, x:x + pw] = orc.resize_linear_exact(wins[int(rng.integers(0, len(wins)))], pw, ph)
    return img
