"""Inputs and yardsticks of the HOG mining and stage-predict tests, shared by the GPU tests (tests/test_gpu_hog_cascade.py) and
the host test that asserts what makes each case worth running (tests/test_hog_mine_cases_host.py): the negative reader's window
walk restated (NegReader::nextImg / get, imagestorage.cpp:57-126, float32 arithmetic, levels by the oracle's
INTER_LINEAR_EXACT resize), the backgrounds, the cascades and the restatement's flags. Nothing here calls the library."""
import functools

import numpy as np

from oracle import oracle as orc
from tests import hog_cascade_factory as hf
from tests import hog_lds_cases as lds
from tests import hog_restatement as hog
from tests.util import frame_natural

f32 = np.float32


def reader_stream(src, W, H, ox, oy):
    """NegReader's stream over one image (nextImg with the given offset, then get until the ladder ends): the ladder as
    (lw, lh, nx, ny) per level and every window's pixels in stream order."""
    src = np.ascontiguousarray(src, np.uint8)
    rows, cols = src.shape
    scale_factor, step = f32(1.4142135623730950488016887242097), f32(0.5)
    scale = max(f32((f32(W) + f32(ox)) / f32(cols)), f32((f32(H) + f32(oy)) / f32(rows)))
    img = orc.resize_linear_exact(src, int(f32(scale * f32(cols)) + f32(0.5)), int(f32(scale * f32(rows)) + f32(0.5)))
    ladder, wins = [], []
    px, py = ox, oy
    nx = ny = 1
    while True:
        wins.append(img[py:py + H, px:px + W].copy())
        if int(f32(f32(px) + f32(f32(1) + step) * f32(W))) < img.shape[1]:
            px += int(f32(step * f32(W)))
            if py == oy:
                nx += 1
        else:
            px = ox
            if int(f32(f32(py) + f32(f32(1) + step) * f32(H))) < img.shape[0]:
                py += int(f32(step * f32(H)))
                ny += 1
            else:
                ladder.append((img.shape[1], img.shape[0], nx, ny))
                nx = ny = 1
                py = oy
                scale = f32(scale * scale_factor)
                if scale <= f32(1):
                    img = orc.resize_linear_exact(src, int(f32(scale * f32(cols))), int(f32(scale * f32(rows))))
                else:
                    break
    return ladder, np.stack(wins)


def predict_planes(feats, stages, hist, norm):
    """The trainer's stage walk on set_image planes."""
    return hf.stage_walk(hf.parsed_model(stages), hf.feature_values(feats, hist, norm))


def predict_windows(feats, stages, windows):
    """setImage of each window + the trainer's stage walk."""
    return predict_planes(feats, stages, *hog.set_images(windows))


def _reference_negative():  # test_integration.cpp:57-64
    r, c = np.mgrid[0:128, 0:256]
    return ((r * 7 + c * 13) & 0xFF).astype(np.uint8)


def edges(w, h, seed):
    """High-contrast patches with edges everywhere: a window's outer ring sees different gradients than the level does."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.where(((x // 5) + (y // 7)) % 2 == 0, 250, 5).astype(np.uint8)
    img[rng.random((h, w)) < 0.05] = 128
    return img


BACKGROUNDS = [("synthetic", _reference_negative(), 0, 0), ("natural", frame_natural(333, 211, 41), 5, 3),
               ("edges", edges(240, 160, 7), 11, 2)]
# The windows at the miner's LDS limit are mined on one small image (a few dozen windows, each a workgroup with 160 KB of LDS
# on the device and a setImage of its own in numpy) and their cascades are calibrated on the windows of a second one.
LARGE_BACKGROUND = [("natural_small", frame_natural(210, 180, 91), 3, 2)]
LARGE_CALIBRATION = ("natural_calibration", frame_natural(300, 220, 92), 0, 0)

OLD_WINDOWS = [(24, 24), (32, 32), (75, 32)]
WINDOWS = OLD_WINDOWS + lds.MINER_WINDOWS


def backgrounds_for(win):
    return LARGE_BACKGROUND if tuple(win) in lds.MINER_LARGE else BACKGROUNDS


@functools.lru_cache(maxsize=None)
def streams(win):
    """Per background of the window: (name, image, ox, oy, ladder, windows)."""
    W, H = win
    return [(name, img, ox, oy) + reader_stream(img, W, H, ox, oy) for name, img, ox, oy in backgrounds_for(win)]


@functools.lru_cache(maxsize=None)
def stream_planes(win):
    """set_images of every background's stream windows: [(hist, norm)]."""
    return [hog.set_images(s[5]) for s in streams(win)]


@functools.lru_cache(maxsize=None)
def _calibration_windows(win):
    W, H = win
    if win in lds.MINER_LARGE:
        _, img, ox, oy = LARGE_CALIBRATION
        return reader_stream(img, W, H, ox, oy)[1]
    return np.concatenate([s[5] for s in streams(win)])


def cascade_for(W, H, depth, seed, stage_sizes=(3, 4, 6)):
    """A cascade calibrated on stream windows, so that a sizeable share of the test's stream passes."""
    wins = _calibration_windows((W, H))
    rng = np.random.default_rng(seed)
    sel = wins[rng.choice(len(wins), min(len(wins), 400), replace=False)]
    return hf.hog_cascade(sel, seed=seed, stage_sizes=stage_sizes, depth=depth, pass_share=0.75)


@functools.lru_cache(maxsize=None)
def mining_case(win, depth):
    """The cascade of test_negative_mining_matches_reader_loop for (window, depth) and the restatement's flags of every
    background's stream: (xml, feats, stages, [flags])."""
    W, H = win
    xml, feats, stages = cascade_for(W, H, depth, seed=W + 11 * depth)
    return xml, feats, stages, [predict_planes(feats, stages, h, n) for h, n in stream_planes(win)]


# ---------------------------------------------------------------------------------------------- both stage walks of the miner
LONG_STAGES = (3, 70, 130)  # lanes 0..63 take a second and a third stump each in walk_stages_wave


@functools.lru_cache(maxsize=None)
def long_stage_case():
    """24x24 stumps with stages of 3, 70 and 130: (xml, feats, stages, [flags], [per-stage (entered, passed) counts])."""
    win = (24, 24)
    xml, feats, stages = cascade_for(24, 24, 1, seed=29, stage_sizes=LONG_STAGES)
    model = hf.parsed_model(stages)
    flags, counts = [], np.zeros((len(stages), 2), np.int64)
    for h, n in stream_planes(win):
        vals = hf.feature_values(feats, h, n)
        flags.append(hf.stage_walk(model, vals))
        for s, (entered, passed) in enumerate(hf.stage_passes(model, vals)):
            counts[s] += (int(entered.sum()), int(passed.sum()))
    return xml, feats, stages, flags, counts


BIG = float(2.0 ** 80)


@functools.lru_cache(maxsize=None)
def order_dependent_case():
    """24x24 stumps whose stage sums depend on the summation order. The stumps of a stage vote, in tree order: +2^80 whatever
    the side, a1, -2^80 whatever the side, a3, then three more votes, the small ones with leaves of +-0.2 to +-0.45.
    In tree order a1 is absorbed by 2^80, the two large votes then cancel exactly, and a3 and the rest add up.
    A wavefront that shares the stumps (lanes 0..6) first adds lanes 0 and 1 and lanes 2 and 3: a1 and a3 are both absorbed
    before the large votes meet. The two orders differ by a3's vote, which is the largest of the small ones.
    Returns (xml, feats, stages, [flags in tree order], [flags in reversed tree order], [flags in the wavefront's order])."""
    win = (24, 24)
    rng = np.random.default_rng(61)
    stage_leaves = []
    for _ in range(2):
        small = [float(rng.uniform(0.2, 0.3) * rng.choice([-1, 1])) for _ in range(4)]
        a3 = float(0.45 * rng.choice([-1, 1]))
        stage_leaves.append([(BIG, BIG), (small[0], -small[0]), (-BIG, -BIG), (a3, -a3)] + [(a, -a) for a in small[1:]])
    xml, feats, stages = hf.stump_cascade(_calibration_windows(win)[::3], stage_leaves, seed=61, pass_share=0.7)
    model = hf.parsed_model(stages)
    reverse = {"stages": [(thr, weaks[::-1]) for thr, weaks in model["stages"]]}
    fwd, rev, wave = [], [], []
    for h, n in stream_planes(win):
        vals = hf.feature_values(feats, h, n)
        fwd.append(hf.stage_walk(model, vals))
        rev.append(hf.stage_walk(reverse, vals))
        wave.append(hf.stage_walk(model, vals, sums=hf.wave_stage_sums))
    return xml, feats, stages, fwd, rev, wave


# ---------------------------------------------------------------------------------------------- predict at 86x85
@functools.lru_cache(maxsize=None)
def predict_case_86x85():
    """predict_cascade at the first window of the setImage kernel's 160 KiB branch: 40 crops of natural frames and a stump
    cascade calibrated on them. Returns (samples, xml, feats, stages, flags)."""
    W, H = 86, 85
    samples = np.stack([frame_natural(W * 2, H * 2, 300 + k)[k:k + H, 2 * k:2 * k + W] for k in range(40)])
    xml, feats, stages = hf.hog_cascade(samples, seed=86, stage_sizes=(3, 5), depth=1, pass_share=0.7)
    return samples, xml, feats, stages, predict_windows(feats, stages, samples)


# ---------------------------------------------------------------------------------------------- stored samples (predict_cascade)
@functools.lru_cache(maxsize=None)
def predict_samples(win):
    """The stored samples of test_predict_cascade_equals_stage_walk at the windows this module adds: 200 crops of natural
    frames, every third at low contrast."""
    W, H = win
    out = np.stack([frame_natural(W * 3, H * 2, 5 + k)[k % H:k % H + H, (3 * k) % W:(3 * k) % W + W] for k in range(200)])
    out[::3] = out[::3] // 4 + 90
    return out


@functools.lru_cache(maxsize=None)
def predict_case(win, depth):
    """(samples, xml, feats, stages, flags) for a window of lds.MINER_WINDOWS."""
    W, H = win
    samples = predict_samples(win)
    xml, feats, stages = hf.hog_cascade(samples, seed=W + depth, stage_sizes=(4, 6, 9), depth=depth, pass_share=0.7)
    return samples, xml, feats, stages, predict_windows(feats, stages, samples)
