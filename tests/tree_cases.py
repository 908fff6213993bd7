"""The cases the tree booster is tested on, shared by tests/test_tree_witness_host.py (which fixes the seeds, with libm's
exp) and the GPU tests: sample sets from tests/test_gpu_split.py's recipe and the oracle's values of every variable."""
import numpy as np

from cascadeclassifier_amd import evaluator as ev
from oracle import oracle as orc
from tests.test_gpu_split import _samples

N = 360  # the depth sweep's sample count, as tests/test_gpu_boost.py
DUP = 12
# Picked by test_the_case_constants_are_worth_using: see its docstring for what they give.
SWEEP_SEED = {"haar": 33, "lbp": 32}
SWEEP_WIN = {"haar": (12, 12), "lbp": (24, 24)}
SWEEP_ROUNDS = {ev.BOOST_DISCRETE: 6, ev.BOOST_GENTLE: 10, ev.BOOST_REAL: 10}
TRIM = 0.95


def values(ftype, mode, win, imgs, var_range=None):
    """[variable][sample] float32 of the oracle's evaluators (Haar, LBP)."""
    s, t, nf = orc.set_images(imgs, want_tilted=False, want_norm=ftype == ev.HAAR)
    cat = orc.haar_catalog(win[0], win[1], mode) if ftype == ev.HAAR else orc.lbp_catalog(*win)
    f0, f1 = var_range or (0, len(cat))
    if ftype == ev.HAAR:
        return orc.haar_eval_batch(cat, f0, f1, s, t, nf, win[0], win[1])
    return orc.lbp_eval_batch(cat, f0, f1, s, win[0], win[1])


def sweep_case(name):
    """(feature type, Haar mode, window, images, labels, values) of the depth sweep: 12x12 Haar CORE (13 168 variables) or
    LBP 24x24, n = 360."""
    ftype, mode = (ev.HAAR, ev.CORE) if name == "haar" else (ev.LBP, 0)
    win = SWEEP_WIN[name]
    imgs, labels = _samples(N, win, SWEEP_SEED[name], dup=DUP)
    return ftype, mode, win, imgs, labels, values(ftype, mode, win, imgs)


def noisy_samples(n, win, seed, dup=0, flip=0.15):
    """tests/test_gpu_split.py's samples with a share of the labels flipped: no split leaves a pure child, so trees grow to
    their depth limit or down to min_sample_count."""
    imgs, labels = _samples(n, win, seed, dup=dup)
    flips = np.random.default_rng(seed + 1000).random(n) < flip
    return imgs, (labels ^ flips.astype(np.uint8)).astype(np.uint8)


def exit_case(n_left, n=60, seed=5):
    """8x8 images for a Discrete round (uniform weights, MISCLASS) whose root split leaves a child of exactly n_left samples
    that is not pure, beside a pure one. Group A (n_left samples, bright left half) holds two negatives among positives, and
    each negative's image is also the image of two of A's positives; group B (bright right half) is all negative. A split
    errs at least once per such triple, so two errors is the least, and only a split that puts A on one side and B on the
    other reaches it: whichever variable wins, the children are A and B. Returns (imgs, labels)."""
    rng = np.random.default_rng(seed)
    imgs = rng.integers(100, 110, (n, 8, 8)).astype(np.uint8)
    a = np.sort(rng.permutation(n)[:n_left])
    side = np.zeros(n, bool)
    side[a] = True
    labels = side.astype(np.uint8)
    labels[a[:2]] = 0
    imgs[a[2]] = imgs[a[3]] = imgs[a[0]]
    imgs[a[4]] = imgs[a[5]] = imgs[a[1]]
    imgs[side, :, :4] += 120
    imgs[~side, :, 4:] += 120
    return imgs, labels
