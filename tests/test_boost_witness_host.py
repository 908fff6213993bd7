"""The boosting witness (tests/boost_witness.py) against arithmetic done by hand: a Discrete AdaBoost case small enough
for exact rationals, and the trimming walk and the stage-status rule on constructed arrays. No device."""
import math
from fractions import Fraction

import numpy as np

from tests import boost_witness as bw

# 12 samples, 3 variables given as value rows. Discrete AdaBoost with the MISCLASS criterion: the quality of a boundary
# is max(lcw0 + rcw1, lcw1 + rcw0) (o_cvboostree.cpp:222-238), so everything but log / exp is rational.
LABELS = [1, 1, 1, 0, 1, 1, 0, 0, 1, 0, 0, 0]
ROWS = np.array([[1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12],
                 [5, 9, 2, 7, 1, 8, 3, 12, 4, 10, 6, 11],
                 [3, 3, 1, 2, 9, 9, 8, 2, 1, 7, 8, 9]], np.float32)
# every figure below is a handful of double operations on the exact value: 64 roundings of 2^-53 bound the relative error
REL = 64 * 2.0 ** -53


def _exact_stump(rows, labels, w):
    """Brute force over variables and boundaries with rational weights: (quality, var, split_point, threshold pair)."""
    best = None
    n = len(labels)
    for v, row in enumerate(rows):
        order = sorted(range(n), key=lambda i: (float(row[i]), i))
        for k in range(n - 1):
            a, b = float(row[order[k]]), float(row[order[k + 1]])
            if not a < b:
                continue
            lcw = [sum((w[i] for i in order[:k + 1] if labels[i] == c), Fraction(0)) for c in (0, 1)]
            rcw = [sum((w[i] for i in order[k + 1:] if labels[i] == c), Fraction(0)) for c in (0, 1)]
            q = max(lcw[0] + rcw[1], lcw[1] + rcw[0])
            if best is None or q > best[0]:
                best = (q, v, k, (a, b), order[:k + 1])
    return best


def test_discrete_two_rounds_against_exact_rationals():
    n = len(LABELS)
    wit = bw.BoostWitness(ROWS, LABELS, boost_type=bw.DISCRETE, weight_trim_rate=1.0, max_false_alarm=0.01, max_weak_count=5)
    w = [Fraction(1, n)] * n
    y = [2 * c - 1 for c in LABELS]
    stage = [0.0] * n
    for rnd in range(2):
        q, var, point, (a, b), left_set = _exact_stump(ROWS, LABELS, w)
        rec = wit.round()
        assert rec["trained"] and rec["n_active"] == n
        assert rec["var_idx"] == var and rec["split_point"] == point, (rnd, rec)
        assert rec["ord_c"] == np.float32((np.float32(a) + np.float32(b)) * np.float32(0.5))
        assert abs(float(rec["quality"]) - float(q)) <= 2.0 ** -23 * float(q)  # the quality is stored as a float
        # leaves +-1 by the weighted majority; err = weight of the samples the stump gets wrong; C = log((1 - err) / err)
        f = {}
        for side in (set(left_set), set(range(n)) - set(left_set)):
            c1 = sum((w[i] for i in side if LABELS[i] == 1), Fraction(0))
            c0 = sum((w[i] for i in side if LABELS[i] == 0), Fraction(0))
            for i in side:
                f[i] = 1 if c1 > c0 else -1
        err = sum((w[i] for i in range(n) if f[i] != y[i]), Fraction(0)) / sum(w)
        assert Fraction(1, 100000) < err < Fraction(1, 2)
        C = math.log(float((1 - err) / err))
        left_leaf = f[left_set[0]]
        assert abs(rec["left_value"] - left_leaf * C) <= REL * C and abs(rec["right_value"] + left_leaf * C) <= REL * C
        # w *= exp(C) = (1 - err) / err where wrong; renormalise
        w = [w[i] * ((1 - err) / err if f[i] != y[i] else 1) for i in range(n)]
        tot = sum(w)
        w = [x / tot for x in w]
        got = wit.state()
        for i in range(n):
            assert abs(got["weights"][i] - float(w[i])) <= REL * float(w[i]), (rnd, i)
            assert got["weak_eval"][i] == f[i]
            stage[i] += f[i] * C
            assert abs(got["stage_sum"][i] - stage[i]) <= REL * (rnd + 1) * abs(C) + 1e-300
        assert (got["mask"] == 1).all()
    assert abs(sum(wit.state()["weights"]) - 1.0) <= REL


def test_trim_walk_on_constructed_weights():
    # dyadic weights: every step of the walk is exact. 1 - 0.75 = 0.25; sorted .0625 .0625 .125 .25 .5
    mask, thr = bw.trim_walk([0.5, 0.25, 0.125, 0.0625, 0.0625], 0.75)
    # sum: .25 -> .1875 -> .125 -> 0.0 -> break at i = 3: threshold .25
    assert thr == 0.25 and mask.tolist() == [1, 1, 0, 0, 0]
    # the walk reaches the end with sum still > 0: threshold DBL_MAX, nothing stays active
    mask, thr = bw.trim_walk([0.0625, 0.0625], 0.75)
    assert thr == bw.DBL_MAX and mask.tolist() == [0, 0]
    # equal weights at the threshold all stay
    mask, thr = bw.trim_walk([0.25, 0.125, 0.25, 0.125, 0.25], 0.75)  # .25 -> .125 -> 0.0 -> break at i = 2
    assert thr == 0.25 and mask.tolist() == [1, 0, 1, 0, 1]
    # sum <= 0 before the first element: threshold = the smallest weight, everything stays
    mask, thr = bw.trim_walk([0.5, 0.25, 0.25], 1.0 - 0.0)  # rate 1 is "disabled" for the trainer; the walk itself breaks at i = 0
    assert thr == 0.25 and mask.tolist() == [1, 1, 1]


def test_is_err_desired_threshold_index_and_ties():
    # thresholdIdx = 0: (1.0f - 0.995f) * 8 < 1; the threshold is the smallest positive sum and every positive passes
    sums = [3.0, 1.0, 2.0, 5.0, 4.0, 8.0, 7.0, 6.0, 0.5, 1.0]
    labels = [1, 1, 1, 1, 1, 1, 1, 1, 0, 0]
    thr, hit, fa, done = bw.is_err_desired(sums, labels, 0.995, 0.5)
    assert thr == np.float32(1.0) and hit == np.float32(1.0) and fa == np.float32(0.5) and done
    # equal sums at the threshold: thresholdIdx = (int)(0.5f * 8) = 4, eval = 0 1 1 1 1 2 3 4: 4 from the index up and
    # the three ties below it
    sums = [1.0, 0.0, 1.0, 2.0, 1.0, 3.0, 1.0, 4.0, 1.0, 0.99999, 0.9999, 1.0 - 5e-6]
    labels = [1] * 8 + [0] * 4
    thr, hit, fa, done = bw.is_err_desired(sums, labels, 0.5, 0.5)
    assert thr == np.float32(1.0) and hit == np.float32(7) / np.float32(8)
    # a negative passes iff !(sum < threshold - 1e-5f): 1.0, 0.99999 (the float bound is 0.9999899864) and 1 - 5e-6 pass
    assert fa == np.float32(3) / np.float32(4) and not done
    # 1.0f - 0.995f is 0.00499999523: 400 positives give index 1, not 2
    sums = [float(i) for i in range(400)] + [-1.0]
    thr, hit, fa, done = bw.is_err_desired(sums, [1] * 400 + [0], 0.995, 0.5)
    assert thr == np.float32(1.0) and hit == np.float32(399) / np.float32(400) and fa == 0 and done
    sums[0] = 1.0  # a tie below the index counts as a hit
    assert bw.is_err_desired(sums, [1] * 400 + [0], 0.995, 0.5)[1] == np.float32(1.0)
