"""Cascades at the edges of the range proofs and shape limits of the cascade kernels, shared by
tests/test_cascade_edges_host.py (which proves on the CPU that every input is what it claims to be) and
tests/test_gpu_cascade_edges.py (which compares the kernels with the oracle on them).

A kernel may sum a stage's votes in another order than the CPU, in int32, or evaluate a feature with integer arithmetic
or from 16-bit tile entries only where a load-time predicate proves that this cannot change a bit:
    stage_sums_order_independent(m, headroom)   sum max(|l|,|r|) * headroom / q < 2^53, q = 2^(emin - 24)   (cc_host.cpp)
    stage_quantum(m, s, q)                      sum max(|l|,|r|) / q < 2^31 - 1                             (cc_host.cpp)
    int_ok                                      integer |w| <= 64 and sum |w| 255 area (tilted: 2x) < 2^24  (cc_spec.hip)
    16-bit tile                                 a stump's value range fits int16, else strips of <= 257 px  (cc_spec.hip)
The predicates are restated here with exact integers (order_independent, quantum_ok, int_form_ok, value_range), and
the cascades below sit just on either side of each bound, at the shape limits (63 / 64 stages, stages of 63 ... 129
stumps, LBP stages and stage runs of 64 / 65 and 14 / 15 stumps) and on exact ties (v == thr, sum == stage threshold).

Two tools make a stage's vote pattern controllable without special images. Forced votes: a node threshold of +-3e38
makes a stump vote left or right on every window, which fixes the vote sequence of a stage; a few stumps with calibrated
thresholds are mixed in so that windows still differ. Tie frames: a random gray value per 16x16 block, on which a
balanced Haar feature that lies in a flat part of the window is exactly 0 while the window's variance is positive.
"""
import functools
from fractions import Fraction

import numpy as np

from oracle import oracle as orc
from tests import cascade_factory as cf
from tests import haar_windows as hw
from tests.util import frame_natural, frame_uniform

F32 = np.float32
EPS = F32(1e-5)        # THRESHOLD_EPS: the kernels and the oracle compare a stage sum with (float)stageThreshold - 1e-5f
ALWAYS_LEFT = 3e38     # node threshold: v < thr on every window
ALWAYS_RIGHT = -3e38
SPEC_PARTS = 8         # cc_eval_common.h: contiguous parts a generated stage is cut into


# ------------------------------------------------------------------ float helpers
def f32_step(x, n):
    """The float32 n ulps above (n > 0) or below (n < 0) x."""
    x = F32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, F32(np.inf if n > 0 else -np.inf), dtype=F32)
    return x


def stage_threshold_for(effective, nearest=False):
    """The float32 stageThreshold t with (float)t - 1e-5f == effective in float32 arithmetic (the comparison every kernel
    makes), found among the neighbours of effective + 1e-5. Not every float is such a difference (just below a power of
    two the floats are denser than the differences): nearest=True then returns the t whose difference is closest."""
    effective = F32(effective)
    t0 = F32(np.float64(effective) + np.float64(EPS))
    for k in sorted(range(-8, 9), key=abs):
        t = f32_step(t0, k)
        if F32(t - EPS) == effective and np.signbit(F32(t - EPS)) == np.signbit(effective):
            return t
    for k in sorted(range(-8, 9), key=abs):  # -0.0 is not a difference of two floats: +0.0 compares the same
        t = f32_step(t0, k)
        if F32(t - EPS) == effective:
            return t
    assert nearest, f"no stageThreshold gives the effective threshold {effective!r}"
    return min((f32_step(t0, k) for k in range(-8, 9)), key=lambda t: abs(np.float64(F32(t - EPS)) - np.float64(effective)))


def effective_threshold(t):
    return F32(F32(t) - EPS)


def exact(v):
    """A float as an exact rational."""
    return Fraction(float(v))


# ------------------------------------------------------------------ the predicates, restated with exact integers
def stage_slices(o):
    first = np.concatenate([[0], np.cumsum(o.stage_ntrees)]).astype(int)
    return [slice(first[s], first[s + 1]) for s in range(o.nstages)]


def _frexp_exponent(v):
    """e with v = f * 2^e, f in [0.5, 1): what std::frexp returns for a float (subnormals included)."""
    return int(np.frexp(np.float64(v))[1])


def stage_magnitude(o, s):
    """(sum over the stage's stumps of max(|left|, |right|), q) as exact rationals; q = None for an all-zero stage."""
    sl = stage_slices(o)[s]
    mag = sum((max(abs(exact(l)), abs(exact(r))) for l, r in zip(o.stump_left[sl], o.stump_right[sl])), Fraction(0))
    es = [_frexp_exponent(v) for v in np.concatenate([o.stump_left[sl], o.stump_right[sl]]) if v != 0]
    return mag, (Fraction(2) ** (min(es) - 24) if es else None)


def stage_ratio(o, s):
    """sum max(|l|,|r|) / q of stage s as an exact rational (0 for an all-zero stage)."""
    mag, q = stage_magnitude(o, s)
    return Fraction(0) if q is None else mag / q


def order_independent(o, headroom=1):
    for s in range(o.nstages):
        sl = stage_slices(o)[s]
        if not (np.isfinite(o.stump_left[sl]).all() and np.isfinite(o.stump_right[sl]).all()):
            return False
        if stage_ratio(o, s) * Fraction(headroom) >= 2 ** 53:
            return False
    return True


def quantum_ok(o, s):
    mag, q = stage_magnitude(o, s)
    return q is not None and mag / q < 2 ** 31 - 1


def int_bound(feat):
    """sum |w| * 255 * area * (tilted ? 2 : 1) of one oracle HAAR_DTYPE feature, exact."""
    return sum(abs(exact(feat["wt"][j])) * 255 * int(feat["r"][j][2]) * int(feat["r"][j][3]) * (2 if feat["tilted"] else 1)
               for j in range(3) if feat["wt"][j] != 0 or j < 2)


def int_form_ok(feat):
    ws = [float(feat["wt"][j]) for j in range(3) if feat["wt"][j] != 0 or j < 2]
    return all(w == int(w) and abs(w) <= 64 for w in ws) and int_bound(feat) < 2 ** 24


def value_range(feat, W, H):
    """[vmin, vmax] of the integer value of an upright integer-weight feature over all 8-bit images."""
    net = np.zeros((H + 1, W + 1), np.int64)
    for j in range(3):
        if feat["wt"][j] != 0:
            x, y, w, h = (int(v) for v in feat["r"][j])
            net[y:y + h, x:x + w] += int(feat["wt"][j])
    return 255 * int(net[net < 0].sum()), 255 * int(net[net > 0].sum())


# ------------------------------------------------------------------ orders in which a kernel could add a stage's votes
def sum_sequential(v):
    a = 0.0
    for x in v:
        a += float(x)
    return a


def sum_reversed(v):
    return sum_sequential(list(v)[::-1])


def sum_tree(v, lanes=None):
    """Pairwise tree over the votes padded with zeros to a power of two (lanes: at least that many leaves)."""
    v = [float(x) for x in v]
    n = lanes or 1
    while n < len(v):
        n *= 2
    v += [0.0] * (n - len(v))
    while len(v) > 1:
        v = [v[i] + v[i + 1] for i in range(0, len(v), 2)]
    return v[0]


def sum_strided(v, ns):
    """The stump-split phase: slice s adds stumps s, s + ns, ...; the slices' sums are added in slice order."""
    v = list(v)
    return sum_sequential([sum_sequential(v[s::ns]) for s in range(ns)])


def sum_wave(v):
    """The Haar wave phase: a 64-lane tree sum per chunk of 64 stumps, one `tot +=` per chunk."""
    v = list(v)
    return sum_sequential([sum_tree(v[c:c + 64], 64) for c in range(0, len(v), 64)])


def sum_negmine_wave(v):
    """k_negmine_wave: lane l adds stumps l, l + 64, ...; then the 64-lane tree."""
    v = list(v)
    return sum_tree([sum_sequential(v[l::64]) for l in range(64)], 64)


def sum_delta(votes, rights, parts):
    """The delta form of a generated stage: per part, the part's right leaves as one constant, then left - right for the
    stumps that vote left. rights: the stumps' real right leaves (vote - right is 0 for a stump that votes right)."""
    votes, rights = list(votes), list(rights)
    nt, a = len(votes), 0.0
    for k in range(parts):
        e0, e1 = k * nt // parts, (k + 1) * nt // parts
        if e0 == e1:
            continue
        a += sum_sequential(rights[e0:e1])
        for i in range(e0, e1):
            a += float(votes[i]) - float(rights[i])
    return a


def other_orders(votes, rights):
    return {"reversed": sum_reversed(votes), "tree": sum_tree(votes), "split2": sum_strided(votes, 2), "split4": sum_strided(votes, 4),
            "wave": sum_wave(votes), "negmine_wave": sum_negmine_wave(votes), "delta1": sum_delta(votes, rights, 1),
            "delta8": sum_delta(votes, rights, SPEC_PARTS)}


# ------------------------------------------------------------------ frames
def tie_frame(w, h, seed, block=16):
    """Piecewise-constant frame: a random gray value per block x block square."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, ((h + block - 1) // block, (w + block - 1) // block), dtype=np.uint8)
    return np.ascontiguousarray(np.kron(g, np.ones((block, block), np.uint8))[:h, :w])


def block_frame(w, h, seed):
    """Noise with all-255 and all-0 blocks side by side: windows with variance and extreme rectangle sums."""
    img = frame_uniform(w, h, seed)
    rng = np.random.default_rng(seed + 1)
    for _ in range(10):
        bw, bh = int(rng.integers(30, 90)), int(rng.integers(24, 60))
        x, y = int(rng.integers(0, w - 2 * bw)), int(rng.integers(0, h - bh))
        img[y:y + bh, x:x + bw] = 0
        img[y:y + bh, x + bw:x + 2 * bw] = 255
        if rng.integers(0, 2):
            img[y:y + bh, x:x + 2 * bw] = 255 - img[y:y + bh, x:x + 2 * bw]
    return img


def bright_frame(w, h, seed):
    """Bright natural frame with a saturated block and a half-saturated one."""
    img = frame_natural(w, h, seed, sigma=30.0, mean=215.0)
    img[h // 5:h // 5 + h // 2, w // 8:w // 8 + w // 2] = 255
    return img


# ------------------------------------------------------------------ Haar stump cascades from stump specifications
def cal(left, right, q=0.5, feat=None):
    """A stump whose node threshold is the q-quantile of its feature over the calibration windows."""
    return ("cal", F32(left), F32(right), q, feat)


def forced(vote, other=None):
    """A stump that votes `vote` on every window (it goes left; the right leaf is `other`, default -vote)."""
    return ("fix", F32(vote), F32(-vote if other is None else other), ALWAYS_LEFT, None)


def forced_right(vote, other=None):
    return ("fix", F32(-vote if other is None else other), F32(vote), ALWAYS_RIGHT, None)


def at(thr, left, right, feat=None):
    """A stump with a given node threshold."""
    return ("fix", F32(left), F32(right), thr, feat)


class Built:
    """A cascade text with what the builder knows about it."""

    def __init__(self, xml, kind, W, H, critical, nstages):
        self.xml, self.kind, self.W, self.H, self.critical, self.nstages = xml, kind, W, H, critical, nstages


def haar_cascade(stages, seed, W=24, H=24, critical=None, pool_kinds=None, max_side=None, wins=None, mode="BASIC"):
    """stages: list of (stage threshold rule, [stump specs]). Rules:
        ("eff", value)         that effective threshold (what the sum is compared with: stageThreshold - 1e-5f);
        ("xml", value)         that stageThreshold as written;
        ("mode",)              the most frequent sum of the calibration windows that reach the stage, as effective threshold;
        ("q", quantile, ulps)  the quantile of those sums, moved by `ulps` float32 ulps, as effective threshold.
    Features: drawn without replacement from the BASIC catalog (rectangles of at
    least 16 pixels; pool_kinds = only balanced two- and four-rectangle kinds; max_side bounds the first rectangle)
    unless a stump names its own (an oracle HAAR_DTYPE record). wins: calibration windows (default: those of
    tests/haar_windows.py, cut from a natural frame)."""
    rng = np.random.default_rng(seed)
    cat = orc.haar_catalog(W, H, 0)
    r0 = cat["r"][:, 0]
    ok = r0[:, 2] * r0[:, 3] >= 16
    if pool_kinds == "balanced":  # -1 over the whole, +2 over half of it (x2, y2) or over two quarters (x2_y2)
        area = (cat["r"][:, :, 2] * cat["r"][:, :, 3]).astype(np.int64)
        ok &= (cat["wt"].astype(np.int64) * area).sum(1) == 0
    if max_side:
        ok &= (r0[:, 2] <= max_side) & (r0[:, 3] <= max_side)
    pool = np.nonzero(ok)[0]
    n = sum(len(st) for _, st in stages)
    feats = cat[rng.choice(pool, n, replace=False)].copy()
    k = 0
    for _, st in stages:
        for sp in st:
            if sp[4] is not None:
                feats[k] = sp[4]
            k += 1
    wins = hw.calibration_windows(W, H) if wins is None else wins
    v = cf.calibration_values(feats, wins, W, H)
    alive = np.ones(v.shape[1], bool)
    out, k = [], 0
    for rule, st in stages:
        sums = np.zeros(v.shape[1], np.float64)
        weaks = []
        for (how, left, right, t, _) in st:
            thr = F32(np.quantile(v[k], t)) if how == "cal" else F32(t)
            sums = sums + np.where(v[k] < thr, np.float64(left), np.float64(right))  # sequential, like the CPU
            weaks.append(([(0, -1, k, thr)], [left, right]))
            k += 1
        pick = sums[alive] if alive.sum() > 20 else sums
        if rule[0] == "eff":
            eff = F32(rule[1])
        elif rule[0] == "xml":
            eff = None
        elif rule[0] == "mode":  # the most frequent sum
            vals, counts = np.unique(pick, return_counts=True)
            eff = F32(vals[np.argmax(counts)])
        else:
            eff = f32_step(F32(np.quantile(pick, rule[1], method="lower")), rule[2])
        thr = F32(rule[1]) if eff is None else stage_threshold_for(eff, nearest=rule[0] != "eff")
        out.append((thr, weaks))
        alive &= sums >= np.float64(effective_threshold(thr))
    xml = cf.haar_xml(feats, out, mode=mode, W=W, H=H)
    return Built(xml, "haar", W, H, critical, len(stages))


def _random_leaves(rng, n, step=None):
    """Leaf pairs (a, -a): random floats in (0.25, 1), or (step given) nonzero multiples of `step` in [-1, 1]."""
    if step is None:
        a = rng.uniform(0.25, 1.0, n).astype(F32) * rng.choice([-1.0, 1.0], n).astype(F32)
        return [(x, -x) for x in a]
    m = int(round(1 / step))
    out = []
    for _ in range(n):
        a, b = 0, 0
        while a == 0 or b == 0 or a == b:
            a, b = int(rng.integers(-m, m + 1)), int(rng.integers(-m, m + 1))
        out.append((F32(a * step), F32(b * step)))
    return out


def windows_of(img, W, H, sx=11, sy=7):
    h, w = img.shape
    return np.stack([img[y:y + H, x:x + W] for y in range(0, h - H + 1, sy) for x in range(0, w - W + 1, sx)])


def _cal_stage(rng, n, q=0.55, step=None, ulps=0):
    return (("q", q, ulps), [cal(l, r) for l, r in _random_leaves(rng, n, step)])


# ---- a. the order-independence bound ---------------------------------------------------------------------------------
ODD = 1 + 2.0 ** -23  # exponent 1: the stage's q is 2^-23
# Forced vote sequences whose sequential double sum differs from the sum in every order of other_orders, whatever the
# two calibrated stumps (+-4) behind them vote. WITNESS_AT: sum max / q = 2^54 + ..., between 2^53 and 2^55. WITNESS_FAR:
# leaves of 2^40 beside multiples of 2^-15, q = 2^-33, far above the bound.
WITNESS_AT = [-2.0 ** 29, 1.5, -ODD, -2.0 ** 30, 1 + 2.0 ** -22, ODD, 2.0 ** 29, -ODD, 2.0 ** 30]
WITNESS_FAR = [-2.0 ** 40, 2.0 ** 40, 22 * 2.0 ** -15, 40 * 2.0 ** -15, 7 * 2.0 ** -15, -2.0 ** 40, -40 * 2.0 ** -15, -40 * 2.0 ** -15, 2.0 ** 40]
WITNESS_TAIL = 4.0  # the two calibrated stumps behind a witness vote +-4


def witness_rights(seq):
    """The right leaves of witness_stage(seq): a forced stump votes its left leaf and carries the opposite on the right."""
    return [-v for v in seq] + [-WITNESS_TAIL, WITNESS_TAIL]


def witness_stage(seq):
    return [forced(v) for v in seq] + [cal(WITNESS_TAIL, -WITNESS_TAIL), cal(-WITNESS_TAIL, WITNESS_TAIL)]


def witness_threshold(seq):
    """The effective stage threshold that separates the sequential sum from every other order on the windows whose two
    calibrated stumps cancel: (threshold, sequential sum passes)."""
    lo, hi, s = None, None, None
    for tail in ([WITNESS_TAIL, -WITNESS_TAIL], [-WITNESS_TAIL, WITNESS_TAIL]):
        votes = list(seq) + tail
        s1 = sum_sequential(votes)
        assert s is None or s == s1
        s = s1
        for x in other_orders(votes, witness_rights(seq)).values():
            lo, hi = (x if lo is None else min(lo, x)), (x if hi is None else max(hi, x))
    assert hi < s or lo > s, "the other orders lie on both sides of the sequential sum"
    if hi < s:  # pass needs sum >= thr: the sequential sum itself
        return F32(s), True
    mid = F32((s + lo) / 2)
    assert s < np.float64(mid) <= lo
    return mid, False


def _a_cascade(name):
    rng = np.random.default_rng({"a_below_quarter": 101, "a_between": 102, "a_at_bound": 103, "a_far_above": 104}[name])
    small = [cal(ODD, -ODD), cal(-(1 + 3 * 2.0 ** -23), 1 + 5 * 2.0 ** -23), cal(1.5, -1.25), cal(-ODD, 1.75), cal(1.0, -ODD), cal(-1.5, ODD)]
    if name == "a_below_quarter":   # sum max / q = (2 (2^27 - 2^19) + 8.25 + ...) 2^23: just below 2^51
        x = 2.0 ** 27 - 2.0 ** 19
        crit = (("q", 0.5, 0), [forced(x)] + small[:3] + [forced(-x)] + small[3:])
        stages = [_cal_stage(rng, 6, 0.5), _cal_stage(rng, 10), _cal_stage(rng, 14), crit]
        return haar_cascade(stages, 201, critical=3)
    if name == "a_between":         # 2^52 + ...: order-independent, but not with headroom 4; critical stage in the middle
        x = 2.0 ** 28
        crit = (("q", 0.5, 0), small[:2] + [forced(x), forced_right(-x)] + small[2:])
        stages = [_cal_stage(rng, 6, 0.5), _cal_stage(rng, 10), crit, _cal_stage(rng, 14)]
        return haar_cascade(stages, 202, critical=2)
    if name == "a_at_bound":        # every kernel must add in stump order; critical stage last
        eff, _ = witness_threshold(WITNESS_AT)
        stages = [_cal_stage(rng, 6, 0.5), _cal_stage(rng, 10, 0.6), (("eff", eff), witness_stage(WITNESS_AT))]
        return haar_cascade(stages, 203, critical=2)
    eff, _ = witness_threshold(WITNESS_FAR)
    stages = [_cal_stage(rng, 6, 0.5), _cal_stage(rng, 6, 0.4), (("eff", eff), witness_stage(WITNESS_FAR)), _cal_stage(rng, 10, 0.5), _cal_stage(rng, 12, 0.5)]
    return haar_cascade(stages, 204, critical=2)


# ---- b. the int32 vote bound -----------------------------------------------------------------------------------------
B_LAST = {"b_below": 1 - 2.0 ** -23, "b_at": 1 - 2.0 ** -24, "b_above": 1 - 2.0 ** -24}  # q = 2^-24 in all three
B_ONES = {"b_below": 127, "b_at": 127, "b_above": 128}  # sum / q = 2^31 - 2, 2^31 - 1, 2^31 + 2^24 - 1


def _b_cascade(name):
    """Stage 2: every forced vote +1 (b_at: -1), so that the sum reaches +-(sum max) on the windows whose calibrated stumps
    agree; stage 3: the forced votes alternate; stage 4: left and right leaves of one sign and different magnitudes."""
    rng = np.random.default_rng({"b_below": 111, "b_at": 112, "b_above": 113}[name])
    ones, last = B_ONES[name], B_LAST[name]
    sign = -1.0 if name == "b_at" else 1.0
    nvar = 3
    # the calibrated stumps of stage 2 have both leaves of the stage's sign: every window's sum is within 1.5 of the extreme.
    # Its threshold passes the windows on which at least two of the three vote 1 (-1: at most one); stage 3 those on which
    # two of its three calibrated stumps vote +1.
    same = [forced(sign)] * (ones - nvar) + [cal(sign, sign * 0.5, 0.5) for _ in range(nvar)] + [forced(sign * last)]
    alt = [forced(1.0 if i % 2 == 0 else -1.0) for i in range(ones - nvar)] + [cal(1.0, -1.0), cal(-1.0, 1.0), cal(1.0, -1.0)] + [forced_right(last)]
    mixed = [cal(0.75, 0.125), cal(-0.5, -0.875), cal(0.25, 1.0), cal(-1.0, -0.375), forced(0.625, 0.5), forced_right(-0.25, -0.125), cal(0.5, 0.0), cal(0.0, -0.5)]
    stages = [_cal_stage(rng, 6, 0.5), _cal_stage(rng, 4, 0.4), (("eff", sign * (ones + 0.25)), same), (("eff", 0.5), alt), (("q", 0.5, 0), mixed)]
    return haar_cascade(stages, 210 + len(name), critical=2)


# ---- c. weights ------------------------------------------------------------------------------------------------------
def _feat(rects, tilted=False):
    return orc.make_haar_feature(tilted, rects)[0]


def c_features(W, H):
    """name -> feature. The 75x32 window holds upright features only; the largest areas and the tilted ones need 128x40."""
    f = {}
    if (W, H) == (75, 32):
        f["w64"] = _feat([(5, 3, 20, 25, 64.0), (30, 3, 20, 25, -64.0)])          # 128 * 500 * 255 < 2^24: integer form
        f["w65"] = _feat([(5, 3, 20, 25, 65.0), (30, 3, 20, 25, -65.0)])          # |w| > 64: float form
        f["frac"] = _feat([(2, 2, 60, 28, 2.5), (10, 8, 40, 20, -0.75)])          # non-integer weights
        # 529 px: 127 * 255 * 529 is odd and > 2^24; 46 x 23 of the window, so that a window with the feature on a saturated
        # block still has variance
        f["sat_odd"] = _feat([(2, 3, 23, 23, 127.0), (25, 3, 23, 23, -127.0)])
        f["tri"] = _feat([(0, 0, 50, 30, 63.0), (12, 1, 50, 30, -61.0), (25, 2, 50, 30, 59.0)])  # 1500 px each: 63 * r > 2^24 from a mean of 178 on
    else:
        f["below"] = _feat([(1, 1, 13, 5, -1.0), (20, 2, 79, 13, 64.0)])          # 65 + 64 * 1027 = 65793: 255 * that = 2^24 - 1
        f["above"] = _feat([(1, 1, 11, 6, -1.0), (20, 2, 79, 13, 64.0)])          # 65794: 2^24 + 254
        f["tilt_below"] = _feat([(64, 0, 18, 18, 64.0), (66, 2, 14, 14, -62.0)], True)  # 2 * 255 * 32888 = 2^24 - 4336
        f["tilt_above"] = _feat([(64, 0, 18, 18, 64.0), (66, 2, 14, 14, -64.0)], True)  # 2 * 255 * 33280 > 2^24
        f["sat_odd"] = _feat([(4, 1, 55, 19, 63.0), (4, 20, 55, 19, -63.0)])      # 1045 px, odd: 63 * 255 * 1045 is odd and > 2^24
        f["sat_odd2"] = _feat([(6, 2, 57, 19, 61.0), (63, 2, 57, 19, -61.0)])     # 1083 px: 61 * 255 * 1083 odd, > 2^24
        f["wide63"] = _feat([(2, 1, 60, 30, 63.0), (64, 0, 64, 40, -1.0)])        # 63 * 1800 + 2560: bound 2.96e7 in [2^24, 3e7)
        f["tri_big"] = _feat([(0, 0, 52, 40, 63.0), (38, 0, 52, 40, -61.0), (76, 0, 52, 40, 59.0)])  # 2080 px each
    return f


def _c_cascade(name):
    W, H = (75, 32) if name == "c_75x32" else (128, 40)
    fs = c_features(W, H)
    rng = np.random.default_rng(121 if W == 75 else 122)
    tiny = F32(1e-30)
    stumps = []
    for key, feat in fs.items():
        l, r = _random_leaves(rng, 1, 0.125)[0]
        if key.startswith("sat"):  # exactly 0 on a saturated block unless the products are fused: thresholds next to 0
            stumps += [at(tiny, l, r, feat), at(-tiny, r, l, feat), at(0.0, l, r, feat)]
        else:
            stumps += [cal(l, r, 0.5, feat), cal(r, l, 0.3, feat)]
    half = len(stumps) // 2
    stages = [(("q", 0.4, 0), stumps[:half]), (("q", 0.5, 0), stumps[half:]), _cal_stage(rng, 5, 0.5, 0.125)]
    wins = np.concatenate([windows_of(bright_frame(400, 300, 70), W, H, 9, 5), hw.calibration_windows(W, H)[::4]])
    return haar_cascade(stages, 220 + W, W=W, H=H, critical=1, wins=wins, mode="ALL" if W == 128 else "BASIC")  # 128x40 holds tilted features


# The upper side of the int_ok bound: integer-weight features with sum |w| 255 area in [2^24, 3e7), outside int_ok although a
# bound widened to 3e7 would let them in. Each has a reference window on which the float expression and the one-int32
# combination give different values; that window is pasted into the frame several times and the stump's node threshold is
# the larger of the two normalised values, so the two forms fall on different sides of it (as the sat_odd thresholds sit
# next to 0). The stumps sit in the last stage behind a stage that passes everything: every window's last sum is reported.
INT_EDGE = [
    _feat([(2, 1, 60, 30, 63.0), (64, 0, 64, 40, -1.0)]),     # 63 * 1800 + 2560 = 115960: bound 2.957e7
    _feat([(1, 2, 62, 30, 61.0), (20, 0, 100, 40, -1.0)]),    # 61 * 1860 + 4000 = 117460: 2.995e7
    _feat([(60, 4, 64, 31, 59.0), (3, 3, 20, 20, 1.0)]),      # 59 * 1984 + 400 = 117456: 2.995e7
]
INT_EDGE_SLOTS = [(x, y) for y in (6, 50, 94, 138, 182, 226) for x in (4, 136, 268)]  # even: on the grid of the first scale


def haar_forms(feat, sums):
    """Value of an upright feature from its rectangle sums (n x nrect int64) as float32 arrays: the float expression
    w0*(float)r0 + w1*(float)r1 [+ w2*(float)r2], the fused form fma(w0, r0, w1*r1) [then fma(w2, r2, .)] with one rounding
    each, and (integer weights) one integer combination with one conversion."""
    w = [F32(x) for x in feat["wt"] if x != 0]
    r = [sums[:, j] for j in range(len(w))]
    sep = w[0] * r[0].astype(F32) + w[1] * r[1].astype(F32)
    fused = (np.float64(w[0]) * r[0] + np.float64(w[1] * r[1].astype(F32))).astype(F32)
    if len(w) == 3:
        sep = sep + w[2] * r[2].astype(F32)
        fused = (np.float64(w[2]) * r[2] + np.float64(fused)).astype(F32)
    whole = None
    if all(float(x) == int(x) for x in w):
        whole = sum(int(x) * rj for x, rj in zip(w, r)).astype(np.float64).astype(F32)
    return sep, fused, whole


def _integral(a):
    ii = np.zeros((a.shape[0] + 1, a.shape[1] + 1), np.int64)
    ii[1:, 1:] = a.astype(np.int64).cumsum(0).cumsum(1)
    return ii


def _rect(ii, ys, xs, x, y, w, h):
    return ii[ys + y + h, xs + x + w] - ii[ys + y, xs + x + w] - ii[ys + y + h, xs + x] + ii[ys + y, xs + x]


def window_values(feat, img, xs, ys, W, H):
    """Normalised values (float, fused, integer form) of an upright feature on the W x H windows of img at (xs, ys), as the
    detector forms them: value * vnf in float32, vnf = (float)(1 / sqrt(area * sqsum - sum^2)) over the window minus a
    one-pixel border. Also returns which windows have variance."""
    ii, sq = _integral(img), _integral(img.astype(np.int64) ** 2)
    area = (W - 2) * (H - 2)
    vs, vq = _rect(ii, ys, xs, 1, 1, W - 2, H - 2), _rect(sq, ys, xs, 1, 1, W - 2, H - 2)
    nf = np.float64(area) * vq.astype(np.float64) - vs.astype(np.float64) * vs.astype(np.float64)
    ok = nf > 0
    vnf = np.where(ok, 1.0 / np.sqrt(np.where(ok, nf, 1.0)), 1.0).astype(F32)
    ok &= np.float64(area) * vnf.astype(np.float64) < 1e-1
    cols = [_rect(ii, ys, xs, *(int(v) for v in feat["r"][j])) for j in range(3) if feat["wt"][j] != 0]
    forms = haar_forms(feat, np.stack(cols, 1))
    return [None if f is None else f * vnf for f in forms], ok


def emulate_first_scale(o, img, sf, form=0):
    """Result codes and stage sums of an upright Haar stump cascade on the first scale (the frame itself) with the feature
    values in the given form (0 float, 1 fused, 2 integer where the weights are integers): the oracle's walk in numpy."""
    sc = orc.scales(o.win_w, o.win_h, img.shape[1], img.shape[0], sf)[0]
    assert (int(sc["w"]), int(sc["h"])) == img.shape[::-1]
    nx, ny, st = int(sc["nx"]), int(sc["ny"]), int(sc["ystep"])
    ys, xs = (v.ravel() for v in np.meshgrid(np.arange(ny) * st, np.arange(nx) * st, indexing="ij"))
    codes, sums, alive, ok = np.ones(nx * ny, np.int32), np.zeros(nx * ny), None, None
    sl = stage_slices(o)
    for s in range(o.nstages):
        acc = np.zeros(nx * ny)
        for k in range(sl[s].start, sl[s].stop):
            vals, ok = window_values(o.haar[o.stump_feature[k]], img, xs, ys, o.win_w, o.win_h)
            v = vals[form] if vals[form] is not None else vals[0]
            acc = acc + np.where(v < o.stump_threshold[k], np.float64(o.stump_left[k]), np.float64(o.stump_right[k]))
        if alive is None:
            alive = ok.copy()
            codes[~ok], sums[~ok] = -1, 0.0
        sums[alive] = acc[alive]
        fail = alive & (acc < np.float64(effective_threshold(o.stage_threshold[s])))
        codes[fail] = -s
        alive &= ~fail
    return codes, sums


def _int_edge_sources():
    """One reference window per INT_EDGE feature, cut from a bright frame: the first on which the float form and the
    integer form of the normalised value differ."""
    src = bright_frame(640, 480, 90)
    out = []
    ys, xs = (v.ravel() for v in np.meshgrid(np.arange(0, 480 - 40, 3), np.arange(0, 640 - 128, 5), indexing="ij"))
    for feat in INT_EDGE:
        (vf, _, vi), ok = window_values(feat, src, xs, ys, 128, 40)
        i = int(np.nonzero(ok & (vf != vi))[0][0])
        out.append((src[ys[i]:ys[i] + 40, xs[i]:xs[i] + 128].copy(), F32(max(vf[i], vi[i]))))
    return out


def int_edge_frame():
    img = bright_frame(400, 300, 91)
    src = _int_edge_sources()
    for n, (x, y) in enumerate(INT_EDGE_SLOTS):
        img[y:y + 40, x:x + 128] = src[n % len(src)][0]
    return img


def _c_int_edge():
    rng = np.random.default_rng(123)
    ties = [at(thr, l, r, feat) for feat, (_, thr), (l, r) in zip(INT_EDGE, _int_edge_sources(), _random_leaves(rng, 3, 0.125))]
    first = (("eff", -100.0), [cal(0.5, -0.5), cal(-0.25, 0.75)])
    last = (("q", 0.5, 0), ties + [cal(l, r) for l, r in _random_leaves(rng, 3, 0.125)])
    wins = np.concatenate([windows_of(int_edge_frame(), 128, 40, 9, 5), hw.calibration_windows(128, 40)[::4]])
    return haar_cascade([first, last], 223, W=128, H=40, critical=1, wins=wins)


# ---- d. 16-bit tile ranges -------------------------------------------------------------------------------------------
def d_features(W, H):
    f = {}
    if (W, H) == (24, 24):
        f["net128"] = [_feat([(x, y, 16, 16, -1.0), (x + 8, y, 8, 16, 2.0)]) for (x, y) in ((0, 0), (3, 5), (8, 8), (5, 2))]   # vmax 32640
        f["area256"] = [_feat([(2, 3, 16, 16, -1.0), (2, 3, 16, 8, 2.0)]), _feat([(7, 1, 16, 16, -1.0), (15, 1, 8, 16, 2.0)])]
        f["area260"] = [_feat([(1, 2, 20, 13, -1.0), (11, 2, 10, 13, 2.0)]), _feat([(4, 0, 13, 20, -1.0), (4, 10, 13, 10, 2.0)])]
        f["area264"] = [_feat([(0, 6, 24, 11, -1.0), (12, 6, 12, 11, 2.0)])]
        f["row"] = [_feat([(0, 11, 24, 1, -1.0), (12, 11, 12, 1, 2.0)]), _feat([(0, 0, 24, 1, -1.0), (0, 0, 12, 1, 2.0)])]
        f["column"] = [_feat([(23, 0, 1, 24, -1.0), (23, 12, 1, 12, 2.0)])]
        # net positive area 129 = 43 x 3 does not fit 24 x 24; 129 pixels as three rectangles: 8 x 16 + 1 x 1 on the +1 side
        f["net129"] = [_feat([(x, y, 16, 16, -1.0), (x + 8, y, 8, 16, 2.0), (x + 16, y + 3, 1, 1, 1.0)]) for (x, y) in ((0, 0), (3, 5), (7, 8), (5, 2))]
        f["neg129"] = [_feat([(x, y, 16, 16, 1.0), (x + 8, y, 8, 16, -2.0), (x + 16, y + 3, 1, 1, -1.0)]) for (x, y) in ((1, 1), (6, 4))]
    else:  # 44 x 12
        f["area258"] = [_feat([(0, 3, 43, 6, -1.0), (0, 3, 43, 3, 2.0)]), _feat([(1, 0, 43, 6, 1.0), (1, 6, 43, 6, -1.0)])]
        f["net129"] = [_feat([(x, y, 43, 6, -1.0), (x, y + 3, 43, 3, 2.0)]) for (x, y) in ((0, 0), (1, 5), (0, 6))]
        f["net128"] = [_feat([(x, y, 32, 8, -1.0), (x, y + 4, 32, 4, 2.0)]) for (x, y) in ((0, 0), (11, 3))]
        f["row"] = [_feat([(0, 5, 44, 1, -1.0), (22, 5, 22, 1, 2.0)])]
    return f


def _d_cascade(name):
    W, H = (24, 24) if name == "d_24x24" else (44, 12)
    rng = np.random.default_rng(131 if W == 24 else 132)
    stumps = []
    for key, feats in d_features(W, H).items():
        for feat in feats:
            l, r = _random_leaves(rng, 1, 0.125)[0]
            stumps += [at(0.0, l, r, feat), cal(r, l, 0.4, feat)]
    rng.shuffle(stumps)
    third = len(stumps) // 3
    stages = [(("q", 0.5, 0), stumps[:third]), (("q", 0.55, 0), stumps[third:2 * third]), (("q", 0.55, 0), stumps[2 * third:])]
    wins = np.concatenate([windows_of(block_frame(400, 300, 79), W, H), hw.calibration_windows(W, H)[::4]])
    return haar_cascade(stages, 230 + W, W=W, H=H, critical=2, wins=wins)


# ---- e. shape limits -------------------------------------------------------------------------------------------------
def _e_many_stages(n):
    """n single-stump stages. Most pass every window (threshold below both leaves); every seventh and the last five let
    80 % of the windows through, so that every exit code up to -(n - 1) occurs and windows reach the end."""
    rng = np.random.default_rng(140 + n)
    stages = []
    for s in range(n):
        l, r = _random_leaves(rng, 1, 0.125)[0]
        real = s % 7 == 0 or s >= n - 5
        if real:
            stages.append((("eff", max(l, r)), [cal(l, r, 0.2 if r > l else 0.8)]))
        else:
            stages.append((("eff", min(l, r) - F32(0.5)), [cal(l, r, 0.5)]))
    return haar_cascade(stages, 240 + n, critical=n - 1)


E_SIZES = {"e_sizes_small": (8, 1, 2, 3, 63, 64, 65), "e_sizes_large": (8, 128, 129)}  # each within the specialiser's 320 stumps


def _e_sizes(name):
    rng = np.random.default_rng(151 if name == "e_sizes_small" else 152)
    sizes = E_SIZES[name]
    stages = [_cal_stage(rng, nt, 0.5, 0.125) for nt in sizes]
    return haar_cascade(stages, 250 + len(sizes), critical=len(sizes) - 1)


LBP_SIZES = {
    "e_lbp_64": ((24, 24), (4, 6, 64, 30, 34, 14, 7, 7)),    # a stage of 64; 30 + 34 = 64: one chunk; groups 14 | 7 + 7
    "e_lbp_65": ((24, 24), (4, 6, 30, 35, 15, 7, 8, 5)),     # 30 + 35 = 65: two chunks; 15 alone; 7 + 8 = 15: two groups
    "e_lbp_long": ((24, 24), (4, 65, 5, 14)),                # a stage of 65: no wave phase
    "e_lbp_31x57": ((31, 57), (3, 5, 64, 7, 7, 8)),
}


def lbp_cascade(W, H, sizes, seed, step=None, tie_thresholds=False, critical=None):
    """LBP stump cascade whose stage thresholds are quantiles of the sums of the calibration windows that reach the
    stage. step: leaves are multiples of it (ties at the stage thresholds, which are reachable sums then)."""
    rng = np.random.default_rng(seed)
    cat = orc.lbp_catalog(W, H)
    n = sum(sizes)
    rects = cat[rng.choice(len(cat), n, replace=False)]
    wins = hw.calibration_windows(W, H)
    s, _, _ = orc.set_images(wins, want_norm=False)
    codes = orc.lbp_eval_batch(rects, 0, n, s, W, H).astype(np.int64)
    alive = np.ones(codes.shape[1], bool)
    stages, k = [], 0
    for si, nt in enumerate(sizes):
        sums = np.zeros(codes.shape[1], np.float64)
        weaks = []
        for (l, r) in _random_leaves(rng, nt, step):
            sub = rng.integers(-2 ** 31, 2 ** 31, 8)
            bit = (sub[codes[k] >> 5] >> (codes[k] & 31)) & 1
            sums = sums + np.where(bit != 0, np.float64(l), np.float64(r))
            weaks.append(([(0, -1, k, sub)], [l, r]))
            k += 1
        pick = sums[alive] if alive.sum() > 20 else sums
        eff = F32(np.quantile(pick, 0.45, method="lower"))
        if tie_thresholds:
            ulps = (0, 0, 1, -1)[si % 4]
            if ulps and eff == 0:  # the floats next to 0 are not differences of a threshold and 1e-5f: take the next sum
                eff = F32(step)
            eff = f32_step(eff, ulps)
        else:
            eff = F32(eff) if step else F32(eff - F32(1e-3))
        thr = stage_threshold_for(eff, nearest=True)
        stages.append((thr, weaks))
        alive &= sums >= np.float64(effective_threshold(thr))
    return Built(cf.lbp_xml(rects, stages, W=W, H=H), "lbp", W, H, len(sizes) - 1 if critical is None else critical, len(sizes))


# ---- f. ties ---------------------------------------------------------------------------------------------------------
def _f_node_ties(plain=False):
    """Balanced features of at most 10 x 10 pixels with node thresholds 0.0 and -0.0; leaves in multiples of 2^-3.
    plain: two forced votes of +-2^25 in stage 2, whose q is 2^-26, put the cascade outside the delta form (sum max / q =
    2^52 + ...), so that the generated stages compare in the plain form `v < thr ? left : right`."""
    rng = np.random.default_rng(161)
    stages = []
    for si, nt in enumerate((6, 8, 10, 12)):
        st = []
        for i, (l, r) in enumerate(_random_leaves(rng, nt, 0.125)):
            st.append(at(-0.0 if i % 3 == 1 else 0.0, l, r))
        if plain and si == 2:
            st = st[:3] + [forced(2.0 ** 25), at(0.0, ODD, -1.0)] + st[3:] + [forced_right(-2.0 ** 25)]
        stages.append((("q", 0.5, 0), st))
    return haar_cascade(stages, 261, critical=3, pool_kinds="balanced", max_side=10, wins=windows_of(tie_frame(400, 300, 80), 24, 24))


def _f_stage_ties():
    """Stage thresholds on reachable sums: the most frequent sum, 0.0, one float32 ulp above a reachable sum, one ulp
    below one, the median sum itself, and a stageThreshold written as -0.0 (an effective threshold of -1e-5f: an effective -0.0 does
    not exist, t - 1e-5f is never -0.0, and +0.0 compares the same)."""
    rng = np.random.default_rng(162)
    stages = []
    for si, nt in enumerate((6, 7, 8, 9, 10, 6)):
        leaves = _random_leaves(rng, nt, 0.125)
        st = [at(0.0, l, r) if i % 2 else cal(l, r) for i, (l, r) in enumerate(leaves)]
        rule = [("mode",), ("eff", 0.0), ("q", 0.5, 1), ("q", 0.5, -1), ("q", 0.5, 0), ("xml", -0.0)][si]
        stages.append((rule, st))
    return haar_cascade(stages, 262, critical=5, pool_kinds="balanced", max_side=10, wins=windows_of(tie_frame(400, 300, 80), 24, 24))


# ---- g. a single stage -----------------------------------------------------------------------------------------------
# Cascades of ONE stage: the dense phase of the cascade kernel emits the candidates itself, nothing is ever queued. One per
# feature kind and weak-classifier form, from the factories of tests/cascade_factory.py; the Haar ones are calibrated on
# the 24 x 24 windows of the frame they run on. name -> (kind, stump cascade, factory)
ONE_STAGE = {
    "g_one_stage_lbp_stump": ("lbp", True, lambda cal: cf.lbp_stump_cascade(24, 24, seed=41, stage_sizes=(3,))),
    "g_one_stage_lbp_tree": ("lbp", False, lambda cal: cf.lbp_tree_cascade(seed=31, stage_sizes=(3,))),
    "g_one_stage_haar_tree": ("haar", False, lambda cal: cf.haar_tree_cascade(cal, seed=21, stage_sizes=(4,))),
    "g_one_stage_tilted_stump": ("haar", True, lambda cal: cf.tilted_stump_cascade(cal, seed=11, stage_sizes=(6,))),
}


def one_stage_frame():
    """200 x 120 at scale factor 1.25: 11 439 grid windows, scales of both steps, a partial tile in each direction."""
    return frame_natural(200, 120, 5), 1.25


def _g_cascade(name):
    kind, _, make = ONE_STAGE[name]
    return Built(make(windows_of(one_stage_frame()[0], 24, 24)), kind, 24, 24, 0, 1)


# ------------------------------------------------------------------ the table
A_NAMES = ["a_below_quarter", "a_between", "a_at_bound", "a_far_above"]
B_NAMES = ["b_below", "b_at", "b_above"]
C_NAMES = ["c_75x32", "c_128x40", "c_int_edge"]
D_NAMES = ["d_24x24", "d_44x12"]
E_HAAR_NAMES = ["e_63_stages", "e_sizes_small", "e_sizes_large"]
E_LBP_NAMES = list(LBP_SIZES)
F_NAMES = ["f_node_ties", "f_node_ties_plain", "f_stage_ties", "f_lbp_ties"]
NAMES = A_NAMES + B_NAMES + C_NAMES + D_NAMES + E_HAAR_NAMES + E_LBP_NAMES + F_NAMES
G_NAMES = list(ONE_STAGE)  # one frame each, tests of their own: not part of NAMES
REFUSED = "e_64_stages"  # built like e_63_stages; the detector refuses it


@functools.lru_cache(maxsize=None)
def built(name):
    if name in A_NAMES:
        return _a_cascade(name)
    if name in B_NAMES:
        return _b_cascade(name)
    if name == "c_int_edge":
        return _c_int_edge()
    if name in C_NAMES:
        return _c_cascade(name)
    if name in D_NAMES:
        return _d_cascade(name)
    if name == "e_63_stages":
        return _e_many_stages(63)
    if name == "e_64_stages":
        return _e_many_stages(64)
    if name in E_SIZES:
        return _e_sizes(name)
    if name in LBP_SIZES:
        (W, H), sizes = LBP_SIZES[name]
        return lbp_cascade(W, H, sizes, 170 + len(name) + W)
    if name == "f_node_ties":
        return _f_node_ties()
    if name == "f_node_ties_plain":
        return _f_node_ties(plain=True)
    if name == "f_stage_ties":
        return _f_stage_ties()
    if name == "f_lbp_ties":
        return lbp_cascade(24, 24, (4, 6, 8, 10, 12, 9), 181, step=0.125, tie_thresholds=True)
    if name in ONE_STAGE:
        return _g_cascade(name)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def frames(name):
    """(frame, scale factor) pairs of a cascade: at most 400 x 300, two scale factors (one-stage cascades: one frame)."""
    if name in ONE_STAGE:
        return [one_stage_frame()]
    b = built(name)
    W, H = b.W, b.H
    if name == "c_int_edge":
        return [(int_edge_frame(), 1.2), (bright_frame(330, 170, 72), 1.45)]
    if name in C_NAMES:
        return [(bright_frame(400, 300, 71), 1.2), (bright_frame(330, 170, 72), 1.45)]
    if name in D_NAMES:
        return [(block_frame(400, 300, 73), 1.15), (block_frame(320, 200, 74), 1.4)]
    if name in ("f_node_ties", "f_node_ties_plain", "f_stage_ties"):
        return [(tie_frame(400, 300, 75), 1.1), (tie_frame(333, 227, 76), 1.3)]
    return [(hw.pasted_frame(W, H, 77), 1.1), (hw.pasted_frame(W, H, 78, 333, 227), 1.3)]


def oracle_cascade(tmp, name):
    return hw.oracle_cascade(tmp, built(name).xml, name + ".xml")


def reached(codes, stage):
    """Windows that entered `stage`, from the oracle's result codes. Code -1 is 'rejected by stage 1' and 'no variance'
    alike, so the windows rejected by stage 1 are counted neither for stage 0 nor for stage 1."""
    if stage == 0:
        return codes != -1
    return (codes == 1) | (codes <= -max(stage, 2))


def truncated(o, k):
    """The oracle's stump cascade cut after stage k."""
    import dataclasses
    n = int(o.stage_ntrees[:k + 1].sum())
    sub = o.subset_size
    return dataclasses.replace(o, stage_ntrees=o.stage_ntrees[:k + 1].copy(), stage_threshold=o.stage_threshold[:k + 1].copy(),
                               stump_feature=o.stump_feature[:n].copy(), stump_threshold=o.stump_threshold[:n].copy(),
                               stump_left=o.stump_left[:n].copy(), stump_right=o.stump_right[:n].copy(),
                               stump_subset=o.stump_subset[:n * sub].copy(), tree_nnodes=o.tree_nnodes[:n].copy(),
                               node_left=o.node_left[:n].copy(), node_right=o.node_right[:n].copy(), node_feature=o.node_feature[:n].copy(),
                               node_threshold=o.node_threshold[:n].copy(), node_subset=o.node_subset[:n * sub].copy(),
                               leaves=o.leaves[:2 * n].copy(), _keep=[])


def tile_counts(o, img, sf, codes, stage):
    """Windows that entered `stage` per tile of 64 x 8 window origins (the cascade kernel's blocks), all scales."""
    h, w = img.shape
    out, first = [], 0
    for sc in orc.scales(o.win_w, o.win_h, w, h, sf):
        nx, ny = int(sc["nx"]), int(sc["ny"])
        m = reached(codes[first:first + nx * ny], stage).reshape(ny, nx)
        first += nx * ny
        for ty in range(0, ny, 8):
            for tx in range(0, nx, 64):
                out.append(int(m[ty:ty + 8, tx:tx + 64].sum()))
    return np.array(out)


def zero_value_pairs(o, img, sf, codes):
    """(window, node) pairs of a Haar cascade of integer-weight upright features with v == thr: the node threshold is
    +-0.0, the feature's integer value is 0 (so v = 0 * vnf = 0), and the window entered the node's stage."""
    h, w = img.shape
    sl = stage_slices(o)
    total, first = 0, 0
    for sc in orc.scales(o.win_w, o.win_h, w, h, sf):
        nx, ny, st = int(sc["nx"]), int(sc["ny"]), int(sc["ystep"])
        small = orc.resize_linear_exact(img, int(sc["w"]), int(sc["h"]))
        ii = np.zeros((small.shape[0] + 1, small.shape[1] + 1), np.int64)
        ii[1:, 1:] = small.astype(np.int64).cumsum(0).cumsum(1)
        c = codes[first:first + nx * ny].reshape(ny, nx)
        first += nx * ny
        ys, xs = np.arange(ny)[:, None] * st, np.arange(nx)[None, :] * st
        for s in range(o.nstages):
            inside = reached(c.ravel(), s).reshape(ny, nx)
            for k in range(sl[s].start, sl[s].stop):
                if o.stump_threshold[k] != 0:
                    continue
                f = o.haar[o.stump_feature[k]]
                val = np.zeros((ny, nx), np.int64)
                for j in range(3):
                    if f["wt"][j] != 0:
                        x, y, rw, rh = (int(v) for v in f["r"][j])
                        val += int(f["wt"][j]) * (ii[ys + y + rh, xs + x + rw] - ii[ys + y, xs + x + rw] - ii[ys + y + rh, xs + x] + ii[ys + y, xs + x])
                total += int(((val == 0) & inside).sum())
    return total


def sample_windows(name, n=500):
    """About n windows of the cascade's size cut from its first frame (training-side predict)."""
    b = built(name)
    img = frames(name)[0][0]
    h, w = img.shape
    pos = [(x, y) for y in range(0, h - b.H + 1, 7) for x in range(0, w - b.W + 1, 5)]
    pos = pos[::max(1, len(pos) // n)][:n]
    return np.stack([img[y:y + b.H, x:x + b.W] for (x, y) in pos])
