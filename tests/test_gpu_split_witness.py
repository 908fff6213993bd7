"""The device split search (cc_eval_presort / cc_eval_find_best_split, the kernels of cc_split.hip) held directly to the
exact witness of tests/split_witness.py. The feature values come from the device's own calc_batch (pinned elsewhere
against the oracle and against direct summation), so this file tests the search alone and never asks the oracle for a
split. Per variable the witness checks (a) legality, (b) the reported quality against the exact one, (c) nearness to
the exact maximum, (d) identity with the exact argmax where the variable is decided, (e) "no split"; then the winner
over variables. LBP variables report only how many categories go left; the witness lists the left sums that count can
stand for (split_witness.Node._sums_of_count), and the winner's subset is judged as a subset.

Which variables are checked (`_subset`): exact arithmetic over a whole catalog is too slow, so of F variables the check
takes every k-th (k = max(1, F // 75); F // 8 for the nodes of 17 000 samples and more, where one variable costs a
second of integer arithmetic), the device's winner, and the twenty variables with the highest device quality.

Every search (`_hold`) also asserts: the device's unrounded double quality within B of the exact one, besides the
float32 window of (b); no checked cut toothless (B infinite) and no LBP count weak (unresolved), since either would
pass (b) unchecked; and, with continuous weights, at least 95 % of the checked variables that have a split decided.
Searches with one weight per class (round 0) are exempt from the last by construction and print their share.
"""
import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import evaluator as ev
from tests import split_witness as sw

pytestmark = pytest.mark.gpu

WIN = (12, 10)
COMBOS = [(ev.BOOST_GENTLE, 0), (ev.BOOST_LOGIT, 0), (ev.BOOST_REAL, 0), (ev.BOOST_DISCRETE, 0), (ev.BOOST_REAL, ev.SPLIT_MISCLASS),
          (ev.BOOST_DISCRETE, ev.SPLIT_GINI)]


def _samples(n, win, seed, dup=0):
    """Template + noise 'positives', uniform-noise 'negatives', shuffled; `dup` samples repeat another one."""
    rng = np.random.default_rng(seed)
    W, H = win
    yy, xx = np.mgrid[0:H, 0:W]
    tmpl = 128 + 60 * np.sin(xx / W * 3.1) * np.cos(yy / H * 2.3)
    npos = n // 2
    pos = np.clip(tmpl[None] + rng.normal(0, 15, (npos, H, W)), 0, 255).astype(np.uint8)
    neg = rng.integers(0, 256, (n - npos, H, W), dtype=np.uint8)
    imgs = np.concatenate([pos, neg])
    labels = np.concatenate([np.ones(npos, np.uint8), np.zeros(n - npos, np.uint8)])
    perm = rng.permutation(n)
    imgs, labels = imgs[perm], labels[perm]
    for k in range(dup):
        imgs[(7 * k + 3) % n] = imgs[(11 * k + 1) % n]
    return imgs, labels


def _setup(ftype, mode, win, n, seed, dup=0):
    imgs, labels = _samples(n, win, seed, dup)
    e = cc.CvFeatureEvaluator.create(ftype)
    e.init(cc.CvFeatureParams.create(ftype) if ftype == ev.HOG else cc.CvFeatureParams(ftype, mode), n, win)
    e.setImages(imgs, labels)
    e.presort()
    return e, labels


def _node_inputs(lab, boost_type, seed, weights="cubic", real=False):
    """weights (n + 2, totals as plain running sums in node order), node_value and responses / class labels."""
    n = len(lab)
    rng = np.random.default_rng(seed)
    if isinstance(weights, str) and weights == "equal":
        w = np.where(lab == 1, 0.5 / max(lab.sum(), 1), 0.5 / max(n - lab.sum(), 1))
    elif isinstance(weights, str):
        w = rng.random(n) ** 3 + 1e-3
        w /= w.sum()
    else:
        w = weights
    classifier = boost_type in (ev.BOOST_DISCRETE, ev.BOOST_REAL)
    if classifier:
        r = [0.0, 0.0]
        for i in range(n):
            r[int(lab[i])] += w[i]
        return np.concatenate([w, r]), 0.0, {"class_labels": lab.astype(np.int32)}
    resp = (lab.astype(np.int32) * 2 - 1).astype(np.float32)
    if real:
        resp = (resp * (rng.random(n) * 3 + 0.01)).astype(np.float32)
    tot = s = 0.0
    for i in range(n):
        tot += w[i]
        s += float(resp[i]) * w[i]
    return np.concatenate([w, [tot, 0.0]]), s * (1.0 / tot), {"responses": resp}


def _subset(F, q, winner, target=75):
    """Every k-th variable (k = max(1, F // target)), the device's winner and the twenty highest device qualities."""
    k = max(1, F // target)
    pick = set(range(0, F, k)) | set(np.argsort(-q, kind="stable")[:20].tolist())
    if winner is not None:
        pick.add(winner)
    return sorted(pick)


def _hold(e, labels, *, boost_type, criteria=0, sample_idx=None, seed=0, weights="cubic", real=False, lo=0):
    """One device search held to the witness. Returns the device result and the share of decided variables."""
    ftype = e.feature_type
    idx = None if sample_idx is None else np.asarray(sample_idx, np.int32)
    lab = labels.astype(np.int64) if idx is None else labels[idx].astype(np.int64)
    n = len(lab)
    W, nv, kw = _node_inputs(lab, boost_type, seed, weights, real)
    got, gq, gpt = e.find_best_split(W, sample_idx=idx, node_value=nv, boost_type=boost_type, split_criteria=criteria, per_var=True, **kw)
    q32 = np.where(gpt >= 0, gq.astype(np.float32), np.float32(-1))  # the reference stores the double as a float
    F = len(gq)
    cat = ftype == ev.LBP
    fails = sw.check_winner(dict(got, var_idx=got["var_idx"] - lo), q32, gpt, cat)
    pick = _subset(F, gq, got["var_idx"] - lo if got["found"] else None, 75 if n < 10000 else 8)
    vals = np.stack([e.calc_batch(lo + f, lo + f + 1, sample_idx=idx, n_samples=None if idx is not None else n)[0] for f in pick]) \
        if len(pick) < F else e.calc_batch(lo, lo + F, sample_idx=idx, n_samples=None if idx is not None else n)
    node = sw.Node(vals, W, tie_key=idx, boost_type=boost_type, split_criteria=criteria, categorical=cat,
                   responses=kw.get("responses"), class_labels=kw.get("class_labels"))
    node.check_totals(W, nv)
    decided = with_split = weak = toothless = 0
    for j, f in enumerate(pick):
        is_winner = got["found"] and f == got["var_idx"] - lo
        if cat:
            if is_winner:
                fl, info = node.verdict_categorical(j, q32[f], subset=got["subset"], quality64=gq[f])
            else:
                fl, info = node.verdict_categorical(j, q32[f], count=int(gpt[f]) + 1, quality64=gq[f])
            weak += info["weak"]
        else:
            fl, info = node.verdict_ordered(j, int(gpt[f]), q32[f], ord_c=got["ord_c"] if is_winner else None, quality64=gq[f])
        toothless += info["toothless"]
        fails += [f"[catalog variable {lo + f}] " + x for x in fl]
        with_split += bool(info["has_split"])
        decided += info["decided"]
    share = decided / max(with_split, 1)
    print(f"\n{n} samples, {len(pick)} of {F} variables checked, {with_split} with a split, decided {share:.3f}")
    assert not fails, "; ".join(fails[:6])
    assert weak == 0 and toothless == 0, f"{weak} counts unresolved, {toothless} cuts with infinite B: (b) did not apply to them"
    if not (isinstance(weights, str) and weights == "equal"):
        assert with_split > 0 and share >= 0.95, f"inputs leave only {share:.3f} of {with_split} variables decided"
    return got, node, pick


@pytest.mark.parametrize("boost_type,criteria", COMBOS)
@pytest.mark.parametrize("ftype,mode", [(ev.HAAR, ev.BASIC), (ev.HAAR, ev.ALL), (ev.LBP, 0)], ids=["haar-basic", "haar-all", "lbp"])
def test_root_sorted_and_permuted_nodes(ftype, mode, boost_type, criteria):
    e, labels = _setup(ftype, mode, WIN, 400, 41, dup=12)
    real = boost_type == ev.BOOST_LOGIT
    got, _, _ = _hold(e, labels, boost_type=boost_type, criteria=criteria, seed=3, real=real)
    assert got["found"]
    rng = np.random.default_rng(9)
    sub = np.sort(rng.choice(400, 257, replace=False))
    _hold(e, labels, boost_type=boost_type, criteria=criteria, sample_idx=sub, seed=4, real=real)
    _hold(e, labels, boost_type=boost_type, criteria=criteria, sample_idx=rng.permutation(sub), seed=5, real=real)


@pytest.mark.parametrize("win", [(16, 16), (32, 32)])
def test_hog(win):
    e, labels = _setup(ev.HOG, 0, win, 300, 43, dup=8)
    for boost_type, criteria in COMBOS:
        _hold(e, labels, boost_type=boost_type, criteria=criteria, seed=6, real=boost_type == ev.BOOST_LOGIT)
    _hold(e, labels, boost_type=ev.BOOST_GENTLE, sample_idx=np.random.default_rng(2).permutation(300)[:131], seed=7)


def test_lbp_small_node_all_bipartitions():
    """About 12 samples: every variable has at most 12 present categories, so the exact maximum over ALL bipartitions
    applies to real LBP codes; it must equal the witness's best cut, which the device must then meet."""
    e, labels = _setup(ev.LBP, 0, WIN, 400, 41, dup=12)
    sub = np.sort(np.random.default_rng(5).choice(400, 12, replace=False))
    for boost_type in (ev.BOOST_GENTLE, ev.BOOST_LOGIT):
        _, node, pick = _hold(e, labels, boost_type=boost_type, sample_idx=sub, seed=8, real=boost_type == ev.BOOST_LOGIT)
        checked = 0
        for j in range(0, len(pick), 4):
            best = node.best_bipartition(j)
            a = node.categories(j)
            if best is not None and "qbest" in a:
                assert best == a["qbest"], pick[j]
                checked += 1
        assert checked >= 10
    _hold(e, labels, boost_type=ev.BOOST_REAL, sample_idx=sub, seed=8)


def test_equal_weights_first_round():
    """Round 0: one weight per class, so prefixes and categories tie exactly; (a), (b), (c), (e) hold, the decided
    share is printed only."""
    for ftype, mode in ((ev.HAAR, ev.BASIC), (ev.LBP, 0)):
        e, labels = _setup(ftype, mode, WIN, 400, 5, dup=30)
        for boost_type in (ev.BOOST_GENTLE, ev.BOOST_REAL, ev.BOOST_DISCRETE):
            _hold(e, labels, boost_type=boost_type, weights="equal")


def test_device_variants(monkeypatch):
    """The weight table in global memory, the streaming LBP kernel and a variable's ranks cut into parts."""
    eh, lh = _setup(ev.HAAR, ev.BASIC, WIN, 300, 11, dup=6)
    el, ll = _setup(ev.LBP, 0, WIN, 500, 21, dup=10)
    sub = np.sort(np.random.default_rng(8).choice(500, 311, replace=False))
    monkeypatch.setenv("CCAMD_SPLIT_GLOBAL_TABLE", "1")
    for bt in (ev.BOOST_GENTLE, ev.BOOST_REAL, ev.BOOST_DISCRETE):
        _hold(eh, lh, boost_type=bt, seed=12, sample_idx=np.arange(0, 300, 2) if bt == ev.BOOST_REAL else None)
        _hold(el, ll, boost_type=bt, seed=12, sample_idx=sub)
    monkeypatch.delenv("CCAMD_SPLIT_GLOBAL_TABLE")
    monkeypatch.setenv("CCAMD_SPLIT_CAT_STREAM", "1")
    for bt in (ev.BOOST_GENTLE, ev.BOOST_REAL):
        _hold(el, ll, boost_type=bt, seed=13, sample_idx=sub)
    monkeypatch.delenv("CCAMD_SPLIT_CAT_STREAM")
    for parts in (2, 5, 28):
        monkeypatch.setenv("CCAMD_SPLIT_CAT_PARTS", str(parts))
        for bt in (ev.BOOST_GENTLE, ev.BOOST_REAL):
            _hold(el, ll, boost_type=bt, seed=14, sample_idx=sub)
            _hold(el, ll, boost_type=bt, seed=15)


@pytest.mark.parametrize("n", [17000, 24577])
def test_presort_below_and_above_the_one_block_limit(n):
    """One block sorts up to 24 576 keys, the segmented sort more; an 8x8 window keeps the catalog short. Few duplicated
    samples, so that the variables stay decided."""
    e, labels = _setup(ev.HAAR, ev.BASIC, (8, 8), n, seed=60 + n % 7, dup=n // 100)
    _hold(e, labels, boost_type=ev.BOOST_GENTLE, seed=3)


def test_shard_range_and_pick_split():
    """Each shard of the catalog is searched on its own and held to the witness; pick_split's winner is the shard result
    with the largest quality, lowest shard first."""
    from cascadeclassifier_amd.distributed import pick_split, shard_range
    for ftype, mode in ((ev.HAAR, ev.BASIC), (ev.LBP, 0)):
        e, labels = _setup(ftype, mode, WIN, 300, 21, dup=6)
        F = e.getNumFeatures()
        parts = []
        for r in range(3):
            lo, hi = shard_range(F, r, 3)
            e.presort(300, lo, hi)
            got, _, _ = _hold(e, labels, boost_type=ev.BOOST_GENTLE, seed=3, lo=lo)
            assert not got["found"] or lo <= got["var_idx"] < hi
            parts.append(got)
        win = pick_split(parts)
        best = max(range(3), key=lambda r: (parts[r]["quality"] if parts[r]["found"] else np.float32(-1), -r))
        assert win["found"] and win["var_idx"] == parts[best]["var_idx"] and win["quality"] == parts[best]["quality"]
        assert win["ord_c"] == parts[best]["ord_c"] and (win["subset"] == parts[best]["subset"]).all()


def test_ten_gentle_adaboost_rounds():
    """Ten rounds of Gentle AdaBoost with stumps (weak response f = weighted mean of y in the leaf, w *= exp(-y f),
    renormalise), the witness's verdict on the device's search every round."""
    for ftype, mode in ((ev.HAAR, ev.CORE), (ev.LBP, 0)):
        n = 360
        e, labels = _setup(ftype, mode, WIN, n, 31, dup=12)
        y = labels.astype(np.float64) * 2 - 1
        w = np.full(n, 1.0 / n)
        chosen = []
        for rnd in range(10):
            got, _, _ = _hold(e, labels, boost_type=ev.BOOST_GENTLE, weights="equal" if rnd == 0 else w)
            assert got["found"], rnd
            chosen.append(got["var_idx"])
            v = e.calc_batch(got["var_idx"], got["var_idx"] + 1)[0]
            if ftype == ev.HAAR:
                left = v <= got["ord_c"]
            else:
                code = v.astype(np.int32)
                left = (got["subset"][code >> 5] >> (code & 31)) & 1 == 1
            f = np.empty(n)
            for side in (left, ~left):
                sw_, sy = 0.0, 0.0
                for i in np.nonzero(side)[0]:
                    sw_ += w[i]
                    sy += y[i] * w[i]
                f[side] = sy * (1.0 / sw_) if sw_ > 0 else 0.0
            w = w * np.exp(-y * f)
            w = w * (1.0 / w.sum())
        assert len(set(chosen)) > 3
