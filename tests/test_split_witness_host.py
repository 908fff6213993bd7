"""The oracle's split search (orc.find_best_split) held to the exact witness of tests/split_witness.py, on the CPU, and the
witness held to seeded faults: a plain double-precision searcher written here must be accepted on every input, and each
deliberately wrong variant of it must be rejected on at least one.

Inputs (`_cases`): n = 2, 3, 64, 65, 300; four weight sets (round-0 equal per class, random cubic, ten Gentle rounds'
spread, twelve orders of magnitude); +-1, LOGIT-style real, all-positive and all-negative responses; all four boost
types with both class criteria and the default; a permuted tie key. Ordered columns: random, heavy ties, one-ulp
steps around 1, 2 (ulp = 2 FLT_EPSILON) and 4 (2 FLT_EPSILON = half an ulp: the float32 sum rounds to even), steps of
31 / 32 / 33 ulps near 0.1, a constant column, values near FLT_MAX. Categorical columns: 1, 2, 3, 12, 40 and 256
present categories, singletons, category 255. In the twelve-orders nodes of 64 samples and more, a sample holding less
than 1e-6 of the node shares all its values with a heavy sample, so that no two cuts differ by such a sample alone.

Figures observed with these inputs (printed by test_bound_has_teeth_and_inputs_are_decided, run with -s):
  B / quality, twelve-orders weights excluded: max 1.22e-10 (2^-32.9); below 2^-30 for 100 % of 1232 checked variables
  twelve-orders weights, their own case: below 2^-30 for 98.5 % of 401 variables, max 1.05e-07, no toothless cut
  |double running-sum searcher - exact| / B, asserted <= 1 on every variable of every node: max 0.024 ordered, 0.0025
    categorical (the oracle hands out float32 only; its distance is check (b), inside the one-rounding window everywhere)
  decided share of the variables that have a split, asserted >= 95 % in every node with continuous weights (cubic, ten
    Gentle rounds, twelve orders): 100 % in each
"""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import split_witness as sw

COMBOS = [(sw.GENTLE, 0), (sw.LOGIT, 0), (sw.REAL, 0), (sw.DISCRETE, 0), (sw.REAL, sw.MISCLASS), (sw.DISCRETE, sw.GINI)]
SIZES = (2, 3, 64, 65, 300)
WEIGHTS = ("equal", "cubic", "gentle10", "orders12")
EPS2 = np.float32(2) * sw.FLT_EPSILON


def _ulp_steps(base, steps, rng, n):
    """n float32 values base + k ulps, k a running sum of `steps` choices, shuffled."""
    v = np.empty(n, np.float32)
    x = np.float32(base)
    for i in range(n):
        v[i] = x
        for _ in range(int(rng.choice(steps))):
            x = np.nextafter(x, np.float32(np.inf))
    return rng.permutation(v)


def _ordered_columns(n, rng):
    cols = [rng.normal(size=n), rng.integers(0, 4, n), _ulp_steps(1.0, (0, 1, 2, 3), rng, n), _ulp_steps(2.0, (0, 1, 2), rng, n),
            _ulp_steps(4.0, (0, 1, 1, 2), rng, n), _ulp_steps(5.0, (1,), rng, n), _ulp_steps(0.1, (0, 31, 32, 33), rng, n),
            np.full(n, 0.25), rng.integers(1, 4, n) * 1e38, rng.random(n) * 0.2]
    return np.array(cols, np.float32)


def _categorical_columns(n, rng):
    cols = []
    for present in (1, 2, 3, 12, 40, 256):
        k = min(present, n)
        cats = np.concatenate([[255], rng.choice(255, k - 1, replace=False)]) if k > 1 else np.array([int(rng.integers(0, 256))])
        col = np.concatenate([cats, rng.choice(cats, n - k)])  # every chosen category present, singletons likely
        cols.append(rng.permutation(col))
    return np.array(cols, np.float32)


def _weights(kind, n, lab, rng):
    if kind == "equal":
        npos = max(int(lab.sum()), 1)
        return np.where(lab == 1, 0.5 / npos, 0.5 / max(n - npos, 1))
    if kind == "cubic":
        w = rng.random(n) ** 3 + 1e-3
    elif kind == "gentle10":  # ten rounds of w *= exp(-y f), |f| < 1
        w = np.exp(-(rng.random((10, n)) * 2 - 1).sum(0) * rng.choice([0.3, 1.0], n))
    else:
        w = 10.0 ** rng.uniform(-12, 0, n)
    return w / w.sum()


def _totals(w, lab, resp, classifier):
    """weights[n], weights[n+1] and node_value as a trainer leaves them: plain running sums in node order."""
    if classifier:
        r = [0.0, 0.0]
        for i in range(len(w)):
            r[int(lab[i])] += w[i]
        return np.concatenate([w, r]), 0.0
    tot = s = 0.0
    for i in range(len(w)):
        tot += w[i]
        s += float(resp[i]) * w[i]
    return np.concatenate([w, [tot, 0.0]]), s * (1.0 / tot)


def _cases():
    out = []
    for categorical in (False, True):
        for n in SIZES:
            for wk in WEIGHTS:
                for ci, (bt, crit) in enumerate(COMBOS):
                    seed = 1000 * n + 10 * ci + WEIGHTS.index(wk) + (5 if categorical else 0)
                    rng = np.random.default_rng(seed)
                    lab = rng.integers(0, 2, n)
                    if n >= 2:
                        lab[:2] = (0, 1)
                    vals = _categorical_columns(n, rng) if categorical else _ordered_columns(n, rng)
                    if not categorical and n >= 64:  # a column that separates the classes fairly well
                        vals = np.concatenate([vals, (lab + rng.normal(0, 0.7, n)).astype(np.float32)[None]])
                    resp = (lab * 2 - 1).astype(np.float32)
                    rk = "pm1"
                    if bt == sw.LOGIT:
                        rk = ("real", "allpos", "allneg", "real")[WEIGHTS.index(wk)]
                        mag = (rng.random(n) * 3 + 0.01).astype(np.float32)
                        resp = {"real": resp * mag, "allpos": mag, "allneg": -mag}[rk]
                    w = _weights(wk, n, lab, rng)
                    if wk == "orders12" and n >= 64:
                        # a sample holding less than 1e-6 of the node moves a quality by about as little as B, so two
                        # cuts that differ by such a sample alone can never be decided: let every such sample share
                        # all its values with a heavy one. The spread of the weights and of the sums stays.
                        heavy = np.nonzero(w >= 1e-6)[0]
                        for i in np.nonzero(w < 1e-6)[0]:
                            vals[:, i] = vals[:, rng.choice(heavy)]
                    classifier = bt in (sw.DISCRETE, sw.REAL)
                    W, nv = _totals(w, lab, resp, classifier)
                    tie = rng.permutation(4 * n)[:n].astype(np.int32) if (seed % 3 == 0) else np.arange(n, dtype=np.int32)
                    out.append(dict(name=f"{'cat' if categorical else 'ord'}-n{n}-{wk}-b{bt}c{crit}-{rk}", vals=vals, tie=tie, W=W,
                                    nv=nv, resp=None if classifier else resp, lab=lab.astype(np.int32) if classifier else None,
                                    bt=bt, crit=crit, categorical=categorical, wk=wk, n=n))
    return out


CASES = _cases()


def _node(c):
    return sw.Node(c["vals"], c["W"], tie_key=c["tie"], responses=c["resp"], class_labels=c["lab"], boost_type=c["bt"],
                   split_criteria=c["crit"], categorical=c["categorical"])


# ------------------------------------------------------------------ a plain double-precision searcher and its faults
FAULTS = ("off_by_one", "le_boundary", "boundary_in_double", "defaults_swapped", "right_not_decremented", "weight_dropped",
          "cat_order_by_sum", "last_best_wins", "ord_c_in_double")


def _quality(crit, l, r):
    if crit == "misclass":
        return max(l[0] + r[1], l[1] + r[0])
    if crit == "reg":
        return (l[1] * l[1] * r[0] + r[1] * r[1] * l[0]) / (l[0] * r[0])
    L, R = l[0] + l[1], r[0] + r[1]
    return ((l[0] * l[0] + l[1] * l[1]) * R + (r[0] * r[0] + r[1] * r[1]) * L) / (L * R)


def _plain_search(c, fault=None):
    """Running sums in double over the sorted samples / the key-ordered categories; per variable the first maximum.
    Returns (winner dict, per-variable list of (point, float32 quality, ord_c or subset))."""
    n, W = c["n"], c["W"]
    reg = c["bt"] in (sw.LOGIT, sw.GENTLE)
    if reg:
        crit = "reg"
    else:
        crit = c["crit"]
        if crit not in (sw.GINI, sw.MISCLASS):
            crit = sw.MISCLASS if (c["bt"] == sw.DISCRETE) != (fault == "defaults_swapped") else sw.GINI
        crit = "gini" if crit == sw.GINI else "misclass"
    w = W[:n]
    vec = [(w[i], float(c["resp"][i]) * w[i]) if reg else ((w[i], 0.0) if c["lab"][i] == 0 else (0.0, w[i])) for i in range(n)]
    tot = (W[n], c["nv"] * W[n]) if reg else (W[n], W[n + 1])
    per, dbl = [], []  # dbl: the unrounded double behind each float32 quality
    for f in range(len(c["vals"])):
        v = c["vals"][f]
        best_q, best = -1.0, None
        if not c["categorical"]:
            order = np.lexsort((c["tie"], v))
            sv = v[order]
            l, r = [0.0, 0.0], list(tot)
            for i in range(n - 1):
                a = vec[order[i]]
                if fault == "weight_dropped" and i == 1:
                    a = ((0.0, a[1]) if reg else (0.0, 0.0))
                l[0] += a[0]
                l[1] += a[1]
                if not (fault == "right_not_decremented"):
                    r[0] -= a[0]
                r[1] -= a[1]
                with np.errstate(over="ignore"):
                    if fault == "boundary_in_double":
                        ok = float(sv[i]) + float(EPS2) < float(sv[i + 1])
                    elif fault == "le_boundary":
                        ok = sv[i] + EPS2 <= sv[i + 1]
                    else:
                        ok = sv[i] + EPS2 < sv[i + 1]
                if ok:
                    q = _quality(crit, l, r)
                    if q > best_q:
                        best_q, best = q, i
            if best is None:
                per.append((-1, np.float32(-1), None))
                dbl.append(None)
                continue
            with np.errstate(over="ignore"):
                mid = np.float32((float(sv[best]) + float(sv[best + 1])) * 0.5) if fault == "ord_c_in_double" else (sv[best] + sv[best + 1]) * np.float32(0.5)
            per.append((best + 1 if fault == "off_by_one" and best + 2 < n else best, np.float32(best_q), mid))
            dbl.append(best_q)
        else:
            sums = [[0.0, 0.0] for _ in range(256)]
            for i in range(n):
                s = sums[int(v[i])]
                s[0] += vec[i][0]
                s[1] += vec[i][1]
            if reg:
                key = [s[1] if fault == "cat_order_by_sum" else (s[1] / s[0] if s[0] > 2.2204460492503131e-16 else 0.0) for s in sums]
                wt = [s[0] for s in sums]
                skip = [x <= float(sw.FLT_EPSILON) for x in wt]
            else:
                key = [s[1] for s in sums]
                wt = [s[0] + s[1] for s in sums]
                skip = [x < float(sw.FLT_EPSILON) for x in wt]
            order = sorted(range(256), key=lambda k: key[k])
            l, r = [0.0, 0.0], [sum(s[0] for s in sums), sum(s[1] for s in sums)]
            for pos in range(255):
                k = order[pos]
                if skip[k]:
                    continue
                for j in (0, 1):
                    l[j] += sums[k][j]
                    r[j] -= sums[k][j]
                if crit != "misclass":
                    L, R = (l[0], r[0]) if reg else (l[0] + l[1], r[0] + r[1])
                    if not (L > float(sw.FLT_EPSILON) and R > float(sw.FLT_EPSILON)):
                        continue
                q = _quality(crit, l, r)
                if q > best_q:
                    best_q, best = q, pos
            if best is None:
                per.append((-1, np.float32(-1), None))
                dbl.append(None)
                continue
            sub = np.zeros(8, np.uint32)
            for k in order[:best + 1]:
                sub[k >> 5] |= np.uint32(1 << (k & 31))
            per.append((best, np.float32(best_q), sub.view(np.int32)))
            dbl.append(best_q)
    win = {"dbl": dbl, "found": 0, "var_idx": -1, "quality": np.float32(-1), "split_point": -1, "subset": np.zeros(8, np.int32), "ord_c": np.float32(0)}
    for f, (pt, q, extra) in enumerate(per):
        if pt >= 0 and (q >= win["quality"] if fault == "last_best_wins" else q > win["quality"]):
            win.update(var_idx=f, quality=q, split_point=pt)
            win["subset" if c["categorical"] else "ord_c"] = extra
    win["found"] = int(win["var_idx"] >= 0 and win["quality"] > 0)
    return win, per


def _judge(c, node, win, per, stats=None):
    """Every variable's candidate and the winner through the witness -> list of failures."""
    fails = []
    dbl = win["dbl"] if isinstance(win, dict) else [None] * len(per)  # the plain searcher's doubles are held to exact +- B as they are
    for f, (pt, q, extra) in enumerate(per):
        if c["categorical"]:
            fl, info = node.verdict_categorical(f, q, subset=extra if pt >= 0 else None, quality64=dbl[f])
        else:
            fl, info = node.verdict_ordered(f, pt, q, ord_c=extra, quality64=dbl[f])
        fails += fl
        if stats is not None:
            stats.append(info)
    q32 = np.array([p[1] for p in per], np.float32)
    pts = np.array([p[0] for p in per])
    fails += sw.check_winner(win, q32, pts, c["categorical"])
    return fails


def _oracle_candidates(c):
    kw = dict(categorical=c["categorical"], node_value=c["nv"], boost_type=c["bt"], split_criteria=c["crit"], tie_key=c["tie"],
              responses=c["resp"], class_labels=c["lab"])
    win, q, pt = orc.find_best_split(c["vals"], c["W"], per_feature=True, **kw)
    per = []
    for f in range(len(c["vals"])):
        one = orc.find_best_split(c["vals"][f:f + 1], c["W"], **kw)  # threshold / subset of this variable on its own
        extra = None
        if pt[f] >= 0 and one["quality"] > 0:
            extra = one["subset"].copy() if c["categorical"] else one["ord_c"]
            assert one["quality"] == q[f]
        per.append((int(pt[f]), q[f], extra))
    return win, per


@pytest.mark.parametrize("wk", WEIGHTS)
@pytest.mark.parametrize("categorical", [False, True], ids=["ordered", "categorical"])
def test_oracle_against_witness(categorical, wk):
    for c in CASES:
        if c["categorical"] != categorical or c["wk"] != wk:
            continue
        node = _node(c)
        node.check_totals(c["W"], c["nv"])
        win, per = _oracle_candidates(c)
        if categorical:  # a variable whose quality is 0 has no subset from the single-variable call: judge it by its count
            fails = []
            for f, (pt, q, extra) in enumerate(per):
                fails += node.verdict_categorical(f, q, subset=extra if pt >= 0 else None, count=pt + 1 if extra is None else None)[0]
            fails += sw.check_winner(win, np.array([p[1] for p in per], np.float32), np.array([p[0] for p in per]), True)
        else:
            fails = _judge(c, node, win, per)
        assert not fails, c["name"] + ": " + "; ".join(fails[:5])


def test_plain_searcher_is_accepted_and_every_fault_is_rejected():
    caught = {k: 0 for k in FAULTS}
    for c in CASES:
        node = _node(c)
        fails = _judge(c, node, *_plain_search(c))
        assert not fails, "clean searcher rejected on " + c["name"] + ": " + "; ".join(fails[:5])
        for k in FAULTS:
            if caught[k] < 3:  # three witnesses of each fault are plenty
                caught[k] += bool(_judge(c, node, *_plain_search(c, k)))
    assert all(caught.values()), f"faults the witness never rejected: {[k for k, v in caught.items() if not v]}"


def test_best_prefix_cut_is_the_best_bipartition():
    """Regression: the best partition of the categories is contiguous in mean order, so the exact maximum over all
    bipartitions of up to 12 present categories equals the witness's best boundary cut."""
    checked = 0
    for c in CASES:
        if not c["categorical"] or c["bt"] not in (sw.LOGIT, sw.GENTLE):
            continue
        node = _node(c)
        for f in range(node.F):
            best = node.best_bipartition(f)
            a = node.categories(f)
            if best is not None and "qbest" in a:
                assert best == a["qbest"], (c["name"], f)
                checked += 1
    assert checked >= 40


def test_bound_has_teeth_and_inputs_are_decided():
    """B < 2^-30 of the exact quality for >= 99 % of checked variables (the twelve-orders weight set on its own), and in
    every node with continuous weights >= 95 % of the variables that have a split are decided. Both are properties of
    the inputs and of the witness; the second needs no candidate at all. The plain searcher's unrounded doubles are
    within B of exact on every variable, ordered (N = n + 8) and categorical (N = n + 520): _judge fails otherwise."""
    ratio = {False: [], True: []}  # keyed by "twelve orders"
    toothless = 0
    worst = {"cubic": 1.0, "gentle10": 1.0, "orders12": 1.0}
    err64 = {False: 0.0, True: 0.0}  # keyed by categorical
    for c in CASES:
        node = _node(c)
        stats = []
        fails = _judge(c, node, *_plain_search(c), stats=stats)
        assert not fails
        for info in stats:
            if "B" in info and info["q"] > 0:
                if np.isfinite(info["B"]):
                    ratio[c["wk"] == "orders12"].append(info["B"] / info["q"])
                else:
                    toothless += 1
            if "err64" in info:
                err64[c["categorical"]] = max(err64[c["categorical"]], info["err64"] / info["B"])
        with_split = [i for i in stats if i["has_split"]]
        if c["wk"] != "equal" and with_split:
            share = sum(i["decided"] for i in with_split) / len(with_split)
            worst[c["wk"]] = min(worst[c["wk"]], share)
            assert share >= 0.95, (c["name"], share)
    r = np.array(ratio[False])
    r12 = np.array(ratio[True])
    print(f"\nB/quality: max {r.max():.3g} (2^{np.log2(r.max()):.1f}), share below 2^-30: {(r < 2.0 ** -30).mean():.4f} of {len(r)}")
    print(f"twelve orders: share below 2^-30 {(r12 < 2.0 ** -30).mean():.4f} of {len(r12)}, max finite {r12.max():.3g}, toothless cuts {toothless}")
    print(f"decided share, minimum over nodes: {worst}")
    print(f"max |double - exact| / B: ordered {err64[False]:.3g}, categorical {err64[True]:.3g}")
    assert (r < 2.0 ** -30).mean() >= 0.99
