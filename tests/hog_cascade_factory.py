"""Synthetic HOG cascades for tests, written in the reference's cascade.xml layout (CvCascadeClassifier::save with a
CvHOGEvaluator: featureParams maxCatCount 0 / featSize 36, ordered internal nodes `left right featIdx threshold`, one
feature per used variable as <rect>x y cw ch comp</rect> = cell 0 of the block and the component; cascadeclassifier.cpp
:439-456, 566-578, HOGfeatures.cpp:155-160), and a numpy stage walk over tests/hog_restatement.py values
(CvCascadeBoost::predict, boost.cpp:461-477)."""
from __future__ import annotations

import numpy as np

from tests import hog_restatement as hog

f32 = np.float32


def _real(v):
    """FileStorage's real: "2." for integral values, else "%.8e" (9 significant digits: a float32 round-trips)."""
    v = float(np.float32(v))
    return ("%d." % int(v)) if v.is_integer() and abs(v) < 1e9 else ("%.8e" % v)


def hog_xml(feats, stages, W, H, max_cat_count=0, feat_size=36):
    """feats: (n, 5) int rows (x, y, cw, ch, comp); stages: list of (threshold, [weak]) with weak = (nodes, leaves),
    nodes = list of (left, right, feature_idx, threshold)."""
    L = ['<?xml version="1.0"?>', "<opencv_storage>", "<cascade>", "  <stageType>BOOST</stageType>", "  <featureType>HOG</featureType>",
         f"  <height>{H}</height>", f"  <width>{W}</width>",
         "  <stageParams>", "    <boostType>GAB</boostType>", "    <minHitRate>9.95000005e-01</minHitRate>",
         "    <maxFalseAlarm>5.00000000e-01</maxFalseAlarm>", "    <weightTrimRate>9.49999988e-01</weightTrimRate>",
         "    <maxDepth>1</maxDepth>", "    <maxWeakCount>100</maxWeakCount></stageParams>",
         "  <featureParams>", f"    <maxCatCount>{max_cat_count}</maxCatCount>", f"    <featSize>{feat_size}</featSize></featureParams>",
         f"  <stageNum>{len(stages)}</stageNum>", "  <stages>"]
    for thr, weaks in stages:
        L.append("    <_>")
        L.append(f"      <maxWeakCount>{len(weaks)}</maxWeakCount>")
        L.append(f"      <stageThreshold>{_real(thr)}</stageThreshold>")
        L.append("      <weakClassifiers>")
        for nodes, leaves in weaks:
            flat = " ".join("%d %d %d %s" % (l, r, fi, _real(t)) for (l, r, fi, t) in nodes)
            L.append("        <_>")
            L.append(f"          <internalNodes>\n            {flat}</internalNodes>")
            L.append("          <leafValues>\n            %s</leafValues></_>" % " ".join(_real(v) for v in leaves))
        L.append("      </weakClassifiers></_>")
    L.append("  </stages>")
    L.append("  <features>")
    for f in feats:
        L.append("    <_>\n      <rect>\n        %d %d %d %d %d</rect></_>" % tuple(int(v) for v in f))
    L += ["  </features>", "</cascade>", "</opencv_storage>"]
    return "\n".join(L) + "\n"


def feature_values(feats, hist, norm):
    """values[f][s] of the cascade's features on set_image planes (hist [n][9][H+1][W+1], norm [n][H+1][W+1]): each
    feature is variable `comp` of its block, evaluated by hog_restatement.eval_vars."""
    feats = np.asarray(feats, np.int32).reshape(-1, 5)
    blocks = feats[:, :4]
    out = np.empty((len(feats), hist.shape[0]), np.float32)
    for i, f in enumerate(feats):
        vi = i * hog.FEATURE_SIZE + int(f[4])
        out[i] = hog.eval_vars(blocks, hist, norm, vi, vi + 1)[0]
    return out


def _tree_leaves(nodes, leaves, vals):
    """Leaf value (float64) of one tree for every sample: ordered splits, `value <= threshold` goes left."""
    n = vals.shape[1]
    idx = np.zeros(n, np.int64)
    done = np.zeros(n, bool)
    for _ in range(len(nodes)):  # node indices increase along a path: len(nodes) steps reach every leaf
        for k, (l, r, fi, t) in enumerate(nodes):
            at = (~done) & (idx == k)
            if at.any():
                idx[at] = np.where(vals[fi, at] <= t, l, r)
        done = idx <= 0
    return np.asarray(leaves, np.float32).astype(np.float64)[-idx]


def stage_sums(weaks, vals):
    """Stage sum per sample: double, in tree order."""
    acc = np.zeros(vals.shape[1], np.float64)
    for nodes, leaves in weaks:
        acc = acc + _tree_leaves(nodes, leaves, vals)
    return acc


def wave_stage_sums(weaks, vals):
    """Stage sum per sample in the order of a 64-lane wavefront that shares a stage's STUMPS (walk_stages_wave,
    cc_train_device.h, and wave_sum_f64, cc_eval_common.h): lane l adds the votes of stumps l, l + 64, ... in that order;
    then every lane adds its neighbour's value in turn by quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror and
    row_mirror (each lane then holds the total of its row of 16), lane 15 of a row is added into the next row for rows 1
    and 3, lane 31 into rows 2 and 3, and lane 63 holds the result. Every addition is an IEEE double addition."""
    n = vals.shape[1]
    v = np.zeros((64, n), np.float64)
    for t, (nodes, leaves) in enumerate(weaks):
        assert len(nodes) == 1, "stumps only"
        v[t % 64] = v[t % 64] + _tree_leaves(nodes, leaves, vals)
    lane = np.arange(64)
    with np.errstate(invalid="ignore", over="ignore"):
        for src in (lane ^ 1, lane ^ 2, (lane & ~7) | (7 - (lane & 7)), (lane & ~15) | (15 - (lane & 15))):
            v = v + v[src]
        add = np.zeros_like(v)
        add[16:32], add[48:64] = v[15], v[47]  # row_bcast15, rows 1 and 3
        v = v + add
        add = np.zeros_like(v)
        add[32:64] = v[31]                     # row_bcast31, rows 2 and 3
        v = v + add
    return v[63]


def stage_walk(model, vals, sums=stage_sums):
    """CvCascadeClassifier::predict of every sample: vals [n_features][n] from feature_values; model from parsed_model
    (float32 values, stage threshold (float)t - 1e-5f). A stage fails iff its sum < threshold. Returns uint8 flags.
    `sums` is the order the stage sum is formed in: tree order, as the reference does, unless a test asks what another
    order would give."""
    alive = np.ones(vals.shape[1], bool)
    for thr, weaks in model["stages"]:
        alive &= ~(sums(weaks, vals) < float(thr))
    return alive.astype(np.uint8)


def parsed_model(stages):
    """The stages as the library stores them: float32 thresholds / leaves, stage threshold (float)t - 1e-5f."""
    out = []
    for thr, weaks in stages:
        w = [([(int(l), int(r), int(fi), f32(t)) for (l, r, fi, t) in nodes], [f32(v) for v in leaves]) for nodes, leaves in weaks]
        out.append((f32(f32(thr) - f32(1e-5)), w))
    return {"stages": out}


def _pick_features(W, H, n, rng):
    """n (x, y, cw, ch, comp) rows from the window's block catalog; about a third of them touch the window's edge."""
    cat = hog.catalog(W, H)
    edge = np.nonzero((cat[:, 0] == 0) | (cat[:, 1] == 0) | (cat[:, 0] + 2 * cat[:, 2] == W) | (cat[:, 1] + 2 * cat[:, 3] == H))[0]
    n_edge = min(len(edge), max(1, n // 3))
    idx = np.concatenate([rng.choice(edge, n_edge, replace=n_edge > len(edge)), rng.choice(len(cat), n - n_edge)])
    rng.shuffle(idx)
    comps = rng.integers(0, hog.FEATURE_SIZE, n)
    return np.concatenate([cat[idx], comps[:, None]], axis=1).astype(np.int32)


def hog_cascade(windows, seed=5, stage_sizes=(3, 5, 8), depth=1, pass_share=0.7):
    """A cascade over `windows` (n, H, W) uint8: stumps (depth 1) or depth-2 trees (three nodes, four leaves) on random
    catalog blocks and components, node thresholds at quantiles of the values on the windows, stage thresholds so that
    about `pass_share` of the windows alive before a stage pass it. Returns (xml, feats, stages)."""
    windows = np.asarray(windows, np.uint8)
    H, W = windows.shape[1:]
    rng = np.random.default_rng(seed)
    per_tree = 1 if depth == 1 else 3
    nf = sum(stage_sizes) * per_tree
    feats = _pick_features(W, H, nf, rng)
    hist, norm = hog.set_images(windows)
    v = feature_values(feats, hist, norm)

    def node_thr(fi):
        nz = v[fi][v[fi] > 0]
        return f32(np.quantile(nz, rng.uniform(0.3, 0.7))) if len(nz) else f32(0.5)

    stages, k = [], 0
    alive = np.ones(windows.shape[0], bool)
    for nw in stage_sizes:
        weaks = []
        for _ in range(nw):
            if depth == 1:
                a = f32(rng.uniform(0.2, 1.0) * rng.choice([-1, 1]))
                weaks.append(([(0, -1, k, node_thr(k))], [a, f32(-a)]))
                k += 1
            else:  # root -> nodes 1 (left) and 2 (right); leaves 0..3
                nodes = [(1, 2, k, node_thr(k)), (0, -1, k + 1, node_thr(k + 1)), (-2, -3, k + 2, node_thr(k + 2))]
                leaves = [f32(x) for x in rng.uniform(-1, 1, 4)]
                weaks.append((nodes, leaves))
                k += 3
        sums = stage_sums(parsed_model([(0, weaks)])["stages"][0][1], v)
        base = sums[alive] if alive.sum() > 20 else sums
        thr = f32(np.quantile(base, 1 - pass_share))
        stages.append((thr, weaks))
        alive &= sums >= float(f32(thr - f32(1e-5)))
    return hog_xml(feats, stages, W, H), feats, stages


def stage_passes(model, vals):
    """Per stage, the samples that pass it given that they entered it: list of (entered, passed) boolean arrays."""
    alive = np.ones(vals.shape[1], bool)
    out = []
    for thr, weaks in model["stages"]:
        ok = ~(stage_sums(weaks, vals) < float(thr))
        out.append((alive.copy(), alive & ok))
        alive = alive & ok
    return out


def order_independent(stages, headroom=1.0):
    """stage_sums_order_independent (cc_host.cpp) restated for a stump cascade: every leaf of a stage is a multiple of
    q = 2^(emin - 24), emin the smallest binary exponent (frexp) among the stage's nonzero leaves; if the sum of the
    stumps' larger magnitudes stays below 2^53 q, every partial sum in any order is an exact double."""
    for _, weaks in parsed_model(stages)["stages"]:
        emin, mag = None, 0.0
        for nodes, leaves in weaks:
            assert len(nodes) == 1 and len(leaves) == 2, "stumps only"
            l, r = (float(v) for v in leaves)
            if not (np.isfinite(l) and np.isfinite(r)):
                return False
            mag += max(abs(l), abs(r))
            for v in (l, r):
                if v != 0.0:
                    e = int(np.frexp(v)[1])
                    emin = e if emin is None else min(emin, e)
        if emin is None:
            continue
        if mag * headroom / float(np.ldexp(1.0, emin - 24)) >= 9007199254740992.0:
            return False
    return True


def stump_cascade(windows, stage_leaves, seed=5, pass_share=0.7):
    """A stump cascade over `windows` (n, H, W) with given leaves: stage_leaves is a list of stages, each a list of
    (left, right) per stump. Blocks and components are random catalog picks, node thresholds quantiles of the values on the
    windows, stage thresholds the (1 - pass_share) quantile of the sequential double sums of the windows alive before the
    stage. Returns (xml, feats, stages)."""
    windows = np.asarray(windows, np.uint8)
    H, W = windows.shape[1:]
    rng = np.random.default_rng(seed)
    feats = _pick_features(W, H, sum(len(s) for s in stage_leaves), rng)
    hist, norm = hog.set_images(windows)
    v = feature_values(feats, hist, norm)
    stages, k = [], 0
    alive = np.ones(windows.shape[0], bool)
    for leaves in stage_leaves:
        weaks = []
        for l, r in leaves:
            nz = v[k][v[k] > 0]
            t = f32(np.quantile(nz, rng.uniform(0.3, 0.7))) if len(nz) else f32(0.5)
            weaks.append(([(0, -1, k, t)], [f32(l), f32(r)]))
            k += 1
        sums = stage_sums(parsed_model([(0, weaks)])["stages"][0][1], v)
        base = sums[alive] if alive.sum() > 20 else sums
        thr = f32(np.quantile(base, 1 - pass_share))
        stages.append((thr, weaks))
        alive &= sums >= float(f32(thr - f32(1e-5)))
    return hog_xml(feats, stages, W, H), feats, stages


def parse_hog_xml(text):
    """The layout hog_xml writes, read back without the library: (W, H, feats (n, 5) int32, stages) with stages a list of
    (threshold, [(nodes, leaves)]), nodes = [(left, right, feature_idx, threshold)], every real as the float32 its text
    rounds to."""
    import xml.etree.ElementTree as ET
    casc = ET.fromstring(text).find("cascade")
    assert casc.find("featureType").text == "HOG" and casc.find("stageType").text == "BOOST"
    W, H = int(casc.find("width").text), int(casc.find("height").text)
    stages = []
    for st in casc.find("stages"):
        weaks = []
        for wk in st.find("weakClassifiers"):
            n = wk.find("internalNodes").text.split()
            assert len(n) % 4 == 0
            nodes = [(int(n[i]), int(n[i + 1]), int(n[i + 2]), f32(float(n[i + 3]))) for i in range(0, len(n), 4)]
            leaves = [f32(float(t)) for t in wk.find("leafValues").text.split()]
            weaks.append((nodes, leaves))
        assert int(st.find("maxWeakCount").text) == len(weaks)
        stages.append((f32(float(st.find("stageThreshold").text)), weaks))
    assert int(casc.find("stageNum").text) == len(stages)
    feats = np.array([[int(t) for t in f.find("rect").text.split()] for f in casc.find("features")], np.int32).reshape(-1, 5)
    return W, H, feats, stages
