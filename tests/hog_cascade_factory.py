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


def stage_walk(model, vals):
    """CvCascadeClassifier::predict of every sample: vals [n_features][n] from feature_values; model from parsed_model
    (float32 values, stage threshold (float)t - 1e-5f). A stage fails iff its sum < threshold. Returns uint8 flags."""
    alive = np.ones(vals.shape[1], bool)
    for thr, weaks in model["stages"]:
        alive &= ~(stage_sums(weaks, vals) < float(thr))
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
