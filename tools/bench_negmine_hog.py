#!/usr/bin/env python3
"""Batched negative mining with a HOG cascade (cc_negminer_run / _run_batch, k_negmine_hog): every window of the reader's
sqrt(2) / half-window-step stream over one 1920x1080 and one 640x480 background through K trained stages of a synthetic
HOG stump cascade, each window with its own setImage. For comparison, the window-by-window loop the miner replaces,
through the evaluator's host mirror (CvFeatureEvaluator.setImage + operator() from the mirror, then the stage walk).
Prints one JSON line; run under rocprofv3 --kernel-trace --stats for kernel times.
usage: bench_negmine_hog.py [K=10] [reps=5] [win_w=24] [win_h=24]"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def restated_flags(windows, stages, feats):
    """The restatement's flags for `windows` (a check that the timed loop computed the values it should)."""
    from tests import hog_cascade_factory as hf
    from tests import hog_restatement as hog
    hist, norm = hog.set_images(windows)
    return hf.stage_walk(hf.parsed_model(stages), hf.feature_values(feats, hist, norm))


def main():
    import cascadeclassifier_amd as cc
    from cascadeclassifier_amd import evaluator as ev
    from tests import hog_cascade_factory as hf
    from tests import hog_restatement as hog
    from tests.util import frame_natural
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    W = int(sys.argv[3]) if len(sys.argv) > 3 else 24
    H = int(sys.argv[4]) if len(sys.argv) > 4 else 24
    calib_img = frame_natural(640, 480, 3)
    calib = np.stack([calib_img[y:y + H, x:x + W] for y in range(0, 480 - H, 23) for x in range(0, 640 - W, 29)])
    xml, feats, stages = hf.hog_cascade(calib, seed=7, stage_sizes=tuple(3 + 2 * k for k in range(K)), pass_share=0.6)
    path = os.path.join(tempfile.mkdtemp(), "hog.xml")
    open(path, "w").write(xml)
    c = cc.CascadeClassifier(path)
    m = ev.NegativeMiner(c)
    out = {"workload": f"HOG negative mining, {W}x{H} window, {K} trained stages ({sum(len(w) for _, w in stages)} stumps)"}
    for (w, h) in ((1920, 1080), (640, 480)):
        plan = m.plan(w, h)
        img = frame_natural(w, h, 5)
        flags = m.run(img, max_keep=256)[0]  # warm-up
        t0 = time.perf_counter()
        for _ in range(reps):
            flags = m.run(img, max_keep=256)[0]
        dt = (time.perf_counter() - t0) / reps
        r = {"stream_windows": plan["n_windows"], "levels": len(plan["levels"]), "run_wall_ms_per_image": round(dt * 1e3, 3),
             "accepted": int(flags.sum())}
        for B in (8, 32):
            imgs = [frame_natural(w, h, 100 + k) for k in range(B)]
            fb = m.run_batch(imgs, max_keep=256)[0]  # warm-up (sizes the workspace)
            t0 = time.perf_counter()
            for _ in range(reps):
                fb = m.run_batch(imgs, max_keep=256)[0]
            dtb = (time.perf_counter() - t0) / reps
            r[f"run_batch_{B}_wall_ms_per_image"] = round(dtb / B * 1e3, 4)
            r[f"run_batch_{B}_last_image_equals_run"] = bool((fb[-1] == m.run(imgs[-1], max_keep=0)[0]).all())
        out[f"{w}x{h}"] = r
    # the loop the miner replaces: setImage of each window through the evaluator's host mirror and the values of the
    # cascade's variables from it (the stage walk itself, a few compares per node in the trainer, is left out of the timing)
    cat = hog.catalog(W, H)
    vi = np.array([np.nonzero((cat == f[:4]).all(1))[0][0] * 36 + f[4] for f in feats], np.int32)
    e = cc.CvFeatureEvaluator.create(ev.HOG)
    e.init(cc.CvFeatureParams.create(ev.HOG), 1, (W, H))
    n = min(len(calib), 400)
    vals = np.empty((len(vi), n), np.float32)
    t0 = time.perf_counter()
    for i in range(n):
        e.setImage(calib[i], 0, 0)
        vals[:, i] = e.calc_list(vi, 0)
    dt = (time.perf_counter() - t0) / n
    assert (hf.stage_walk(hf.parsed_model(stages), vals) == restated_flags(calib[:n], stages, feats)).all()
    out["host_mirror_loop_us_per_window"] = round(dt * 1e6, 2)
    out["host_mirror_loop_ms_per_1920x1080"] = round(dt * out["1920x1080"]["stream_windows"] * 1e3, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
