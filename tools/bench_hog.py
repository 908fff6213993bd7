"""HOG evaluator timing: setImage of a batch (k_hog_set_images) and full-range operator() into device memory
(k_hog_eval_batch), after warm-up, on seeded random windows. Prints one JSON line per size with the bytes each step
moves and the rate. The bulk step's time comes from device events around its kernel (cc_eval_last_kernel_ms); the
setImage step is timed on the host and includes the upload of the pixels. Kernel-only times: run this under
`rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cascadeclassifier_amd as cc  # noqa: E402
from cascadeclassifier_amd import evaluator as ev  # noqa: E402

SIZES = [((32, 32), 20000), ((24, 24), 20000), ((75, 32), 10000)]


def run(win, n, reps, seed):
    import torch
    W, H = win
    imgs = np.random.default_rng(seed).integers(0, 256, (n, H, W), dtype=np.uint8)
    e = cc.CvFeatureEvaluator.create(ev.HOG)
    e.init(cc.CvFeatureParams.create(ev.HOG), n, win)
    nv = e.getNumVariables()
    out = torch.empty((nv, n), dtype=torch.float32, device="cuda:0")
    for _ in range(2):  # warm-up
        e.setImages(imgs)
        e.calc_batch_device(0, nv, out.data_ptr())
    set_ms, eval_ms = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        e.setImages(imgs)
        set_ms.append((time.perf_counter() - t0) * 1e3)
        e.calc_batch_device(0, nv, out.data_ptr())
        eval_ms.append(e.last_kernel_ms())
    plane_bytes = n * (W + 1) * (H + 1) * 40
    out_bytes = nv * n * 4
    s, v = float(np.median(set_ms)), float(np.median(eval_ms))
    return {"window": f"{W}x{H}", "samples": n, "blocks": e.getNumFeatures(), "variables": nv,
            "set_images_ms_host": round(s, 4), "set_images_bytes": plane_bytes + n * W * H,
            "set_images_GBps": round((plane_bytes + n * W * H) / s / 1e6, 1),
            "calc_batch_ms": round(v, 4), "calc_batch_out_bytes": out_bytes,
            "calc_batch_out_GBps": round(out_bytes / v / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    for win, n in SIZES:
        print(json.dumps(run(win, n, a.reps, a.seed)), flush=True)


if __name__ == "__main__":
    main()
