#!/usr/bin/env python3
"""Sample synthesis (section 8 of the C ABI): samples per second for two workloads,

  barcode : the reference README's command (600 x 280 image, -maxzangle 1.6 alone, 75 x 32 windows), checked against
            tests/golden/barcode.vec for its first 100 samples;
  default : a 24 x 24 window with the tool's default angles from a 64 x 64 object,

each split into the host plan (cc_sample_plan: draws, LU solve, row spans) and the device part (cc_sampler_render: upload of
records and spans, one kernel per batch, copy back). Wall time around calls that end in a device synchronise, best of
`reps`. There is no speed baseline: the only reference program that makes samples needs OpenCV. Prints one JSON line.
usage: bench_createsamples.py [n=10000] [reps=5]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import cascadeclassifier_amd as cc
    from cascadeclassifier_amd import _lib as L
    from tests.sample_cases import BARCODE, barcode_image, barcode_vec_samples, obj_image
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out = {"workload": f"createsamples, {n} samples per call", "reps": reps, "shapes": {}}
    for name, img, win, kw in (("barcode_75x32", barcode_image(), (75, 32), BARCODE), ("default_24x24", obj_image(64, 64, 1), (24, 24), {})):
        s = cc.Sampler(img)
        p = cc.SampleParams(**kw)
        first = s.generate(100, win, p, cc.CvRNG())  # warm-up; the barcode workload is checked against the recorded file
        if name.startswith("barcode"):
            assert (first == barcode_vec_samples()).all()
        t_plan, t_render = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            recs, spans = s.plan(n, win, p, cc.CvRNG())
            t1 = time.perf_counter()
            res = np.empty((n, win[1], win[0]), np.uint8)
            L.check(L.lib().cc_sampler_render(s._s, C.cast(recs, C.c_void_p), spans.ctypes.data_as(C.c_void_p), n, win[0], win[1], None, 0,
                                              res.ctypes.data_as(C.c_void_p)))
            t2 = time.perf_counter()
            t_plan.append(t1 - t0)
            t_render.append(t2 - t1)
        pl, re = min(t_plan), min(t_render)
        out["shapes"][name] = {"source": [int(img.shape[1]), int(img.shape[0])], "samples_per_s": round(n / (pl + re), 1),
                               "host_plan_ms": round(pl * 1e3, 3), "device_render_ms": round(re * 1e3, 3),
                               "host_plan_share": round(pl / (pl + re), 3)}
        s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
