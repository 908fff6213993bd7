#!/usr/bin/env python3
"""Test mode of sample synthesis (cvCreateTestSamples; section 8 of the C ABI): test images per second
for n backgrounds of 640 x 480, a 24 x 24 window, the tool's default angles and automatic maxscale, a 64 x 64 object. Split
into the host plan (cc_testset_plan) and the device part (cc_sampler_render_testset: upload of records and spans, one
device-to-device copy per image, one kernel per batch), the latter once with the images copied back to the host and once
left in a caller's device buffer. Wall time around calls that end in a device synchronise, best of `reps`. There is no
speed baseline: the reference's tool needs OpenCV. Prints one JSON line.
usage: bench_testsamples.py [n=1000] [reps=5]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch

    import cascadeclassifier_amd as cc
    from cascadeclassifier_amd import _lib as L
    from cascadeclassifier_amd import samples as S
    from tests.sample_cases import obj_image
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    w, h, win = 640, 480, (24, 24)
    r = np.random.RandomState(5)
    distinct = [r.randint(0, 256, (h, w)).astype(np.uint8) for _ in range(8)]
    bgs = [distinct[i % 8] for i in range(n)]
    sizes = [(w, h)] * n
    s = cc.Sampler(obj_image(64, 64, 1))
    s.set_backgrounds(bgs)
    p = cc.SampleParams()
    s.generate_testset(min(n, 16), win, p, cc.CvRNG())  # warm-up
    dev = torch.from_numpy(np.zeros((n, h, w), np.uint8)).cuda()
    torch.cuda.synchronize()
    t_plan, t_host, t_dev = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        items, recs, spans = S.plan_testset(s.w, s.h, win, p, cc.CvRNG(), n, S.TestsetState(sizes))
        t1 = time.perf_counter()
        k = len(items)
        its = (L.TestsetItem * k)(*[L.TestsetItem(*it) for it in items])
        out = np.empty((k, h, w), np.uint8)
        ptrs = (C.c_void_p * k)(*[out[i].ctypes.data for i in range(k)])
        args = (s._s, C.cast(its, C.c_void_p), C.cast(recs, C.c_void_p), spans.ctypes.data_as(C.c_void_p), k, 0)
        t2 = time.perf_counter()
        L.check(L.lib().cc_sampler_render_testset(*args, C.cast(ptrs, C.c_void_p), None, 0))
        t3 = time.perf_counter()
        L.check(L.lib().cc_sampler_render_testset(*args, None, dev.data_ptr(), 0))
        t4 = time.perf_counter()
        t_plan.append(t1 - t0)
        t_host.append(t3 - t2)
        t_dev.append(t4 - t3)
    assert k == n and (dev.cpu().numpy()[:k] == out).all()
    pl, ho, de = min(t_plan), min(t_host), min(t_dev)
    mean_area = float(np.mean([it[4] * it[5] for it in items]))
    print(json.dumps({"workload": f"createsamples test mode, {n} backgrounds of {w} x {h}, window {win[0]} x {win[1]}, 64 x 64 object",
                      "reps": reps, "emitted": k, "mean_rectangle_pixels": round(mean_area, 1),
                      "host_plan_ms": round(pl * 1e3, 3),
                      "device_render_to_host_ms": round(ho * 1e3, 3), "images_per_s_to_host": round(k / (pl + ho), 1),
                      "device_render_to_device_ms": round(de * 1e3, 3), "images_per_s_to_device": round(k / (pl + de), 1)}))
    s.close()


if __name__ == "__main__":
    main()
