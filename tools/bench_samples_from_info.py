#!/usr/bin/env python3
"""The -info mode of sample synthesis (cvCreateTrainingSamplesFromInfo; section 8 of the C ABI): samples per
second for n_rects annotated rectangles with sides drawn from 24..480, spread evenly over n_images images of 640 x 480, resized
to a 24 x 24 window. Reported apart: the host's walk over the info file (scan_info), and of cc_samples_from_info the upload
of images and tables, the kernel and the copy back, as stream time between events (cc_samples_from_info_last_ms) of the call
with the best wall time of `reps`. The images are in memory: reading them from disk is not part of any figure. There is no
speed baseline: the reference's tool needs OpenCV. Prints one JSON line.
usage: bench_samples_from_info.py [n_rects=10000] [n_images=1000] [reps=5]"""
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import cascadeclassifier_amd as cc
    from cascadeclassifier_amd import _lib as L
    from cascadeclassifier_amd import samples as S
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    n_images = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    w, h, win = 640, 480, (24, 24)
    r = np.random.RandomState(5)
    distinct = [r.randint(0, 256, (h, w)).astype(np.uint8) for _ in range(8)]
    images = [distinct[i % 8] for i in range(n_images)]
    per = [n // n_images + (1 if i < n % n_images else 0) for i in range(n_images)]
    entries = []
    for i, k in enumerate(per):
        rects = []
        for _ in range(k):
            rw, rh = int(r.randint(24, 481)), int(r.randint(24, 481))
            rects.append((int(r.randint(0, w - rw + 1)), int(r.randint(0, h - rh + 1)), rw, rh))
        entries.append(("%05d.pgm" % i, rects))
    with tempfile.TemporaryDirectory() as tmp:
        info = os.path.join(tmp, "info.dat")
        S.write_info(info, entries)
        t_parse = []
        for _ in range(reps):
            t0 = time.perf_counter()
            got, bad = S.scan_info(info, n)
            t_parse.append(time.perf_counter() - t0)
    assert bad is None and got == entries
    records = np.array([(i,) + rc for i, (_, rects) in enumerate(got) for rc in rects], np.int32).reshape(-1, 5)
    cc.samples_from_info(images[:2], records[:per[0]], win)  # warm-up
    best, parts = None, None
    ms = [C.c_double(0.0) for _ in range(3)]
    for _ in range(reps):
        t0 = time.perf_counter()
        out = cc.samples_from_info(images, records, win)
        t1 = time.perf_counter()
        L.check(L.lib().cc_samples_from_info_last_ms(*[C.byref(m) for m in ms]))
        if best is None or t1 - t0 < best:
            best, parts = t1 - t0, [m.value for m in ms]
    assert out.shape == (n, win[1], win[0])
    pa = min(t_parse)
    print(json.dumps({"workload": f"createsamples -info mode, {n} rectangles with sides 24..480 over {n_images} images of {w} x {h}, "
                                  f"window {win[0]} x {win[1]}",
                      "reps": reps, "mean_rectangle_pixels": round(float(np.mean(records[:, 3].astype(np.int64) * records[:, 4])), 1),
                      "host_parse_ms": round(pa * 1e3, 3), "call_wall_ms": round(best * 1e3, 3),
                      "upload_ms": round(parts[0], 3), "kernel_ms": round(parts[1], 3), "copy_back_ms": round(parts[2], 3),
                      "uploaded_image_bytes": int(n_images) * w * h,
                      "samples_per_s": round(n / (pa + best), 1)}))


if __name__ == "__main__":
    main()
