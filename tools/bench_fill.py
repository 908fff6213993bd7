#!/usr/bin/env python3
"""Filling one stage's negatives (section 6c) at the shapes of tools/bench_negmine.py: 32 backgrounds of one size per call,
the first K stages of the synthetic Haar cascade, want = 1000 slots. Two routes in the same build, alternating, with the
same result (checked):

  host  : cc_negminer_run_batch (all flags and the kept pixels to the host), the host's walk over the flags to find where
          the loop stops, cc_eval_set_images of the kept pixels;
  device: cc_negminer_fill.

Wall time per call around calls that end in a device synchronise; bytes over PCIe from the shapes. Prints one JSON line.
usage: bench_fill.py [K=10] [reps=20] [want=1000]"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import cascadeclassifier_amd as cc
    from cascadeclassifier_amd import evaluator as ev
    from tests.util import frame_natural
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    want = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
    B, first = 32, 1000
    xml = os.path.join(tempfile.mkdtemp(), "trunc.xml")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "truncate_cascade.py"),
                           os.path.join(ROOT, "data", "haarcascade_frontalface_synthetic.xml"), str(K), xml])
    m = ev.NegativeMiner(cc.CascadeClassifier(xml))
    e = cc.CvFeatureEvaluator.create(ev.HAAR)
    e.init(cc.CvFeatureParams(ev.HAAR, ev.BASIC), first + want, (24, 24))
    out = {"workload": f"fill {want} negative slots from {B} backgrounds per call, {K} trained stages", "reps": reps, "shapes": {}}
    for (w, h) in ((1920, 1080), (640, 480)):
        imgs = [frame_natural(w, h, 100 + k) for k in range(B)]
        per = m.plan(w, h)["n_windows"]

        def host_route():
            flags, pix, idx = m.run_batch(imgs, max_keep=want)
            n = len(idx)
            # where the per-window loop stops: behind the last kept window, or at the end of the stream
            consumed = int(idx[-1]) + 1 if n == want else flags.size
            if n:
                e.setImages(pix, labels=np.zeros(n, np.uint8), first_idx=first)
            return n, consumed

        def device_route():
            r = m.fill(e, imgs, first, want)
            return r["n_filled"], r["n_consumed"]

        res_h, res_d = host_route(), device_route()  # warm-up: sizes the workspaces
        bits_h = None
        times = {"host": [], "device": []}
        for _ in range(reps):  # alternating
            for name, fn in (("host", host_route), ("device", device_route)):
                t0 = time.perf_counter()
                res = fn()
                times[name].append(time.perf_counter() - t0)
                assert res == res_h == res_d, (name, res, res_h, res_d)
                probe = [e.get_sample(first + i) for i in sorted({0, res[0] // 2, res[0] - 1}) if res[0] > 0]
                bits = [(s.tobytes(), nf) for s, _, nf in probe]
                assert bits_h is None or bits == bits_h, "the two routes filled different samples"
                bits_h = bits
        n, consumed = res_h
        img_bytes = B * ((w + 3) // 4 * 4) * h
        out["shapes"][f"{w}x{h} x {B}"] = {
            "stream_windows": per * B, "n_filled": n, "n_consumed": consumed,
            "host_ms_per_call": {"median": round(float(np.median(times["host"])) * 1e3, 3), "min": round(min(times["host"]) * 1e3, 3),
                                 "max": round(max(times["host"]) * 1e3, 3)},
            "device_ms_per_call": {"median": round(float(np.median(times["device"])) * 1e3, 3), "min": round(min(times["device"]) * 1e3, 3),
                                   "max": round(max(times["device"]) * 1e3, 3)},
            "pcie_bytes": {"host_route": {"to_device": img_bytes + n * 576 + n * 8, "to_host": per * B + n * 576},
                           "device_route": {"to_device": img_bytes, "to_host": 16}},
        }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
