#!/usr/bin/env python3
"""Where the result lives: step time of bench.py's workload (64 Full-HD frames per step resident on the device, the synthetic
stock-profile Haar cascade, scaleFactor 1.1, minNeighbors 3, 7 stages specialised) with the rectangles returned to the host
(detect_batch: candidates copied back, sorted and grouped by host threads) against the rectangles left in device memory
(detect_batch_to_device: ordered and grouped by kernels). Legs:
  host_pipelined    detect_batch_submit / _collect, step i + 1 submitted before step i is collected (bench.py's headline form)
  host_sync         one detect_batch per step
  device_out        one detect_batch_to_device per step (the entry point has no submit / collect pair)
  device_out_scores the same with levels_ptr / weights_ptr: the scored ordering and grouping kernels. Its time against
                    device_out's in the same run is what the scores cost.
The legs alternate round by round in one process; a round times `--chunk` steps of one leg and the median over rounds is
reported. The rectangles of the legs must be identical, and the scored leg's levels the number of stages. Prints one JSON
line (--out also writes it to a file)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from bench import make_frames  # noqa: E402  (bench.py's frames: natural 1/f noise with pasted faces)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--chunk", type=int, default=4, help="steps per leg per round")
    ap.add_argument("--specialize", type=int, default=7)
    ap.add_argument("--out", help="also write the JSON line here")
    args = ap.parse_args()

    import torch

    import cascadeclassifier_amd as cc

    B, W, H = args.frames, args.width, args.height
    sf, mn = 1.1, 3
    frames = torch.from_numpy(make_frames(B, W, H, seed0=0)).cuda()
    clf = cc.CascadeClassifier(os.path.join(ROOT, "data", "haarcascade_frontalface_synthetic.xml"), max_batch=B)
    spec = 0
    if args.specialize > 0:
        try:
            spec = clf.specialize(args.specialize)
        except cc.CascadeError as e:
            print(f"[bench_device_out] specialisation unavailable: {e}", file=sys.stderr)
    cap = 256 * B
    d_out = torch.zeros((cap, 4), dtype=torch.int32, device="cuda")
    d_off = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
    s_out, s_off = torch.zeros_like(d_out), torch.zeros_like(d_off)  # the scored leg's own outputs
    s_lv = torch.zeros(cap, dtype=torch.int32, device="cuda")
    s_wt = torch.zeros(cap, dtype=torch.float64, device="cuda")
    src = dict(device_ptr=frames.data_ptr(), shape=(B, H, W))
    torch.cuda.synchronize()  # the buffers are filled on torch's stream, the detector writes them on its own

    def host_pipelined(k):
        prev = None
        for _ in range(k):
            t = clf.detect_batch_submit(None, sf, mn, **src)
            if prev is not None:
                clf.detect_batch_collect(prev)
            prev = t
        return clf.detect_batch_collect(prev)

    def host_sync(k):
        for _ in range(k):
            out = clf.detect_batch(None, sf, mn, **src)
        return out

    def device_out(k):
        for _ in range(k):
            clf.detect_batch_to_device(None, sf, mn, out_ptr=d_out.data_ptr(), cap=cap, offsets_ptr=d_off.data_ptr(), **src)
        return None  # read back after the timing, below

    def device_out_scores(k):
        for _ in range(k):
            clf.detect_batch_to_device(None, sf, mn, out_ptr=s_out.data_ptr(), cap=cap, offsets_ptr=s_off.data_ptr(),
                                       levels_ptr=s_lv.data_ptr(), weights_ptr=s_wt.data_ptr(), **src)
        return None

    legs = {"host_pipelined": host_pipelined, "host_sync": host_sync, "device_out": device_out, "device_out_scores": device_out_scores}
    last, per = {}, {}
    for name, fn in legs.items():
        last[name] = fn(2)  # warm-up: plan, workspaces, candidate lists
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            last[name] = fn(args.chunk)  # every leg ends with its results complete: collected, or the stream waited for
            per.setdefault(name, []).append((time.perf_counter() - t0) / args.chunk * 1e3)
    off, rects = d_off.cpu().numpy(), d_out.cpu().numpy()
    dev = [rects[off[i]:off[i + 1]] for i in range(B)]
    identical = all(len(r) == B and all(x.shape == y.shape and (x == y).all() for x, y in zip(r, dev))
                    for r in (last["host_pipelined"], last["host_sync"]))
    n = int(off[B])
    identical = identical and (s_off.cpu().numpy() == off).all() and (s_out.cpu().numpy()[:n] == rects[:n]).all()
    identical = identical and (s_lv.cpu().numpy()[:n] == clf.info()["n_stages"]).all() and bool(np.isfinite(s_wt.cpu().numpy()[:n]).all())
    out = {"metric": "ms_per_step", "frames_per_step": B, "width": W, "height": H, "specialized_stages": spec,
           "rounds": args.rounds, "steps_per_round": args.chunk, "rectangles_identical": bool(identical),
           "rectangles_per_step": int(off[B])}
    for name in legs:
        out[name] = {"median_ms": round(float(np.median(per[name])), 4), "min_ms": round(float(np.min(per[name])), 4),
                     "max_ms": round(float(np.max(per[name])), 4)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if identical else 3


if __name__ == "__main__":
    sys.exit(main())
