#!/usr/bin/env python3
"""Colour frames against gray frames: step time of bench.py's workload (64 Full-HD frames per step, the synthetic
stock-profile Haar cascade, scaleFactor 1.1, minNeighbors 3, 7 stages specialised, pipelined submit / collect) for gray,
BGR, BGRA and RGB-planar frames, each resident on the device and from pageable host memory. The gray frames ARE the
conversion of the colour frames (COLOR_BGR2GRAY's integer form), so every format must return identical rectangles.
Formats alternate round by round in one process; a round times `--chunk` pipelined steps of one format and the median over
rounds is reported. Prints one JSON line (--out also writes it to a file)."""
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
    ap.add_argument("--rounds", type=int, default=6, help="rounds; each times --chunk steps of every format and memory kind")
    ap.add_argument("--chunk", type=int, default=4, help="pipelined steps per format per round")
    ap.add_argument("--specialize", type=int, default=7)
    ap.add_argument("--formats", default="gray,bgr,bgra,rgb_planar")
    ap.add_argument("--no-host", action="store_true", help="device-resident frames only")
    ap.add_argument("--out", help="also write the JSON line here")
    args = ap.parse_args()

    import torch

    import cascadeclassifier_amd as cc

    B, W, H = args.frames, args.width, args.height
    sf, mn = 1.1, 3
    rng = np.random.default_rng(2024)
    base = make_frames(B, W, H, seed0=0).astype(np.int16)
    bgr = np.empty((B, H, W, 3), np.uint8)
    for c in range(3):  # channels that differ from each other, all carrying the faces
        bgr[..., c] = np.clip(base + rng.integers(-24, 25, base.shape, dtype=np.int16), 0, 255)
    del base
    a = bgr.astype(np.uint32)
    gray = ((a[..., 0] * 1868 + a[..., 1] * 9617 + a[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)
    del a
    host = {"gray": gray, "bgr": bgr}
    fmts = args.formats.split(",")
    if "bgra" in fmts:
        host["bgra"] = np.concatenate([bgr, rng.integers(0, 256, (B, H, W, 1), dtype=np.uint8)], -1)
    if "rgb_planar" in fmts:
        host["rgb_planar"] = np.ascontiguousarray(bgr[..., ::-1].transpose(0, 3, 1, 2))
    kw = {"gray": None, "bgr": None, "bgra": None, "rgb_planar": "rgb_planar"}
    dev = {f: torch.from_numpy(host[f]).cuda() for f in fmts}
    clf = cc.CascadeClassifier(os.path.join(ROOT, "data", "haarcascade_frontalface_synthetic.xml"), max_batch=B)
    spec = 0
    if args.specialize > 0:
        try:
            spec = clf.specialize(args.specialize)
        except cc.CascadeError as e:
            print(f"[bench_color] specialisation unavailable: {e}", file=sys.stderr)

    def submit(fmt, where):
        if where == "device":
            t = dev[fmt]
            return clf.detect_batch_submit(None, sf, mn, device_ptr=t.data_ptr(), shape=tuple(t.shape), pixel_format=kw[fmt])
        return clf.detect_batch_submit(host[fmt], sf, mn, pixel_format=kw[fmt])

    def steps(fmt, where, k):
        out, prev = None, None
        for _ in range(k):
            t = submit(fmt, where)
            if prev is not None:
                out = clf.detect_batch_collect(prev)
            prev = t
        return clf.detect_batch_collect(prev)

    wheres = ["device"] + ([] if args.no_host else ["host"])
    results, per = {}, {}
    for where in wheres:
        for f in fmts:
            results[(where, f)] = steps(f, where, 2)  # warm-up: plans, graphs, staging areas, colour buffer
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for where in wheres:
            for f in fmts:
                t0 = time.perf_counter()
                results[(where, f)] = steps(f, where, args.chunk)
                per.setdefault((where, f), []).append((time.perf_counter() - t0) / args.chunk * 1e3)
    ref = results[("device", "gray")]
    identical = all(len(r) == len(ref) and all(x.shape == y.shape and (x == y).all() for x, y in zip(r, ref))
                    for r in results.values())
    # profiled pass: conversion time (counted under resize_ms) per format, device frames
    prof = {}
    for f in fmts:
        clf.set_profiling(True)
        clf.timings(reset=True)
        steps(f, "device", 2)
        tm = clf.timings(reset=True)
        clf.set_profiling(False)
        prof[f] = {"resize_ms_per_step": round(tm["resize_ms"] / 2, 4), "resize_launches_per_step": tm["resize_launches"] / 2}
    out = {"metric": "ms_per_step", "frames_per_step": B, "width": W, "height": H, "specialized_stages": spec,
           "rounds": args.rounds, "steps_per_round": args.chunk, "rectangles_identical_across_formats": bool(identical),
           "rectangles_frame0": int(len(ref[0]))}
    for where in wheres:
        g = float(np.median(per[(where, "gray")]))
        out[where] = {f: {"median_ms": round(float(np.median(per[(where, f)])), 4),
                          "min_ms": round(float(np.min(per[(where, f)])), 4),
                          "vs_gray": round(float(np.median(per[(where, f)])) / g - 1.0, 4)} for f in fmts}
    out["device_profiled"] = prof
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if identical else 3


if __name__ == "__main__":
    sys.exit(main())
