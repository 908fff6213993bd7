#!/usr/bin/env python3
"""What a variable outside the sorted tables costs: Gentle AdaBoost stumps on 24x24 Haar BASIC (162 336 variables) x
20 000 samples (BASELINE.json configs[4]'s set), per-round device time from CascadeBoost.last_round_ms(), with
resident_vars = F (every table resident: the path without streaming, the yardstick), F / 2 and 0 (cc_eval_presort_split).
Each setting runs `rounds` rounds `repeats` times from a fresh booster; the figure is the best repeat's mean round. The
share of a streamed search that is evaluate, sort, interleave, search and winner comes from the events of
cc_eval_stream_profile in one more, separate run (the timed runs carry no such events). Writes
profiles/bench_boost_streamed.json and prints it as one JSON line.
usage: bench_boost_streamed.py [rounds=5] [n_samples=20000] [repeats=5] [chunk_vars=plan's]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_training_eval import samples  # noqa: E402


def rounds_ms(cc, e, n, rounds):
    """Mean device time of a round, by part, over `rounds` rounds of a fresh booster; and the chosen variables."""
    b = cc.CascadeBoost(e, n, weight_trim_rate=0.95, max_weak_count=rounds + 1, max_false_alarm=1e-6)
    parts = {k: 0.0 for k in cc.CascadeBoost.ROUND_PARTS}
    chosen = []
    for _ in range(rounds):
        rec = b.round()
        assert rec["trained"]
        chosen.append(int(rec["var_idx"]))
        for k, v in b.last_round_ms().items():
            parts[k] += v / rounds
    return parts, chosen


def main():
    import cascadeclassifier_amd as cc
    from cascadeclassifier_amd import evaluator as ev
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    imgs, labels = samples(n=n // 2)
    e = cc.CvFeatureEvaluator.create(ev.HAAR)
    e.init(cc.CvFeatureParams(ev.HAAR, ev.BASIC), n, (24, 24))
    e.setImages(imgs, labels)
    f = e.getNumVariables()
    # the chunk the plan takes when the tables do not fit: a full pass of the presort (2^28 values)
    chunk = int(sys.argv[4]) if len(sys.argv) > 4 else min((f + 63) // 64 * 64, max(64, ((1 << 28) // n) // 64 * 64))
    out = {"workload": f"Gentle AdaBoost stumps, Haar BASIC 24x24 ({f} variables) x {n} samples (seed 7), trimming 0.95, {rounds} rounds, "
                       f"best of {repeats}", "chunk_vars": chunk, "settings": {}}
    want = None
    for name, resident in (("resident", f), ("half", f // 2 // 64 * 64), ("none", 0)):
        e.presort(n, resident_vars=resident, chunk_vars=chunk)
        best, chosen = None, None
        for _ in range(repeats):
            parts, chosen = rounds_ms(cc, e, n, rounds)
            if best is None or sum(parts.values()) < sum(best.values()):
                best = parts
        want = want or chosen
        rec = {"resident_vars": resident, "table_bytes": e.table_bytes(), "per_round_ms": round(sum(best.values()), 4),
               "per_round_kernel_ms": {k: round(v, 4) for k, v in best.items()}, "same_variables_as_resident": chosen == want}
        if resident < f:  # one more run with events between the steps of every chunk
            e.stream_profile(True)
            b = cc.CascadeBoost(e, n, weight_trim_rate=0.95, max_weak_count=rounds + 1, max_false_alarm=1e-6)
            phases = {k: 0.0 for k in e.STREAM_PHASES}
            for _ in range(rounds):
                assert b.round()["trained"]
                for k, v in e.stream_phase_ms().items():
                    phases[k] += v / rounds
            e.stream_profile(False)
            total = sum(phases.values())
            rec["streamed_tail_ms"] = {k: round(v, 4) for k, v in phases.items()}
            rec["streamed_tail_share"] = {k: round(v / total, 4) for k, v in phases.items()} if total > 0 else None
            rec["streamed_vars"] = f - resident
            rec["streamed_ns_per_value"] = round(total * 1e6 / ((f - resident) * n), 4)
        out["settings"][name] = rec
    base = out["settings"]["resident"]["per_round_ms"]
    out["ratio_to_resident"] = {k: round(v["per_round_ms"] / base, 3) for k, v in out["settings"].items()}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "bench_boost_streamed.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
