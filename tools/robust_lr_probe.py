#!/usr/bin/env python
"""Time the robust learning rate's pass (fa_sign_vote_sum_tiled, with a center and without one) against
the weighted sum it extends (fa_weighted_sum_tiled, FA_MODE_MUL_W) over the same rows of a tiled
float32 arena group.

The three are timed in INTERLEAVED repetitions on one device (HIP events on the stream), so a drift of
the machine hits all alike; the JSON holds every repetition, the medians, the spread (min, max), the
ratios of the medians to the baseline's and the ratios the bytes moved predict (P x 4 bytes each: the
baseline and the plain form K reads and one write, the centered form one more read, of the center).
The threshold is max(1, round(0.8 sqrt(K))), so both outcomes of the vote occur; the share of negated
elements is reported.

    python tools/robust_lr_probe.py --k 8 32 64 128 --log2p 24 --reps 15 --out profiles/robust_lr/probe.json
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, stream):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def probe(k, log2p, reps, warmup):
    import torch

    from fedml_amd.engine import MUL_W, get_engine
    eng = get_engine(0)
    p = 1 << log2p
    E = 1024
    buf = torch.empty(p // E, k, E, dtype=torch.float32, device=eng.device).normal_()
    rows = list(range(k))
    coef = [1.0 / k] * k
    threshold = max(1, round(0.8 * math.sqrt(k)))
    center = torch.empty(p, dtype=torch.float32, device=eng.device).normal_(0.0, 0.05)
    out = torch.empty(p, dtype=torch.float32, device=eng.device)
    st = torch.cuda.current_stream(eng.device)
    forms = {"baseline": lambda: (eng.weighted_sum_tiled(buf, rows, MUL_W, coef, out=out), None),
             "plain": lambda: eng.sign_vote_sum_tiled(buf, rows, None, coef, threshold, out=out),
             "centered": lambda: eng.sign_vote_sum_tiled(buf, rows, center, coef, threshold, out=out)}
    flipped = {}
    for _ in range(warmup):
        for name, fn in forms.items():
            f = fn()[1]
            if f is not None:
                flipped[name] = int(f.item())
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            ms[name].append(timed(fn, st))
    base_bytes = (k + 1) * p * 4
    moved = {"baseline": base_bytes, "plain": base_bytes, "centered": base_bytes + p * 4}
    res = {"k": k, "p": p, "dtype": "float32", "layout": "tiled", "threshold": threshold,
           "input_bytes": k * p * 4, "reps": reps}
    for name, v in ms.items():
        med = statistics.median(v)
        res[name] = {"ms": [round(x, 4) for x in v], "median_ms": round(med, 4), "min_ms": round(min(v), 4),
                     "max_ms": round(max(v), 4), "moved_bytes": moved[name],
                     "moved_tb_per_s": round(moved[name] / med / 1e9, 3)}
        if name in flipped:
            res[name]["flipped_share"] = round(flipped[name] / p, 4)
    for name in ("plain", "centered"):
        ratio = res[name]["median_ms"] / res["baseline"]["median_ms"]
        pred = moved[name] / base_bytes
        res[name + "_over_baseline"] = round(ratio, 4)
        res[name + "_byte_ratio"] = round(pred, 4)
        res[name + "_over_prediction"] = round(ratio / pred, 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, nargs="+", default=[8, 32, 64, 128])
    ap.add_argument("--log2p", type=int, default=24)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "robust_lr_probe.json"))
    a = ap.parse_args()
    res = [probe(k, a.log2p, a.reps, a.warmup) for k in a.k]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps([{key: ({q: w for q, w in v.items() if q != "ms"} if isinstance(v, dict) else v)
                       for key, v in r.items()} for r in res]))


if __name__ == "__main__":
    main()
