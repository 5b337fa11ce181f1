#!/usr/bin/env python
"""Time the centered-clipping passes (fa_centered_sum_sqdist_tiled: the fused update, and its
distance-only mode) against the geometric median's fused pass (fa_weighted_sum_sqdist_tiled) over the
same rows of a tiled float32 arena group.

The three are timed in INTERLEAVED repetitions on one device (HIP events on the stream), so a drift of
the machine hits all alike; the JSON holds every repetition, the medians, the spread (min, max), the
ratios of the medians to the baseline's and the ratios the bytes moved predict (P x 4 bytes each: the
baseline K reads and one write in the single-read form, float32 with K <= 32, and 2K reads and one
write in the generic form; the centered pass one more read, of the center; the distance-only pass
K + 1 reads in one walk and no write).

    python tools/cclip_probe.py --k 8 32 64 128 --log2p 24 --reps 15 --out profiles/cclip/probe.json
"""
from __future__ import annotations

import argparse
import json
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

    from fedml_amd.engine import get_engine
    eng = get_engine(0)
    p = 1 << log2p
    E = 1024
    buf = torch.empty(p // E, k, E, dtype=torch.float32, device=eng.device).normal_()
    rows = list(range(k))
    coef = [1.0 / k] * k
    center = torch.empty(p, dtype=torch.float32, device=eng.device).normal_()
    out = torch.empty(p, dtype=torch.float32, device=eng.device)
    st = torch.cuda.current_stream(eng.device)
    forms = {"baseline": lambda: eng.weighted_sum_sqdist_tiled(buf, rows, coef, out=out),
             "centered": lambda: eng.centered_sum_sqdist_tiled(buf, rows, center, coef, out=out),
             "dist": lambda: eng.centered_sum_sqdist_tiled(buf, rows, center, None)}
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            ms[name].append(timed(fn, st))
    reg = k <= 32
    base_bytes = (k + 1 if reg else 2 * k + 1) * p * 4
    moved = {"baseline": base_bytes, "centered": base_bytes + p * 4, "dist": (k + 1) * p * 4}
    res = {"k": k, "p": p, "dtype": "float32", "layout": "tiled", "form": "register" if reg else "generic",
           "input_bytes": k * p * 4, "reps": reps}
    for name, v in ms.items():
        med = statistics.median(v)
        res[name] = {"ms": [round(x, 4) for x in v], "median_ms": round(med, 4), "min_ms": round(min(v), 4),
                     "max_ms": round(max(v), 4), "moved_bytes": moved[name],
                     "moved_tb_per_s": round(moved[name] / med / 1e9, 3)}
    for name in ("centered", "dist"):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "cclip_probe.json"))
    a = ap.parse_args()
    res = [probe(k, a.log2p, a.reps, a.warmup) for k in a.k]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps([{key: ({q: w for q, w in v.items() if q != "ms"} if isinstance(v, dict) else v)
                       for key, v in r.items()} for r in res]))


if __name__ == "__main__":
    main()
