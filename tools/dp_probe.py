#!/usr/bin/env python
"""Time the fused clipped-sum-and-noise launch (fa_centered_sum_noise, float32, device-resident rows of
one allocation, with a center) against, in the same process and over the same K and n:

  * ``sum``: fa_sign_vote_sum at threshold 0 over the same rows, center and coefficients -- the same
    sum without the noise;
  * ``sum_then_noise``: that launch followed by fa_add_noise in place on its result -- the route
    without the fused kernel;
  * the box's read ceiling (fa_read_probe over the rows' own pages).

Byte counts come from the shapes: sum and fused 4 (K + 1) n read + 4 n written; sum_then_noise 8 n more.
All forms are timed in INTERLEAVED repetitions (HIP events on the stream) after a warm-up, so a drift of
the machine hits all alike; the JSON holds every repetition, the medians and the spread (min, max).

    python tools/dp_probe.py --k 1 8 32 128 --n 16777216 125000000 --out bench_outputs/dp_probe.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x0123456789ABCDEF


def timed(fn, stream):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def probe(k, n, mech, reps, warmup):
    import torch

    from fedml_amd.engine import get_engine
    eng = get_engine(0)
    g = torch.Generator().manual_seed(k)
    counts = torch.randint(50, 601, (k,), generator=g).tolist()
    w = [c / sum(counts) for c in counts]
    x = torch.empty(k, n, dtype=torch.float32, device=eng.device).normal_()
    xs = list(x.unbind(0))
    cen = torch.empty(n, dtype=torch.float32, device=eng.device).normal_()
    out = torch.empty(n, dtype=torch.float32, device=eng.device)
    st = torch.cuda.current_stream(eng.device)
    rnd = [0]

    def fused():
        rnd[0] += 1
        eng.centered_sum_noise([xs], [cen], w, mech, 0.01, SEED, rnd[0], [0], outs=[out])

    def plain():
        eng.sign_vote_sum([xs], [cen], w, 0, outs=[out])

    def composed():
        rnd[0] += 1
        eng.sign_vote_sum([xs], [cen], w, 0, outs=[out])
        eng.add_noise([out], mech, 0.01, SEED, rnd[0], [0], outs=[out])

    forms = {"fused": fused, "sum": plain, "sum_then_noise": composed, "read_probe": lambda: eng.read_probe(x, 128)}
    base = 4 * (k + 1) * n + 4 * n
    moved = {"fused": base, "sum": base, "sum_then_noise": base + 8 * n, "read_probe": 4 * k * n}
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            ms[name].append(timed(fn, st))
    ceiling = 4 * k * n / min(ms["read_probe"]) / 1e9  # TB/s: bytes / ms / 1e9
    res = {"k": k, "n": n, "mech": mech, "reps": reps, "read_ceiling_tb_per_s": round(ceiling, 3)}
    for name, v in ms.items():
        med = statistics.median(v)
        res[name] = {"ms": [round(t, 4) for t in v], "median_ms": round(med, 4), "min_ms": round(min(v), 4),
                     "max_ms": round(max(v), 4), "moved_bytes": moved[name],
                     "moved_tb_per_s": round(moved[name] / med / 1e9, 3)}
    res["fused_over_sum"] = round(res["fused"]["median_ms"] / res["sum"]["median_ms"], 4)
    res["fused_over_sum_then_noise"] = round(res["fused"]["median_ms"] / res["sum_then_noise"]["median_ms"], 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, nargs="+", default=[1, 8, 32, 128])
    ap.add_argument("--n", type=int, nargs="+", default=[1 << 24, 125_000_000], help="elements per client")
    ap.add_argument("--mech", nargs="+", default=["gaussian"], choices=["gaussian", "laplace"])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "dp_probe.json"))
    a = ap.parse_args()
    res = []
    for n in a.n:
        for k in a.k:
            for mech in a.mech:
                res.append(probe(k, n, mech, a.reps, a.warmup))
                r = res[-1]
                print(json.dumps({key: ({q: w for q, w in v.items() if q != "ms"} if isinstance(v, dict) else v)
                                  for key, v in r.items()}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
