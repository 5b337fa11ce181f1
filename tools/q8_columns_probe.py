#!/usr/bin/env python
"""Time the coordinate-wise operators on block-quantized int8 clients (fa_coord_median_q8,
fa_coord_trimmed_mean_q8, fa_coord_mean_around_median_q8) against, in the same process and over the same K, n
and block size B, for each operator:

  * ``q8``: the new entry, straight from the quantized bytes (K n (1 + 4 / B) bytes);
  * ``f32``: the float32 entry over tensors dequantized BEFORE the clock starts;
  * ``deq_f32``: the dequantization of the K clients (fa_weighted_sum_q8 with k = 1 and SUM, all K clients as K
    segments of ONE launch) plus ``f32`` -- what a caller without these entries pays;
  * ``read_probe``: fa_read_probe over the same q bytes, the floor of any kernel that reads them once.

All forms are timed in INTERLEAVED repetitions (HIP events on the stream) after a warm-up; the JSON holds every
repetition, the medians and the spread (min, max).  The routing rule of the defenses reads ``q8`` against
``deq_f32``; ``f32`` and ``read_probe`` show which resource binds.

    python tools/q8_columns_probe.py --k 16 32 64 128 --block 128 1024 --reps 11
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.q8_geomed_probe import timed  # noqa: E402


def probe(k, n, block, reps, warmup):
    import torch

    from fedml_amd.engine import SUM, get_engine
    eng = get_engine(0)
    st = torch.cuda.current_stream(eng.device)
    deq = torch.empty(k, n, dtype=torch.float32, device=eng.device).normal_()
    ds = list(deq.unbind(0))
    q = torch.empty(k, n, dtype=torch.int8, device=eng.device)
    sc = torch.empty(k, -(-n // block), dtype=torch.float32, device=eng.device)
    qs, scs = list(q.unbind(0)), list(sc.unbind(0))
    eng.quantize_q8(ds, block, outs=(qs, scs))
    out = torch.empty(n, dtype=torch.float32, device=eng.device)
    trim, keep = k // 10, k - 2 * (k // 5)

    def dequantize():
        eng.weighted_sum_q8([[t] for t in qs], [[t] for t in scs], SUM, None, block, outs=ds)

    dequantize()
    ops = {"median": (lambda: eng.coord_median_q8([qs], [scs], block, outs=[out]),
                      lambda: eng.coord_median([ds], outs=[out])),
           "trimmed_mean": (lambda: eng.coord_trimmed_mean_q8([qs], [scs], trim, block, outs=[out]),
                            lambda: eng.coord_trimmed_mean([ds], trim, outs=[out])),
           "mean_around_median": (lambda: eng.coord_mean_around_median_q8([qs], [scs], keep, block, outs=[out]),
                                  lambda: eng.coord_mean_around_median([ds], keep, outs=[out]))}
    forms = {"read_probe": lambda: eng.read_probe(q, 128)}
    for name, (fq, ff) in ops.items():
        forms[name + ".q8"] = fq
        forms[name + ".f32"] = ff
        forms[name + ".deq_f32"] = lambda ff=ff: (dequantize(), ff())
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            ms[name].append(timed(fn, st))
    ceiling = k * n / min(ms["read_probe"]) / 1e9  # TB/s: bytes / ms / 1e9
    q8_read = k * n + 4 * k * (-(-n // block))
    res = {"k": k, "n": n, "block": block, "reps": reps, "trim": trim, "keep": keep,
           "read_ceiling_tb_per_s": round(ceiling, 3), "q8_bytes_over_ceiling_ms": round(q8_read / ceiling / 1e9, 4)}
    for name, v in ms.items():
        res[name] = {"ms": [round(t, 4) for t in v], "median_ms": round(statistics.median(v), 4),
                     "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    for name in ops:
        a, c = res[name + ".q8"], res[name + ".deq_f32"]
        res[name + ".q8_range_below_deq_f32"] = a["max_ms"] < c["min_ms"]  # the routing rule
        res[name + ".f32_over_q8"] = round(res[name + ".f32"]["median_ms"] / a["median_ms"], 3)
        res[name + ".deq_f32_over_q8"] = round(c["median_ms"] / a["median_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, nargs="+", default=[16, 32, 64, 128])
    ap.add_argument("--n", type=int, default=1 << 24, help="elements per client")
    ap.add_argument("--block", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "q8_columns_probe.json"))
    a = ap.parse_args()
    res = [probe(k, a.n, b, a.reps, a.warmup) for b in a.block for k in a.k]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    for r in res:
        print(json.dumps({key: (v["median_ms"], v["min_ms"], v["max_ms"]) if isinstance(v, dict) else v
                          for key, v in r.items()}))


if __name__ == "__main__":
    main()
