#!/usr/bin/env python
"""Time the fused dequantize-and-sum of block-quantized int8 clients (fa_weighted_sum_q8, FedAvg
weights) against, in the same process and over the same K and n:

  * ``f32``: fa_weighted_sum_multi over the K float32 rows the q8 rows were quantized from (the route
    of a caller that uploads float32);
  * ``unfused``: the route without the fused kernel -- every client dequantized to float32
    (fa_weighted_sum_q8 with k = 1 and SUM; all K clients as K segments of ONE launch, the form most
    favourable to this route) followed by fa_weighted_sum_multi over the K dequantized rows;
  * the box's read ceiling (fa_read_probe over the float32 rows' own pages).

The q8 forms run at every block size given; the quantizer (fa_quantize_q8, float32 input) is timed once
per block size against its byte count.  Byte counts come from the shapes:
  q8       K n (1 + 4 / B) read + 4 n written
  f32      4 K n read + 4 n written
  unfused  K n (1 + 4 / B) read + 4 K n written, then f32's
  quantize 4 K n read + K n (1 + 4 / B) written
All forms are timed in INTERLEAVED repetitions (HIP events on the stream) after a warm-up, so a drift of
the machine hits all alike; the JSON holds every repetition, the medians and the spread (min, max).

    python tools/q8_probe.py --k 16 32 128 --block 128 16 --reps 11 --out bench_outputs/q8_probe.json
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


def probe(k, n, blocks, reps, warmup):
    import torch

    from fedml_amd.engine import MUL_W, SUM, get_engine
    eng = get_engine(0)
    g = torch.Generator().manual_seed(k)
    counts = torch.randint(50, 601, (k,), generator=g).tolist()
    w = [c / sum(counts) for c in counts]
    x = torch.empty(k, n, dtype=torch.float32, device=eng.device).normal_()
    deq = torch.empty(k, n, dtype=torch.float32, device=eng.device)  # the unfused route's float32 rows
    xs, ds = list(x.unbind(0)), list(deq.unbind(0))
    out = torch.empty(n, dtype=torch.float32, device=eng.device)
    st = torch.cuda.current_stream(eng.device)

    forms = {"f32": lambda: eng.weighted_sum_multi([xs], MUL_W, w, outs=[out]),
             "read_probe": lambda: eng.read_probe(x, 128)}
    moved = {"f32": 4 * k * n + 4 * n, "read_probe": 4 * k * n}
    q8_read = {}
    for b in blocks:
        q = torch.empty(k, n, dtype=torch.int8, device=eng.device)
        sc = torch.empty(k, -(-n // b), dtype=torch.float32, device=eng.device)
        qs, scs = list(q.unbind(0)), list(sc.unbind(0))
        eng.quantize_q8(xs, b, outs=(qs, scs))
        q8_read[b] = k * n + 4 * k * (-(-n // b))

        def fused(qs=qs, scs=scs, b=b):
            eng.weighted_sum_q8([qs], [scs], MUL_W, w, b, outs=[out])

        def unfused(qs=qs, scs=scs, b=b):
            eng.weighted_sum_q8([[t] for t in qs], [[t] for t in scs], SUM, None, b, outs=ds)
            eng.weighted_sum_multi([ds], MUL_W, w, outs=[out])

        def quantize(qs=qs, scs=scs, b=b):
            eng.quantize_q8(xs, b, outs=(qs, scs))  # rewrites the same bits
        forms[f"q8_b{b}"], forms[f"unfused_b{b}"], forms[f"quantize_b{b}"] = fused, unfused, quantize
        moved[f"q8_b{b}"] = q8_read[b] + 4 * n
        moved[f"unfused_b{b}"] = q8_read[b] + 4 * k * n + moved["f32"]
        moved[f"quantize_b{b}"] = 4 * k * n + q8_read[b]
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            ms[name].append(timed(fn, st))
    ceiling = 4 * k * n / min(ms["read_probe"]) / 1e9  # TB/s: bytes / ms / 1e9
    res = {"k": k, "n": n, "blocks": list(blocks), "reps": reps, "read_ceiling_tb_per_s": round(ceiling, 3)}
    for name, v in ms.items():
        med = statistics.median(v)
        res[name] = {"ms": [round(t, 4) for t in v], "median_ms": round(med, 4), "min_ms": round(min(v), 4),
                     "max_ms": round(max(v), 4), "moved_bytes": moved[name],
                     "moved_tb_per_s": round(moved[name] / med / 1e9, 3),
                     "bytes_over_ceiling_ms": round(moved[name] / ceiling / 1e9, 4)}
    for b in blocks:
        med = res[f"q8_b{b}"]["median_ms"]
        res[f"q8_b{b}"]["q8_read_gb_per_s"] = round(q8_read[b] / med / 1e6, 1)
        res[f"q8_b{b}"]["q8_read_over_ceiling"] = round(q8_read[b] / med / 1e9 / ceiling, 4)
        res[f"f32_over_q8_b{b}"] = round(res["f32"]["median_ms"] / med, 4)
        res[f"unfused_over_q8_b{b}"] = round(res[f"unfused_b{b}"]["median_ms"] / med, 4)
        res[f"bytes_f32_over_q8_b{b}"] = round(moved["f32"] / moved[f"q8_b{b}"], 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, nargs="+", default=[16, 32, 128])
    ap.add_argument("--n", type=int, default=1 << 24, help="elements per client")
    ap.add_argument("--block", type=int, nargs="+", default=[128, 16])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "q8_probe.json"))
    a = ap.parse_args()
    res = [probe(k, a.n, a.block, a.reps, a.warmup) for k in a.k]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps([{key: ({q: w for q, w in v.items() if q != "ms"} if isinstance(v, dict) else v)
                       for key, v in r.items()} for r in res], indent=1))


if __name__ == "__main__":
    main()
