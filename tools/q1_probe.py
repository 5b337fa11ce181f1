#!/usr/bin/env python
"""Time the two server kernels of the 1-bit sign format (fa_weighted_sum_q1 with FedAvg weights and
fa_sign_vote_q1) against, in the same process and over the same K and n:

  * ``f32``: fa_weighted_sum_multi over the K float32 rows the q1 rows were compressed from;
  * ``q8``: fa_weighted_sum_q8 over the same rows block-quantized to int8, at the same block size;
  * ``read_probe``: fa_read_probe over the q1 rows' own bytes (bits, then scales), the time the bytes
    alone take on this box; and over the float32 rows, the box's read ceiling.

Byte counts come from the shapes:
  q1    K n (1/8 + 4 / B) read + 4 n written
  vote  K n / 8 read + 4 n written
  q8    K n (1 + 4 / B) read + 4 n written
  f32   4 K n read + 4 n written
All forms are timed in INTERLEAVED repetitions (HIP events on the stream) after a warm-up, so a drift of
the machine hits all alike; the JSON holds every repetition, the medians and the spread (min, max).

    python tools/q1_probe.py --k 16 32 128 --block 128 --reps 11 --out bench_outputs/q1_probe.json
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


def probe(k, n, block, reps, warmup):
    import torch

    from fedml_amd.engine import MUL_W, get_engine
    eng = get_engine(0)
    g = torch.Generator().manual_seed(k)
    counts = torch.randint(50, 601, (k,), generator=g).tolist()
    w = [c / sum(counts) for c in counts]
    nw, nb = -(-n // 32), -(-n // block)
    x = torch.empty(k, n, dtype=torch.float32, device=eng.device).normal_()
    xs = list(x.unbind(0))
    out = torch.empty(n, dtype=torch.float32, device=eng.device)
    st = torch.cuda.current_stream(eng.device)
    # one client's q1 row is contiguous: its bit words, then its scales (reinterpreted, never computed on)
    q1 = torch.empty(k, nw + nb, dtype=torch.int32, device=eng.device)
    bits = [q1[i, :nw] for i in range(k)]
    scs = [q1[i, nw:].view(torch.float32) for i in range(k)]
    eng.quantize_q1(xs, block, outs=(bits, scs))
    q = torch.empty(k, n, dtype=torch.int8, device=eng.device)
    s8 = torch.empty(k, nb, dtype=torch.float32, device=eng.device)
    q8s, s8s = list(q.unbind(0)), list(s8.unbind(0))
    eng.quantize_q8(xs, block, outs=(q8s, s8s))

    forms = {"f32": lambda: eng.weighted_sum_multi([xs], MUL_W, w, outs=[out]),
             "q8": lambda: eng.weighted_sum_q8([q8s], [s8s], MUL_W, w, block, outs=[out]),
             "q1": lambda: eng.weighted_sum_q1([bits], [scs], [n], MUL_W, w, block, outs=[out]),
             "vote": lambda: eng.sign_vote_q1([bits], [n], 1, 1.0, outs=[out]),
             "read_probe_q1": lambda: eng.read_probe(q1, 128),
             "read_probe_f32": lambda: eng.read_probe(x, 128)}
    q1_read, vote_read = 4 * k * (nw + nb), 4 * k * nw
    moved = {"f32": 4 * k * n + 4 * n, "q8": k * n + 4 * k * nb + 4 * n, "q1": q1_read + 4 * n,
             "vote": vote_read + 4 * n, "read_probe_q1": q1_read, "read_probe_f32": 4 * k * n}
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            ms[name].append(timed(fn, st))
    ceiling = 4 * k * n / min(ms["read_probe_f32"]) / 1e9  # TB/s: bytes / ms / 1e9
    res = {"k": k, "n": n, "block": block, "reps": reps, "read_ceiling_tb_per_s": round(ceiling, 3)}
    for name, v in ms.items():
        med = statistics.median(v)
        res[name] = {"ms": [round(t, 4) for t in v], "median_ms": round(med, 4), "min_ms": round(min(v), 4),
                     "max_ms": round(max(v), 4), "moved_bytes": moved[name],
                     "moved_tb_per_s": round(moved[name] / med / 1e9, 3),
                     "bytes_over_ceiling_ms": round(moved[name] / ceiling / 1e9, 4),
                     "time_over_bytes_time": round(med / (moved[name] / ceiling / 1e9), 2)}
    for name in ("q1", "vote"):
        res[f"f32_over_{name}"] = round(res["f32"]["median_ms"] / res[name]["median_ms"], 3)
        res[f"q8_over_{name}"] = round(res["q8"]["median_ms"] / res[name]["median_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, nargs="+", default=[16, 32, 128])
    ap.add_argument("--n", type=int, default=1 << 24, help="elements per client")
    ap.add_argument("--block", type=int, default=128)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "q1_probe.json"))
    a = ap.parse_args()
    res = [probe(k, a.n, a.block, a.reps, a.warmup) for k in a.k]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps([{key: ({q: w for q, w in v.items() if q != "ms"} if isinstance(v, dict) else v)
                       for key, v in r.items()} for r in res], indent=1))


if __name__ == "__main__":
    main()
