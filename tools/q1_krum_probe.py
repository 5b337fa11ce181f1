#!/usr/bin/env python
"""Time Krum's distance pass on 1-bit sign clients (fa_pairwise_gram_q1) against, in the same process and
over the same K, n and block size B:

  * ``deq_f32``: what a caller does without it -- every client decompressed to float32 (fa_weighted_sum_q1
    with one client and SUM, one launch per client) followed by eng.pairwise_sqdist over the K float32
    rows (4 K n bytes written and read back);
  * ``sqdist_f32``: eng.pairwise_sqdist alone over the rows decompressed beforehand.

Before timing, D of the q1 form and D of the float32 form are compared on the timed inputs (1e-5 relative
to the largest distance; the probe stops if they disagree).  All forms are timed in INTERLEAVED repetitions
(HIP events on the stream) after a warm-up; the JSON holds every repetition, the medians and the spread
(min, max), the ratios, and -- from OPS_PER_PAIR_BLOCK, the vector instructions per client pair and block
counted in the kernel's assembly (DESIGN.md, 1-bit sign family) -- the share of the vector issue rate the
q1 form reaches: its wave instructions (the upper-triangular pairs of ceil(K / 32) tiles, times n / B
blocks, times a lane's 16 pairs, times the ops) over the device's rate of CUs * 4 SIMDs * clock / 4 cycles
per wave instruction.

    python tools/q1_krum_probe.py --k 16 32 128 --block 32 128 1024 --reps 11
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# vector instructions per owned pair and block in k_gram_q1's stage loop: B / 32 XORs and as many counts,
# then shift, subtract, convert, multiply and fma
OPS_PER_PAIR_BLOCK = {32: 2 + 5, 128: 8 + 5, 1024: 64 + 5}


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

    from fedml_amd.engine import SUM, get_engine
    eng = get_engine(0)
    props = torch.cuda.get_device_properties(eng.device)
    wave_rate = props.multi_processor_count * 4 * getattr(props, "clock_rate", 2400000) * 1e3 / 4  # wave instructions per second
    x = torch.empty(k, n, dtype=torch.float32, device=eng.device).normal_()
    xs = list(x.unbind(0))
    deq = torch.empty(k, n, dtype=torch.float32, device=eng.device)
    ds = list(deq.unbind(0))
    st = torch.cuda.current_stream(eng.device)
    forms, agree = {}, {}
    for b in blocks:
        bits, scs = eng.quantize_q1(xs, b)

        def gram(bits=bits, scs=scs, b=b):
            return eng.pairwise_gram_q1([bits], [scs], [n], b)[1]

        def deq_f32(bits=bits, scs=scs, b=b):
            for i in range(k):
                eng.weighted_sum_q1([[bits[i]]], [[scs[i]]], [n], SUM, None, b, outs=[ds[i]])
            return eng.pairwise_sqdist([ds])

        d1, d32 = gram().double(), deq_f32().double()
        agree[b] = float((d1 - d32).abs().max() / d32.max())
        if not agree[b] <= 1e-5:
            raise SystemExit(f"K={k} B={b}: the q1 and the float32 distances differ by {agree[b]:.3g} relative")
        forms[f"q1_b{b}"], forms[f"deq_f32_b{b}"] = gram, deq_f32
    del x, xs
    forms["sqdist_f32"] = lambda: eng.pairwise_sqdist([ds])  # over the last block size's rows
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            ms[name].append(timed(fn, st))
    res = {"k": k, "n": n, "blocks": list(blocks), "reps": reps, "d_rel_diff": agree}
    for name, v in ms.items():
        res[name] = {"ms": [round(t, 4) for t in v], "median_ms": round(statistics.median(v), 4),
                     "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    nt = -(-k // 32)
    for b in blocks:
        a, d = res[f"q1_b{b}"], res[f"deq_f32_b{b}"]
        if b in OPS_PER_PAIR_BLOCK:
            a["wave_instr"] = nt * (nt + 1) // 2 * 16 * (n // b) * OPS_PER_PAIR_BLOCK[b]
            a["vector_issue_share"] = round(a["wave_instr"] / (a["median_ms"] * 1e-3) / wave_rate, 4)
        res[f"q1_over_deq_f32_b{b}"] = {"median": round(a["median_ms"] / d["median_ms"], 4),
                                        "min": round(a["min_ms"] / d["max_ms"], 4),
                                        "max": round(a["max_ms"] / d["min_ms"], 4)}
        res[f"q1_over_sqdist_f32_b{b}"] = round(a["median_ms"] / res["sqdist_f32"]["median_ms"], 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, nargs="+", default=[16, 32, 128])
    ap.add_argument("--n", type=int, default=1 << 24, help="elements per client")
    ap.add_argument("--block", type=int, nargs="+", default=[32, 128, 1024])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "q1_krum_probe.json"))
    a = ap.parse_args()
    res = {"timing": [probe(k, a.n, a.block, a.reps, a.warmup) for k in a.k]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps([{key: ({q: w for q, w in v.items() if q != "ms"} if isinstance(v, dict) else v)
                       for key, v in r.items()} for r in res["timing"]], indent=1))


if __name__ == "__main__":
    main()
