#!/usr/bin/env python
"""Time the randomized Hadamard rotation (fa_hadamard_rotate, include/fedagg_rotate.h) in one process.

(i) ``kernel``: P float32 elements (a whole number of blocks at every b), forward and inverse at each
    --b, every timed case ALTERNATED with ``sum_k1``: fa_weighted_sum_multi with one client over the same
    float32 buffer, which moves the same 8 bytes per element (4 read, 4 written) and does one multiply.
    A timed sample is --batch back-to-back calls inside one HIP event pair, divided by the batch: the
    host preparation of all calls but the first runs under the kernel before it, so the figure is close
    to the kernel time and is named ``ms_per_call_in_batch``.  It is reported as GB/s over 8 P bytes and
    as a ratio to the ``sum_k1`` samples taken next to it.  Kernel times proper come from a run under
    `rocprofv3 --kernel-trace --stats`, in a run of its own.

(ii) ``calls``: K clients of one key of n elements, FedAvg weights:
    ``rot_q1`` / ``rot_fp4``  aggregate_rotated over rotated q1 (block 128) / MXFP4 uploads;
    ``q1`` / ``fp4``          the same aggregate_q1 / aggregate_mx call without rotation;
    ``f32``                   aggregate over the float32 clients the uploads were made from.
    These are whole CALL times (the Python layers, the tables, the kernels), interleaved, one call per
    event pair.  ``rot_over_plain`` is what the rotation adds to a round, ``f32_over_rot_q1`` what the
    rotated compressed round still saves.

The JSON holds every sample, the medians and the spread (min, max) of both sides of every ratio.

    python tools/rht_probe.py --out bench_outputs/rht_probe.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED, ROUND = 0x0123456789ABCDEF, 1


def timed(fn, stream, batch=1):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(batch):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / batch


def summary(v):
    return {"ms": [round(t, 4) for t in v], "median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
            "max_ms": round(max(v), 4)}


def kernel_probe(p, bs, reps, warmup, batch):
    import torch

    from fedml_amd.engine import SUM, get_engine
    eng = get_engine(0)
    x = torch.empty(p, dtype=torch.float32, device=eng.device).normal_()
    y = torch.empty(p, dtype=torch.float32, device=eng.device)
    st = torch.cuda.current_stream(eng.device)

    def base():
        eng.weighted_sum_multi([[x]], SUM, None, outs=[y])
    cases = {f"b{b}_{'inverse' if inv else 'forward'}":
             (lambda b=b, inv=inv: eng.hadamard_rotate([x], b, SEED, ROUND, [0], inverse=inv,
                                                       numels=[p] if inv else None, outs=[y]))
             for b in bs for inv in (False, True)}
    for _ in range(warmup):
        base()
        for fn in cases.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: ([], []) for name in cases}  # the case, and the sum_k1 sample taken next to it
    for _ in range(reps):
        for name, fn in cases.items():
            ms[name][0].append(timed(fn, st, batch))
            ms[name][1].append(timed(base, st, batch))
    res = {"p": p, "bytes": 8 * p, "reps": reps, "batch": batch}
    for name, (v, s) in ms.items():
        r, rs = summary(v), summary(s)
        res[name] = {"ms_per_call_in_batch": r, "sum_k1_ms_per_call_in_batch": rs,
                     "gb_per_s": round(8 * p / r["median_ms"] / 1e6, 1),
                     "sum_k1_gb_per_s": round(8 * p / rs["median_ms"] / 1e6, 1),
                     "time_over_sum_k1": round(r["median_ms"] / rs["median_ms"], 4)}
    return res


def call_probe(k, n, log2_block, reps, warmup):
    import torch

    from fedml_amd.engine import MUL_W, get_engine
    from fedml_amd.ml.aggregator.microscaled import aggregate_mx, mx_quantize_state_dict
    from fedml_amd.ml.aggregator.rotated import Rotation, aggregate_rotated, rotate_state_dict
    from fedml_amd.ml.aggregator.signcompressed import aggregate_q1, sign_compress_state_dict
    from fedml_amd.ml.aggregator.state_dict_agg import aggregate
    eng = get_engine(0)
    g = torch.Generator().manual_seed(k)
    counts = torch.randint(50, 601, (k,), generator=g).tolist()
    w = [c / sum(counts) for c in counts]
    x = torch.empty(k, n, dtype=torch.float32, device=eng.device).normal_()
    f32 = [OrderedDict(w=row) for row in x.unbind(0)]
    rot = Rotation(SEED, ROUND, log2_block)
    ups = {"q1": [sign_compress_state_dict(d, 128) for d in f32],
           "fp4": [mx_quantize_state_dict(d, "fp4") for d in f32],
           "rot_q1": [rotate_state_dict(d, rot, "q1") for d in f32],
           "rot_fp4": [rotate_state_dict(d, rot, "fp4") for d in f32]}
    forms = {"f32": lambda: aggregate(f32, MUL_W, w),
             "q1": lambda: aggregate_q1(ups["q1"], MUL_W, w),
             "rot_q1": lambda: aggregate_rotated(ups["rot_q1"], MUL_W, w, SEED),
             "fp4": lambda: aggregate_mx(ups["fp4"], MUL_W, w),
             "rot_fp4": lambda: aggregate_rotated(ups["rot_fp4"], MUL_W, w, SEED)}
    st = torch.cuda.current_stream(eng.device)
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            ms[name].append(timed(fn, st))
    res = {"k": k, "n": n, "log2_block": log2_block, "reps": reps}
    res.update({name: summary(v) for name, v in ms.items()})
    for fam in ("q1", "fp4"):
        res[f"rot_over_plain_{fam}"] = round(res[f"rot_{fam}"]["median_ms"] / res[fam]["median_ms"], 4)
        res[f"rot_minus_plain_{fam}_ms"] = round(res[f"rot_{fam}"]["median_ms"] - res[fam]["median_ms"], 4)
    res["f32_over_rot_q1"] = round(res["f32"]["median_ms"] / res["rot_q1"]["median_ms"], 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--p", type=int, default=1 << 27, help="elements of the kernel cases")
    ap.add_argument("--b", type=int, nargs="+", default=[5, 10, 13])
    ap.add_argument("--k", type=int, nargs="*", default=[16, 128])
    ap.add_argument("--n", type=int, default=1 << 24, help="elements per client of the whole calls")
    ap.add_argument("--log2-block", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "rht_probe.json"))
    a = ap.parse_args()
    res = {"kernel": kernel_probe(a.p, a.b, a.reps, a.warmup, a.batch),
           "calls": [call_probe(k, a.n, a.log2_block, a.reps, a.warmup) for k in a.k]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)

    def brief(v):
        if isinstance(v, dict):
            return {q: brief(w) for q, w in v.items() if q != "ms"}
        return [brief(w) for w in v] if isinstance(v, list) else v
    print(json.dumps(brief(res), indent=1))


if __name__ == "__main__":
    main()
