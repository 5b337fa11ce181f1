#!/usr/bin/env python
"""Time Krum's distance pass on block-quantized int8 clients (fa_pairwise_gram_q8) against, in the same
process and over the same K, n and block size B:

  * ``deq_f32``: what a caller does without it -- every client dequantized to float32 (fa_weighted_sum_q8
    with k = 1 and SUM, all K clients as K segments of ONE launch) followed by eng.pairwise_sqdist over the
    K float32 rows (4 K n bytes written and read back);
  * ``read_probe``: fa_read_probe over the same q bytes, the floor of any kernel that reads them once.

All forms are timed in INTERLEAVED repetitions (HIP events on the stream) after a warm-up; the JSON holds
every repetition, the medians and the spread (min, max).  The q8 form's K n (1 + 4 / B) bytes over its
time are given in GB/s and as a share of the read ceiling of the same process.  The MFMA count does not
depend on B and the float64 scale steps fall by B / 64, so the q8 times across B at one K separate the
scale step from the rest.

--selection T: on T attacked cohorts (a small state_dict, a quarter of the clients at a shifted mean, as
tests/test_gpu_q8_krum.py) count how often Krum (m = 1) and multi-Krum (m = K / 4) select the same
clients from the q8 distances as from the unquantized float32 originals -- in the same order, and as a
set.  A record, not a contract: quantization legitimately moves near-ties.

    python tools/q8_krum_probe.py --k 16 32 128 --block 64 128 1024 --reps 11 --selection 20
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import types
from collections import OrderedDict

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

    from fedml_amd.engine import SUM, get_engine
    eng = get_engine(0)
    x = torch.empty(k, n, dtype=torch.float32, device=eng.device).normal_()
    deq = torch.empty(k, n, dtype=torch.float32, device=eng.device)
    xs, ds = list(x.unbind(0)), list(deq.unbind(0))
    st = torch.cuda.current_stream(eng.device)
    q = torch.empty(k, n, dtype=torch.int8, device=eng.device)
    forms = {"read_probe": lambda: eng.read_probe(q, 128)}
    q8_read = {}
    for b in blocks:
        qb = q if b == blocks[0] else torch.empty_like(q)
        sc = torch.empty(k, -(-n // b), dtype=torch.float32, device=eng.device)
        qs, scs = list(qb.unbind(0)), list(sc.unbind(0))
        eng.quantize_q8(xs, b, outs=(qs, scs))
        q8_read[b] = k * n + 4 * k * (-(-n // b))

        def gram(qs=qs, scs=scs, b=b):
            eng.pairwise_gram_q8([qs], [scs], b)

        def deq_f32(qs=qs, scs=scs, b=b):
            eng.weighted_sum_q8([[t] for t in qs], [[t] for t in scs], SUM, None, b, outs=ds)
            eng.pairwise_sqdist([ds])
        forms[f"q8_b{b}"], forms[f"deq_f32_b{b}"] = gram, deq_f32
    del x, xs
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            ms[name].append(timed(fn, st))
    ceiling = k * n / min(ms["read_probe"]) / 1e9  # TB/s: bytes / ms / 1e9
    res = {"k": k, "n": n, "blocks": list(blocks), "reps": reps, "read_ceiling_tb_per_s": round(ceiling, 3)}
    for name, v in ms.items():
        res[name] = {"ms": [round(t, 4) for t in v], "median_ms": round(statistics.median(v), 4),
                     "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    for b in blocks:
        a, d = res[f"q8_b{b}"], res[f"deq_f32_b{b}"]
        a["q8_read_gb_per_s"] = round(q8_read[b] / a["median_ms"] / 1e6, 1)
        a["q8_read_over_ceiling"] = round(q8_read[b] / a["median_ms"] / 1e9 / ceiling, 4)
        a["over_read_probe"] = round(a["median_ms"] / res["read_probe"]["median_ms"], 3)
        res[f"q8_over_deq_f32_b{b}"] = {"median": round(a["median_ms"] / d["median_ms"], 4),
                                        "min": round(a["min_ms"] / d["max_ms"], 4),
                                        "max": round(a["max_ms"] / d["min_ms"], 4)}
    return res


def selection(k, trials, block):
    import torch

    from fedml_amd.core.security.defense.krum_defense import KrumDefense
    from fedml_amd.ml.aggregator.quantized import quantize_state_dict
    f = k // 4
    same, same_set = {1: 0, f: 0}, {1: 0, f: 0}
    for trial in range(trials):
        g = torch.Generator().manual_seed(1000 * k + trial)
        base = OrderedDict([("conv.weight", torch.randn(16, 8, 3, 3, generator=g)),
                            ("bn.running_mean", torch.randn(16, generator=g)),
                            ("fc.weight", torch.randn(10, 37, generator=g))])
        bad = set(torch.randperm(k, generator=g)[:f].tolist())
        plain = [(1, OrderedDict((key, (v + (2.0 if i in bad else 0.0)
                                        + 0.1 * torch.randn(v.shape, generator=g)).cuda()) for key, v in base.items()))
                 for i in range(k)]
        q8 = [(1, quantize_state_dict(sd, block)) for _, sd in plain]
        for m in same:
            d = KrumDefense(types.SimpleNamespace(byzantine_client_num=f, krum_param_m=m))
            pick = [[next(i for i, c in enumerate(cl) if c is p) for p in d.defend_before_aggregation(cl)]
                    for cl in (plain, q8)]
            same[m] += pick[0] == pick[1]
            same_set[m] += set(pick[0]) == set(pick[1])
    return {"k": k, "byzantine": f, "block": block, "trials": trials,
            "same_order": {f"m={m}": c for m, c in same.items()},
            "same_set": {f"m={m}": c for m, c in same_set.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, nargs="+", default=[16, 32, 128])
    ap.add_argument("--n", type=int, default=1 << 24, help="elements per client")
    ap.add_argument("--block", type=int, nargs="+", default=[64, 128, 1024])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--selection", type=int, default=0, help="attacked cohorts per K for the selection record")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "q8_krum_probe.json"))
    a = ap.parse_args()
    res = {"timing": [probe(k, a.n, a.block, a.reps, a.warmup) for k in a.k],
           "selection": [selection(k, a.selection, 128) for k in a.k if a.selection and k >= 32]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    brief = [{key: ({q: w for q, w in v.items() if q != "ms"} if isinstance(v, dict) else v) for key, v in r.items()}
             for r in res["timing"]]
    print(json.dumps({"timing": brief, "selection": res["selection"]}, indent=1))


if __name__ == "__main__":
    main()
