#!/usr/bin/env python
"""Time one geometric-median pass on block-quantized int8 clients (fa_weighted_sum_sqdist_q8) against, in
the same process and over the same K, n and block size B:

  * ``q8``: the new entry, straight from the quantized bytes (K n (1 + 4 / B) bytes per pass);
  * ``f32``: fa_weighted_sum_sqdist on float32 tensors dequantized BEFORE the clock starts -- what every pass
    after the first costs a caller who keeps a float32 copy of the cohort (4 K n bytes resident);
  * ``deq_f32``: the dequantization of the K clients (fa_weighted_sum_q8 with k = 1 and SUM, all K clients as
    K segments of ONE launch) plus ``f32`` -- the first pass of that caller, or every pass of one who cannot
    keep the copy;
  * ``read_probe``: fa_read_probe over the same q bytes, the floor of any kernel that reads them once.

All forms are timed in INTERLEAVED repetitions (HIP events on the stream) after a warm-up; the JSON holds
every repetition, the medians and the spread (min, max).  ``centered`` adds the same three forms of one
centered-clipping pass.  FA_WSDQ_REG=0 in the environment times the generic kernel at K <= 32 (A/B).

    python tools/q8_geomed_probe.py --k 16 32 64 128 --block 128 --reps 11
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


def probe(k, n, block, reps, warmup, centered):
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
    out, cen = (torch.empty(n, dtype=torch.float32, device=eng.device) for _ in range(2))
    cen.normal_()
    coef = [1.0 / k] * k

    def dequantize():
        eng.weighted_sum_q8([[t] for t in qs], [[t] for t in scs], SUM, None, block, outs=ds)

    dequantize()
    forms = {"read_probe": lambda: eng.read_probe(q, 128),
             "q8": lambda: eng.weighted_sum_sqdist_q8([qs], [scs], coef, block, outs=[out]),
             "f32": lambda: eng.weighted_sum_sqdist([ds], coef, outs=[out]),
             "deq_f32": lambda: (dequantize(), eng.weighted_sum_sqdist([ds], coef, outs=[out]))}
    if centered:
        forms.update({"q8_centered": lambda: eng.centered_sum_sqdist_q8([qs], [scs], [cen], coef, block, outs=[out]),
                      "f32_centered": lambda: eng.centered_sum_sqdist([ds], [cen], coef, outs=[out]),
                      "q8_dist": lambda: eng.centered_sum_sqdist_q8([qs], [scs], [cen], None, block),
                      "f32_dist": lambda: eng.centered_sum_sqdist([ds], [cen], None)})
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
    res = {"k": k, "n": n, "block": block, "reps": reps, "read_ceiling_tb_per_s": round(ceiling, 3),
           "reg_form": os.environ.get("FA_WSDQ_REG", "1") != "0" and k <= 32}
    for name, v in ms.items():
        res[name] = {"ms": [round(t, 4) for t in v], "median_ms": round(statistics.median(v), 4),
                     "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    med = lambda name: res[name]["median_ms"]  # noqa: E731
    res["q8"]["bytes_over_ceiling_ms"] = round(q8_read / ceiling / 1e9, 4)
    res["q8"]["over_its_bytes"] = round(med("q8") / (q8_read / ceiling / 1e9), 3)
    res["f32_over_q8"] = round(med("f32") / med("q8"), 3)
    res["deq_f32_over_q8"] = round(med("deq_f32") / med("q8"), 3)
    if centered:
        res["f32_centered_over_q8_centered"] = round(med("f32_centered") / med("q8_centered"), 3)
        res["f32_dist_over_q8_dist"] = round(med("f32_dist") / med("q8_dist"), 3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, nargs="+", default=[16, 32, 64, 128])
    ap.add_argument("--n", type=int, default=1 << 24, help="elements per client")
    ap.add_argument("--block", type=int, default=128)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--centered", action="store_true", help="also time the centered-clipping forms")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "q8_geomed_probe.json"))
    a = ap.parse_args()
    res = [probe(k, a.n, a.block, a.reps, a.warmup, a.centered) for k in a.k]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps([{key: ({q: w for q, w in v.items() if q != "ms"} if isinstance(v, dict) else v)
                       for key, v in r.items()} for r in res], indent=1))


if __name__ == "__main__":
    main()
