#!/usr/bin/env python
"""Time the fused geometric-median pass (fa_weighted_sum_sqdist_tiled) against the weighted sum it
contains (fa_weighted_sum_tiled, MUL_W) over the same rows of a tiled float32 arena group.

The weighted sum is the floor: it reads the same K x P x 4 bytes and does no distance work.  The two
are timed in INTERLEAVED repetitions on one device (HIP events on the stream), so a drift of the
machine hits both alike; the JSON holds every repetition, the medians, the spread (min, max) and the
ratio of the medians.  Where the library picks a single-read form (float32, K <= 32) the generic
kernel (FA_WSD_REG=0, read per call) is a third interleaved form.

    python tools/geomed_probe.py --k 32 128 --log2p 24 --reps 15 --out bench_outputs/geomed_probe.json

Counter run (one kernel, one counter set per run; ``rocprofv3 --pmc FETCH_SIZE WRITE_SIZE
--output-format csv -d DIR -- python tools/geomed_probe.py --k 32 --only fused --reps 3``), then
``--pmc-dir DIR`` summarises the fused kernel's dispatches against K x P x 4 bytes.  On gfx950 FETCH_SIZE
counts half the bytes of a wide streaming read (tools/pmc_traffic.py), so read = 2 x FETCH_SIZE KiB.
"""
from __future__ import annotations

import argparse
import csv
import glob
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


def probe(k, log2p, reps, warmup, only):
    import torch

    from fedml_amd.engine import MUL_W, get_engine
    eng = get_engine(0)
    p = 1 << log2p
    E = 1024
    buf = torch.empty(p // E, k, E, dtype=torch.float32, device=eng.device).normal_()
    rows = list(range(k))
    coef = [1.0 / k] * k
    out = torch.empty(p, dtype=torch.float32, device=eng.device)
    st = torch.cuda.current_stream(eng.device)
    forms = {"wsum": lambda: eng.weighted_sum_tiled(buf, rows, MUL_W, coef, out=out),
             "fused": lambda: eng.weighted_sum_sqdist_tiled(buf, rows, coef, out=out)}

    def generic():  # the generic two-walk kernel where the library would pick a single-read form
        os.environ["FA_WSD_REG"] = "0"
        try:
            eng.weighted_sum_sqdist_tiled(buf, rows, coef, out=out)
        finally:
            del os.environ["FA_WSD_REG"]

    if k <= 32:
        forms["fused_generic"] = generic
    if only:
        forms = {only: forms[only]}
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            ms[name].append(timed(fn, st))
    res = {"k": k, "p": p, "dtype": "float32", "layout": "tiled", "input_bytes": k * p * 4, "reps": reps}
    for name, v in ms.items():
        med = statistics.median(v)
        res[name] = {"ms": [round(x, 4) for x in v], "median_ms": round(med, 4), "min_ms": round(min(v), 4),
                     "max_ms": round(max(v), 4), "input_tb_per_s": round(k * p * 4 / med / 1e9, 3)}
    if "wsum" in ms and "fused" in ms:
        res["fused_over_wsum"] = round(res["fused"]["median_ms"] / res["wsum"]["median_ms"], 4)
    if "fused_generic" in ms and "fused" in ms:
        res["fused_over_generic"] = round(res["fused"]["median_ms"] / res["fused_generic"]["median_ms"], 4)
    return res


def pmc_summary(d, k, log2p):
    vals = {}
    for f in sorted(glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name = row.get("Kernel_Name", "")
                if "k_wsd" in name and "k_wsd_reduce" not in name:
                    vals.setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
    res = {"k": k, "p": 1 << log2p, "input_bytes": k * (1 << log2p) * 4,
           "kernel": "k_wsd_reg" if k <= 32 else "k_wsd"}
    for name, v in vals.items():
        res[name + "_kib_median"] = statistics.median(v)
        res[name + "_dispatches"] = len(v)
    if "FETCH_SIZE" in vals:
        res["read_bytes"] = 2.0 * statistics.median(vals["FETCH_SIZE"]) * 1024
        res["read_over_input"] = round(res["read_bytes"] / res["input_bytes"], 4)
    if "WRITE_SIZE" in vals:
        res["write_bytes"] = statistics.median(vals["WRITE_SIZE"]) * 1024
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--log2p", type=int, default=24)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["wsum", "fused", "fused_generic"], default=None)
    ap.add_argument("--pmc-dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "geomed_probe.json"))
    a = ap.parse_args()
    if a.pmc_dir:
        res = [pmc_summary(a.pmc_dir, a.k[0], a.log2p)]
    else:
        res = [probe(k, a.log2p, a.reps, a.warmup, a.only) for k in a.k]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    for r in res:
        print(json.dumps({key: v for key, v in r.items() if not isinstance(v, dict)} |
                         {key: {q: w for q, w in v.items() if q != "ms"} for key, v in r.items() if isinstance(v, dict)}))


if __name__ == "__main__":
    main()
