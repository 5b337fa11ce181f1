#!/usr/bin/env python
"""Times fa_coord_mean_around_median_tiled against fa_coord_trimmed_mean_tiled on the SAME rows of a
tiled arena (modelled on tools/time_trimmed_mean.py).

Workload: float32, K client rows of ResNet-18 size (bench.py's `median` config) in a tile-interleaved
ClientArena; the trimmed mean with trim b = K // 10 and the mean around the median with
keep = K - 2 b: the same sort and the same number of kept values, so the difference is the window
search and the per-lane walk.  The baseline is the shipped trimmed-mean kernel.  Per K: one untimed
launch of each, then `--reps` (>= 20) pairs of launches, trimmed mean first and mean around the median
second in every pair, each launch timed with its own HIP events; the medians of the two series are
reported with min / max and GB/s over K*P*4 + P*4 bytes.

PREDICTED holds the ratio expected from the instruction counts of the cross-compiled kernels (the
fast path's instructions, the in-order fall-back's left out), written down before the first run; it
assumes both kernels are bound by instruction issue, so where the trimmed mean sits at the read
pattern's floor (K <= 32) the measured ratio should come out lower, down to 1.0.

The measurement runs in a fresh child process under a time limit (the parent never opens the GPU):

    python tools/time_mean_around_median.py [--k 16 32 64 128] [--params P] [--reps 30] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESNET18_P = 11_699_132  # bench.py
HBM_BYTES_PER_S = 8e12
# instructions of k_mam_off<F32, B> / k_mam_2l<F32, 64> over k_tmean_off / k_tmean_2l, fall-backs left out:
# 674 / 549, 1414 / 1124, 3088 / 2661, 5317 / 4205.  (K = 128: written for k_mam_2l's first form, which compared
# all N - 1 ranks under a predicate; the branch on the range leaves 24 of 63 at this keep: 1.11, re-counted later.)
PREDICTED = {16: 1.23, 32: 1.26, 64: 1.16, 128: 1.26}


def child(args):
    sys.path.insert(0, ROOT)
    import torch

    from fedml_amd.arena import ArenaLayout, ClientArena
    from fedml_amd.engine import get_engine
    dev = "cuda:0"
    eng = get_engine(0)
    P = args.params
    rows_out = []
    for K in args.k:
        b = K // 10
        keep = K - 2 * b
        arena = ClientArena(ArenaLayout([("w", (P,), torch.float32)]), capacity=K, device=dev, zero=False, tiled=True)
        g = torch.Generator(device=dev).manual_seed(21)
        for i in range(K):
            arena.write(i, {"w": torch.randn(P, generator=g, device=dev)})
        torch.cuda.synchronize()
        buf, rows = arena.bufs[torch.float32], list(range(K))
        out_t = torch.empty(P, device=dev)
        out_m = torch.empty(P, device=dev)
        eng.coord_trimmed_mean_tiled(buf, rows, b, n=P, out=out_t)
        eng.coord_mean_around_median_tiled(buf, rows, keep, n=P, out=out_m)
        torch.cuda.synchronize()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(args.reps)]
        for e in ev:
            e[0].record()
            eng.coord_trimmed_mean_tiled(buf, rows, b, n=P, out=out_t)
            e[1].record()
            e[2].record()
            eng.coord_mean_around_median_tiled(buf, rows, keep, n=P, out=out_m)
            e[3].record()
        torch.cuda.synchronize()
        tm = [e[0].elapsed_time(e[1]) for e in ev]
        mam = [e[2].elapsed_time(e[3]) for e in ev]
        nbytes = K * P * 4 + P * 4
        rec = {"K": K, "trim": b, "keep": keep, "params": P, "reps": args.reps, "bytes": nbytes}
        for name, series in (("trimmed_mean", tm), ("mean_around_median", mam)):
            ms = statistics.median(series)
            rec[name] = {"ms": round(ms, 4), "min_ms": round(min(series), 4), "max_ms": round(max(series), 4),
                         "GBps": round(nbytes / (ms * 1e-3) / 1e9, 1),
                         "frac_of_8TBps": round(nbytes / (ms * 1e-3) / HBM_BYTES_PER_S, 3)}
        rec["ratio"] = round(statistics.median(mam) / statistics.median(tm), 3)
        rec["predicted_ratio"] = PREDICTED.get(K)
        rows_out.append(rec)
        print(json.dumps(rec), flush=True)
        del arena, buf, out_m, out_t
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/time_mean_around_median.py", "dtype": "float32", "layout": "tiled",
                       "baseline": "fa_coord_trimmed_mean_tiled", "note": "one run on one machine",
                       "rows": rows_out}, f, indent=1)
            f.write("\n")


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--k", type=int, nargs="+", default=[16, 32, 64, 128])
    p.add_argument("--params", type=int, default=RESNET18_P)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--out", default=None)
    p.add_argument("--limit", type=float, default=240.0, help="time limit of the measuring process, seconds")
    p.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.reps < 20:
        p.error("--reps must be >= 20")
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    try:
        rc = subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        print(f"time_mean_around_median: the measuring process exceeded {args.limit} s and was ended", file=sys.stderr)
        rc = 124
    sys.exit(rc)


if __name__ == "__main__":
    main()
