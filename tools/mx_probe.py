#!/usr/bin/env python
"""Time the fused decode-and-sum of Microscaling clients (fa_weighted_sum_mx, FedAvg weights, MXFP8 and
MXFP4) against, in the same process and over the same K and n:

  * ``f32``: fa_weighted_sum_multi over the K float32 rows the mx rows were quantized from;
  * ``q8_b128``: fa_weighted_sum_q8 over the same rows quantized to q8 at B = 128;
  * ``unfused_<fmt>``: the route without the fused kernel -- every client decoded to float32
    (fa_weighted_sum_mx with k = 1 and SUM; all K clients as K segments of ONE launch, the form most
    favourable to this route) followed by fa_weighted_sum_multi over the K decoded rows;
  * ``quantize_<fmt>``: fa_quantize_mx of the K float32 rows;
  * the box's read ceiling (fa_read_probe over the float32 rows' own pages).

Byte counts come from the shapes (b = 1 byte per element for fp8, 1/2 for fp4, plus 1/32 of scale):
  mx       K n (b + 1/32) read + 4 n written
  q8       K n (1 + 4/128) read + 4 n written
  f32      4 K n read + 4 n written
  unfused  K n (b + 1/32) read + 4 K n written, then f32's
  quantize 4 K n read + K n (b + 1/32) written
All forms are timed in INTERLEAVED repetitions (HIP events on the stream) after a warm-up, so a drift of
the machine hits all alike; the JSON holds every repetition, the medians and the spread (min, max).

What the times are: the event pair brackets the whole engine call on an idle stream -- the Python
argument checks over 2 K tensors, the ctypes tables, the staging copy and the kernel -- so they are
CALL times, the figure a server sees, and hold some 0.05-0.18 ms of host preparation that grows with K.
KERNEL times come from a run of this tool under `rocprofv3 --kernel-trace --stats`, in a run of its own
(`profiles/mx/k*_kernel_stats.csv`; DESIGN, microscaled family, gives both).

``valu_per_client_element_counted_by_hand`` is NOT measured: it was counted by hand in the whole-group
client loop of k_wsum_mx<fmt, MUL_W> in the gfx950 assembly (`make -C fedml_amd/csrc asm`), and is recorded so that a reader of the JSON has the count the
times were read against.  Recount it when the kernel or its build flags change.

    python tools/mx_probe.py --k 16 32 128 --reps 11 --out bench_outputs/mx_probe.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# counted by hand (see above), per client: conversions + packed multiplies + packed adds + the scale
# shift, the coefficient's conversion and the two 64-bit address adds, over the lane's elements
VALU_PER_CLIENT_ELEMENT = {"fp8": (8 + 8 + 8 + 4) / 16, "fp4": (16 + 16 + 16 + 4) / 32}


def timed(fn, stream):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def probe(k, n, reps, warmup):
    import torch

    from fedml_amd.engine import MUL_W, SUM, get_engine
    eng = get_engine(0)
    g = torch.Generator().manual_seed(k)
    counts = torch.randint(50, 601, (k,), generator=g).tolist()
    w = [c / sum(counts) for c in counts]
    dev = eng.device
    x = torch.empty(k, n, dtype=torch.float32, device=dev).normal_()
    deq = torch.empty(k, n, dtype=torch.float32, device=dev)  # the unfused route's float32 rows
    xs, ds = list(x.unbind(0)), list(deq.unbind(0))
    out = torch.empty(n, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev)

    q = torch.empty(k, n, dtype=torch.int8, device=dev)
    qsc = torch.empty(k, -(-n // 128), dtype=torch.float32, device=dev)
    qs, qscs = list(q.unbind(0)), list(qsc.unbind(0))
    eng.quantize_q8(xs, 128, outs=(qs, qscs))
    forms = {"f32": lambda: eng.weighted_sum_multi([xs], MUL_W, w, outs=[out]),
             "read_probe": lambda: eng.read_probe(x, 128),
             "q8_b128": lambda: eng.weighted_sum_q8([qs], [qscs], MUL_W, w, 128, outs=[out])}
    moved = {"f32": 4 * k * n + 4 * n, "read_probe": 4 * k * n, "q8_b128": k * n + 4 * k * (-(-n // 128)) + 4 * n}
    read = {"q8_b128": moved["q8_b128"] - 4 * n}
    for fmt, epb in (("fp8", 1), ("fp4", 2)):
        d = torch.empty(k, -(-n // epb), dtype=torch.uint8, device=dev)
        sc = torch.empty(k, -(-n // 32), dtype=torch.uint8, device=dev)
        dl, scl = list(d.unbind(0)), list(sc.unbind(0))
        eng.quantize_mx(xs, fmt, outs=(dl, scl))
        read[f"mx_{fmt}"] = d.numel() + sc.numel()

        def fused(dl=dl, scl=scl, fmt=fmt):
            eng.weighted_sum_mx([dl], [scl], [n], fmt, MUL_W, w, outs=[out])

        def unfused(dl=dl, scl=scl, fmt=fmt):
            eng.weighted_sum_mx([[t] for t in dl], [[t] for t in scl], [n] * k, fmt, SUM, None, outs=ds)
            eng.weighted_sum_multi([ds], MUL_W, w, outs=[out])

        def quantize(dl=dl, scl=scl, fmt=fmt):
            eng.quantize_mx(xs, fmt, outs=(dl, scl))  # rewrites the same bytes
        forms[f"mx_{fmt}"], forms[f"unfused_{fmt}"], forms[f"quantize_{fmt}"] = fused, unfused, quantize
        moved[f"mx_{fmt}"] = read[f"mx_{fmt}"] + 4 * n
        moved[f"unfused_{fmt}"] = read[f"mx_{fmt}"] + 4 * k * n + moved["f32"]
        moved[f"quantize_{fmt}"] = 4 * k * n + read[f"mx_{fmt}"]
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            ms[name].append(timed(fn, st))
    ceiling = 4 * k * n / min(ms["read_probe"]) / 1e9  # TB/s: bytes / ms / 1e9
    res = {"k": k, "n": n, "reps": reps, "read_ceiling_tb_per_s": round(ceiling, 3),
           "valu_per_client_element_counted_by_hand": VALU_PER_CLIENT_ELEMENT}
    for name, v in ms.items():
        med = statistics.median(v)
        res[name] = {"ms": [round(t, 4) for t in v], "median_ms": round(med, 4), "min_ms": round(min(v), 4),
                     "max_ms": round(max(v), 4), "moved_bytes": moved[name],
                     "moved_tb_per_s": round(moved[name] / med / 1e9, 3),
                     "bytes_over_ceiling_ms": round(moved[name] / ceiling / 1e9, 4)}
    for name, rd in read.items():
        med = res[name]["median_ms"]
        res[name]["read_bytes_per_client_element"] = round(rd / (k * n), 4)
        res[name]["time_over_bytes_at_ceiling"] = round(med / res[name]["bytes_over_ceiling_ms"], 3)
        res[f"f32_over_{name}"] = round(res["f32"]["median_ms"] / med, 4)
    for fmt in ("fp8", "fp4"):
        res[f"q8_b128_over_mx_{fmt}"] = round(res["q8_b128"]["median_ms"] / res[f"mx_{fmt}"]["median_ms"], 4)
        res[f"unfused_over_mx_{fmt}"] = round(res[f"unfused_{fmt}"]["median_ms"] / res[f"mx_{fmt}"]["median_ms"], 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, nargs="+", default=[16, 32, 128])
    ap.add_argument("--n", type=int, default=1 << 24, help="elements per client")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "mx_probe.json"))
    a = ap.parse_args()
    res = [probe(k, a.n, a.reps, a.warmup) for k in a.k]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps([{key: ({q: w for q, w in v.items() if q != "ms"} if isinstance(v, dict) else v)
                       for key, v in r.items()} for r in res], indent=1))


if __name__ == "__main__":
    main()
