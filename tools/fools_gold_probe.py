#!/usr/bin/env python
"""Time FoolsGold's device pass (fa_pairwise_dot) on float32 clients, in two modes -- (a) no history,
(b) the history updated in place -- against, in the same process and on the same buffers:

  * ``sqdist``: fa_pairwise_sqdist's direct kernel at the same K and P, the existing kernel of the same
    structure (K P 4 bytes read);
  * ``unfused``: the alternative to (b) without the fused kernel, one torch in-place add of the updates
    into the histories followed by mode (a) over the histories;
  * the box's read ceiling (fa_read_probe over the inputs' own pages), and from it the least time the
    bytes each mode must move would take: K P 4 for (a), 3 K P 4 for (b) (the inputs and the histories
    read, the histories written).

The forms are timed in INTERLEAVED repetitions (HIP events on the stream), so a drift of the machine
hits all alike; the JSON holds every repetition, the medians and the spread (min, max).  The default P
makes K P 4 = 2 GiB at every K, well beyond the caches.

    python tools/fools_gold_probe.py --k 16 32 128 --reps 11 --out bench_outputs/fools_gold_probe.json
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


def probe(k, input_bytes, reps, warmup):
    import torch

    from fedml_amd.engine import get_engine
    eng = get_engine(0)
    p = input_bytes // (4 * k) // 1024 * 1024
    x = torch.empty(k, p, dtype=torch.float32, device=eng.device).normal_()
    hist = torch.zeros(k, p, dtype=torch.float32, device=eng.device)   # (b)'s histories
    hist2 = torch.zeros(k, p, dtype=torch.float32, device=eng.device)  # the unfused alternative's
    xs, hs, hs2 = [list(x.unbind(0))], [list(hist.unbind(0))], [list(hist2.unbind(0))]
    st = torch.cuda.current_stream(eng.device)

    def unfused():
        hist2.add_(x)
        eng.pairwise_dot(hs2)

    forms = {"a_no_history": lambda: eng.pairwise_dot(xs),
             "b_history": lambda: eng.pairwise_dot(xs, None, hs),
             "sqdist": lambda: eng._pairwise_launch(xs, form="direct"),
             "unfused": unfused,
             "read_probe": lambda: eng.read_probe(x, 128)}
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    # both routes have added the same updates the same number of times: the same histories, bit for bit
    same = bool(torch.equal(hist, hist2))
    ms = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            ms[name].append(timed(fn, st))
    same = same and bool(torch.equal(hist, hist2))
    kp4 = k * p * 4
    moved = {"a_no_history": kp4, "b_history": 3 * kp4, "sqdist": kp4, "unfused": 4 * kp4, "read_probe": kp4}
    ceiling = kp4 / min(ms["read_probe"]) / 1e9  # TB/s: bytes / ms / 1e9
    res = {"k": k, "p": p, "dtype": "float32", "layout": "flat", "input_bytes": kp4, "reps": reps,
           "read_ceiling_tb_per_s": round(ceiling, 3), "histories_equal": same}
    for name, v in ms.items():
        med = statistics.median(v)
        res[name] = {"ms": [round(t, 4) for t in v], "median_ms": round(med, 4), "min_ms": round(min(v), 4),
                     "max_ms": round(max(v), 4), "moved_bytes": moved[name],
                     "moved_tb_per_s": round(moved[name] / med / 1e9, 3),
                     "bytes_over_ceiling_ms": round(moved[name] / ceiling / 1e9, 4)}
    res["b_over_unfused"] = round(res["b_history"]["median_ms"] / res["unfused"]["median_ms"], 4)
    res["a_over_sqdist"] = round(res["a_no_history"]["median_ms"] / res["sqdist"]["median_ms"], 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, nargs="+", default=[16, 32, 128])
    ap.add_argument("--input-gib", type=float, default=2.0, help="K P 4 bytes of inputs at every K")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "fools_gold_probe.json"))
    a = ap.parse_args()
    res = [probe(k, int(a.input_gib * (1 << 30)), a.reps, a.warmup) for k in a.k]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps([{key: ({q: w for q, w in v.items() if q != "ms"} if isinstance(v, dict) else v)
                       for key, v in r.items()} for r in res], indent=1))


if __name__ == "__main__":
    main()
