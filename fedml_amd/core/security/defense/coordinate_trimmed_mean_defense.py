"""Coordinate-wise trimmed mean (Yin et al. 2018, "Byzantine-Robust Distributed Learning: Towards
Optimal Statistical Rates") on the HIP engine: ``defense_type="coordinate_trimmed_mean"``.

The reference has no such defense -- its ``trimmed_mean`` (coordinate_wise_trimmed_mean_defense.py,
mirrored next to this file) trims whole CLIENTS by sample count.  This one is the operator the name
promises: for every coordinate the K client values are sorted, the b = int(beta * K) smallest and b
largest dropped, and the rest averaged (contract, bit for bit: include/fedagg_robust.h,
fa_coord_trimmed_mean).  It acts on aggregation, like the median, and is unweighted: sample counts
are ignored.

Every floating-point key of client 0's dict -- BatchNorm running statistics included -- gets the
trimmed mean over the clients, in that key's dtype, one launch per dtype group.  Non-float keys (a
BatchNorm ``num_batches_tracked``) take the base aggregation's value.  The result is a new
OrderedDict in client 0's key order on the clients' device; the inputs are not modified.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Any, Callable, List, Tuple

import torch

from ....arena import resident_rows
from ....engine import get_engine

_NATIVE = (torch.float32, torch.bfloat16, torch.float16, torch.float64)


class CoordinateTrimmedMeanDefense(object):
    def __init__(self, config):
        self.config = config
        self.beta = float(config.beta)
        if not self.beta >= 0.0:
            raise ValueError(f"coordinate_trimmed_mean: beta must be >= 0 (got {config.beta})")

    def trim_count(self, k: int) -> int:
        b = int(self.beta * k)
        if not (0 <= b and 2 * b < k):
            raise ValueError(f"coordinate_trimmed_mean: beta {self.beta} trims {b} of {k} clients at each end")
        return b

    def defend_on_aggregation(self, raw_client_grad_list: List[Tuple[float, OrderedDict]],
                              base_aggregation_func: Callable = None, extra_auxiliary_info: Any = None):
        grads = [g for _, g in raw_client_grad_list]
        if len(grads) == 0:
            raise ValueError("coordinate_trimmed_mean: no client updates")
        b = self.trim_count(len(grads))
        first = grads[0]
        fkeys = [k for k, v in first.items() if v.dtype in _NATIVE]
        okeys = [k for k in first if k not in set(fkeys)]
        if okeys and base_aggregation_func is None:
            raise TypeError(f"coordinate_trimmed_mean: keys {okeys} are not floating point and no base aggregation "
                            f"function was given for them")
        result = {}
        hit = resident_rows(grads) if fkeys and not okeys else None
        if hit is not None and all(dt in _NATIVE for dt in hit[0].bufs):
            # updates adopted into ONE arena's rows, float groups only: one launch per dtype group over
            # the rows (tiled arenas read tile-interleaved); same bits
            arena, rows = hit
            result.update(arena.trimmed_mean(b, rows))
        elif fkeys:
            dev = next((g[k].device for g in grads for k in fkeys if g[k].is_cuda), None)
            eng = get_engine(dev.index if dev is not None else None)
            groups = OrderedDict()  # dtype -> keys
            for k in fkeys:
                groups.setdefault(first[k].dtype, []).append(k)
            for dt, keys in groups.items():
                segs = []
                for k in keys:
                    col = []
                    for g in grads:
                        t = g[k]
                        if t.dtype != dt or t.shape != first[k].shape:
                            raise ValueError(f"coordinate_trimmed_mean: key {k!r} differs in dtype or shape "
                                             f"between clients")
                        col.append(t.to(eng.device).contiguous().reshape(-1))
                    segs.append(col)
                vec = torch.empty(sum(c[0].numel() for c in segs), dtype=dt, device=eng.device)
                outs, pos = [], 0
                for c in segs:
                    outs.append(vec[pos:pos + c[0].numel()])
                    pos += c[0].numel()
                eng.coord_trimmed_mean(segs, b, outs=outs)
                if dev is None:
                    vec = vec.cpu()  # CPU dicts in, CPU tensors out (the copy waits for the launch)
                pos = 0
                for k in keys:
                    n = first[k].numel()
                    result[k] = vec[pos:pos + n].view(first[k].shape)
                    pos += n
        if okeys:
            base = base_aggregation_func(args=self.config, raw_grad_list=[
                (n, OrderedDict((k, g[k]) for k in okeys)) for n, g in raw_client_grad_list])
            for k in okeys:
                result[k] = base[k].to(first[k].device)
        return OrderedDict((k, result[k]) for k in first)
