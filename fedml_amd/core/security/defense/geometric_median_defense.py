"""Geometric median by the smoothed Weiszfeld iteration (Pillutla, Kakade, Harchaoui, "Robust
Aggregation for Federated Learning") on the HIP engine: ``defense_type="geometric_median"``.

The reference tree's own RFA code is not mirrored here, so this defense is defined by its contract
(include/fedagg_robust.h, fa_weighted_sum_sqdist; fedml_amd/weiszfeld.py) under a name of its own.  It
acts on aggregation and is weighted: alpha_i is client i's sample count.  Pass 0 is the FedAvg mean;
each of the ``geomed_iters`` (default 3, the paper's budget) iterations reweights the clients by
alpha_i / max(geomed_nu, |x_i - z|) and averages again.  One pass is ONE launch per dtype group -- the
weighted sum and every client's distance to it from the same read -- plus a copy of 2K doubles to the
host.  Its breakdown point is 1/2.

Every floating-point key of client 0's dict takes part, BatchNorm running statistics included, as ONE
vector: the distances are summed over all float keys (per dtype group on the device, across groups on
the host).  Non-float keys (a BatchNorm ``num_batches_tracked``) take the base aggregation's value.
A client whose update holds a NaN or Inf is dropped and reported by ``get_malicious_client_idxs()``.
The result is a new OrderedDict in client 0's key order on the clients' device (CPU dicts in, CPU
tensors out); the inputs are not modified.  ``last_info`` holds the last call's traces.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Any, Callable, List, Tuple

import torch

from ....arena import resident_rows, sum_stats
from ....engine import get_engine
from ....weiszfeld import weiszfeld_driver

_NATIVE = (torch.float32, torch.bfloat16, torch.float16, torch.float64)


class GeometricMedianDefense(object):
    def __init__(self, config):
        self.config = config
        iters = getattr(config, "geomed_iters", 3)
        nu = getattr(config, "geomed_nu", 1e-6)
        if isinstance(iters, bool) or not isinstance(iters, int) or iters < 0:
            raise ValueError(f"geometric_median: geomed_iters must be an integer >= 0 (got {iters!r})")
        if isinstance(nu, bool) or not isinstance(nu, (int, float)) or not (nu > 0 and math.isfinite(nu)):
            raise ValueError(f"geometric_median: geomed_nu must be a positive finite number (got {nu!r})")
        self.iters = iters
        self.nu = float(nu)
        self.last_info = None

    def get_malicious_client_idxs(self) -> List[int]:
        return list(self.last_info["dropped"]) if self.last_info else []

    def defend_on_aggregation(self, raw_client_grad_list: List[Tuple[float, OrderedDict]],
                              base_aggregation_func: Callable = None, extra_auxiliary_info: Any = None):
        grads = [g for _, g in raw_client_grad_list]
        if len(grads) == 0:
            raise ValueError("geometric_median: no client updates")
        counts = [float(n) for n, _ in raw_client_grad_list]
        first = grads[0]
        fkeys = [k for k, v in first.items() if v.dtype in _NATIVE]
        okeys = [k for k in first if k not in set(fkeys)]
        if okeys and base_aggregation_func is None:
            raise TypeError(f"geometric_median: keys {okeys} are not floating point and no base aggregation "
                            f"function was given for them")
        result = {}
        hit = resident_rows(grads) if fkeys and not okeys else None
        if hit is not None and all(dt in _NATIVE for dt in hit[0].bufs):
            # updates adopted into ONE arena's rows, float groups only: the passes run over the rows
            arena, rows = hit
            info = {}
            result.update(arena.geometric_median(counts, self.iters, self.nu, rows, info=info))
            self.last_info = info
        elif fkeys:
            dev = next((g[k].device for g in grads for k in fkeys if g[k].is_cuda), None)
            eng = get_engine(dev.index if dev is not None else None)
            groups = OrderedDict()  # dtype -> keys
            for k in fkeys:
                groups.setdefault(first[k].dtype, []).append(k)
            work = []  # per dtype group: (segments [key][client], outs per key, the flat output)
            for dt, keys in groups.items():
                segs = []
                for k in keys:
                    col = []
                    for g in grads:
                        t = g[k]
                        if t.dtype != dt or t.shape != first[k].shape:
                            raise ValueError(f"geometric_median: key {k!r} differs in dtype or shape between clients")
                        col.append(t.to(eng.device).contiguous().reshape(-1))
                    segs.append(col)
                vec = torch.empty(sum(c[0].numel() for c in segs), dtype=dt, device=eng.device)
                outs, pos = [], 0
                for c in segs:
                    outs.append(vec[pos:pos + c[0].numel()])
                    pos += c[0].numel()
                work.append((segs, outs, vec))

            def step(coef, idx):
                return sum_stats([eng.weighted_sum_sqdist([[col[i] for i in idx] for col in segs], coef, outs=outs)[1]
                                  for segs, outs, _ in work])

            self.last_info = weiszfeld_driver(counts, self.iters, self.nu, step)
            for (dt, keys), (_, _, vec) in zip(groups.items(), work):
                if dev is None:
                    vec = vec.cpu()  # CPU dicts in, CPU tensors out (the copy waits for the launches)
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
