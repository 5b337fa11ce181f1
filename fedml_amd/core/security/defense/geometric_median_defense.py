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

from ....arena import sum_stats
from ....weiszfeld import weiszfeld_driver
from ._float_keys import defend_float_keys


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
        if len(raw_client_grad_list) == 0:
            raise ValueError("geometric_median: no client updates")
        counts = [float(n) for n, _ in raw_client_grad_list]

        def on_arena(arena, rows):  # the passes run over the rows
            info = {}
            res = arena.geometric_median(counts, self.iters, self.nu, rows, info=info)
            self.last_info = info
            return res

        def on_engine(eng, work):
            def step(coef, idx):
                return sum_stats([eng.weighted_sum_sqdist([[col[i] for i in idx] for col in segs], coef, outs=outs)[1]
                                  for segs, outs in work])

            self.last_info = weiszfeld_driver(counts, self.iters, self.nu, step)

        return defend_float_keys("geometric_median", self.config, raw_client_grad_list, base_aggregation_func,
                                 on_arena, on_engine)
