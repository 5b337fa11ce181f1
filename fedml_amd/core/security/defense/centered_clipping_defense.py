"""Centered clipping (Karimireddy, He, Jaggi, "Learning from History for Byzantine Robust
Optimization") on the HIP engine: ``defense_type="centered_clipping"``.

The reference tree's own cclip and norm_diff_clipping code is not mirrored here, so this defense is
defined by its contract (include/fedagg_robust.h, fa_centered_sum_sqdist; fedml_amd/cclip.py) under a
name of its own.  It acts on aggregation and is weighted: w_i is client i's share of the samples.
From a center v, each of the ``cclip_iters`` (default 1) iterations moves v by the clipped differences,
v <- v + sum_i w_i min(1, cclip_tau / |x_i - v|) (x_i - v), ``cclip_tau`` (default 10.0) the clipping
radius.  ``cclip_center`` = "global" (default) starts from the server's current model, which
``ServerAggregator.aggregate`` passes as ``extra_auxiliary_info`` -- one iteration is then
norm-difference clipping followed by FedAvg -- and from the sample-weighted mean when no dict is
given; "mean" always starts from the mean.  One iteration is ONE launch per dtype group -- the update
and every client's distance to it from the same read -- plus a copy of 2K doubles to the host; the
distances to the start point cost one more launch.  No iteration returns the start point.

Every floating-point key of client 0's dict takes part, BatchNorm running statistics included, as ONE
vector: the distances are summed over all float keys (per dtype group on the device, across groups on
the host).  The center needs every one of those keys with client 0's dtype and shape (ValueError
otherwise; CPU tensors are moved to the engine's device; its other keys are ignored).  Non-float keys
(a BatchNorm ``num_batches_tracked``) take the base aggregation's value.  A client whose update holds
a NaN or Inf is dropped and reported by ``get_malicious_client_idxs()``.  The result is a new
OrderedDict in client 0's key order on the clients' device (CPU dicts in, CPU tensors out); neither
the inputs nor the center are modified.  ``last_info`` holds the last call's traces.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Any, Callable, List, Tuple

import torch

from ....arena import sum_stats
from ....cclip import cclip_driver
from ._float_keys import _NATIVE, defend_float_keys


class CenteredClippingDefense(object):
    def __init__(self, config):
        self.config = config
        tau = getattr(config, "cclip_tau", 10.0)
        iters = getattr(config, "cclip_iters", 1)
        center = getattr(config, "cclip_center", "global")
        if isinstance(tau, bool) or not isinstance(tau, (int, float)) or not (tau > 0 and math.isfinite(tau)):
            raise ValueError(f"centered_clipping: cclip_tau must be a positive finite number (got {tau!r})")
        if isinstance(iters, bool) or not isinstance(iters, int) or iters < 0:
            raise ValueError(f"centered_clipping: cclip_iters must be an integer >= 0 (got {iters!r})")
        if center not in ("global", "mean"):
            raise ValueError(f"centered_clipping: cclip_center must be 'global' or 'mean' (got {center!r})")
        self.tau = float(tau)
        self.iters = iters
        self.center = center
        self.last_info = None

    def get_malicious_client_idxs(self) -> List[int]:
        return list(self.last_info["dropped"]) if self.last_info else []

    @staticmethod
    def _center_keys(first: OrderedDict, center: dict) -> "OrderedDict[str, torch.Tensor]":
        """The center's tensor of every float key of client 0's dict, checked against it."""
        cen = OrderedDict()
        for key, v in first.items():
            if v.dtype not in _NATIVE:
                continue
            if key not in center:
                raise ValueError(f"centered_clipping: the center lacks key {key!r}")
            c = center[key]
            if not torch.is_tensor(c) or c.dtype != v.dtype or c.shape != v.shape:
                raise ValueError(f"centered_clipping: the center's key {key!r} differs in dtype or shape from the "
                                 f"clients'")
            cen[key] = c
        return cen

    def defend_on_aggregation(self, raw_client_grad_list: List[Tuple[float, OrderedDict]],
                              base_aggregation_func: Callable = None, extra_auxiliary_info: Any = None):
        if len(raw_client_grad_list) == 0:
            raise ValueError("centered_clipping: no client updates")
        counts = [float(n) for n, _ in raw_client_grad_list]
        first_sd = raw_client_grad_list[0][1]
        cen = None
        if self.center == "global" and isinstance(extra_auxiliary_info, dict):
            cen = self._center_keys(first_sd, extra_auxiliary_info)

        def on_arena(arena, rows):  # the passes run over the rows, in place on the packed center
            packed = None
            if cen is not None:
                packed = {dt: torch.zeros(n, dtype=dt, device=arena.device) for dt, n in arena.layout.group_numel.items()}
                for key, c in cen.items():
                    dt, off, _, n = arena.layout.where[key]
                    packed[dt][off:off + n].copy_(c.reshape(-1))
            info = {}
            res = arena.centered_clip(counts, self.tau, self.iters, center=packed, clients=rows, out=packed, info=info)
            self.last_info = info
            return res

        def on_engine(eng, work):
            groups = OrderedDict()  # dtype -> keys, as defend_float_keys groups them
            for key, v in first_sd.items():
                if v.dtype in _NATIVE:
                    groups.setdefault(v.dtype, []).append(key)

            def run(idx, coef, centered):  # v = the group's outs, in place
                stats = []
                for segs, outs in work:
                    sel = [[col[i] for i in idx] for col in segs]
                    stats.append(eng.centered_sum_sqdist(sel, outs, coef, outs=outs)[1] if centered
                                 else eng.weighted_sum_sqdist(sel, coef, outs=outs)[1])
                return sum_stats(stats)

            def first(idx):
                if cen is None:
                    tot = sum(counts[j] for j in idx)
                    return run(idx, [counts[j] / tot for j in idx], False)
                for keys, (_, outs) in zip(groups.values(), work):
                    for key, o in zip(keys, outs):
                        o.copy_(cen[key].reshape(-1))
                return run(idx, None, True)

            self.last_info = cclip_driver(counts, self.iters, self.tau, first,
                                          lambda scales, idx: run(idx, scales, True))

        return defend_float_keys("centered_clipping", self.config, raw_client_grad_list, base_aggregation_func,
                                 on_arena, on_engine)
