"""Robust learning rate (Ozdayi, Kantarcioglu, Gel, "Defending against Backdoors in Federated Learning
with Robust Learning Rate", AAAI 2021) on the HIP engine: ``defense_type="robust_lr"``.

The reference tree lists this defense as ``robust_learning_rate``; its code is not mirrored here, so
the defense is defined by its contract (include/fedagg_robust.h, fa_sign_vote_sum) under a name of its
own.  It acts on aggregation.  Per coordinate the clients' updates vote with their signs, one vote per
client (unweighted, as in the paper); where the net vote |sum_i sign(u_i)| is below
``robust_lr_threshold`` (required: an integer >= 0, at most the number of clients) the server's
learning rate ``robust_lr_server_lr`` (default 1.0) is negated for that coordinate, so a backdoor a few
colluding clients push is moved away from, not towards.  ``robust_lr_center`` = "global" (default)
takes the updates around the server's current model g, which ``ServerAggregator.aggregate`` passes as
``extra_auxiliary_info``: the result is g + eta (.) sum_i w_i (x_i - g), w_i client i's share of the
samples, eta = +-server_lr per coordinate.  Without a dict, or with "none", the clients' values are the
updates themselves and the result is +-eta sum_i w_i x_i.  The vote, the sum and the flip are ONE
launch per dtype group, one read of the clients.

Every floating-point key of client 0's dict takes part, BatchNorm running statistics included.  The
center needs every one of those keys with client 0's dtype and shape (ValueError otherwise; CPU
tensors are moved to the engine's device; its other keys are ignored).  Non-float keys (a BatchNorm
``num_batches_tracked``) take the base aggregation's value.  Non-finite values propagate as the
contract says (a NaN votes 0 and gives NaN there); no client is dropped, so
``get_malicious_client_idxs()`` is empty.  The result is a new OrderedDict in client 0's key order on
the clients' device (CPU dicts in, CPU tensors out); neither the inputs nor the center are modified.
``last_info`` holds the last call's ``flipped`` (the number of negated coordinates) and ``elements``.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Any, Callable, List, Tuple

import torch

from ....arena import sign_vote_coef
from ._float_keys import _NATIVE, center_keys, defend_float_keys


class RobustLearningRateDefense(object):
    def __init__(self, config):
        self.config = config
        if not hasattr(config, "robust_lr_threshold"):
            raise ValueError("robust_lr: robust_lr_threshold is required (an integer >= 0)")
        threshold = config.robust_lr_threshold
        lr = getattr(config, "robust_lr_server_lr", 1.0)
        center = getattr(config, "robust_lr_center", "global")
        if isinstance(threshold, bool) or not isinstance(threshold, int) or threshold < 0:
            raise ValueError(f"robust_lr: robust_lr_threshold must be an integer >= 0 (got {threshold!r})")
        if isinstance(lr, bool) or not isinstance(lr, (int, float)) or not (lr > 0 and math.isfinite(lr)):
            raise ValueError(f"robust_lr: robust_lr_server_lr must be a positive finite number (got {lr!r})")
        if not isinstance(center, str) or center not in ("global", "none"):
            raise ValueError(f"robust_lr: robust_lr_center must be 'global' or 'none' (got {center!r})")
        self.threshold = threshold
        self.server_lr = float(lr)
        self.center = center
        self.last_info = None

    def get_malicious_client_idxs(self) -> List[int]:
        return []

    @staticmethod
    def _center_keys(first: OrderedDict, center: dict) -> "OrderedDict[str, torch.Tensor]":
        """The center's tensor of every float key of client 0's dict, checked against it."""
        return center_keys("robust_lr", first, center, [key for key, v in first.items() if v.dtype in _NATIVE])

    def defend_on_aggregation(self, raw_client_grad_list: List[Tuple[float, OrderedDict]],
                              base_aggregation_func: Callable = None, extra_auxiliary_info: Any = None):
        k = len(raw_client_grad_list)
        if k == 0:
            raise ValueError("robust_lr: no client updates")
        if self.threshold > k:
            raise ValueError(f"robust_lr: robust_lr_threshold {self.threshold} exceeds the number of clients ({k})")
        coef = sign_vote_coef([n for n, _ in raw_client_grad_list], self.server_lr)
        first_sd = raw_client_grad_list[0][1]
        cen = None
        if self.center == "global" and isinstance(extra_auxiliary_info, dict):
            cen = self._center_keys(first_sd, extra_auxiliary_info)
        info = {"flipped": 0, "elements": 0}

        def on_arena(arena, rows):  # in place on the packed copy of the center
            packed = None
            if cen is not None:
                packed = {dt: torch.zeros(n, dtype=dt, device=arena.device) for dt, n in arena.layout.group_numel.items()}
                for key, c in cen.items():
                    dt, off, _, n = arena.layout.where[key]
                    packed[dt][off:off + n].copy_(c.reshape(-1))
            return arena.sign_vote_sum([n for n, _ in raw_client_grad_list], self.threshold, self.server_lr,
                                       center=packed, clients=rows, out=packed, info=info)

        def on_engine(eng, work):
            groups = OrderedDict()  # dtype -> keys, as defend_float_keys groups them
            for key, v in first_sd.items():
                if v.dtype in _NATIVE:
                    groups.setdefault(v.dtype, []).append(key)
            flips = []
            for keys, (segs, outs) in zip(groups.values(), work):
                if cen is not None:  # the group's outs start as the center and are updated in place
                    for key, o in zip(keys, outs):
                        o.copy_(cen[key].reshape(-1))
                flips.append(eng.sign_vote_sum(segs, outs if cen is not None else None, coef, self.threshold,
                                               outs=outs)[1])
                info["elements"] += sum(o.numel() for o in outs)
            info["flipped"] = sum(int(f.item()) for f in flips)

        out = defend_float_keys("robust_lr", self.config, raw_client_grad_list, base_aggregation_func,
                                on_arena, on_engine)
        self.last_info = info
        return out
