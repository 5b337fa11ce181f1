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

from ._float_keys import defend_float_keys


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
        if len(raw_client_grad_list) == 0:
            raise ValueError("coordinate_trimmed_mean: no client updates")
        b = self.trim_count(len(raw_client_grad_list))
        # one launch per dtype group, over the arena's rows (tiled arenas read tile-interleaved) or the
        # clients' tensors; same bits
        return defend_float_keys(
            "coordinate_trimmed_mean", self.config, raw_client_grad_list, base_aggregation_func,
            lambda arena, rows: arena.trimmed_mean(b, rows),
            lambda eng, work: [eng.coord_trimmed_mean(segs, b, outs=outs) for segs, outs in work])
