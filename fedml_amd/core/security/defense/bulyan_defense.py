"""Bulyan (El Mhamdi, Guerraoui, Rouault 2018, "The Hidden Vulnerability of Distributed Learning in
Byzantium") on the HIP engine: ``defense_type="bulyan"``, on aggregation.

With K clients and f = ``byzantine_client_num`` (the Krum defense's config name), K >= 4f + 3:

1. the K x K squared distances of the clients' weight vectors in ONE device pass
   (``KrumDefense.pairwise_sq_distances``: weight parameters only, BatchNorm statistics skipped, as
   Krum), then Krum repeated on the host over those K^2 numbers until theta = K - 2f clients are
   chosen (fedml_amd/bulyan.py, ``bulyan_select``; the distances are taken as returned);
2. for every floating-point key -- BatchNorm running statistics included -- and every coordinate, the
   mean of the beta = theta - 2f = K - 4f values nearest to the median over the chosen clients, in
   that key's dtype, one launch per dtype group that reads only the chosen clients, in place
   (contract, bit for bit: include/fedagg_robust.h, fa_coord_mean_around_median).

The contract is the paper's as written in fedagg_robust.h; it is not pinned to a reference fixture.
Sample counts play no part in the float keys.  Non-float keys (a BatchNorm ``num_batches_tracked``)
take the base aggregation's value over the chosen clients.  The result is a new OrderedDict in client
0's key order on the clients' device; the inputs are not modified.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Any, Callable, List, Tuple

from ....bulyan import bulyan_select
from ._float_keys import defend_float_keys
from .krum_defense import KrumDefense


class BulyanDefense(object):
    def __init__(self, config):
        self.config = config
        self.byzantine_client_num = int(config.byzantine_client_num)
        self.selected: List[int] = []   # the last aggregation's chosen clients, in selection order
        self.malicious: List[int] = []  # and the 2f it left out

    def check(self, k: int) -> int:
        f = self.byzantine_client_num
        if f < 0 or k < 4 * f + 3:
            raise ValueError(f"bulyan: needs byzantine_client_num >= 0 and at least 4 * byzantine_client_num + 3 "
                             f"clients (byzantine_client_num {f}, clients {k})")
        return f

    def defend_on_aggregation(self, raw_client_grad_list: List[Tuple[float, OrderedDict]],
                              base_aggregation_func: Callable = None, extra_auxiliary_info: Any = None):
        k = len(raw_client_grad_list)
        f = self.check(k)
        if f == 0:
            sel = list(range(k))  # everyone is chosen: no distance is needed
        else:
            D = KrumDefense(self.config).pairwise_sq_distances([g for _, g in raw_client_grad_list])
            sel = bulyan_select(D.tolist(), f)
        self.selected = sel
        self.malicious = sorted(set(range(k)) - set(sel))
        keep = k - 4 * f
        return defend_float_keys(
            "bulyan", self.config, [raw_client_grad_list[i] for i in sorted(sel)], base_aggregation_func,
            lambda arena, rows: arena.mean_around_median(keep, rows),
            lambda eng, work: [eng.coord_mean_around_median(segs, keep, outs=outs) for segs, outs in work])

    def get_malicious_client_idxs(self):
        return list(self.malicious)
