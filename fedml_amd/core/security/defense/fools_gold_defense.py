"""FoolsGold (Fung, Yoon, Beschastnikh, "Mitigating Sybils in Federated Learning Poisoning", 2018; RAID
2020) on the HIP engine: ``defense_type="fools_gold"``.

The reference ships this defense as ``foolsgold``; its code is not mirrored here, so the defense is
defined by its contract (include/fedagg_robust.h, fa_pairwise_dot; fedml_amd/foolsgold.py) under a name
of its own.  It acts BEFORE aggregation and is the one defense here that looks at a client's behaviour
across rounds: every client's update is added into a running history, the pairwise cosine similarity
of the histories is measured, and clients whose histories point the same way -- sybils pushing one
poisoned direction -- are down-weighted (``foolsgold_weights``).  The history update and all
K (K + 1) / 2 inner products are ONE launch per dtype group, one read of the clients.

Config: ``fools_gold_use_memory`` (bool, default True; False: no history, the similarity is of this
round's updates), ``fools_gold_confidence`` (a positive finite number, default 1.0: the scale of the
logit), ``fools_gold_center`` ("global", default, or "none").  With "global" the updates are taken
around the server's current model, which ``ServerAggregator.on_before_aggregation`` passes as
``extra_auxiliary_info`` (checked key by key: every participating key with client 0's dtype and shape;
ValueError otherwise); without a dict, or with "none", the clients' values are the updates themselves.

The keys that take part are the floating-point weight keys of client 0's dict (``is_weight_param``, as
Krum's vectorisation: BatchNorm statistics stay out).  ``defend_before_aggregation(raw, extra)`` returns
``[(n_i if w_i == 1.0 else n_i * w_i, grad_i) for w_i > 0]`` in client order, the same dict objects: with
no suspicion the list -- and therefore the aggregate -- is bit-identical to the undefended one.  The
weights n_i * w_i are floats; ``FedMLAggOperator.agg`` divides them by their sum and accepts floats in
every branch that weighs clients (FedAvg, FedProx), so no path insists on integer counts.

The memory is flat zero-initialised device tensors per dtype group, created on first use and keyed by
LIST POSITION, as the reference's is: position i of every round must be the same client.  A change of
the number of clients, the participating keys, their dtypes or shapes -- or of the route, arena rows
against plain dicts -- raises ValueError naming ``reset()``, which drops the memory.
``get_malicious_client_idxs()`` returns the positions with w_i == 0 in the last call; ``last_info``
holds ``weights`` and ``max_cs`` (each client's largest similarity after the pardoning).  When every
w_i is 0 the call raises ValueError ("fools_gold: every client was weighted 0"): falling back to FedAvg
would hide an attack.  Neither the inputs nor the center are modified.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Any, List, Optional, Tuple

import torch

from ....arena import resident_rows
from ....foolsgold import foolsgold_weights, largest_similarity
from ..common.utils import is_weight_param
from ._float_keys import _NATIVE, center_keys, dtype_segments, engine_of

_ALIGN = 16  # bytes: every key's history starts 16-byte aligned inside its group's tensor


class FoolsGoldDefense(object):
    def __init__(self, config):
        self.config = config
        memory = getattr(config, "fools_gold_use_memory", True)
        confidence = getattr(config, "fools_gold_confidence", 1.0)
        center = getattr(config, "fools_gold_center", "global")
        if not isinstance(memory, bool):
            raise ValueError(f"fools_gold: fools_gold_use_memory must be a bool (got {memory!r})")
        if isinstance(confidence, bool) or not isinstance(confidence, (int, float)) or \
                not (confidence > 0 and math.isfinite(confidence)):
            raise ValueError(f"fools_gold: fools_gold_confidence must be a positive finite number (got {confidence!r})")
        if not isinstance(center, str) or center not in ("global", "none"):
            raise ValueError(f"fools_gold: fools_gold_center must be 'global' or 'none' (got {center!r})")
        self.use_memory = memory
        self.confidence = float(confidence)
        self.center = center
        self.last_info = None
        self._malicious: List[int] = []
        self.reset()

    def reset(self) -> None:
        """Drops the memory: the next call starts every client's history at zero."""
        self._signature = None
        self._memory = None  # (route, dtype -> [K, elements] history)

    def get_malicious_client_idxs(self) -> List[int]:
        return list(self._malicious)

    @staticmethod
    def _keys(first: OrderedDict) -> List[str]:
        return [k for k, v in first.items() if torch.is_tensor(v) and v.dtype in _NATIVE and is_weight_param(k)]

    def _histories(self, route, sizes: "OrderedDict[torch.dtype, int]", k: int, device):
        """dtype -> the [K, elements] history of the group (None without memory), created zeroed on
        first use; a memory made for another route or layout is a ValueError."""
        if not self.use_memory:
            return None
        if self._memory is None:
            self._memory = (route, OrderedDict((dt, torch.zeros((k, n), dtype=dt, device=device))
                                               for dt, n in sizes.items()))
        r, hists = self._memory
        if r != route or [(dt, tuple(h.shape), h.device) for dt, h in hists.items()] != \
                [(dt, (k, n), device) for dt, n in sizes.items()]:
            raise ValueError("fools_gold: the updates' layout (arena rows or plain dicts, device) differs from the "
                             "one the memory was built for; call reset() to drop the memory")
        return hists

    def _gram(self, grads: List[OrderedDict], keys: List[str], cen: Optional[OrderedDict]) -> torch.Tensor:
        """The K x K Gram matrix of this round's y (the updated histories with memory, else the updates):
        one launch per dtype group, the groups' matrices added."""
        k = len(grads)
        hit = resident_rows(grads) if len(keys) == len(grads[0]) else None
        if hit is not None and all(dt in _NATIVE for dt in hit[0].bufs):
            arena, rows = hit
            packed = None
            if cen is not None:
                packed = {dt: torch.zeros(n, dtype=dt, device=arena.device) for dt, n in arena.layout.group_numel.items()}
                for key, c in cen.items():
                    dt, off, _, n = arena.layout.where[key]
                    packed[dt][off:off + n].copy_(c.reshape(-1))
            hists = self._histories("arena", OrderedDict(arena.layout.group_numel), k, arena.device)
            return arena.pairwise_dot(center=packed, hists=hists, clients=rows)
        _, eng = engine_of(grads, keys)
        groups = dtype_segments("fools_gold", grads, keys, eng)
        offs, sizes = {}, OrderedDict()
        for dt, (ks, segs) in groups.items():
            step = _ALIGN // segs[0][0].element_size()
            pos = 0
            for key, col in zip(ks, segs):
                offs[key] = pos
                pos += -(-col[0].numel() // step) * step
            sizes[dt] = pos
        hists = self._histories("dict", sizes, k, eng.device)
        total = None
        for dt, (ks, segs) in groups.items():
            centers = None if cen is None else [cen[key].to(eng.device).contiguous().reshape(-1) for key in ks]
            hs = None if hists is None else [[hists[dt][i, offs[key]:offs[key] + col[0].numel()] for i in range(k)]
                                             for key, col in zip(ks, segs)]
            g = eng.pairwise_dot(segs, centers, hs)
            total = g if total is None else total + g
        return total

    def defend_before_aggregation(self, raw_client_grad_list: List[Tuple[float, OrderedDict]],
                                  extra_auxiliary_info: Any = None):
        k = len(raw_client_grad_list)
        if k == 0:
            raise ValueError("fools_gold: no client updates")
        grads = [g for _, g in raw_client_grad_list]
        first = grads[0]
        keys = self._keys(first)
        if not keys:
            raise ValueError("fools_gold: the clients' dicts hold no floating-point weight key")
        signature = (k, tuple((key, first[key].dtype, tuple(first[key].shape)) for key in keys))
        if self.use_memory:
            if self._signature is not None and signature != self._signature:
                raise ValueError("fools_gold: the number of clients or the keys, dtypes or shapes of their updates "
                                 "changed since the memory was built (it is keyed by list position); call reset() "
                                 "to drop the memory")
            self._signature = signature
        cen = None
        if self.center == "global" and isinstance(extra_auxiliary_info, dict):
            cen = center_keys("fools_gold", first, extra_auxiliary_info, keys)
        G = self._gram(grads, keys, cen)
        weights, cs = foolsgold_weights(G, self.confidence)
        self._malicious = [i for i, w in enumerate(weights) if w == 0]
        self.last_info = {"weights": weights, "max_cs": largest_similarity(cs)}
        if len(self._malicious) == k:
            raise ValueError("fools_gold: every client was weighted 0")
        return [(n if w == 1.0 else n * w, g) for (n, g), w in zip(raw_client_grad_list, weights) if w > 0]
