"""FedMLDifferentialPrivacy singleton (reference: python/fedml/core/dp/fedml_differential_privacy.py)
on the HIP engine: central DP (``dp_solution_type="cdp"``: the server adds noise to the aggregate,
after clipping the clients' updates around the global model when ``clipping_norm`` is given) and local
DP ("ldp": every client adds noise to its own update).  The per-element work is the engine's
(include/fedagg_dp.h: fa_add_noise, fa_centered_sum_noise); the scales and the clipped weights are
fedml_amd/dp.py's.

Config: ``enable_dp``; ``dp_solution_type`` in {"cdp", "ldp"}; ``mechanism_type`` in {"gaussian",
"laplace"}; ``epsilon``; ``delta`` (Gaussian only); ``sensitivity`` (optional under cdp when
``clipping_norm`` is given: it then defaults per round to clipping_norm * max_i w_i, the most one
client can move the clipped weighted sum); ``clipping_norm`` (optional, cdp only); ``dp_seed`` (64
bits, default ``secrets.randbits(64)``, never logged).  Unknown values raise ValueError at init.

The noise of an element depends on (seed, round, segment id, element index): the segment id is the
position of the key among the dict's floating-point keys, ``round`` counts this singleton's noise
applications from 1, and a local client's seed is dp_seed ^ (client_id * 0x9E3779B97F4A7C15 mod 2^64).
Non-float keys get no noise.  Under clipping every float key takes part as ONE vector, BatchNorm
statistics included, as in centered_clipping.

Limits: float32 noise with truncated tails (5.77 sigma for Gaussian, 15.9 b for Laplace); no privacy
accountant; no protection against floating-point attacks on the noise's low bits (Mironov 2012); in
16-bit storage, noise below half an ulp of the value it is added to vanishes.
"""
from __future__ import annotations

import logging
import math
import secrets
from collections import OrderedDict
from typing import List, Optional, Tuple

import torch

from ... import dp as _dp

DP_CDP, DP_LDP = "cdp", "ldp"
_FLOAT = (torch.float32, torch.bfloat16, torch.float16, torch.float64)


class FedMLDifferentialPrivacy:
    _dp_instance = None

    @staticmethod
    def get_instance():
        if FedMLDifferentialPrivacy._dp_instance is None:
            FedMLDifferentialPrivacy._dp_instance = FedMLDifferentialPrivacy()
        return FedMLDifferentialPrivacy._dp_instance

    def __init__(self):
        self._off()

    def _off(self):
        self.is_enabled = False
        self.dp_solution_type = None
        self.mechanism_type = None
        self.epsilon = self.delta = self.sensitivity = self.clipping_norm = None
        self.dp_seed = None
        self.round = 0

    def init(self, args):
        self._off()
        if not getattr(args, "enable_dp", False):
            return
        kind = getattr(args, "dp_solution_type", None)
        kind = kind.strip() if isinstance(kind, str) else kind
        if kind not in (DP_CDP, DP_LDP):
            raise ValueError(f"dp: dp_solution_type must be 'cdp' or 'ldp' (got {kind!r})")
        mech = getattr(args, "mechanism_type", None)
        mech = mech.strip().lower() if isinstance(mech, str) else mech
        if mech not in _dp.MECHANISMS:
            raise ValueError(f"dp: mechanism_type must be 'gaussian' or 'laplace' (got {mech!r})")
        clip = getattr(args, "clipping_norm", None)
        if clip is not None:
            if kind != DP_CDP:
                raise ValueError("dp: clipping_norm belongs to dp_solution_type 'cdp'")
            clip = _dp._positive("clipping_norm", clip)
        sens = getattr(args, "sensitivity", None)
        if sens is None and clip is None:
            raise ValueError("dp: sensitivity is required (it may be left out only when clipping_norm is given)")
        delta = getattr(args, "delta", None)
        # checks epsilon, delta (Gaussian) and the sensitivity
        _dp.noise_scale(mech, getattr(args, "epsilon", None), delta, 1.0 if sens is None else sens)
        seed = getattr(args, "dp_seed", None)
        if seed is None:
            seed = secrets.randbits(64)
        _dp.check_seed_round(seed, 0)
        self.is_enabled = True
        self.dp_solution_type, self.mechanism_type = kind, mech
        self.epsilon, self.delta = float(args.epsilon), delta
        self.sensitivity = None if sens is None else float(sens)
        self.clipping_norm = clip
        self.dp_seed = seed
        logging.info("------init dp: %s, %s", kind, mech)  # never the seed

    def is_dp_enabled(self):
        return self.is_enabled

    def is_local_dp_enabled(self):
        return self.is_enabled and self.dp_solution_type == DP_LDP

    def is_global_dp_enabled(self):
        return self.is_enabled and self.dp_solution_type == DP_CDP

    def is_clipping_enabled(self):
        return self.is_global_dp_enabled() and self.clipping_norm is not None

    def scale(self, sensitivity: Optional[float] = None) -> float:
        """The noise's scale for the configured sensitivity (or the one given)."""
        s = self.sensitivity if sensitivity is None else sensitivity
        if s is None:
            raise ValueError("dp: no sensitivity configured (clipping_norm only serves the clipped aggregation)")
        return _dp.noise_scale(self.mechanism_type, self.epsilon, self.delta, s)

    def next_round(self) -> int:
        self.round += 1
        if self.round >= 1 << 32:
            raise OverflowError("dp: the round counter left 32 bits")
        return self.round

    def _add_noise(self, sd, seed: int, like=None) -> OrderedDict:
        """A new OrderedDict in sd's key order: every float key plus its noise (one launch per dtype
        group, the key's position among the float keys as its segment id), the others as they are;
        CPU tensors in, CPU tensors out.  ``like`` (a dict, optional): a key it holds with a non-float
        dtype is no float key here either -- the float32 average of the clients' int64 counters."""
        from ..security.defense._float_keys import engine_of
        fkeys = [k for k, v in sd.items() if torch.is_tensor(v) and v.dtype in _FLOAT and not (
            isinstance(like, dict) and torch.is_tensor(like.get(k)) and like[k].dtype not in _FLOAT)]
        rnd = self.next_round()
        result = dict(sd)
        if fkeys:
            _, eng = engine_of([sd], fkeys)
            scale = self.scale()
            groups = OrderedDict()
            for pos, k in enumerate(fkeys):
                groups.setdefault(sd[k].dtype, []).append((pos, k))
            for dt, items in groups.items():
                flat = [sd[k].to(eng.device).contiguous().reshape(-1) for _, k in items]
                outs = eng.add_noise(flat, self.mechanism_type, scale, seed, rnd, [p for p, _ in items])
                for (_, k), o in zip(items, outs):
                    result[k] = o.view(sd[k].shape).to(sd[k].device)
        return OrderedDict((k, result[k]) for k in sd)

    def add_local_noise(self, local_grad, client_id: int = 0) -> OrderedDict:
        """ldp: the client's dict plus noise under its own seed (fedml_amd.dp.client_seed)."""
        if not self.is_local_dp_enabled():
            raise RuntimeError("dp: local DP is not enabled")
        return self._add_noise(local_grad, _dp.client_seed(self.dp_seed, client_id))

    def add_global_noise(self, global_model, like=None) -> OrderedDict:
        """cdp: the aggregate plus noise.  ``like``: the model before aggregation (ServerAggregator
        passes get_model_params()); its non-float keys (a BatchNorm counter, averaged to float32 by the
        aggregation) get no noise and do not count as float keys."""
        if not self.is_global_dp_enabled():
            raise RuntimeError("dp: central DP is not enabled")
        return self._add_noise(global_model, self.dp_seed, like)

    def aggregate_clipped(self, args, raw_client_grad_list: List[Tuple[float, OrderedDict]], center: dict,
                          base_aggregation_func) -> OrderedDict:
        """DP-FedAvg's server step (McMahan et al. 2018), cdp with ``clipping_norm`` C: over every
        float key as one vector, the norms |x_i - g| to the global model g (one distance-only launch
        per dtype group), the weights w_i min(1, C / |x_i - g|) with w_i client i's share of the
        samples, and g + the clipped weighted sum of the x_i - g + the noise in ONE launch per dtype
        group (fa_centered_sum_noise).  Non-float keys take ``base_aggregation_func``'s value.  One
        noise application."""
        from ...arena import sum_stats
        from ..security.defense._float_keys import _NATIVE, center_keys, defend_float_keys
        if not self.is_clipping_enabled():
            raise RuntimeError("dp: clipped aggregation needs dp_solution_type 'cdp' and clipping_norm")
        if len(raw_client_grad_list) == 0:
            raise ValueError("dp: no client updates")
        if not isinstance(center, dict):
            raise ValueError("dp: the clipped aggregation needs the global model as its center")
        counts = [float(n) for n, _ in raw_client_grad_list]
        if not all(c > 0 and math.isfinite(c) for c in counts):
            raise ValueError("dp: every client weight must be positive and finite")
        tot = sum(counts)
        w = [c / tot for c in counts]
        first_sd = raw_client_grad_list[0][1]
        fkeys = [k for k, v in first_sd.items() if v.dtype in _NATIVE]
        cen = center_keys("dp", first_sd, center, fkeys)
        clip, mech, seed = self.clipping_norm, self.mechanism_type, self.dp_seed
        scale = self.scale(self.sensitivity if self.sensitivity is not None else clip * max(w))
        rnd = self.next_round()

        def on_arena(arena, rows):
            packed = {dt: torch.zeros(n, dtype=dt, device=arena.device) for dt, n in arena.layout.group_numel.items()}
            for key, c in cen.items():
                dt, off, _, n = arena.layout.where[key]
                packed[dt][off:off + n].copy_(c.reshape(-1))
            return arena.dp_aggregate(counts, clip, scale, mech, seed, rnd, center=packed, clients=rows, out=packed)

        def on_engine(eng, work):
            groups = OrderedDict()  # dtype -> [(position among the float keys, key)], as defend_float_keys groups them
            for pos, key in enumerate(fkeys):
                groups.setdefault(first_sd[key].dtype, []).append((pos, key))
            for items, (_, outs) in zip(groups.values(), work):
                for (_, key), o in zip(items, outs):
                    o.copy_(cen[key].reshape(-1))
            d2, _ = sum_stats([eng.centered_sum_sqdist(segs, outs, None)[1] for segs, outs in work])
            scales = _dp.clip_scales(w, d2, clip)
            for items, (segs, outs) in zip(groups.values(), work):
                eng.centered_sum_noise(segs, outs, scales, mech, scale, seed, rnd, [p for p, _ in items], outs=outs)

        return defend_float_keys("dp", args, raw_client_grad_list, base_aggregation_func, on_arena, on_engine)
