"""The scaffold shared by the defenses that run one engine operator over every floating-point key of
the clients' dicts (coordinate_trimmed_mean_defense.py, geometric_median_defense.py, centered_clipping_defense.py, bulyan_defense.py, robust_lr_defense.py; fools_gold_defense.py takes the engine and the per-dtype segments): which keys take
part, the resident-arena form, the per-dtype segments of the engine form, and the way back to a dict.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Callable, List, Tuple

import torch

from ....arena import resident_rows
from ....engine import get_engine

_NATIVE = (torch.float32, torch.bfloat16, torch.float16, torch.float64)


def engine_of(grads, keys):
    """(device, engine): the device of the first CUDA tensor among the clients' ``keys`` (None: CPU
    dicts) and that device's engine (the default device's for CPU dicts)."""
    dev = next((g[k].device for g in grads for k in keys if g[k].is_cuda), None)
    return dev, get_engine(dev.index if dev is not None else None)


def center_keys(name: str, first, center: dict, keys) -> "OrderedDict":
    """The center's tensor of every one of ``keys``, checked key by key against client 0's dict
    ``first`` (present, a tensor, the same dtype and shape); ValueErrors start with ``name``."""
    cen = OrderedDict()
    for key in keys:
        if key not in center:
            raise ValueError(f"{name}: the center lacks key {key!r}")
        c = center[key]
        if not torch.is_tensor(c) or c.dtype != first[key].dtype or c.shape != first[key].shape:
            raise ValueError(f"{name}: the center's key {key!r} differs in dtype or shape from the clients'")
        cen[key] = c
    return cen


def dtype_segments(name: str, grads, keys, eng) -> "OrderedDict":
    """dtype -> (keys, segs) over ``keys`` in the order of their first appearance: segs[key][client] the
    clients' flat contiguous tensors on the engine's device.  A key whose dtype or shape differs between
    clients is a ValueError that starts with ``name``."""
    first = grads[0]
    by_dt = OrderedDict()
    for k in keys:
        by_dt.setdefault(first[k].dtype, []).append(k)
    groups = OrderedDict()
    for dt, ks in by_dt.items():
        segs = []
        for k in ks:
            col = []
            for g in grads:
                t = g[k]
                if t.dtype != dt or t.shape != first[k].shape:
                    raise ValueError(f"{name}: key {k!r} differs in dtype or shape between clients")
                col.append(t.to(eng.device).contiguous().reshape(-1))
            segs.append(col)
        groups[dt] = (ks, segs)
    return groups


def defend_float_keys(name: str, config, raw_client_grad_list: List[Tuple[float, OrderedDict]],
                      base_aggregation_func: Callable, on_arena: Callable, on_engine: Callable) -> OrderedDict:
    """Every floating-point key of client 0's dict gets the defense's operator over the (>= 1) clients,
    every other key ``base_aggregation_func``'s value; the result is a new OrderedDict in client 0's
    key order on the clients' device (CPU dicts in, CPU tensors out).

    ``on_arena(arena, rows)`` -> {key: tensor}: the updates are rows of ONE arena, float groups only.
    ``on_engine(eng, work)``: otherwise; work = per dtype group (segs, outs), segs[key][client] flat
    tensors on the engine's device and outs[key] the views of the group's flat output to write.
    Messages start with ``name``."""
    grads = [g for _, g in raw_client_grad_list]
    first = grads[0]
    fkeys = [k for k, v in first.items() if v.dtype in _NATIVE]
    okeys = [k for k in first if k not in set(fkeys)]
    if okeys and base_aggregation_func is None:
        raise TypeError(f"{name}: keys {okeys} are not floating point and no base aggregation "
                        f"function was given for them")
    result = {}
    hit = resident_rows(grads) if fkeys and not okeys else None
    if hit is not None and all(dt in _NATIVE for dt in hit[0].bufs):
        result.update(on_arena(*hit))
    elif fkeys:
        dev, eng = engine_of(grads, fkeys)
        groups = dtype_segments(name, grads, fkeys, eng)  # dtype -> (keys, segs)
        work, vecs = [], []
        for dt, (keys, segs) in groups.items():
            vec = torch.empty(sum(c[0].numel() for c in segs), dtype=dt, device=eng.device)
            outs, pos = [], 0
            for c in segs:
                outs.append(vec[pos:pos + c[0].numel()])
                pos += c[0].numel()
            work.append((segs, outs))
            vecs.append(vec)
        on_engine(eng, work)
        for (keys, _), vec in zip(groups.values(), vecs):
            if dev is None:
                vec = vec.cpu()  # CPU dicts in, CPU tensors out (the copy waits for the launches)
            pos = 0
            for k in keys:
                n = first[k].numel()
                result[k] = vec[pos:pos + n].view(first[k].shape)
                pos += n
    if okeys:
        base = base_aggregation_func(args=config, raw_grad_list=[
            (n, OrderedDict((k, g[k]) for k in okeys)) for n, g in raw_client_grad_list])
        for k in okeys:
            result[k] = base[k].to(first[k].device)
    return OrderedDict((k, result[k]) for k in first)
