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
from ....ml.aggregator.microscaled import MXTensor
from ....ml.aggregator.quantized import Q8Tensor, _restore, dequantize_state_dict
from ....ml.aggregator.rotated import RotatedTensor
from ....ml.aggregator.signcompressed import Q1Tensor

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


def q8_cohort_block(name: str, grads):
    """The block size when every floating-point key of every client is a `Q8Tensor` of one block size and
    shape (a block-quantized int8 cohort), None when no client holds a compressed tensor.  Any other
    compressed format, or plain and Q8 float keys mixed, is a TypeError that names what is supported; a
    block or shape that differs is a ValueError (as KrumDefense._q8_block).  Messages start with ``name``."""
    other = next((type(v).__name__ for g in grads for v in g.values()
                  if isinstance(v, (Q1Tensor, MXTensor, RotatedTensor))), None)
    if other is not None:
        raise TypeError(f"{name}: {other} state_dicts are not supported: this defense takes plain tensors or "
                        "block-quantized int8 (Q8Tensor) floating-point keys")
    first = grads[0]
    if not any(isinstance(v, Q8Tensor) for g in grads for v in g.values()):
        return None
    fkeys = [k for k, v in first.items() if v.dtype in _NATIVE]
    for i, g in enumerate(grads):
        for k in fkeys:
            if not isinstance(g[k], Q8Tensor):
                raise TypeError(f"{name}: key {k!r} of client {i} is a plain tensor in a Q8Tensor cohort: plain and "
                                "Q8Tensor floating-point keys are mixed; supported are all plain tensors or every "
                                "floating-point key of every client a Q8Tensor")
        extra = next((k for k, v in g.items() if isinstance(v, Q8Tensor) and k not in set(fkeys)), None)
        if extra is not None:
            raise TypeError(f"{name}: key {extra!r} of client {i} is a Q8Tensor where client 0 has none: supported "
                            "are all plain tensors or every floating-point key of every client a Q8Tensor")
    block = first[fkeys[0]].block
    for i, g in enumerate(grads):
        for k in fkeys:
            if g[k].block != block:
                raise ValueError(f"{name}: key {k!r}: client {i} block {g[k].block} != {block} (one block size per call)")
            if g[k].shape != first[k].shape:
                raise ValueError(f"{name}: key {k!r}: client {i} shape {g[k].shape} != {first[k].shape}")
    return block


def _defend_q8_keys(name: str, grads, block: int, on_q8: Callable) -> dict:
    """The Q8Tensor keys of a block-quantized cohort as ONE float32 group: on_q8(eng, qsegs, ssegs, outs,
    block) runs the defense's passes straight on the quantized tensors -- qsegs[key][client] /
    ssegs[key][client] flat on the engine's device, outs[key] the views of the group's flat float32 vector to
    write, each starting on a 16-byte boundary so that whole slots take vector loads and stores.  Returns
    {key: tensor} in the original shapes and dtypes (one cast, quantized._restore)."""
    first = grads[0]
    keys = [k for k, v in first.items() if isinstance(v, Q8Tensor)]
    dev = next((g[k].q.device for g in grads for k in keys if g[k].q.is_cuda), None)
    eng = get_engine(dev.index if dev is not None else None)
    on = lambda t: (t if t.device == eng.device else t.to(eng.device)).contiguous().reshape(-1)  # noqa: E731
    qsegs = [[on(g[k].q) for g in grads] for k in keys]
    ssegs = [[on(g[k].scale) for g in grads] for k in keys]
    starts, pos = [], 0
    for k in keys:
        starts.append(pos)
        pos += -(-first[k].numel() // 4) * 4
    vec = torch.empty(pos, dtype=torch.float32, device=eng.device)
    on_q8(eng, qsegs, ssegs, [vec[a:a + first[k].numel()] for k, a in zip(keys, starts)], block)
    if dev is None:
        vec = vec.cpu()  # CPU dicts in, CPU tensors out (the copy waits for the launches)
    return {k: _restore(vec[a:a + first[k].numel()], first[k]) for k, a in zip(keys, starts)}


def defend_float_keys(name: str, config, raw_client_grad_list: List[Tuple[float, OrderedDict]],
                      base_aggregation_func: Callable, on_arena: Callable, on_engine: Callable,
                      on_q8: Callable = None, q8_max_k: int = None) -> OrderedDict:
    """Every floating-point key of client 0's dict gets the defense's operator over the (>= 1) clients,
    every other key ``base_aggregation_func``'s value; the result is a new OrderedDict in client 0's
    key order on the clients' device (CPU dicts in, CPU tensors out).

    ``on_arena(arena, rows)`` -> {key: tensor}: the updates are rows of ONE arena, float groups only.
    ``on_engine(eng, work)``: otherwise; work = per dtype group (segs, outs), segs[key][client] flat
    tensors on the engine's device and outs[key] the views of the group's flat output to write.
    ``on_q8(eng, qsegs, ssegs, outs, block)``: the defenses that take block-quantized int8 cohorts
    (`q8_cohort_block`, `_defend_q8_keys`); the result holds plain tensors.  ``q8_max_k``: the largest
    cohort ``on_q8``'s kernels take; a larger block-quantized cohort is dequantized (`dequantize_state_dict`:
    the sum kernel with one client) and takes the plain route, in each key's original dtype.
    Messages start with ``name``."""
    grads = [g for _, g in raw_client_grad_list]
    q8_block = q8_cohort_block(name, grads) if on_q8 is not None else None
    if q8_block is not None and q8_max_k is not None and len(grads) > q8_max_k:
        raw_client_grad_list = [(n, dequantize_state_dict(g)) for n, g in raw_client_grad_list]
        grads, q8_block = [g for _, g in raw_client_grad_list], None
    first = grads[0]
    fkeys = [k for k, v in first.items() if v.dtype in _NATIVE]
    okeys = [k for k in first if k not in set(fkeys)]
    if okeys and base_aggregation_func is None:
        raise TypeError(f"{name}: keys {okeys} are not floating point and no base aggregation "
                        f"function was given for them")
    result = {}
    hit = resident_rows(grads) if fkeys and not okeys and q8_block is None else None
    if q8_block is not None:
        result.update(_defend_q8_keys(name, grads, q8_block, on_q8))
    elif hit is not None and all(dt in _NATIVE for dt in hit[0].bufs):
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
