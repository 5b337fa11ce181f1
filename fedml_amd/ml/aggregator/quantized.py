"""Block-quantized int8 ("q8") state_dicts: a compressed client upload aggregated without a float32
round trip through device memory.

The format is include/fedagg_quant.h's: per tensor, int8 values ``q`` and one float32 ``scale`` per
block of ``block`` elements, element e worth ``q[e] * scale[e // block]``.  `quantize_state_dict`
produces it on the device (fa_quantize_q8), `aggregate_q8` sums K clients' dicts in ONE launch of the
fused dequantize-and-sum kernel (fa_weighted_sum_q8: 1 + 4/block bytes read per client element instead
of 4), `dequantize_state_dict` is that kernel with one client.  All arithmetic is the HIP kernels';
nothing here computes on the CPU.

A quantized dict maps every float32 / bfloat16 / float16 key to a `Q8Tensor` and keeps every other key
(the int64 BatchNorm counters) as a plain tensor; those go through the ordinary `aggregate`.  The sum
is float32; a key whose original dtype is a 16-bit type is cast to it once, at the end.
`FedMLAggOperator.agg` routes FedAvg / FedProx and FedAvg_seq / FedDyn here when the dicts hold
`Q8Tensor` values.
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from ...engine import MUL_W, SUM, AggEngine, get_engine
from .state_dict_agg import _to_engine, aggregate

Q8_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


@dataclass
class Q8Tensor:
    """One tensor in the q8 format: ``q`` int8 (``shape``), ``scale`` float32 (one per block of
    ``block`` elements of the flattened tensor), ``dtype`` the original tensor's dtype."""
    q: torch.Tensor
    scale: torch.Tensor
    block: int
    shape: Tuple[int, ...]
    dtype: torch.dtype

    def __post_init__(self):
        self.shape = tuple(self.shape)
        self.block = int(self.block)
        if self.q.dtype != torch.int8 or self.scale.dtype != torch.float32:
            raise TypeError(f"Q8Tensor: q must be int8 and scale float32 (got {self.q.dtype}, {self.scale.dtype})")
        if self.dtype not in Q8_DTYPES:
            raise TypeError(f"Q8Tensor: original dtype {self.dtype} is not float32, bfloat16 or float16")
        n = 1
        for d in self.shape:
            n *= d
        if self.q.numel() != n or self.scale.numel() != -(-n // self.block):
            raise ValueError(f"Q8Tensor: shape {self.shape} in blocks of {self.block} needs {n} values and "
                             f"{-(-n // self.block)} scales (got {self.q.numel()}, {self.scale.numel()})")

    def numel(self) -> int:
        return self.q.numel()


def _engine_of(tensors, engine: Optional[AggEngine]) -> AggEngine:
    if engine is not None:
        return engine
    for t in tensors:
        if t.is_cuda:
            return get_engine(t.device.index)
    return get_engine(None)


def _restore(out: torch.Tensor, t: Q8Tensor) -> torch.Tensor:
    """A float32 result in the key's original shape and, for a 16-bit key, dtype (one cast)."""
    out = out.view(t.shape)
    return out if t.dtype == torch.float32 else out.to(t.dtype)


def quantize_state_dict(sd: Dict[str, torch.Tensor], block: int = 128,
                        engine: Optional[AggEngine] = None) -> "OrderedDict[str, object]":
    """Every float32 / bfloat16 / float16 key as a `Q8Tensor` (one fa_quantize_q8 launch per dtype),
    every other key unchanged; key order kept.  Tensors not on the engine's device are moved there."""
    fkeys = [k for k, v in sd.items() if v.dtype in Q8_DTYPES]
    eng = _engine_of([sd[k] for k in fkeys], engine) if fkeys else None
    groups: Dict[torch.dtype, List[str]] = {}
    for k in fkeys:
        groups.setdefault(sd[k].dtype, []).append(k)
    done: Dict[str, Q8Tensor] = {}
    for dt, ks in groups.items():
        xs = [_to_engine(sd[k], eng) for k in ks]
        qs, scales = eng.quantize_q8(xs, block)
        for k, x, q, sc in zip(ks, xs, qs, scales):
            done[k] = Q8Tensor(q, sc, block, tuple(sd[k].shape), dt)
    return OrderedDict((k, done.get(k, v)) for k, v in sd.items())


def dequantize_state_dict(sd: Dict[str, object], engine: Optional[AggEngine] = None) -> "OrderedDict[str, torch.Tensor]":
    """The inverse: every `Q8Tensor` key as a tensor of its original shape and dtype (the sum kernel
    with one client, one launch per block size), every other key unchanged."""
    qkeys = [k for k, v in sd.items() if isinstance(v, Q8Tensor)]
    eng = _engine_of([sd[k].q for k in qkeys], engine) if qkeys else None
    groups: Dict[int, List[str]] = {}
    for k in qkeys:
        groups.setdefault(sd[k].block, []).append(k)
    done: Dict[str, torch.Tensor] = {}
    for block, ks in groups.items():
        outs = eng.weighted_sum_q8([[sd[k].q] for k in ks], [[sd[k].scale] for k in ks], SUM, None, block)
        for k, o in zip(ks, outs):
            done[k] = _restore(o, sd[k])
    return OrderedDict((k, done.get(k, v)) for k, v in sd.items())


def aggregate_q8(dicts: Sequence[Dict[str, object]], mode: int, coef: Optional[Sequence[float]] = None,
                 engine: Optional[AggEngine] = None) -> "OrderedDict[str, torch.Tensor]":
    """Ordered per-key reduction over quantized client state_dicts: every `Q8Tensor` key in ONE
    fa_weighted_sum_q8 launch, the plain keys through `aggregate`; client 0's key order, the original
    shapes, float32 results cast once to a 16-bit key's original dtype.  ``mode``: MUL_W or SUM.

    Clients that disagree on which keys are quantized raise TypeError; clients (or keys, for the block)
    that disagree on block, shape or original dtype raise ValueError."""
    if len(dicts) == 0:
        raise IndexError("list index out of range")  # as aggregate: the reference indexes raw_grad_list[0]
    if mode not in (MUL_W, SUM):
        raise ValueError(f"aggregate_q8: mode {mode} not supported (MUL_W, SUM)")
    first = dicts[0]
    keys = list(first.keys())
    qkeys = [k for k in keys if isinstance(first[k], Q8Tensor)]
    qset = set(qkeys)
    for i, d in enumerate(dicts):
        for k in keys:
            v = d[k]  # KeyError on a missing key, like aggregate
            if isinstance(v, Q8Tensor) != (k in qset):
                raise TypeError(f"key {k!r}: client {i} {'has' if isinstance(v, Q8Tensor) else 'lacks'} a Q8Tensor "
                                f"where client 0 {'has' if k in qset else 'lacks'} one")
    out: Dict[str, torch.Tensor] = {}
    if qkeys:
        block = first[qkeys[0]].block
        for k in qkeys:
            t0 = first[k]
            if t0.block != block:
                raise ValueError(f"key {k!r}: block {t0.block} != {block} (one block size per call)")
            for i, d in enumerate(dicts):
                t = d[k]
                if t.block != block:
                    raise ValueError(f"key {k!r}: client {i} block {t.block} != {block}")
                if t.shape != t0.shape:
                    raise ValueError(f"key {k!r}: client {i} shape {t.shape} != {t0.shape}")
                if t.dtype != t0.dtype:
                    raise ValueError(f"key {k!r}: client {i} original dtype {t.dtype} != {t0.dtype}")
        eng = _engine_of([first[k].q for k in qkeys], engine)
        sums = eng.weighted_sum_q8([[_to_engine(d[k].q, eng) for d in dicts] for k in qkeys],
                                   [[_to_engine(d[k].scale, eng) for d in dicts] for k in qkeys], mode, coef, block)
        for k, o in zip(qkeys, sums):
            out[k] = _restore(o, first[k])
    plain = [k for k in keys if k not in qset]
    if plain:
        out.update(aggregate([OrderedDict((k, d[k]) for k in plain) for d in dicts], mode, coef, engine=engine))
    return OrderedDict((k, out[k]) for k in keys)
