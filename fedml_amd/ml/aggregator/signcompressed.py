"""1-bit sign-compressed ("q1") state_dicts: one sign bit per element and one float32 magnitude per
block, aggregated without a float32 round trip through device memory.

The format is include/fedagg_sign.h's: per tensor, ``bits`` (32 elements per int32 word, 1 = negative)
and one float32 ``scale`` per block of ``block`` elements, element e worth ``-scale[e // block]`` where
its bit is set and ``+scale[e // block]`` where not.  `sign_compress_state_dict` produces it on the
device (fa_quantize_q1: the scale is the block's mean magnitude, the scaled sign of EF-signSGD),
`aggregate_q1` sums K clients' dicts in ONE launch of the fused decompress-and-sum kernel
(fa_weighted_sum_q1: 1/8 + 4/block bytes read per client element instead of 4), `decompress_state_dict`
is that kernel with one client, and `majority_vote_q1` is signSGD with majority vote
(fa_sign_vote_q1: the bits alone are read).  All arithmetic is the HIP kernels'; nothing here computes
on the CPU.  Error feedback and stochastic signs are the client's business.

The key rules are quantized.py's: every float32 / bfloat16 / float16 key becomes a `Q1Tensor`, every
other key (the int64 BatchNorm counters) stays plain and goes through the ordinary `aggregate`; results
are float32, cast once to a 16-bit key's original dtype.  `FedMLAggOperator.agg` routes here when the
dicts hold `Q1Tensor` values.
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from ...engine import MUL_W, SUM, AggEngine
from .quantized import Q8_DTYPES as Q1_DTYPES
from .quantized import _engine_of, _restore
from .state_dict_agg import _to_engine, aggregate


@dataclass
class Q1Tensor:
    """One tensor in the q1 format: ``bits`` int32 (ceil(numel / 32) words), ``scale`` float32 (one per
    block of ``block`` elements of the flattened tensor), ``shape`` and ``dtype`` the original tensor's."""
    bits: torch.Tensor
    scale: torch.Tensor
    block: int
    shape: Tuple[int, ...]
    dtype: torch.dtype

    def __post_init__(self):
        self.shape = tuple(self.shape)
        self.block = int(self.block)
        if self.bits.dtype != torch.int32 or self.scale.dtype != torch.float32:
            raise TypeError(f"Q1Tensor: bits must be int32 and scale float32 (got {self.bits.dtype}, "
                            f"{self.scale.dtype})")
        if self.dtype not in Q1_DTYPES:
            raise TypeError(f"Q1Tensor: original dtype {self.dtype} is not float32, bfloat16 or float16")
        n = self.numel()
        if self.bits.numel() != -(-n // 32) or self.scale.numel() != -(-n // self.block):
            raise ValueError(f"Q1Tensor: shape {self.shape} in blocks of {self.block} needs {-(-n // 32)} words and "
                             f"{-(-n // self.block)} scales (got {self.bits.numel()}, {self.scale.numel()})")

    def numel(self) -> int:
        n = 1
        for d in self.shape:
            n *= d
        return n


def sign_compress_state_dict(sd: Dict[str, torch.Tensor], block: int = 128,
                             engine: Optional[AggEngine] = None) -> "OrderedDict[str, object]":
    """Every float32 / bfloat16 / float16 key as a `Q1Tensor` (one fa_quantize_q1 launch per dtype),
    every other key unchanged; key order kept.  Tensors not on the engine's device are moved there."""
    fkeys = [k for k, v in sd.items() if v.dtype in Q1_DTYPES]
    eng = _engine_of([sd[k] for k in fkeys], engine) if fkeys else None
    groups: Dict[torch.dtype, List[str]] = {}
    for k in fkeys:
        groups.setdefault(sd[k].dtype, []).append(k)
    done: Dict[str, Q1Tensor] = {}
    for dt, ks in groups.items():
        bits, scales = eng.quantize_q1([_to_engine(sd[k], eng).contiguous() for k in ks], block)
        for k, b, sc in zip(ks, bits, scales):
            done[k] = Q1Tensor(b, sc, block, tuple(sd[k].shape), dt)
    return OrderedDict((k, done.get(k, v)) for k, v in sd.items())


def decompress_state_dict(sd: Dict[str, object], engine: Optional[AggEngine] = None) -> "OrderedDict[str, torch.Tensor]":
    """The inverse: every `Q1Tensor` key as a tensor of its original shape and dtype (the sum kernel
    with one client, one launch per block size), every other key unchanged."""
    qkeys = [k for k, v in sd.items() if isinstance(v, Q1Tensor)]
    eng = _engine_of([sd[k].bits for k in qkeys], engine) if qkeys else None
    groups: Dict[int, List[str]] = {}
    for k in qkeys:
        groups.setdefault(sd[k].block, []).append(k)
    done: Dict[str, torch.Tensor] = {}
    for block, ks in groups.items():
        outs = eng.weighted_sum_q1([[sd[k].bits] for k in ks], [[sd[k].scale] for k in ks],
                                   [sd[k].numel() for k in ks], SUM, None, block)
        for k, o in zip(ks, outs):
            done[k] = _restore(o, sd[k])
    return OrderedDict((k, done.get(k, v)) for k, v in sd.items())


def _checked_keys(what: str, dicts) -> Tuple[List[str], List[str]]:
    """(all keys, the Q1Tensor keys) of client 0, after checking that every client agrees on which keys
    are compressed (TypeError) and, per compressed key, on shape and original dtype (ValueError)."""
    if len(dicts) == 0:
        raise IndexError("list index out of range")  # as aggregate: the reference indexes raw_grad_list[0]
    first = dicts[0]
    keys = list(first.keys())
    qset = {k for k in keys if isinstance(first[k], Q1Tensor)}
    for i, d in enumerate(dicts):
        for k in keys:
            v = d[k]  # KeyError on a missing key, like aggregate
            if isinstance(v, Q1Tensor) != (k in qset):
                raise TypeError(f"{what}: key {k!r}: client {i} {'has' if isinstance(v, Q1Tensor) else 'lacks'} a "
                                f"Q1Tensor where client 0 {'has' if k in qset else 'lacks'} one")
            if k in qset and v.shape != first[k].shape:
                raise ValueError(f"{what}: key {k!r}: client {i} shape {v.shape} != {first[k].shape}")
            if k in qset and v.dtype != first[k].dtype:
                raise ValueError(f"{what}: key {k!r}: client {i} original dtype {v.dtype} != {first[k].dtype}")
    return keys, [k for k in keys if k in qset]


def aggregate_q1(dicts: Sequence[Dict[str, object]], mode: int, coef: Optional[Sequence[float]] = None,
                 engine: Optional[AggEngine] = None) -> "OrderedDict[str, torch.Tensor]":
    """Ordered per-key reduction over sign-compressed client state_dicts: every `Q1Tensor` key in ONE
    fa_weighted_sum_q1 launch, the plain keys through `aggregate`; client 0's key order, the original
    shapes, float32 results cast once to a 16-bit key's original dtype.  ``mode``: MUL_W or SUM.

    Clients that disagree on which keys are compressed raise TypeError; clients (or keys, for the block)
    that disagree on block, shape or original dtype raise ValueError."""
    if mode not in (MUL_W, SUM) and len(dicts):
        raise ValueError(f"aggregate_q1: mode {mode} not supported (MUL_W, SUM)")
    keys, qkeys = _checked_keys("aggregate_q1", dicts)
    first = dicts[0]
    out: Dict[str, torch.Tensor] = {}
    if qkeys:
        block = first[qkeys[0]].block
        for k in qkeys:
            for i, d in enumerate(dicts):
                if d[k].block != block:
                    raise ValueError(f"key {k!r}: client {i} block {d[k].block} != {block} (one block size per call)")
        eng = _engine_of([first[k].bits for k in qkeys], engine)
        sums = eng.weighted_sum_q1([[_to_engine(d[k].bits, eng) for d in dicts] for k in qkeys],
                                   [[_to_engine(d[k].scale, eng) for d in dicts] for k in qkeys],
                                   [first[k].numel() for k in qkeys], mode, coef, block)
        for k, o in zip(qkeys, sums):
            out[k] = _restore(o, first[k])
    plain = [k for k in keys if k not in out]
    if plain:
        out.update(aggregate([OrderedDict((k, d[k]) for k in plain) for d in dicts], mode, coef, engine=engine))
    return OrderedDict((k, out[k]) for k in keys)


def majority_vote_q1(dicts: Sequence[Dict[str, object]], threshold: int = 1, step: float = 1.0,
                     engine: Optional[AggEngine] = None) -> "OrderedDict[str, torch.Tensor]":
    """signSGD with majority vote over sign-compressed client state_dicts: every `Q1Tensor` key in ONE
    fa_sign_vote_q1 launch (the scales and blocks play no part): +step where at least ``threshold`` more
    clients are positive than negative, -step for the converse, 0 otherwise; every client has one vote.
    The plain keys take the ordinary plain sum (`aggregate`, SUM).  Same key rules and errors as
    `aggregate_q1`, the block apart."""
    keys, qkeys = _checked_keys("majority_vote_q1", dicts)
    first = dicts[0]
    out: Dict[str, torch.Tensor] = {}
    if qkeys:
        eng = _engine_of([first[k].bits for k in qkeys], engine)
        votes = eng.sign_vote_q1([[_to_engine(d[k].bits, eng) for d in dicts] for k in qkeys],
                                 [first[k].numel() for k in qkeys], threshold, step)
        for k, o in zip(qkeys, votes):
            out[k] = _restore(o, first[k])
    plain = [k for k in keys if k not in out]
    if plain:
        out.update(aggregate([OrderedDict((k, d[k]) for k in plain) for d in dicts], SUM, engine=engine))
    return OrderedDict((k, out[k]) for k in keys)
