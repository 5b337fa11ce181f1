"""Rotated state_dicts: a randomized Hadamard rotation in front of the compressed uploads, undone once on
the server's sum.

The rotation is include/fedagg_rotate.h's: per tensor, a random +-1 diagonal from (seed, round, seg_id)
followed by a Walsh-Hadamard transform over blocks of ``2 ** log2_block`` elements.  It spreads an
outlier coordinate over its block, so the block scale of q8 / mx and the mean magnitude of q1 stop being
set by one element.  Every client of a round uses the same `Rotation` and the rotation is linear:
`rotate_state_dict` rotates (fa_hadamard_rotate, one launch per dtype) and then compresses with the
family's existing quantizer, `aggregate_rotated` sums the clients in the rotated domain with the
family's existing `aggregate*`, unchanged, and undoes the rotation in ONE inverse launch on the float32
sums.  All arithmetic is the HIP kernels'; nothing here computes on the CPU.

The key rules are quantized.py's: every float32 / bfloat16 / float16 key becomes a `RotatedTensor` whose
seg_id is the key's position in the dict, every other key (the int64 BatchNorm counters) stays plain;
results are float32, cast once to a 16-bit key's original dtype.  `FedMLAggOperator.agg` routes here
when the dicts hold `RotatedTensor` values.
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from ...engine import MUL_W, SUM, AggEngine
from .microscaled import MXTensor, aggregate_mx, mx_quantize_state_dict
from .quantized import Q8_DTYPES as ROT_DTYPES
from .quantized import Q8Tensor, _engine_of, aggregate_q8, quantize_state_dict
from .signcompressed import Q1Tensor, aggregate_q1, sign_compress_state_dict
from .state_dict_agg import _to_engine, aggregate


@dataclass(frozen=True)
class Rotation:
    """What the clients of a round share: the seed, the round and log2 of the rotation block."""
    seed: int
    round: int
    log2_block: int = 10


@dataclass
class RotatedTensor:
    """One rotated tensor: ``inner`` holds the n_pad rotated elements (numel rounded up to whole blocks
    of ``2 ** log2_block``) as a flat float32 tensor, a `Q8Tensor`, a `Q1Tensor` or an `MXTensor`;
    ``shape`` and ``dtype`` are the original tensor's."""
    inner: object
    shape: Tuple[int, ...]
    dtype: torch.dtype
    seg_id: int
    round: int
    log2_block: int

    def __post_init__(self):
        self.shape = tuple(self.shape)
        if self.dtype not in ROT_DTYPES:
            raise TypeError(f"RotatedTensor: original dtype {self.dtype} is not float32, bfloat16 or float16")
        if not isinstance(self.inner, (torch.Tensor, Q8Tensor, Q1Tensor, MXTensor)):
            raise TypeError(f"RotatedTensor: inner is a {type(self.inner).__name__}")
        if self.inner.dtype != torch.float32:
            raise TypeError(f"RotatedTensor: the rotated elements are float32 (got {self.inner.dtype})")
        if self.inner.numel() != self.padded():
            raise ValueError(f"RotatedTensor: shape {self.shape} in blocks of {1 << self.log2_block} needs "
                             f"{self.padded()} rotated elements (got {self.inner.numel()})")

    def numel(self) -> int:
        n = 1
        for d in self.shape:
            n *= d
        return n

    def padded(self) -> int:
        return -(-self.numel() >> self.log2_block) << self.log2_block


def _compress(flat: "OrderedDict[str, torch.Tensor]", compress, block, eng) -> Dict[str, object]:
    if compress is None:
        return flat
    if compress == "q8":
        return quantize_state_dict(flat, 128 if block is None else block, engine=eng)
    if compress == "q1":
        return sign_compress_state_dict(flat, 128 if block is None else block, engine=eng)
    if block is not None:
        raise ValueError(f"rotate_state_dict: compress={compress!r} has a fixed block of 32")
    return mx_quantize_state_dict(flat, compress, engine=eng)


def rotate_state_dict(sd: Dict[str, torch.Tensor], rotation: Rotation, compress: Optional[str] = None,
                      block: Optional[int] = None, engine: Optional[AggEngine] = None) -> "OrderedDict[str, object]":
    """Every float32 / bfloat16 / float16 key as a `RotatedTensor` (one forward launch per dtype, then
    ``compress``'s quantizer on the rotated tensors: None, "q8", "q1", "fp8" or "fp4"; ``block`` is the
    q8 / q1 block, 128 by default), every other key unchanged; key order kept.  A key's seg_id is its
    position in ``sd``.  Tensors not on the engine's device are moved there."""
    if compress not in (None, "q8", "q1", "fp8", "fp4"):
        raise ValueError(f'rotate_state_dict: compress {compress!r} must be None, "q8", "q1", "fp8" or "fp4"')
    ids = {k: i for i, k in enumerate(sd.keys())}
    fkeys = [k for k, v in sd.items() if v.dtype in ROT_DTYPES]
    if not fkeys:
        return OrderedDict(sd.items())
    eng = _engine_of([sd[k] for k in fkeys], engine)
    groups: Dict[torch.dtype, List[str]] = {}
    for k in fkeys:
        groups.setdefault(sd[k].dtype, []).append(k)
    flat: Dict[str, torch.Tensor] = {}
    for dt, ks in groups.items():
        outs = eng.hadamard_rotate([_to_engine(sd[k], eng) for k in ks], rotation.log2_block, rotation.seed,
                                   rotation.round, [ids[k] for k in ks])
        flat.update(zip(ks, outs))
    inner = _compress(OrderedDict((k, flat[k]) for k in fkeys), compress, block, eng)
    return OrderedDict(
        (k, RotatedTensor(inner[k], tuple(v.shape), v.dtype, ids[k], rotation.round, rotation.log2_block)
         if k in flat else v) for k, v in sd.items())


_INNER_AGG = ((Q8Tensor, aggregate_q8), (Q1Tensor, aggregate_q1), (MXTensor, aggregate_mx))


def aggregate_rotated(dicts: Sequence[Dict[str, object]], mode: int, coef: Optional[Sequence[float]] = None,
                      seed: Optional[int] = None, engine: Optional[AggEngine] = None
                      ) -> "OrderedDict[str, torch.Tensor]":
    """Ordered per-key reduction over rotated client state_dicts: the wrappers are stripped, the inner
    family's `aggregate` / `aggregate_q8` / `aggregate_q1` / `aggregate_mx` sums in the rotated domain,
    and ONE inverse launch undoes the rotation on the float32 sums; client 0's key order, the original
    shapes, a 16-bit key cast once to its original dtype.  ``mode``: MUL_W or SUM; ``seed``: the
    round's `Rotation.seed`.

    Clients that disagree on which keys are rotated raise TypeError; clients that disagree on shape,
    original dtype, seg_id, round or log2_block (the last two: keys too) raise ValueError."""
    if len(dicts) == 0:
        raise IndexError("list index out of range")  # as aggregate: the reference indexes raw_grad_list[0]
    if mode not in (MUL_W, SUM):
        raise ValueError(f"aggregate_rotated: mode {mode} not supported (MUL_W, SUM)")
    if seed is None:
        raise ValueError("aggregate_rotated: the rotation's seed is required")
    first = dicts[0]
    keys = list(first.keys())
    rkeys = [k for k in keys if isinstance(first[k], RotatedTensor)]
    rset = set(rkeys)
    for i, d in enumerate(dicts):
        for k in keys:
            v = d[k]  # KeyError on a missing key, like aggregate
            if isinstance(v, RotatedTensor) != (k in rset):
                raise TypeError(f"key {k!r}: client {i} {'has' if isinstance(v, RotatedTensor) else 'lacks'} a "
                                f"RotatedTensor where client 0 {'has' if k in rset else 'lacks'} one")
            if k not in rset:
                continue
            # shape, dtype and seg_id against client 0's key; round and block against client 0's first key
            for name, ref in (("shape", first[k]), ("dtype", first[k]), ("seg_id", first[k]),
                              ("round", first[rkeys[0]]), ("log2_block", first[rkeys[0]])):
                if getattr(v, name) != getattr(ref, name):
                    raise ValueError(f"key {k!r}: client {i} {name} {getattr(v, name)} != {getattr(ref, name)} "
                                     "(one rotation per round)")
    inner_agg = aggregate
    if rkeys:
        inner_agg = next((f for t, f in _INNER_AGG if isinstance(first[rkeys[0]].inner, t)), aggregate)
    sums = inner_agg([OrderedDict((k, v.inner if k in rset else v) for k, v in ((k, d[k]) for k in keys))
                      for d in dicts], mode, coef, engine=engine)
    if not rkeys:
        return sums
    eng = _engine_of([sums[k] for k in rkeys], engine)
    r0 = first[rkeys[0]]
    outs = eng.hadamard_rotate([_to_engine(sums[k].reshape(-1), eng) for k in rkeys], r0.log2_block, seed, r0.round,
                               [first[k].seg_id for k in rkeys], inverse=True,
                               numels=[first[k].numel() for k in rkeys])
    for k, o in zip(rkeys, outs):
        t = first[k]
        o = o.view(t.shape)
        sums[k] = o if t.dtype == torch.float32 else o.to(t.dtype)
    return OrderedDict((k, sums[k]) for k in keys)


def unrotate_state_dict(sd: Dict[str, object], seed: int,
                        engine: Optional[AggEngine] = None) -> "OrderedDict[str, torch.Tensor]":
    """The inverse of `rotate_state_dict`: `aggregate_rotated` with one client and SUM."""
    return aggregate_rotated([sd], SUM, None, seed, engine=engine)
