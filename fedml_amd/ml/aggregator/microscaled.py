"""OCP Microscaling ("mx") state_dicts: MXFP8 / MXFP4 client uploads aggregated without a float32
round trip through device memory.

The format is include/fedagg_mx.h's: per tensor, one FP8 E4M3 byte or FP4 E2M1 nibble per element and
one E8M0 scale byte per block of 32 elements, element e worth ``element[e] * 2 ** (scale[e // 32] - 127)``.
It is what MXFP8 / MXFP4 training stacks hold, so a client can upload exactly that.
`mx_quantize_state_dict` produces it on the device (fa_quantize_mx), `aggregate_mx` sums K clients'
dicts in ONE launch of the fused decode-and-sum kernel (fa_weighted_sum_mx), bit for bit the float32
ordered sum over the decoded tensors; `mx_dequantize_state_dict` is that kernel with one client.  All
arithmetic is the HIP kernels'; nothing here computes on the CPU.

A quantized dict maps every float32 / bfloat16 / float16 key to an `MXTensor` and keeps every other key
(the int64 BatchNorm counters) as a plain tensor; those go through the ordinary `aggregate`.  The sum
is float32; a key whose original dtype is a 16-bit type is cast to it once, at the end.
`FedMLAggOperator.agg` routes FedAvg / FedProx and FedAvg_seq / FedDyn here when the dicts hold
`MXTensor` values.
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from ...engine import MUL_W, SUM, AggEngine
from .quantized import Q8_DTYPES as MX_DTYPES
from .quantized import _engine_of, _restore
from .state_dict_agg import _to_engine, aggregate

MX_BLOCK = 32
_BYTE_VIEWS = tuple(getattr(torch, n) for n in ("float8_e4m3fn", "float8_e8m0fnu") if hasattr(torch, n))


def _as_bytes(t: torch.Tensor) -> torch.Tensor:
    """A one-byte tensor (torch's float8 types among them) viewed as flat uint8."""
    if t.dtype in _BYTE_VIEWS:
        t = t.view(torch.uint8)
    return t.reshape(-1)


@dataclass
class MXTensor:
    """One tensor in the mx format: ``data`` uint8 (numel bytes for "fp8", ceil(numel / 2) for "fp4", the
    even element in the low nibble), ``scale`` uint8 (one E8M0 byte per 32 elements of the flattened
    tensor), ``dtype`` the original tensor's dtype.  ``torch.float8_e4m3fn`` data and
    ``torch.float8_e8m0fnu`` scales are accepted and viewed as bytes."""
    data: torch.Tensor
    scale: torch.Tensor
    fmt: str
    shape: Tuple[int, ...]
    dtype: torch.dtype

    def __post_init__(self):
        self.shape = tuple(self.shape)
        self.data, self.scale = _as_bytes(self.data), _as_bytes(self.scale)
        if self.fmt not in ("fp8", "fp4"):
            raise ValueError(f'MXTensor: fmt {self.fmt!r} must be "fp8" or "fp4"')
        if self.data.dtype != torch.uint8 or self.scale.dtype != torch.uint8:
            raise TypeError(f"MXTensor: data and scale must be one-byte tensors (got {self.data.dtype}, "
                            f"{self.scale.dtype})")
        if self.dtype not in MX_DTYPES:
            raise TypeError(f"MXTensor: original dtype {self.dtype} is not float32, bfloat16 or float16")
        n = self.numel()
        nd, nb = (n if self.fmt == "fp8" else -(-n // 2)), -(-n // MX_BLOCK)
        if self.data.numel() != nd or self.scale.numel() != nb:
            raise ValueError(f"MXTensor: shape {self.shape} as {self.fmt} needs {nd} data and {nb} scale bytes "
                             f"(got {self.data.numel()}, {self.scale.numel()})")

    def numel(self) -> int:
        n = 1
        for d in self.shape:
            n *= d
        return n


def mx_quantize_state_dict(sd: Dict[str, torch.Tensor], fmt: str,
                           engine: Optional[AggEngine] = None) -> "OrderedDict[str, object]":
    """Every float32 / bfloat16 / float16 key as an `MXTensor` (one fa_quantize_mx launch per dtype),
    every other key unchanged; key order kept.  Tensors not on the engine's device are moved there."""
    fkeys = [k for k, v in sd.items() if v.dtype in MX_DTYPES]
    eng = _engine_of([sd[k] for k in fkeys], engine) if fkeys else None
    groups: Dict[torch.dtype, List[str]] = {}
    for k in fkeys:
        groups.setdefault(sd[k].dtype, []).append(k)
    done: Dict[str, MXTensor] = {}
    for dt, ks in groups.items():
        data, scales = eng.quantize_mx([_to_engine(sd[k], eng) for k in ks], fmt)
        for k, d, sc in zip(ks, data, scales):
            done[k] = MXTensor(d, sc, fmt, tuple(sd[k].shape), dt)
    return OrderedDict((k, done.get(k, v)) for k, v in sd.items())


def _sum_mx(eng: AggEngine, keys, dicts, fmt, mode, coef) -> List[torch.Tensor]:
    return eng.weighted_sum_mx([[_to_engine(d[k].data, eng) for d in dicts] for k in keys],
                               [[_to_engine(d[k].scale, eng) for d in dicts] for k in keys],
                               [dicts[0][k].numel() for k in keys], fmt, mode, coef)


def mx_dequantize_state_dict(sd: Dict[str, object],
                             engine: Optional[AggEngine] = None) -> "OrderedDict[str, torch.Tensor]":
    """The inverse: every `MXTensor` key as a tensor of its original shape and dtype (the sum kernel with
    one client, one launch per element format), every other key unchanged."""
    mkeys = [k for k, v in sd.items() if isinstance(v, MXTensor)]
    eng = _engine_of([sd[k].data for k in mkeys], engine) if mkeys else None
    done: Dict[str, torch.Tensor] = {}
    for fmt in ("fp8", "fp4"):
        ks = [k for k in mkeys if sd[k].fmt == fmt]
        if ks:
            for k, o in zip(ks, _sum_mx(eng, ks, [sd], fmt, SUM, None)):
                done[k] = _restore(o, sd[k])
    return OrderedDict((k, done.get(k, v)) for k, v in sd.items())


def aggregate_mx(dicts: Sequence[Dict[str, object]], mode: int, coef: Optional[Sequence[float]] = None,
                 engine: Optional[AggEngine] = None) -> "OrderedDict[str, torch.Tensor]":
    """Ordered per-key reduction over MX client state_dicts: every `MXTensor` key in ONE
    fa_weighted_sum_mx launch, the plain keys through `aggregate`; client 0's key order, the original
    shapes, float32 results cast once to a 16-bit key's original dtype.  ``mode``: MUL_W or SUM.

    Clients that disagree on which keys are quantized, or a round that holds both FP8 and FP4 tensors,
    raise TypeError; clients that disagree on a key's shape or original dtype raise ValueError."""
    if len(dicts) == 0:
        raise IndexError("list index out of range")  # as aggregate: the reference indexes raw_grad_list[0]
    if mode not in (MUL_W, SUM):
        raise ValueError(f"aggregate_mx: mode {mode} not supported (MUL_W, SUM)")
    first = dicts[0]
    keys = list(first.keys())
    mkeys = [k for k in keys if isinstance(first[k], MXTensor)]
    mset = set(mkeys)
    for i, d in enumerate(dicts):
        for k in keys:
            v = d[k]  # KeyError on a missing key, like aggregate
            if isinstance(v, MXTensor) != (k in mset):
                raise TypeError(f"key {k!r}: client {i} {'has' if isinstance(v, MXTensor) else 'lacks'} an MXTensor "
                                f"where client 0 {'has' if k in mset else 'lacks'} one")
    out: Dict[str, torch.Tensor] = {}
    if mkeys:
        fmt = first[mkeys[0]].fmt
        for k in mkeys:
            t0 = first[k]
            for i, d in enumerate(dicts):
                t = d[k]
                if t.fmt != fmt:
                    raise TypeError(f"key {k!r}: client {i} holds {t.fmt} where the round holds {fmt}: one "
                                    "element format per round")
                if t.shape != t0.shape:
                    raise ValueError(f"key {k!r}: client {i} shape {t.shape} != {t0.shape}")
                if t.dtype != t0.dtype:
                    raise ValueError(f"key {k!r}: client {i} original dtype {t.dtype} != {t0.dtype}")
        eng = _engine_of([first[k].data for k in mkeys], engine)
        for k, o in zip(mkeys, _sum_mx(eng, mkeys, dicts, fmt, mode, coef)):
            out[k] = _restore(o, first[k])
    plain = [k for k in keys if k not in mset]
    if plain:
        out.update(aggregate([OrderedDict((k, d[k]) for k in plain) for d in dicts], mode, coef, engine=engine))
    return OrderedDict((k, out[k]) for k in keys)
