"""Coordinate-wise median on the HIP engine (drop-in for the reference's
python/fedml/core/security/defense/coordinate_wise_median_defense.py).

The reference vectorizes every client's weights (BatchNorm statistics skipped, utils.py:8-21),
stacks them and takes ``torch.median(dim=-1)``, then walks ALL keys of client 0's dict, slicing
the median vector by each key's size (:33-43) -- so a model with BatchNorm statistics misaligns
and ends in a ``view`` RuntimeError; client 0's dict is modified in place and returned.  This
mirror keeps all of that; the median itself is ONE ``fa_coord_median`` launch over the weight
keys (a selection, bit-identical to ATen's: NaN first, lower median, ties by client index;
tests/golden/g16_*).

Block-quantized uploads: when every weight key of every client is a `Q8Tensor` of one block size, the
median is ONE ``fa_coord_median_q8`` launch straight from the int8 bytes (include/fedagg_quant_col.h: the
value of rank (K-1)/2, no tie by client index among zeros of both signs) in float32, each key's slice cast
once to its original dtype; more than 128 clients are dequantized first.  Mixed plain and Q8Tensor weight
keys, and the other compressed formats, raise TypeError.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Any, Callable, List, Tuple

import torch

from ...._native import Q8_COL_MAX_K
from ....arena import resident_rows
from ....engine import get_engine
from ....ml.aggregator.microscaled import MXTensor
from ....ml.aggregator.quantized import Q8Tensor, _restore, dequantize_state_dict
from ....ml.aggregator.rotated import RotatedTensor
from ....ml.aggregator.signcompressed import Q1Tensor
from ..common.utils import is_weight_param

_NATIVE = (torch.float32, torch.bfloat16, torch.float16, torch.float64)


class CoordinateWiseMedianDefense(object):
    def __init__(self, config):
        pass

    @staticmethod
    def _q8_block(grads, keys):
        """The block size when every weight key of every client is a `Q8Tensor` of one block size, None for
        plain dicts; plain and Q8 weight keys mixed, and the other compressed formats, are a TypeError."""
        name = "coordinate_wise_median"
        other = next((type(v).__name__ for g in grads for v in g.values()
                      if isinstance(v, (Q1Tensor, MXTensor, RotatedTensor))), None)
        if other is not None:
            raise TypeError(f"{name}: {other} state_dicts are not supported: this defense takes plain tensors or "
                            "block-quantized int8 (Q8Tensor) weight keys")
        if not any(isinstance(g[k], Q8Tensor) for g in grads for k in keys):
            return None
        for i, g in enumerate(grads):
            for k in keys:
                if not isinstance(g[k], Q8Tensor):
                    raise TypeError(f"{name}: key {k!r} of client {i} is a plain tensor in a Q8Tensor cohort: plain "
                                    "and Q8Tensor weight keys are mixed; supported are all plain tensors or every "
                                    "weight key of every client a Q8Tensor")
                if g[k].block != grads[0][keys[0]].block:
                    raise ValueError(f"{name}: key {k!r}: client {i} block {g[k].block} != "
                                     f"{grads[0][keys[0]].block} (one block size per call)")
        return grads[0][keys[0]].block

    @staticmethod
    def _defend_q8(raw_client_grad_list, grads, keys, block):
        """ONE fa_coord_median_q8 launch over the weight keys straight from the int8 bytes into one float32
        vector, then the reference's write-back walk with each slice cast once to its key's dtype."""
        first = grads[0]
        dev = next((g[k].q.device for g in grads for k in keys if g[k].q.is_cuda), None)
        eng = get_engine(dev.index if dev is not None else None)
        on = lambda t: (t if t.device == eng.device else t.to(eng.device)).contiguous().reshape(-1)  # noqa: E731
        for k in keys:
            if any(g[k].numel() != first[k].numel() for g in grads):
                raise RuntimeError(f"Sizes of tensors must match (key {k!r})")
        starts, pos = [], 0
        for k in keys:  # every key's output on a 16-byte boundary: vector stores
            starts.append(pos)
            pos += -(-first[k].numel() // 4) * 4
        pad = torch.empty(pos, dtype=torch.float32, device=eng.device)
        eng.coord_median_q8([[on(g[k].q) for g in grads] for k in keys], [[on(g[k].scale) for g in grads] for k in keys],
                            block, outs=[pad[a:a + first[k].numel()] for k, a in zip(keys, starts)])
        vec = torch.cat([pad[a:a + first[k].numel()] for k, a in zip(keys, starts)])
        if dev is None:
            vec = vec.cpu()
        index = 0
        averaged_params = raw_client_grad_list[0][1]
        for k, params in list(averaged_params.items()):
            n = params.numel()
            piece = vec[index: index + n]
            averaged_params[k] = (_restore(piece, params) if isinstance(params, Q8Tensor)
                                  else piece.view(params.size()))
            index += n
        return averaged_params

    def defend_on_aggregation(self, raw_client_grad_list: List[Tuple[float, OrderedDict]],
                              base_aggregation_func: Callable = None, extra_auxiliary_info: Any = None):
        grads = [g for _, g in raw_client_grad_list]
        if len(grads) == 0:
            raise RuntimeError("torch.cat(): expected a non-empty list of Tensors")
        keys = [k for k in grads[0].keys() if is_weight_param(k)]
        if not keys:
            raise RuntimeError("torch.cat(): expected a non-empty list of Tensors")
        block = self._q8_block(grads, keys)
        if block is not None and len(grads) > Q8_COL_MAX_K:  # past the q8 kernel: dequantize, the plain route
            grads = [dequantize_state_dict(g) for g in grads]
            raw_client_grad_list = [(n, g) for (n, _), g in zip(raw_client_grad_list, grads)]
        elif block is not None:
            return self._defend_q8(raw_client_grad_list, grads, keys, block)
        hit = resident_rows(grads) if len(keys) == len(grads[0]) else None
        if hit is not None and len(hit[0].bufs) == 1 and next(iter(hit[0].bufs)) in _NATIVE:
            # updates adopted into ONE arena's rows, one float dtype group, weights only: the median
            # is one launch over the rows (tiled arenas read tile-interleaved); same bits, and the
            # write-back below gives client 0's dict the same per-key values
            arena, rows = hit
            med = arena.median(rows)
            averaged_params = raw_client_grad_list[0][1]
            for k in list(averaged_params.keys()):
                averaged_params[k] = med[k]
            return averaged_params
        dev = next((g[k].device for g in grads for k in keys if g[k].is_cuda), None)
        eng = get_engine(dev.index if dev is not None else None)
        cat_dtype = grads[0][keys[0]].dtype
        for k in keys[1:]:
            cat_dtype = torch.promote_types(cat_dtype, grads[0][k].dtype)
        if cat_dtype not in _NATIVE:
            raise TypeError(f"coordinate-wise median of {cat_dtype} weights is not supported")
        segs, numels = [], []
        for k in keys:
            col = []
            for g in grads:
                t = g[k]
                if t.device != eng.device:
                    t = t.to(eng.device)
                if t.dtype != cat_dtype:
                    t = t.to(cat_dtype)  # torch.cat's type promotion
                col.append(t.contiguous().reshape(-1))
            if any(c.numel() != col[0].numel() for c in col):
                raise RuntimeError(f"Sizes of tensors must match (key {k!r})")
            segs.append(col)
            numels.append(col[0].numel())
        vec = torch.empty(sum(numels), dtype=cat_dtype, device=eng.device)
        outs, pos = [], 0
        for n in numels:
            outs.append(vec[pos:pos + n])
            pos += n
        eng.coord_median(segs, outs=outs)
        if dev is None:
            vec = vec.cpu()
        # the reference's write-back walk over every key of client 0's dict (:36-43)
        index = 0
        averaged_params = raw_client_grad_list[0][1]
        for k, params in averaged_params.items():
            median_params = vec[index: index + params.numel()].view(params.size())
            index += params.numel()
            averaged_params[k] = median_params
        return averaged_params
