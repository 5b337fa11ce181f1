"""Krum / multi-Krum on the HIP engine (drop-in for the reference's
python/fedml/core/security/defense/krum_defense.py).

The reference computes every pairwise distance with a separate float32 ``(v_i - v_j).norm()``
(K(K-1) passes over the model on the CPU, :52-66).  Here ONE ``fa_pairwise_sqdist`` launch reads
each client's weights once and produces all K(K-1)/2 squared distances; the score bookkeeping
(ascending distances, sum of the K - f - 2 smallest, float32 ``argsort``) is the reference's,
on the host, over K numbers.  Distances are rounded to the reference's ``norm`` result before
squaring -- float32, or the model's dtype for bfloat16 / float16 models, whose differences the
reference also rounds to that dtype (``vectorize_weight`` keeps it; the device pass does the same,
``fa_pairwise_sqdist_rt``) -- so near-equal scores order the same way; the selection is checked
against the reference (tests/golden/g18_*, including bf16 / f16 models).  float64 models are
measured in float64 throughout, as the reference measures them (fa_pairwise_sqdist_rt with
FA_DTYPE_F64; g18_krum_f64_* includes a near-tie that float32 distances would order differently).

Block-quantized uploads: when every weight key of every client is a `Q8Tensor` of one block size of at
least 64, the distances come from ``fa_pairwise_gram_q8`` -- the Gram matrix straight from the int8
bytes on the int8 matrix cores, no float32 copy of the clients -- and the selected clients' Q8 dicts
are returned untouched for `aggregate_q8`.  Blocks of 16 or 32 (below one int8 matrix instruction) are
dequantized key by key (``weighted_sum_q8`` with one client) and take the float32 path.

1-bit sign uploads: a cohort whose weight keys are all `Q1Tensor` of one block size (any the format has)
gets its distances from ``fa_pairwise_gram_q1`` -- XOR and population counts on the uploaded words -- and
the selected clients' Q1 dicts are returned untouched for `aggregate_q1`.
"""
from __future__ import annotations

import functools
from collections import OrderedDict
from typing import Any, List, Tuple

import numpy as np
import torch

from ....engine import SUM, get_engine
from ....ml.aggregator.microscaled import MXTensor
from ....ml.aggregator.quantized import Q8Tensor
from ....ml.aggregator.rotated import RotatedTensor
from ....ml.aggregator.signcompressed import Q1Tensor
from ..common.utils import is_weight_param

Q8_GRAM_BLOCK_MIN = 64  # FA_Q8_GRAM_BLOCK_MIN: one v_mfma_i32_16x16x64_i8


class KrumDefense(object):
    def __init__(self, config):
        self.config = config
        self.byzantine_client_num = config.byzantine_client_num
        self.krum_param_m = 1  # krum_param_m = 1: krum; > 1: multi-krum
        if hasattr(config, "krum_param_m") and isinstance(config.krum_param_m, int):
            self.krum_param_m = config.krum_param_m

    def defend_before_aggregation(self, raw_client_grad_list: List[Tuple[float, OrderedDict]],
                                  extra_auxiliary_info: Any = None):
        num_client = len(raw_client_grad_list)
        if not 2 * self.byzantine_client_num + 2 <= num_client - self.krum_param_m:
            raise ValueError(
                "byzantine_client_num conflicts with requirements in Krum: 2 * byzantine_client_num + 2 < "
                "client number - krum_param_m")
        krum_scores = self._compute_krum_score([g for _, g in raw_client_grad_list])
        score_index = torch.argsort(torch.Tensor(krum_scores)).tolist()  # ascending, as the reference
        score_index = score_index[0: self.krum_param_m]
        return [raw_client_grad_list[i] for i in score_index]

    def get_malicious_client_idxs(self):
        return []

    @staticmethod
    def vector_dtype(grads) -> torch.dtype:
        """dtype of the reference's vectorize_weight result (torch.cat promotes the weight tensors;
        core/security/common/utils.py:8-13), over every client."""
        keys = [k for k in grads[0].keys() if is_weight_param(k)]
        return functools.reduce(torch.promote_types, [g[k].dtype for g in grads for k in keys])

    def pairwise_sq_distances(self, grads) -> np.ndarray:
        """(K, K) squared distances of the clients' weight vectors (BatchNorm statistics skipped,
        as vectorize_weight does), one device pass; for bf16 / f16 models every difference is
        rounded to that dtype as the reference's ``v_i - v_j`` does."""
        keys = [k for k in grads[0].keys() if is_weight_param(k)]
        fmt = self._block_format(grads, keys)
        if fmt is not None:
            cls, block = fmt
            data = "q" if cls is Q8Tensor else "bits"
            dev = next((getattr(g[k], data).device for g in grads for k in keys if getattr(g[k], data).is_cuda), None)
            eng = get_engine(dev.index if dev is not None else None)
            on = lambda t: t if t.device == eng.device else t.to(eng.device)  # noqa: E731
            dseg = [[on(getattr(g[k], data)).reshape(-1) for g in grads] for k in keys]
            sseg = [[on(g[k].scale) for g in grads] for k in keys]
            if cls is Q1Tensor:
                return eng.pairwise_gram_q1(dseg, sseg, [grads[0][k].numel() for k in keys], block)[1].cpu().numpy()
            if block >= Q8_GRAM_BLOCK_MIN:
                return eng.pairwise_gram_q8(dseg, sseg, block)[1].cpu().numpy()
            # blocks of 16 or 32: the weight keys dequantized (one launch per client), then the float path
            grads = [dict(zip(keys, eng.weighted_sum_q8([[on(g[k].q)] for k in keys], [[on(g[k].scale)] for k in keys],
                                                        SUM, None, block))) for g in grads]
        vdt = self.vector_dtype(grads)
        diff_dt = vdt if vdt in (torch.bfloat16, torch.float16, torch.float64) else torch.float32
        in_dt = torch.float64 if diff_dt == torch.float64 else torch.float32
        dev = next((g[k].device for g in grads for k in keys if g[k].is_cuda), None)
        eng = get_engine(dev.index if dev is not None else None)
        segs = []
        for k in keys:
            col = []
            for g in grads:
                t = g[k]
                if t.device != eng.device:
                    t = t.to(eng.device)
                col.append(t.to(in_dt).contiguous().reshape(-1))
            segs.append(col)
        return eng.pairwise_sqdist(segs, diff_dtype=diff_dt).cpu().numpy()

    @staticmethod
    def _block_format(grads, keys):
        """(Q8Tensor or Q1Tensor, the block size) when every weight key of every client is of that one class,
        None when none is of either; anything else is an error."""
        other = next((type(g[k]).__name__ for g in grads for k in keys
                      if isinstance(g[k], (MXTensor, RotatedTensor))), None)
        if other is not None:
            raise TypeError(f"KrumDefense: {other} state_dicts are not supported: Krum takes plain tensors, "
                            "block-quantized int8 (Q8Tensor) or 1-bit sign (Q1Tensor) weight keys")
        first = grads[0]
        cls = next((type(g[k]) for g in grads for k in keys if isinstance(g[k], (Q8Tensor, Q1Tensor))), None)
        if cls is None:
            return None
        name = cls.__name__
        qset = {k for k in keys if isinstance(first[k], cls)}
        for i, g in enumerate(grads):
            for k in keys:
                if isinstance(g[k], cls) != (k in qset):
                    raise TypeError(f"key {k!r}: client {i} {'has' if isinstance(g[k], cls) else 'lacks'} a "
                                    f"{name} where client 0 {'has' if k in qset else 'lacks'} one")
        if not qset:
            return None
        if len(qset) != len(keys):
            raise TypeError(f"KrumDefense: {name} and other weight keys are mixed: compress every weight key the "
                            "same way or none")
        block = first[keys[0]].block
        for i, g in enumerate(grads):
            for k in keys:
                if g[k].block != block:
                    raise ValueError(f"key {k!r}: client {i} block {g[k].block} != {block} (one block size per call)")
                if g[k].shape != first[k].shape:
                    raise ValueError(f"key {k!r}: client {i} shape {g[k].shape} != {first[k].shape}")
        return cls, block

    def _compute_krum_score(self, grads):
        D = self.pairwise_sq_distances(grads)
        num_client = len(grads)
        # the reference's compute_euclidean_distance(...).item() ** 2: the norm in the vector's dtype
        # (rounded to float32 / bf16 / f16; a float64 vector's norm stays float64), squared
        vdt = self.vector_dtype(grads)
        norms = torch.from_numpy(np.sqrt(D))
        if vdt != torch.float64:
            norms = norms.to(torch.float32)
            if vdt in (torch.bfloat16, torch.float16):
                norms = norms.to(vdt)
        norms = norms.to(torch.float64).numpy()
        krum_scores = []
        for i in range(num_client):
            dists = [float(norms[i, j]) ** 2 for j in range(num_client) if i != j]
            dists.sort()
            krum_scores.append(sum(dists[0: num_client - self.byzantine_client_num - 2]))
        return krum_scores
