"""Krum on 1-bit sign uploads: KrumDefense over Q1Tensor dicts (fa_pairwise_gram_q1) against the route through
decompressed dicts, and the distances against numpy float64.  The cohort is tests/test_gpu_q8_krum.py's.

The seed: with the Krum scores taken in numpy float64 from the decompressed weight keys, the gap between the
m-th and the (m + 1)-th smallest score is 1.4e-2 relative for m = 1 and 2.4e-2 for m = 4, and every gap among
the five smallest scores is 5e-4 or more, at B = 32 and B = 128 alike (the float32 route is good to about
1e-6), so both routes must select the same clients in the same order; the test checks the gaps again on the
device's own compression.  The distance tolerance is the one derived in tests/test_gpu_q8_krum.py, with the
sign times the scale exact in float64.
"""
from __future__ import annotations

import types
from collections import OrderedDict

import numpy as np
import pytest
import torch

from fedml_amd.core.security.defense.krum_defense import KrumDefense
from fedml_amd.engine import MUL_W
from fedml_amd.ml.aggregator.agg_operator import FedMLAggOperator
from fedml_amd.ml.aggregator.signcompressed import Q1Tensor, aggregate_q1, decompress_state_dict, sign_compress_state_dict

pytestmark = pytest.mark.gpu
K, F, SEED, KEYS = 12, 3, 5, ["conv.weight", "fc.weight"]


def clients(block):
    g = torch.Generator().manual_seed(SEED)
    base = OrderedDict([("conv.weight", torch.randn(16, 8, 3, 3, generator=g)),
                        ("bn.running_mean", torch.randn(16, generator=g)), ("bn.num_batches_tracked", torch.tensor(7)),
                        ("fc.weight", torch.randn(10, 37, generator=g))])
    out = []
    for i in range(K):
        shift = 2.0 if i in (1, 6, 10) else 0.0  # the attackers: a shifted mean
        sd = OrderedDict((k, v if v.dtype == torch.int64 else
                          (v + shift + 0.1 * torch.randn(v.shape, generator=g)).cuda()) for k, v in base.items())
        out.append((10 + i, sign_compress_state_dict(sd, block)))
    return out


def vectors(q1):
    """the decompressed weight keys in float64 (sign * scale is exact)"""
    return np.stack([np.concatenate([sd[k].cpu().numpy().reshape(-1).astype(np.float64) for k in KEYS])
                     for sd in (decompress_state_dict(sd) for _, sd in q1)])


def select(m, grads):
    d = KrumDefense(types.SimpleNamespace(byzantine_client_num=F, krum_param_m=m))
    picked = d.defend_before_aggregation(grads)
    return [next(i for i, g in enumerate(grads) if g[1] is p[1]) for p in picked], picked


@pytest.mark.parametrize("block", [128, 32])
@pytest.mark.parametrize("m", [1, 4])
def test_selection_matches_the_decompressed_route(m, block):
    q1 = clients(block)
    v = vectors(q1)
    d = np.sort(((v[:, None, :] - v[None, :, :]) ** 2).sum(2), 1)[:, 1:K - F - 1].sum(1)  # the Krum scores
    s = np.sort(d)[:m + 1]
    assert (np.diff(s) > 1e-4 * s[1:]).all(), "the seed leaves a near-tie: choose another"
    plain = [(n, decompress_state_dict(sd)) for n, sd in q1]
    idx, picked = select(m, q1)
    assert idx == select(m, plain)[0] and not set(idx) & {1, 6, 10}
    assert all(p is q1[i] and isinstance(p[1]["fc.weight"], Q1Tensor) for p, i in zip(picked, idx))
    got = FedMLAggOperator.agg(types.SimpleNamespace(federated_optimizer="FedAvg"), picked)
    total = sum(n for n, _ in picked)
    want = aggregate_q1([sd for _, sd in picked], MUL_W, [n / total for n, _ in picked])
    for k in want:
        assert got[k].dtype == want[k].dtype
        assert torch.equal(got[k].reshape(-1).view(torch.uint8), want[k].reshape(-1).view(torch.uint8))


@pytest.mark.parametrize("block", [128, 32])
def test_distances_match_numpy_float64(block):
    q1 = clients(block)
    D = KrumDefense(types.SimpleNamespace(byzantine_client_num=F)).pairwise_sq_distances([sd for _, sd in q1])
    v = vectors(q1)
    M = sum(q1[0][1][k].scale.numel() for k in KEYS)
    A = (v * v).sum(1)
    want = ((v[:, None, :] - v[None, :, :]) ** 2).sum(2)
    tol = (M + 3) * 2.0 ** -52 * (A[:, None] + A[None, :]) + v.shape[1] * 2.0 ** -53 * want
    assert (np.abs(D - want) <= tol).all() and (np.diag(D) == 0).all()
