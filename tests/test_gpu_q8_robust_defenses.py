"""geometric_median and centered_clipping through FedMLDefender on block-quantized int8 cohorts (one
fa_weighted_sum_sqdist_q8 / fa_centered_sum_sqdist_q8 launch per pass) against the same host driver run with a
numpy float64 step over the dequantized float32 values x = rnd(q * scale).

The tolerance is measured at run time against code that predates this route: e0 = the error, against that
float64 reference, of the same defense over `dequantize_state_dict` of the same clients; the q8 route must stay
within 4 e0, key by key (the same arithmetic with one rounding per term placed differently, plus stats with
the same 1e-6 bound).  Seen on an MI355X: DESIGN.md, block-quantized family.
"""
from __future__ import annotations

import types
from collections import OrderedDict

import numpy as np
import pytest
import torch

from fedml_amd.cclip import cclip_driver
from fedml_amd.core.security.fedml_defender import FedMLDefender
from fedml_amd.engine import SUM, get_engine
from fedml_amd.ml.aggregator.agg_operator import FedMLAggOperator
from fedml_amd.ml.aggregator.quantized import Q8Tensor, dequantize_state_dict, quantize_state_dict
from fedml_amd.weiszfeld import weiszfeld_driver

pytestmark = pytest.mark.gpu
K, BLOCK, FKEYS = 12, 128, ("fc.weight", "bn.weight")
CFG = {"geometric_median": dict(geomed_iters=3, geomed_nu=1e-6),
       "centered_clipping": dict(cclip_tau=3.0, cclip_iters=2, cclip_center="global")}


def cohort():
    g = torch.Generator().manual_seed(3)
    base = OrderedDict([("fc.weight", torch.randn(50, 101, generator=g)),
                        ("bn.weight", torch.randn(15, 20, generator=g).to(torch.bfloat16)),
                        ("bn.num_batches_tracked", torch.tensor(7))])
    raw = []
    for i in range(K):
        sd = OrderedDict((k, v + i if v.dtype == torch.int64 else
                          ((v.float() + 0.1 * torch.randn(v.shape, generator=g)) * (100.0 if i in (2, 5, 9) else 1.0))
                          .to(v.dtype).cuda()) for k, v in base.items())
        raw.append((10 + i, quantize_state_dict(sd, BLOCK)))
    return base, raw


def defend(kind, raw, center=None):
    d = FedMLDefender.get_instance()
    try:
        d.init(types.SimpleNamespace(enable_defense=True, defense_type=kind, federated_optimizer="FedAvg", **CFG[kind]))
        return d.defend_on_aggregation(raw, FedMLAggOperator.agg, center), d.get_malicious_client_idxs()
    finally:
        FedMLDefender._defender_instance = None


def reference(kind, raw, center):
    """The defense's own driver over x = rnd(q * scale) widened to float64: {key: float64 array}."""
    eng = get_engine()
    x = [np.concatenate([eng.weighted_sum_q8([[sd[k].q]], [[sd[k].scale]], SUM, None, BLOCK)[0].double().cpu().numpy()
                         .reshape(-1) for k in FKEYS]) for _, sd in raw]
    counts = [float(n) for n, _ in raw]
    v = [None]
    stats = lambda idx: ([((x[i] - v[0]) ** 2).sum() for i in idx], [(x[i] ** 2).sum() for i in idx])  # noqa: E731

    def wsum(coef, idx):
        v[0] = sum(c * x[i] for c, i in zip(coef, idx))
        return stats(idx)

    def first(idx):
        v[0] = np.concatenate([center[k].double().numpy().reshape(-1) for k in FKEYS])
        return stats(idx)

    def clip(scales, idx):
        v[0] = v[0] + sum(s * (x[i] - v[0]) for s, i in zip(scales, idx))
        return stats(idx)

    if kind == "geometric_median":
        weiszfeld_driver(counts, CFG[kind]["geomed_iters"], CFG[kind]["geomed_nu"], wsum)
    else:
        cclip_driver(counts, CFG[kind]["cclip_iters"], CFG[kind]["cclip_tau"], first, clip)
    n0 = raw[0][1][FKEYS[0]].numel()
    return {FKEYS[0]: v[0][:n0], FKEYS[1]: v[0][n0:]}


@pytest.mark.parametrize("kind", ["geometric_median", "centered_clipping"])
def test_q8_route_against_float64_and_the_dequantized_route(kind):
    base, raw = cohort()
    got, dropped = defend(kind, raw, base)
    old, _ = defend(kind, [(n, dequantize_state_dict(sd)) for n, sd in raw], base)
    ref = reference(kind, raw, base)
    assert list(got.keys()) == list(base.keys()) and dropped == []
    for k in FKEYS:
        assert got[k].dtype == base[k].dtype and got[k].shape == base[k].shape and got[k].is_cuda
        err = lambda t: np.abs(t.double().cpu().numpy().reshape(-1) - ref[k]).max()  # noqa: E731
        e0, e = err(old[k]), err(got[k])
        print(f"{kind} {k}: e0 = {e0:.3g}, q8 route = {e:.3g}")
        assert e <= 4 * e0
    want = FedMLAggOperator.agg(types.SimpleNamespace(federated_optimizer="FedAvg"),
                                [(n, OrderedDict([("c", sd["bn.num_batches_tracked"])])) for n, sd in raw])["c"]
    cnt = got["bn.num_batches_tracked"]  # the base aggregation's value, whatever dtype it gives a counter
    assert cnt.dtype == want.dtype and torch.equal(cnt.cpu(), want.cpu())


@pytest.mark.parametrize("kind", ["geometric_median", "centered_clipping"])
def test_poisoned_client_is_reported_and_mixed_cohorts_are_refused(kind):
    base, raw = cohort()
    t = raw[4][1]["fc.weight"]
    scale = t.scale.clone()
    scale[7] = float("nan")
    raw[4] = (raw[4][0], OrderedDict(raw[4][1], **{"fc.weight": Q8Tensor(t.q, scale, t.block, t.shape, t.dtype)}))
    got, dropped = defend(kind, raw, base)
    assert dropped == [4] and all(torch.isfinite(got[k].float()).all() for k in FKEYS)
    raw[1] = (raw[1][0], dequantize_state_dict(raw[1][1]))
    with pytest.raises(TypeError, match="Q8Tensor"):
        defend(kind, raw, base)
