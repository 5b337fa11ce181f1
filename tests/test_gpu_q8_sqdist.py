"""fa_weighted_sum_sqdist_q8 / fa_centered_sum_sqdist_q8 (include/fedagg_quant_dist.h) against the header:
out bit for bit the torch-CPU restatement (one rounded float32 op per line), the stats within the header's
1e-6 of numpy float64 sums over x_i = rnd(q * scale), the same bits from the same call.

K covers: below one load group, past KM = 8, the last register-form K, the first generic K, past one
128-client LDS block.  One call holds two whole slots and a ragged one, a segment below one block, an empty
one, and a whole slot whose q tensors start 1 byte into their storage (the byte path).
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from fedml_amd import _native as N
from fedml_amd.engine import get_engine
from test_quantized_cpu import sum_ref

pytestmark = pytest.mark.gpu
NUMEL = (2 * 4096 + 37, 5, 0, 4096)
TOL = 1e-6


@functools.lru_cache(maxsize=None)
def inputs(k, block):
    """(q[s][i] int8, scale[s][i] float32, coef, center[s]) on the CPU; scales are no powers of two."""
    g = torch.Generator().manual_seed(1000 * k + block)
    q = [[torch.randint(-127, 128, (n,), generator=g, dtype=torch.int8) for _ in range(k)] for n in NUMEL]
    sc = [[(torch.rand(-(-n // block), generator=g) * 0.9 + 0.55) * 3e-3 for _ in range(k)] for n in NUMEL]
    w = torch.rand(k, generator=g, dtype=torch.float64) + 0.1
    return q, sc, (w / w.sum()).tolist(), [torch.randn(n, generator=g) * 0.2 for n in NUMEL]


def dequant(q, sc, block):
    return q.to(torch.float32) * sc.repeat_interleave(block)[:q.numel()]


def center_ref(qs, scs, cen, coef, block):
    acc = None
    for q, sc, w in zip(qs, scs, coef):
        u = dequant(q, sc, block) - cen
        t = u * torch.full_like(u, 0.0).add_(torch.tensor(w, dtype=torch.float64).to(torch.float32))
        acc = t if acc is None else acc + t
    return cen + acc


def on_device(q, sc, cen):
    dev = get_engine().device
    dq = [[t.to(dev) for t in seg] for seg in q]
    dq[3] = [torch.empty(t.numel() + 1, dtype=torch.int8, device=dev)[1:].copy_(t) for t in q[3]]  # 1 byte in
    return dq, [[t.to(dev) for t in seg] for seg in sc], [t.to(dev) for t in cen]


def run(eng, mode, dq, dsc, dcen, coef, block):
    if mode == "plain":
        return eng.weighted_sum_sqdist_q8(dq, dsc, coef, block)
    return eng.centered_sum_sqdist_q8(dq, dsc, dcen, coef if mode == "center" else None, block)


@pytest.mark.parametrize("mode", ["plain", "center", "dist"])
@pytest.mark.parametrize("block", [16, 128, 1024])
@pytest.mark.parametrize("k", [1, 3, 9, 32, 33, 130])
def test_out_bits_and_stats(k, block, mode):
    eng = get_engine()
    q, sc, coef, cen = inputs(k, block)
    dq, dsc, dcen = on_device(q, sc, cen)
    outs, stats = run(eng, mode, dq, dsc, dcen, coef, block)
    stats2 = run(eng, mode, dq, dsc, dcen, coef, block)[1]
    assert torch.equal(stats.view(torch.int64), stats2.view(torch.int64))
    ref = []
    for s, n in enumerate(NUMEL):
        if mode == "dist":
            ref.append(cen[s])
            continue
        want = (sum_ref(q[s], sc[s], N.MUL_W, coef, block) if mode == "plain"
                else center_ref(q[s], sc[s], cen[s], coef, block)) if n else torch.empty(0)
        assert torch.equal(outs[s].cpu().view(torch.int32), want.view(torch.int32)), (s, n)
        ref.append(want)
    x = [[dequant(q[s][i], sc[s][i], block).double().numpy() for s in range(len(NUMEL))] for i in range(k)]
    d2 = np.array([sum(((xi[s] - ref[s].double().numpy()) ** 2).sum() for s in range(len(NUMEL))) for xi in x])
    ss = np.array([sum((xs ** 2).sum() for xs in xi) for xi in x])
    got = stats.cpu().numpy()
    print("max relative error: d2 %.3g ss %.3g" % ((np.abs(got[0] - d2) / np.maximum(d2, 1e-300)).max(),
                                                    (np.abs(got[1] - ss) / ss).max()))
    assert (np.abs(got[0] - d2) <= TOL * d2).all() and (np.abs(got[1] - ss) <= TOL * ss).all()
    if k == 1 and mode == "plain":
        assert eng.weighted_sum_sqdist_q8(dq, dsc, [1.0], block)[1][0, 0].item() == 0.0


def test_center_out_is_the_float_entry_over_dequantized_tensors():
    eng = get_engine()
    k, block = 9, 128
    q, sc, coef, cen = inputs(k, block)
    dq, dsc, dcen = on_device(q, sc, cen)
    deq = [[eng.weighted_sum_q8([[a]], [[b]], N.SUM, None, block)[0] for a, b in zip(qs, ss)] for qs, ss in zip(dq, dsc)]
    want, wstats = eng.centered_sum_sqdist(deq, dcen, coef)
    got, stats = eng.centered_sum_sqdist_q8(dq, dsc, dcen, coef, block)
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.allclose(stats, wstats, rtol=2 * TOL, atol=0)


def test_nan_scale_marks_its_client_only():
    eng = get_engine()
    k, block = 9, 128
    q, sc, _, cen = inputs(k, block)
    dq, dsc, dcen = on_device(q, sc, cen)
    dsc[0][4] = dsc[0][4].clone()
    dsc[0][4][3] = float("nan")
    stats = eng.centered_sum_sqdist_q8(dq, dsc, dcen, None, block)[1].cpu()
    bad = ~torch.isfinite(stats)
    assert bad[1].tolist() == [i == 4 for i in range(k)] and not bad[0, [i for i in range(k) if i != 4]].any()
