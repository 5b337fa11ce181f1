"""fa_pairwise_gram_q8 (include/fedagg_quant_gram.h) on the device against an exact reference: the block
products in int64, the scales as integers times a power of two, every sum in Python integers.

Shapes (by the header's work split): a segment shorter than a block; 3 B + 37 (ragged, no multiple of 16);
(2 MIN_UNITS + 1) UNIT + 37 elements = 10 units = 3 workgroups of 3 or 4 units, each at least 3 stages;
three segments whose q tensors are views at byte offsets 0, 1 and 7 (16-byte loads and byte loads).
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import pytest
import torch

from fedml_amd import _native as N
from fedml_amd.engine import get_engine

pytestmark = pytest.mark.gpu

KS, BS = [1, 2, 16, 17, 33, 128], [64, 128, 1024]
LONG = (2 * N.Q8_GRAM_MIN_UNITS + 1) * N.Q8_GRAM_UNIT + 37
SHAPES = {"short": lambda B: ([B - 5], [0]), "ragged": lambda B: ([3 * B + 37], [0]), "long": lambda B: ([LONG], [0]),
          "views": lambda B: ([2 * B + 5, N.Q8_GRAM_UNIT + 300, 3 * B + 37], [0, 1, 7])}
grid = pytest.mark.parametrize("K,B,shape", [(K, B, s) for K in KS for B in BS for s in SHAPES])


def gram_ref(qs, scs, B):
    """(num, mag, e, M): G_ij = num_ij * 2^e and sum_b |t_ij[b]| = mag_ij * 2^e exactly, M blocks."""
    K = qs[0].shape[0]
    I = []
    for q in qs:
        nb = -(-q.shape[1] // B)
        p = np.zeros((K, nb * B))
        p[:, :q.shape[1]] = q
        p = p.reshape(K, nb, B).transpose(1, 0, 2)
        I.append(p @ p.transpose(0, 2, 1))  # exact in float64: |I| <= 2^24
    I = np.concatenate(I).astype(np.int64).astype(object)
    m, e = np.frexp(np.concatenate(scs, 1).astype(np.float64))
    mi, e = (m * 2.0 ** 24).astype(np.int64), e - 24
    emin = int(e[mi != 0].min()) if (mi != 0).any() else 0
    S = np.array([[int(a) << int(b - emin) if a else 0 for a, b in zip(ra, rb)] for ra, rb in zip(mi.T, e.T)],
                 dtype=object)
    T = S[:, :, None] * S[:, None, :] * I
    return T.sum(0), np.abs(T).sum(0), 2 * emin, len(I)


def dist_of(G):
    """the header's D from G's bits (numpy float64: every op rounded once)"""
    d = (np.diag(G)[:, None] + np.diag(G)[None, :]) - 2.0 * G
    d = np.where(np.isnan(d), d, np.where(d > 0, d, 0.0))
    np.fill_diagonal(d, 0.0)
    return d


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


def on_device(qs, scs, offs):
    dq, ds = [], []
    for q, sc, off in zip(qs, scs, offs):
        col = []
        for row in q:  # one allocation per client: 16-byte aligned at offset 0
            buf = torch.zeros((len(row) + 15) // 16 * 16 + 16, dtype=torch.int8, device="cuda")
            buf[off:off + len(row)].copy_(torch.from_numpy(row))
            col.append(buf[off:off + len(row)])
        dq.append(col)
        ds.append([torch.from_numpy(r).cuda() for r in sc])
    return dq, ds


def run(qs, scs, offs, B):
    return [t.cpu().numpy() for t in get_engine(0).pairwise_gram_q8(*on_device(qs, scs, offs), B)]


def random_q(rng, K, B, numels):
    qs = [rng.integers(-127, 128, (K, n), dtype=np.int8) for n in numels]
    if B == 1024 and K >= 2:  # the int32 range: 127^2 * 1024, both signs
        for q in qs:
            q[0], q[-1] = 127, -127
    return qs


def quantized(K, B, numels, seed):
    g, eng, qs, scs = torch.Generator().manual_seed(seed), get_engine(0), [], []
    for n in numels:
        x = (torch.randn(K, n, generator=g) * torch.exp(2 * torch.randn(K, n, generator=g))).cuda()
        q, sc = eng.quantize_q8(list(x), B)
        qs.append(torch.stack(q).cpu().numpy())
        scs.append(torch.stack(sc).cpu().numpy())
    return qs, scs


@grid
def test_power_of_two_scales_are_exact(K, B, shape):
    numels, offs = SHAPES[shape](B)
    rng = np.random.default_rng(K * 7 + B)
    qs = random_q(rng, K, B, numels)
    scs = [(2.0 ** rng.integers(-3, 4, (K, -(-n // B)))).astype(np.float32) for n in numels]
    G, D = run(qs, scs, offs, B)
    num, _, e, _ = gram_ref(qs, scs, B)
    Gx = np.array([[float(Fraction(int(v)) * Fraction(2) ** e) for v in r] for r in num])  # representable: exact
    assert same_bits(G, Gx) and same_bits(D, dist_of(Gx))  # every operation of D is exact here too


@grid
def test_quantizer_output_within_the_bound(K, B, shape):
    numels, offs = SHAPES[shape](B)
    qs, scs = quantized(K, B, numels, K * 11 + B)
    G, D = run(qs, scs, offs, B)
    num, mag, e, M = gram_ref(qs, scs, B)
    for i in range(K):
        for j in range(K):
            err = abs(Fraction(float(G[i, j])) - Fraction(int(num[i, j])) * Fraction(2) ** e)
            assert err <= (M + 2) * Fraction(2) ** -53 * int(mag[i, j]) * Fraction(2) ** e, (i, j)
    assert same_bits(G, G.T) and same_bits(D, dist_of(G)) and same_bits(np.diag(D), np.zeros(K))
    assert all(same_bits(x, y) for x, y in zip((G, D), run(qs, scs, offs, B)))  # a second call: the same bits


@grid
def test_identical_clients_are_at_distance_zero(K, B, shape):
    numels, offs = SHAPES[shape](B)
    qs, scs = quantized(K, B, numels, K * 13 + B)
    a, b = (3, 5) if K >= 6 else (0, K - 1)
    for q, sc in zip(qs, scs):
        q[b], sc[b] = q[a], sc[a]
    _, D = run(qs, scs, offs, B)
    assert same_bits(D[a, b], 0.0) and same_bits(D[b, a], 0.0)


@grid
def test_nan_scale_poisons_one_row_and_column_only(K, B, shape):
    numels, offs = SHAPES[shape](B)
    qs, scs = quantized(K, B, numels, K * 17 + B)
    c = K // 2
    qs[-1][c, :B] = 0  # the quantizer's poisoned block: q = 0, scale = NaN
    scs[-1][c, 0] = 0.0
    G0, D0 = run(qs, scs, offs, B)
    scs[-1][c, 0] = np.float32(np.nan)
    G, D = run(qs, scs, offs, B)
    rest = np.ones((K, K), bool)
    rest[c, :] = rest[:, c] = False
    assert np.isnan(G[~rest]).all() and same_bits(G[rest], G0[rest])
    off_diag = ~rest & ~np.eye(K, dtype=bool)
    assert np.isnan(D[off_diag]).all() and same_bits(D[c, c], 0.0) and same_bits(D[rest], D0[rest])


def test_more_than_128_clients_split_into_launches_with_the_same_bits():
    K, B = 130, 64
    numels, offs = SHAPES["ragged"](B)
    qs, scs = quantized(K, B, numels, 3)
    G, D = run(qs, scs, offs, B)
    ids = list(range(40, 64)) + [128, 129]  # one launch: the split changes no pair's sums
    Gs, Ds = run([q[ids] for q in qs], [sc[ids] for sc in scs], offs, B)
    assert same_bits(G[np.ix_(ids, ids)], Gs) and same_bits(D[np.ix_(ids, ids)], Ds)
    assert same_bits(G, G.T) and same_bits(D, dist_of(G))
