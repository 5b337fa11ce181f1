"""fa_pairwise_gram_q1 (include/fedagg_sign_gram.h) on the device against an exact reference: the signs
unpacked to +-1, the block products as integers, the scales as integers times a power of two.

Shapes (by the header's work split): a segment shorter than a block; 3 B + 37 (a ragged block and a ragged
word); (2 MIN_UNITS + 1) UNIT + 37 elements = 10 units = 3 workgroups of 3 or 4 units of 2 stages each, a
block of 1024 crossing the stages; three segments whose bits are views at word offsets 0, 1 and 3 (16-byte
loads and dword loads).
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import pytest
import torch

from fedml_amd import _native as N
from fedml_amd.engine import get_engine

pytestmark = pytest.mark.gpu

KS, BS = [1, 2, 17, 33, 128], [32, 128, 1024]
LONG = (2 * N.Q1_GRAM_MIN_UNITS + 1) * N.Q1_GRAM_UNIT + 37
SHAPES = {"short": lambda B: ([B - 5], [0]), "ragged": lambda B: ([3 * B + 37], [0]), "long": lambda B: ([LONG], [0]),
          "views": lambda B: ([2 * B + 5, N.Q1_GRAM_UNIT + 300, 3 * B + 37], [0, 1, 3])}
grid = pytest.mark.parametrize("K,B,shape", [(K, B, s) for K in KS for B in BS for s in SHAPES])
LIMB = 17  # bits: two limbs, |I| <= 2^10 and fewer than 2^9 blocks multiply and add exactly in float64


def gram_ref(ws, scs, numels, B):
    """(num, mag, e, M): G_ij = num_ij * 2^e and sum_b |t_ij[b]| = mag_ij * 2^e exactly, M blocks.  Bits past a
    segment's end are dropped here; scales are non-negative."""
    K, I = ws[0].shape[0], []
    for w, n in zip(ws, numels):
        nb = -(-n // B)
        p = np.zeros((K, nb * B))
        p[:, :n] = 1.0 - 2.0 * ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(K, -1)[:, :n]
        p = p.reshape(K, nb, B).transpose(1, 0, 2)
        I.append(p @ p.transpose(0, 2, 1))  # exact: |I| <= 1024
    I = np.concatenate(I)
    m, e = np.frexp(np.concatenate(scs, 1).astype(np.float64).T)
    mi, e = (m * 2.0 ** 24).astype(np.int64), e - 24
    emin = int(e[mi != 0].min()) if (mi != 0).any() else 0
    sh = np.where(mi != 0, e - emin, 0)
    assert (mi >= 0).all() and sh.max() < 38 and len(I) < 512
    a = mi << sh  # the scales as integers times 2^emin, below 2^62
    nl = max(1, -(-int(a.max()).bit_length() // LIMB))
    limbs = [((a >> (LIMB * l)) & ((1 << LIMB) - 1)).astype(np.float64) for l in range(nl)]
    num, mag = np.zeros((K, K), object), np.zeros((K, K), object)
    for l in range(nl):
        for r in range(nl):
            w = limbs[l][:, :, None] * limbs[r][:, None, :]
            num += (w * I).sum(0).astype(np.int64).astype(object) << (LIMB * (l + r))
            mag += (w * np.abs(I)).sum(0).astype(np.int64).astype(object) << (LIMB * (l + r))
    return num, mag, 2 * emin, len(I)


def dist_of(G):
    """the header's D from G's bits (numpy float64: every op rounded once)"""
    d = (np.diag(G)[:, None] + np.diag(G)[None, :]) - 2.0 * G
    d = np.where(np.isnan(d), d, np.where(d > 0, d, 0.0))
    np.fill_diagonal(d, 0.0)
    return d


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


def run(ws, scs, numels, offs, B):
    """ws[s]: (K, words) uint32, scs[s]: (K, blocks) float32; client i's bits of segment s start off words into
    an allocation of their own (16-byte aligned at offset 0)"""
    db, ds = [], []
    for w, sc, off in zip(ws, scs, offs):
        bufs = [torch.zeros(w.shape[1] + 8, dtype=torch.int32, device="cuda") for _ in w]
        for buf, row in zip(bufs, w):
            buf[off:off + len(row)].copy_(torch.from_numpy(row.view(np.int32)))
        db.append([buf[off:off + w.shape[1]] for buf in bufs])
        ds.append([torch.from_numpy(r).cuda() for r in sc])
    return [t.cpu().numpy() for t in get_engine(0).pairwise_gram_q1(db, ds, numels, B)]


def quantized(K, B, numels, seed):
    g, eng, ws, scs = torch.Generator().manual_seed(seed), get_engine(0), [], []
    for n in numels:
        x = (torch.randn(K, n, generator=g) * torch.exp(2 * torch.randn(K, n, generator=g))).cuda()
        w, sc = eng.quantize_q1(list(x), B)
        ws.append(torch.stack(w).cpu().numpy().view(np.uint32))
        scs.append(torch.stack(sc).cpu().numpy())
    return ws, scs


@grid
def test_power_of_two_scales_are_exact(K, B, shape):
    numels, offs = SHAPES[shape](B)
    rng = np.random.default_rng(K * 7 + B)
    ws = [rng.integers(0, 1 << 32, (K, -(-n // 32)), dtype=np.uint32) for n in numels]  # garbage past the end too
    scs = [(2.0 ** rng.integers(-3, 4, (K, -(-n // B)))).astype(np.float32) for n in numels]
    G, D = run(ws, scs, numels, offs, B)
    num, _, e, _ = gram_ref(ws, scs, numels, B)
    Gx = np.ldexp(num.astype(np.float64), e)  # terms <= 2^16 * 2^-6, fewer than 2^9 of them: representable
    assert same_bits(G, Gx) and same_bits(D, dist_of(Gx))  # every operation of D is exact here too


@grid
def test_quantizer_output_within_the_bound(K, B, shape):
    numels, offs = SHAPES[shape](B)
    ws, scs = quantized(K, B, numels, K * 11 + B)
    G, D = run(ws, scs, numels, offs, B)
    num, mag, e, M = gram_ref(ws, scs, numels, B)
    for i in range(K):
        for j in range(K):
            err = abs(Fraction(float(G[i, j])) - Fraction(int(num[i, j])) * Fraction(2) ** e)
            assert err <= (M + 2) * Fraction(2) ** -53 * int(mag[i, j]) * Fraction(2) ** e, (i, j)
    assert same_bits(G, G.T) and same_bits(D, dist_of(G)) and same_bits(np.diag(D), np.zeros(K))
    assert all(same_bits(x, y) for x, y in zip((G, D), run(ws, scs, numels, offs, B)))  # a second call: the same bits
    a, b = (3, 5) if K >= 6 else (0, K - 1)  # the sybil case: client a copied onto client b
    for w, sc in zip(ws, scs):
        w[b], sc[b] = w[a], sc[a]
    _, D = run(ws, scs, numels, offs, B)
    assert same_bits(D[a, b], 0.0) and same_bits(D[b, a], 0.0)


@grid
def test_nan_scale_poisons_one_row_and_column_only(K, B, shape):
    numels, offs = SHAPES[shape](B)
    ws, scs = quantized(K, B, numels, K * 17 + B)
    c = K // 2
    scs[-1][c, 0] = 0.0
    G0, D0 = run(ws, scs, numels, offs, B)
    scs[-1][c, 0] = np.float32(np.nan)
    G, D = run(ws, scs, numels, offs, B)
    rest = np.ones((K, K), bool)
    rest[c, :] = rest[:, c] = False
    assert np.isnan(G[~rest]).all() and same_bits(G[rest], G0[rest])
    off_diag = ~rest & ~np.eye(K, dtype=bool)
    assert np.isnan(D[off_diag]).all() and same_bits(D[c, c], 0.0) and same_bits(D[rest], D0[rest])


def test_more_than_128_clients_split_into_launches_with_the_same_bits():
    K, B = 130, 32
    numels, offs = SHAPES["ragged"](B)
    ws, scs = quantized(K, B, numels, 3)
    G, D = run(ws, scs, numels, offs, B)
    ids = list(range(40, 64)) + [100, 128, 129]  # both halves and the tail, in one launch
    Gs, Ds = run([w[ids] for w in ws], [sc[ids] for sc in scs], numels, offs, B)
    assert same_bits(G[np.ix_(ids, ids)], Gs) and same_bits(D[np.ix_(ids, ids)], Ds)
    assert same_bits(G, G.T) and same_bits(D, dist_of(G))
