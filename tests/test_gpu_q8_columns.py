"""coord_median_q8, coord_trimmed_mean_q8 and coord_mean_around_median_q8 (include/fedagg_quant_col.h) bit for
bit against a numpy reference over x = rnd(q * scale): a total-order sort over the clients (-0.0 below +0.0,
NaN on top), the median at rank (K-1)/2, the sums a float64 walk over the ranks.  NaN payloads are
unspecified, so every NaN compares as one value.

One call holds a whole slot plus a ragged one, a segment of 5, an empty segment and a whole slot whose q
tensors start one byte into their storage.  The data makes the ORDER of the float64 sum matter: clients 2j and
2j+1 (j < K/4) hold q and -q under one scale near 2^40..2^60, the rest scales near 2^0..2^10, so a kernel that
adds two partial sums gives other bits; the test asserts that this holds on its own columns (a condition on the
inputs, from the reference alone) before it compares.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from fedml_amd.engine import SUM, get_engine

pytestmark = pytest.mark.gpu
NUMELS = (1024 + 37, 5, 0, 1024)
F64 = np.float64


def make(k, block, seed=3):
    """q[s]: [k, n] int8, sc[s]: [k, ceil(n / block)] float32 of the four segments."""
    rng = np.random.default_rng(seed + 1000 * k + block)
    qs, scs = [], []
    for n in NUMELS:
        nb = -(-n // block)
        q = rng.integers(-127, 128, (k, n)).astype(np.int8)
        e = rng.integers(0, 11, (k, nb)).astype(F64)
        for j in range(k // 4):
            q[2 * j][q[2 * j] == 0] = 1
            q[2 * j + 1] = -q[2 * j]
            e[2 * j] = e[2 * j + 1] = rng.integers(40, 61, nb)
        sc = (2.0 ** e * (1 + rng.random((k, nb)))).astype(np.float32)
        for j in range(k // 4):
            sc[2 * j + 1] = sc[2 * j]
        qs.append(q)
        scs.append(sc)
    return qs, scs


def dequant(q, sc, block):
    return (q.astype(np.float32) * np.repeat(sc, block, axis=1)[:, :q.shape[1]]).astype(np.float32)


def tsort(x):
    u = x.view(np.uint32).astype(np.int64)
    key = np.where(np.isnan(x), 1 << 33, np.where(u >> 31 == 1, 0xFFFFFFFF - u, u + 0x80000000))
    return np.take_along_axis(x, np.argsort(key, axis=0, kind="stable"), 0)


def walk(s, lo, cnt):
    """float64 sum of ranks lo .. lo + cnt - 1 (lo a number or one per column), from the first one."""
    lo = np.broadcast_to(np.asarray(lo), s.shape[1:])[None]
    acc = np.take_along_axis(s, lo, 0)[0].astype(F64)
    for r in range(1, cnt):
        acc = acc + np.take_along_axis(s, lo + r, 0)[0].astype(F64)
    return acc


def ref_tmean(s, b):
    return (walk(s, b, len(s) - 2 * b) / (len(s) - 2 * b)).astype(np.float32)


def ref_mam(s, keep):
    k, h = len(s), (len(s) - 1) // 2
    m = s[h].astype(F64)
    dist = lambda v: np.where(v == m, 0.0, np.where(np.isnan(v), np.inf, np.abs(v.astype(F64) - m)))  # noqa: E731
    lomin, lomax = max(0, h - keep + 1), min(h, k - keep)
    lo = lomin + sum((dist(s[r]) > dist(s[r + keep])).astype(np.int64) for r in range(lomin, lomax))
    out = (walk(s, lo + np.zeros(s.shape[1], np.int64), keep) / keep).astype(np.float32)
    return np.where(np.isnan(m), np.float32(np.nan), out)


def bits(a):
    a = np.asarray(a, np.float32).reshape(-1)
    return np.where(np.isnan(a), 0x7FC00000, a.view(np.uint32))


def upload(qs, scs):
    """The device tensors; the last segment's q start one byte into their storage."""
    dq, ds = [], []
    for s, (q, sc) in enumerate(zip(qs, scs)):
        col = []
        for row in q:
            buf = torch.empty(row.size + 1, dtype=torch.int8, device="cuda")
            t = buf[1:] if s == len(qs) - 1 else buf[:-1]
            t.copy_(torch.from_numpy(row))
            col.append(t)
        dq.append(col)
        ds.append([torch.from_numpy(r.copy()).cuda() for r in sc])
    return dq, ds


def check(got, want, what):
    for s, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy()
        bad = np.flatnonzero(bits(g) != bits(w))
        assert bad.size == 0, f"{what} segment {s}: {bad.size} columns differ, first {bad[0]}: {g[bad[0]]} != {w[bad[0]]}"


def run_all(k, block, qs, scs, trims, keeps):
    eng = get_engine()
    dq, ds = upload(qs, scs)
    srt = [tsort(dequant(q, sc, block)) for q, sc in zip(qs, scs)]
    with np.errstate(all="ignore"):
        check(eng.coord_median_q8(dq, ds, block),  # s[-1]: the column's NaN, if it holds one
              [np.where(np.isnan(s[-1]), s[-1], s[(k - 1) // 2]) for s in srt], "median")
        for b in trims:
            check(eng.coord_trimmed_mean_q8(dq, ds, b, block), [ref_tmean(s, b) for s in srt], f"trim {b}")
        for keep in keeps:
            check(eng.coord_mean_around_median_q8(dq, ds, keep, block), [ref_mam(s, keep) for s in srt], f"keep {keep}")
    return dq, ds, srt


@pytest.mark.parametrize("block", [16, 128, 1024])
@pytest.mark.parametrize("k", [1, 8, 9, 57, 64, 65, 72, 121, 128])
def test_bits_against_numpy(k, block):
    qs, scs = make(k, block)
    trims = sorted({0, min(1, (k - 1) // 2), (k - 1) // 2})
    _, _, srt = run_all(k, block, qs, scs, trims, sorted({1, k - 2 * (k // 5), k}))
    if k >= 8:  # the inputs' own property: summing the kept ranks as two halves changes the result's bits
        s = np.concatenate(srt, axis=1)
        for b in (t for t in trims if t <= k // 10):
            cnt = k - 2 * b
            two = ((walk(s, b, cnt // 2) + walk(s, b + cnt // 2, cnt - cnt // 2)) / cnt).astype(np.float32)
            share = np.mean(bits(two) != bits(ref_tmean(s, b)))
            print(f"K {k} block {block} trim {b}: order-sensitive share {share:.2f}")
            assert share >= 0.15


@pytest.mark.parametrize("k", [9, 100])
def test_special_values_and_the_float_entries(k):
    """Block 2 of client 1 has a NaN scale; block 0 of client 2 an infinite one over q of both signs and zero
    (+-inf, and NaN where q = 0); block 3 of client 3 a zero scale under negative q (-0.0).  The NaN-scale
    block alone: the median is NaN, the trimmed mean finite with trim >= 1 and NaN with trim 0.  Everywhere
    the median is NaN exactly where the column holds a NaN, and all three operators match the reference; the
    two means also match the float entries over the dequantized tensors bit for bit."""
    block = 128
    qs, scs = make(k, block, seed=7)
    q, sc = qs[0], scs[0]
    one, two, three = 2 * (k // 4) + 0, 2 * (k // 4) + 1, 2 * (k // 4) + 2
    sc[one, 2] = np.nan
    sc[two, 0] = np.inf
    q[two, :block:3] = 0
    sc[three, 3] = 0.0
    q[three, 3 * block:4 * block] = -5
    eng = get_engine()
    trims, keeps = (0, 1, (k - 1) // 2), (1, k - 2 * (k // 5), k)
    dq, ds, srt = run_all(k, block, qs, scs, trims, keeps)
    x = dequant(q, sc, block)
    assert np.signbit(x[three, 3 * block]) and x[three, 3 * block] == 0
    blk2 = slice(2 * block, 3 * block)
    med = eng.coord_median_q8(dq, ds, block)[0].cpu().numpy()
    assert np.array_equal(np.isnan(med), np.isnan(x).any(axis=0)) and np.isnan(med[blk2]).all()
    assert np.isfinite(eng.coord_trimmed_mean_q8(dq, ds, 1, block)[0].cpu().numpy()[blk2]).all()
    assert np.isnan(eng.coord_trimmed_mean_q8(dq, ds, 0, block)[0].cpu().numpy()[blk2]).all()
    deq = [[eng.weighted_sum_q8([[a]], [[b]], SUM, None, block)[0] for a, b in zip(cq, cs)] for cq, cs in zip(dq, ds)]
    for b in trims:
        check(eng.coord_trimmed_mean_q8(dq, ds, b, block), [t.cpu().numpy() for t in eng.coord_trimmed_mean(deq, b)],
              f"float entry, trim {b}")
    for keep in keeps:
        check(eng.coord_mean_around_median_q8(dq, ds, keep, block),
              [t.cpu().numpy() for t in eng.coord_mean_around_median(deq, keep)], f"float entry, keep {keep}")


def test_too_many_clients_is_refused():
    k = 129
    q = [[torch.zeros(16, dtype=torch.int8, device="cuda") for _ in range(k)]]
    sc = [[torch.ones(1, dtype=torch.float32, device="cuda") for _ in range(k)]]
    with pytest.raises(ValueError, match="exceed 128"):
        get_engine().coord_median_q8(q, sc, 16)
