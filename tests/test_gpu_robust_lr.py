"""The robust learning rate on the device: the fused pass fa_sign_vote_sum (out bit for bit, and the
count of negated elements by value, equal to the per-op restatement below), its two identities with
the existing passes, hand-built boundary columns, wide votes, the in-place update, the tiled entry,
determinism, the raw entry's argument checks, and the defense built on it taken through every route
(separate tensors, client-major and tiled arenas, ServerAggregator + FedMLDefender with the global
model as the center) and through a backdoor scenario.

Shapes and data are the geometric median tests' (test_gpu_geometric_median.py).  A workgroup owns one
4-KiB slot per client -- E = 1024 float32 / 2048 16-bit / 512 float64 elements -- so besides SEGS and
SINGLE every dtype also runs TILE_SEGS = [E, 2 E + 5] (one whole aligned slot; two slots and a ragged
remainder) at element offsets 0 and 1 (offset 1: unaligned, every slot on the element path).

The 10 % - 90 % band on the restatement's share of negated elements at the third threshold
max(1, round(0.8 sqrt(K))) is asserted for every K >= 2 on ``voting_pair`` / ``voting_data`` (with a
center and without one): normal data around a narrow center in which a further quarter of the entries
sit AT the center and abstain.  With signs alone the band cannot hold at K = 3 -- the threshold is 1
and |net| is odd unless a client abstains, which ``normal_data``'s 6 % of zeros give in under 10 % of
the columns and a center in none -- and ``normal_pair``'s center is as wide as its data, so it decides
most signs itself once K is large (8 % negated at K = 129).  So ``normal_pair`` and the clustered data
(no random signs: without a center every client but one is positive, and in the 16-bit types the
cluster collapses onto the center) run for the equality with the restatement only, whatever share
they negate."""
from __future__ import annotations

import math
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_centered_clipping import OP, centered_cluster, normal_pair  # noqa: E402
from test_gpu_geometric_median import (DEV, SEGS, SINGLE, _cfg, _reset_defender, cluster_data, coefs,  # noqa: E402
                                       normal_data, same_bits, segments, tiled_buf)

from fedml_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu

F32_K = [1, 2, 8, 17, 32, 33, 65, 129, 150]
OTHER_K = [3, 40]
OTHER_DT = [torch.bfloat16, torch.float16, torch.float64]
ALL_DT = [torch.float32] + OTHER_DT


@pytest.fixture(scope="module")
def eng():
    from fedml_amd.engine import get_engine
    return get_engine(0)


def slot_elems(dt):
    return N.TILE_BYTES // torch.empty((), dtype=dt).element_size()


def thresholds(k):
    return sorted({0, 1, max(1, round(0.8 * math.sqrt(k))), k})


def third(k):
    return max(1, round(0.8 * math.sqrt(k)))


def parts(x, c, coef):
    """The contract up to the vote's use, per op, with torch CPU ops in the storage dtype: x [k, n],
    c [n] or None.  Returns (acc, net): the ordered sum of t_i = rnd(u_i * coef_i) and the exact
    integer net vote.  Differences and sums are the dtype's own ops (float32 math rounded once for the
    16-bit types); the product is op-type math with the coefficient cast to the op type, rounded once."""
    dt, a = x.dtype, OP[x.dtype]
    cf = torch.tensor(list(coef), dtype=torch.float64).to(a)
    acc = None
    net = torch.zeros(x.shape[1], dtype=torch.int64)
    for i in range(x.shape[0]):
        u = x[i] - c if c is not None else x[i]
        net += (u > 0).to(torch.int64) - (u < 0).to(torch.int64)  # +-0 and NaN: neither holds
        t = (u.to(a) * cf[i]).to(dt)
        acc = t if acc is None else acc + t
    return acc, net


def finish(acc, net, c, threshold):
    flip = net.abs() < threshold
    acc = torch.where(flip, -acc, acc)
    return (c + acc if c is not None else acc), int(flip.sum()), flip


def restate(x, c, coef, threshold):
    """(out, flipped) of the contract in include/fedagg_robust.h."""
    out, flipped, _ = finish(*parts(x, c, coef), c, threshold)
    return out, flipped


def run_flat(eng, x, c, sizes, offset, coef, ths, what, inplace=False, band=None):
    """Every threshold of ``ths`` over one set of device segments; returns {threshold: (out, flipped)}."""
    segs = segments(x, sizes, offset)
    acc, net = parts(x, c, coef)
    got = {}
    for th in ths:
        cens = None if c is None else [col[0] for col in segments(c[None], sizes, offset)]
        outs, flipped = eng.sign_vote_sum(segs, cens, coef, th, outs=cens if inplace else None)
        torch.cuda.synchronize()
        out = torch.cat([o.reshape(-1) for o in outs]).cpu()
        ref, nref, _ = finish(acc, net, c, th)
        assert flipped.dtype == torch.int64 and tuple(flipped.shape) == (1,)
        if band is not None and th == band:
            share = nref / x.shape[1]
            print(f"{what} threshold={th}: the restatement negates {share:.3f} of the elements")
            assert 0.10 <= share <= 0.90, (what, th, share)
        assert same_bits(out, ref), (what, th)
        assert int(flipped.item()) == nref, (what, th, int(flipped.item()), nref)
        got[th] = (out, int(flipped.item()))
    xs = torch.stack([torch.cat([col[i] for col in segs]) for i in range(x.shape[0])]).cpu()
    assert same_bits(xs, x), what  # the inputs are only read
    return got


def voting_pair(g, k, n, dt):
    """Normal data around a center 0.05 wide (a center as wide as the data would decide most signs
    by itself), a further quarter of the entries AT the center: random signs and frequent abstentions,
    so every net vote is reachable for every K (odd ones included)."""
    x = normal_data(g, k, n, dt)
    c = (0.05 * torch.randn(n, generator=g, dtype=torch.float64)).to(dt)
    at = torch.rand(k, n, generator=g) < 0.25
    x[at] = c[None, :].expand(k, n)[at]
    return x, c


def voting_data(g, k, n, dt):
    x = normal_data(g, k, n, dt)
    x[torch.rand(k, n, generator=g) < 0.25] = 0.0
    return x


def none_pair(make):
    def f(g, k, n, dt):
        return make(g, k, n, dt), None
    f.__name__ = make.__name__ + "_no_center"
    return f


def layouts(dt):
    e = slot_elems(dt)
    return ((SEGS, (0, 1)), ([SINGLE], (0,)), ([e, 2 * e + 5], (0, 1)))


def _flat_cases(eng, k, dt, seed):
    g = torch.Generator().manual_seed(seed)
    ths = thresholds(k)
    for make in (normal_pair, centered_cluster, voting_pair, none_pair(voting_data), none_pair(cluster_data)):
        random_signs = "voting" in make.__name__
        for sizes, offsets in layouts(dt):
            for offset in offsets:
                x, c = make(g, k, sum(sizes), dt)
                run_flat(eng, x, c, sizes, offset, coefs(g, k), ths,
                         f"{make.__name__} k={k} {dt} n={sum(sizes)} offset={offset}",
                         band=third(k) if k >= 2 and random_signs else None)


@pytest.mark.parametrize("k", F32_K)
def test_fused_pass_f32(eng, k):
    _flat_cases(eng, k, torch.float32, 2100 + k)


@pytest.mark.parametrize("k", OTHER_K)
@pytest.mark.parametrize("dt", OTHER_DT, ids=str)
def test_fused_pass_dtypes(eng, dt, k):
    _flat_cases(eng, k, dt, 2200 + k)


# ----------------------------------------------------------------------------- the two identities
@pytest.mark.parametrize("dt,k", [(torch.float32, 17), (torch.float32, 40), (torch.bfloat16, 3)], ids=str)
def test_threshold_zero_is_the_existing_pass(eng, dt, k):
    from fedml_amd.engine import MUL_W
    g = torch.Generator().manual_seed(2300 + k)
    for sizes, offset in layouts(dt)[0:1] + layouts(dt)[2:3]:
        for off in offset:
            x, c = normal_pair(g, k, sum(sizes), dt)
            x[k - 1, 11] = float("nan")  # NaNs included
            c[13] = float("nan")
            coef = coefs(g, k)
            segs = segments(x, sizes, off)
            cens = [col[0] for col in segments(c[None], sizes, off)]
            outs, flipped = eng.sign_vote_sum(segs, cens, coef, 0)
            exp, _ = eng.centered_sum_sqdist(segs, cens, coef)
            torch.cuda.synchronize()
            assert all(same_bits(a, b) for a, b in zip(outs, exp)) and int(flipped.item()) == 0
            outs, flipped = eng.sign_vote_sum(segs, None, coef, 0)
            exp = eng.weighted_sum_multi(segs, MUL_W, coef)
            torch.cuda.synchronize()
            assert all(same_bits(a, b) for a, b in zip(outs, exp)) and int(flipped.item()) == 0
            assert bool(torch.cat(outs)[11].isnan())


# ----------------------------------------------------------------------------- boundary columns
def _boundary(k, dt):
    """Hand-built columns for threshold 3: (x [k, n], c [n], flips [n], nan [n], name [n]).  Every value
    is exact in every dtype, so u_i = x_i - c is the value written down here."""
    inf, nan = float("inf"), float("nan")
    cols = []  # (name, c, u_0 .. u_{k-1} as x = c + u given directly, flips)

    def col(name, c, xs, flips):
        assert len(xs) == k
        cols.append((name, c, xs, flips))

    def votes(p, m, c=1.0):  # p clients above the center, m below, the rest AT it
        return [c + 0.5] * p + [c - 0.5] * m + [c] * (k - p - m)

    for p, flips in ((2, True), (3, False), (4, False)):  # |net| = theta - 1, theta, theta + 1: < not <=
        col(f"net=+{p}", 1.0, votes(p, 0), flips)
        col(f"net=-{p}", 1.0, votes(0, p), flips)
    col("net=+3 of 4 up 1 down", 1.0, votes(4, 1), False)
    col("net=+2 of 4 up 2 down", 1.0, votes(4, 2), True)
    col("every x == c", 1.0, votes(0, 0), True)  # every vote 0
    col("zeros around +0", 0.0, [0.0, -0.0] * (k // 2) + [0.0] * (k % 2), True)
    col("zeros around -0", -0.0, [-0.0, 0.0] * (k // 2) + [-0.0] * (k % 2), True)
    col("+0 and -0 beside three up", 0.0, [0.5, 0.5, 0.5, -0.0, 0.0] + [-0.0] * (k - 5), False)
    col("+0 and -0 beside two up", 0.0, [0.5, 0.5, -0.0, 0.0] + [0.0] * (k - 4), True)
    col("NaN beside three up", 1.0, [nan] + votes(3, 0)[:k - 1], False)  # the NaN votes 0; out is NaN
    col("NaN beside two up", 1.0, [nan] + votes(2, 0)[:k - 1], True)
    col("+Inf beside two up", 1.0, [inf] + votes(2, 0)[:k - 1], False)  # the Inf votes +1: net 3
    col("+Inf beside one up", 1.0, [inf] + votes(1, 0)[:k - 1], True)
    col("-Inf beside two down", 1.0, votes(0, 2)[:k - 1] + [-inf], False)
    col("-Inf beside one down", 1.0, votes(0, 1)[:k - 1] + [-inf], True)
    # all-negative values, three of them negated (an odd count): out = c - acc stays negative, where
    # -(c + acc) would be positive
    col("negative, 3 up 3 down", -8.0, votes(3, 3, -8.0), True)
    col("negative, 2 up", -8.0, votes(2, 0, -8.0), True)
    col("negative, 2 down 1 up", -4.0, votes(1, 2, -4.0), True)
    col("negative, 4 down", -8.0, votes(0, 4, -8.0), False)
    x = torch.tensor([xs for _, _, xs, _ in cols], dtype=torch.float64).t().contiguous().to(dt)
    c = torch.tensor([cv for _, cv, _, _ in cols], dtype=torch.float64).to(dt)
    flips = torch.tensor([f for _, _, _, f in cols])
    return x, c, flips, [name for name, _, _, _ in cols]


@pytest.mark.parametrize("k", [6, 7])
@pytest.mark.parametrize("dt", ALL_DT, ids=str)
def test_boundary_columns(eng, dt, k):
    x, c, flips, names = _boundary(k, dt)
    n = x.shape[1]
    coef = [0.05 * (i + 1) for i in range(k)]  # unequal, so a column with as many up as down sums to non-zero
    neg = [i for i, name in enumerate(names) if name.startswith("negative")]
    assert sum(bool(flips[i]) for i in neg) == 3
    for centered in (True, False):
        # without a center the same columns are read as updates: u = x - c is formed on the host (exact)
        xs = x if centered else (x.double() - c.double()[None, :]).to(dt)
        cc = c if centered else None
        acc, net = parts(xs, cc, coef)
        ref, nref, mask = finish(acc, net, cc, 3)
        assert torch.equal(mask, flips), [names[i] for i in range(n) if mask[i] != flips[i]]  # the restatement itself
        segs = segments(xs, [n], 0)
        outs, flipped = eng.sign_vote_sum(segs, None if cc is None else [cc.to(DEV)], coef, 3)
        torch.cuda.synchronize()
        out = outs[0].cpu()
        isn = ref.isnan()
        assert [names[i] for i in range(n) if isn[i]] == ["NaN beside three up", "NaN beside two up"]
        assert torch.equal(out.isnan(), isn)  # a NaN: compared by isnan, not by bits
        bad = [names[i] for i in range(n) if not isn[i] and not same_bits(out[i:i + 1], ref[i:i + 1])]
        assert not bad, (bad, centered)
        assert int(flipped.item()) == nref == int(flips.sum())
        inf = {name: float(out[i]) for i, name in enumerate(names) if "Inf" in name}
        assert inf == {"+Inf beside two up": math.inf, "+Inf beside one up": -math.inf,
                       "-Inf beside two down": -math.inf, "-Inf beside one down": math.inf}
        if centered:
            assert all(float(out[i]) < 0 for i in neg)  # the flip came before c + acc
            assert float(out[names.index("every x == c")]) == 1.0


# ----------------------------------------------------------------------------- wide votes
@pytest.mark.parametrize("k", [129, 300])
def test_wide_votes(eng, k):
    """|net| = K must not be negated at threshold K, |net| = K - 2 must: a vote counter narrower than K
    (8 bits: 129 -> -127, 300 -> 44) fails one of the two."""
    g = torch.Generator().manual_seed(2400 + k)
    n = 4096 + 17
    x = torch.rand(k, n, generator=g) + 0.1
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    x = x * sign[None, :]  # every client agrees: net = +-K
    odd = torch.rand(n, generator=g) < 0.4
    who = torch.randint(0, k, (n,), generator=g)
    idx = torch.nonzero(odd).reshape(-1)
    x[who[idx], idx] *= -1.0  # one client against: net = +-(K - 2)
    coef = coefs(g, k)
    for c in (None, torch.zeros(n)):
        acc, net = parts(x, c, coef)
        assert torch.equal(net.abs(), torch.where(odd, k - 2, k))
        ref, nref, mask = finish(acc, net, c, k)
        assert torch.equal(mask, odd) and 0 < nref < n
        got = run_flat(eng, x, c, [n], 0, coef, [k], f"wide k={k} center={c is not None}")[k]
        assert got[1] == int(odd.sum())
        assert torch.equal(torch.sign(got[0]), torch.where(odd, -sign, sign))  # sum coef = 1, every |x| >= 0.1


def test_count_over_more_than_1024_workgroups(eng):
    """k_sign_vote_count is one workgroup of 1,024 lanes striding over the workgroups' counts; every
    other case here has at most twenty of them.  n = 2049 * 1024 + 5 float32 elements are 2,050
    workgroups, so each lane takes three strides: the count equals the restatement's exactly and out
    matches bit for bit."""
    k, n = 3, 2049 * 1024 + 5
    assert -(-n // slot_elems(torch.float32)) > 2 * 1024
    g = torch.Generator().manual_seed(2450)
    x, c = voting_pair(g, k, n, torch.float32)
    got = run_flat(eng, x, c, [n], 0, coefs(g, k), [third(k)], f"count k={k} n={n}", band=third(k))
    assert 0 < got[third(k)][1] < n


# ----------------------------------------------------------------------------- in place, tiled, determinism
@pytest.mark.parametrize("dt,k", [(torch.float32, 8), (torch.float32, 40), (torch.bfloat16, 3)], ids=str)
def test_in_place_equals_separate_buffers(eng, dt, k):
    g = torch.Generator().manual_seed(2500 + k)
    for sizes, offsets in layouts(dt):
        for offset in offsets:
            x, c = normal_pair(g, k, sum(sizes), dt)
            coef = coefs(g, k)
            ths = [0, third(k)]
            sep = run_flat(eng, x, c, sizes, offset, coef, ths, f"separate k={k} {dt}")
            inp = run_flat(eng, x, c, sizes, offset, coef, ths, f"in place k={k} {dt}", inplace=True)
            for th in ths:
                assert same_bits(sep[th][0], inp[th][0]) and sep[th][1] == inp[th][1]


@pytest.mark.parametrize("tiles", [3, 9], ids=["3E+17", "9E+17"])
@pytest.mark.parametrize("dt,k", [(torch.float32, 3), (torch.float32, 32), (torch.float32, 129),
                                  (torch.bfloat16, 40), (torch.float16, 3), (torch.float64, 3)], ids=str)
def test_tiled_equals_flat(eng, dt, k, tiles):
    g = torch.Generator().manual_seed(2600 + k + tiles)
    E = slot_elems(dt)
    n = tiles * E + 17  # not a multiple of the tile
    buf, rows, x, _ = tiled_buf(g, normal_data, k, k + 3, n, dt)  # a subset of the rows, out of order
    assert len(set(rows)) == k
    keep = buf.clone()
    x = x.contiguous()
    c = normal_data(g, 1, n, dt)[0]
    coef = coefs(g, k)
    for th in (0, third(k), k):
        for cen in (c, None):
            what = f"k={k} {dt} n={n} threshold={th} center={cen is not None}"
            cd = None if cen is None else cen.to(DEV)
            out_t, fl_t = eng.sign_vote_sum_tiled(buf, rows, cd, coef, th, n=n)
            flat = run_flat(eng, x, cen, [n], 0, coef, [th], "flat " + what)[th]
            torch.cuda.synchronize()
            assert out_t.shape == (n,) and same_bits(out_t.cpu(), flat[0]), what
            assert int(fl_t.item()) == flat[1], what
            if cd is not None:
                assert same_bits(cd.cpu(), cen)  # the center is only read
                out_i, fl_i = eng.sign_vote_sum_tiled(buf, rows, cd, coef, th, n=n, out=cd)  # in place
                assert out_i.data_ptr() == cd.data_ptr() and same_bits(cd.cpu(), flat[0]), what
                assert int(fl_i.item()) == flat[1], what
    # another order of the same rows is another client order: bit for bit the flat entry over it
    perm = torch.randperm(k, generator=g).tolist()
    out_p, fl_p = eng.sign_vote_sum_tiled(buf, [rows[j] for j in perm], c.to(DEV), [coef[j] for j in perm], third(k), n=n)
    ref, nref = restate(x[perm], c, [coef[j] for j in perm], third(k))
    assert same_bits(out_p.cpu(), ref) and int(fl_p.item()) == nref
    # a subset of them
    sub = list(range(0, k, 2))
    out_s, fl_s = eng.sign_vote_sum_tiled(buf, [rows[j] for j in sub], None, [coef[j] for j in sub], 1, n=n)
    ref, nref = restate(x[sub], None, [coef[j] for j in sub], 1)
    assert same_bits(out_s.cpu(), ref) and int(fl_s.item()) == nref
    assert same_bits(buf.cpu(), keep.cpu())  # the arena is only read
    # nothing to read: the count is written as 0
    for cen in (c[:0].to(DEV), None):
        out0, fl0 = eng.sign_vote_sum_tiled(buf, rows, cen, coef, third(k), n=0)
        assert out0.numel() == 0 and int(fl0.item()) == 0


def test_all_segments_empty_writes_zero(eng):
    empty = [[torch.empty(0, device=DEV) for _ in range(3)] for _ in range(2)]
    fl = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    L = N.lib()
    rc = L.fa_sign_vote_sum(eng._ctx, N.F32, 2, N.i64_array([0, 0]), 3, N.ptr_array([0] * 6), None,
                            N.f64_array([0.2, 0.3, 0.5]), 2, N.ptr_array([0, 0]), fl.data_ptr(), None)
    assert rc == N.FA_OK, L.fa_last_error()
    torch.cuda.synchronize()
    assert int(fl.item()) == 0
    outs, flipped = eng.sign_vote_sum(empty, None, [0.2, 0.3, 0.5], 2)
    assert int(flipped.item()) == 0 and all(o.numel() == 0 for o in outs)


def test_same_call_gives_the_same_bits(eng):
    g = torch.Generator().manual_seed(26)
    for k in (17, 33):
        x, c = normal_pair(g, k, sum(SEGS) + SINGLE, torch.float32)
        segs = segments(x, SEGS + [SINGLE], 0)
        cens = [col[0] for col in segments(c[None], SEGS + [SINGLE], 0)]
        coef = coefs(g, k)
        for cn in (cens, None):
            runs = [eng.sign_vote_sum(segs, cn, coef, third(k)) for _ in range(2)]
            torch.cuda.synchronize()
            assert all(same_bits(a, b) for a, b in zip(runs[0][0], runs[1][0]))
            assert int(runs[0][1].item()) == int(runs[1][1].item()) > 0


# ----------------------------------------------------------------------------- argument checks
def _raw(eng, entry, dtype, sizes, k, in_ptrs, cen_ptrs, coef, threshold, out_ptrs, flipped_ptr,
         tile_stride=N.TILE_BYTES):
    L = N.lib()
    args = [eng._ctx, dtype, len(sizes), N.i64_array(sizes), k, N.ptr_array(in_ptrs)]
    args += [tile_stride] if entry.endswith("_tiled") else []
    args += [None if cen_ptrs is None else N.ptr_array(cen_ptrs), None if coef is None else N.f64_array(coef),
             threshold, None if out_ptrs is None else N.ptr_array(out_ptrs), flipped_ptr, None]
    return getattr(L, entry)(*args), L.fa_last_error()


@pytest.mark.parametrize("entry", ["fa_sign_vote_sum", "fa_sign_vote_sum_tiled"])
def test_entry_rejects_bad_arguments(eng, entry):
    K, NUMEL = 3, 8
    xs = [torch.ones(1024, device=DEV) for _ in range(K)]
    cen = torch.zeros(NUMEL, device=DEV)
    out = torch.full((NUMEL,), 7.0, device=DEV)
    fl = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    good = [x.data_ptr() for x in xs]

    def call(dtype=N.F32, numel=NUMEL, k=K, ptrs=good, cens=(cen.data_ptr(),), coef=(0.2, 0.3, 0.5), threshold=2,
             outs=(out.data_ptr(),), flp=fl.data_ptr(), tile_stride=N.TILE_BYTES):
        return _raw(eng, entry, dtype, [numel], k, ptrs, None if cens is None else list(cens), coef, threshold,
                    None if outs is None else list(outs), flp, tile_stride=tile_stride)

    def named(err):
        return err.startswith(entry.encode() + b":")

    for cens in ((cen.data_ptr(),), None):  # with a center and without one
        for bad in (-1, K + 1):
            rc, err = call(cens=cens, threshold=bad)
            assert rc == N.FA_ERR_INVALID and b"threshold" in err and named(err), err
        rc, err = call(cens=cens, coef=None)
        assert rc == N.FA_ERR_INVALID and b"coef" in err and named(err), err
        rc, err = call(cens=cens, dtype=N.I64)
        assert rc == N.FA_ERR_DTYPE and named(err), err
        rc, err = call(cens=cens, k=0)
        assert rc == N.FA_ERR_INVALID and named(err), err
        rc, err = call(cens=cens, outs=None)
        assert rc == N.FA_ERR_INVALID and named(err), err
        rc, err = call(cens=cens, ptrs=[good[0], None, good[2]])
        assert rc == N.FA_ERR_INVALID and b"input NULL" in err and named(err), err
        rc, err = call(cens=cens, numel=-NUMEL)
        assert rc == N.FA_ERR_INVALID and named(err), err
        if entry.endswith("_tiled"):
            for bad in (1000, 0, -4096):
                rc, err = call(cens=cens, tile_stride=bad)
                assert rc == N.FA_ERR_INVALID and b"tile_stride" in err and named(err), err
    rc, err = call(cens=(None,))  # d_center given, a non-empty segment's center NULL
    assert rc == N.FA_ERR_INVALID and b"center NULL" in err and named(err), err
    # the documented order: coef before the threshold before the dtype before a segment's center
    rc, err = call(coef=None, threshold=-1, dtype=N.I64, cens=(None,))
    assert rc == N.FA_ERR_INVALID and b"coef" in err, err
    rc, err = call(threshold=-1, dtype=N.I64, cens=(None,))
    assert rc == N.FA_ERR_INVALID and b"threshold" in err, err
    rc, err = call(dtype=N.I64, cens=(None,))
    assert rc == N.FA_ERR_DTYPE, err
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and int(fl.item()) == 7  # nothing was launched
    rc, err = call(flp=None)  # d_flipped NULL is accepted
    assert rc == N.FA_OK, err
    torch.cuda.synchronize()
    assert bool((out == 1.0).all()) and int(fl.item()) == 7  # three votes up: 0 + (0.2 + 0.3 + 0.5), not negated
    out.fill_(7.0)
    rc, err = call(threshold=K)
    assert rc == N.FA_OK, err
    torch.cuda.synchronize()
    assert bool((out == 1.0).all()) and int(fl.item()) == 0


def test_engine_argument_checks(eng):
    xs = [torch.zeros(8, device=DEV) for _ in range(3)]
    c = torch.zeros(8, device=DEV)
    w = [0.2, 0.3, 0.5]
    with pytest.raises(ValueError):
        eng.sign_vote_sum([], None, [], 0)
    with pytest.raises(ValueError):
        eng.sign_vote_sum([xs], [c], [0.5, 0.5], 1)
    with pytest.raises(ValueError):
        eng.sign_vote_sum([xs], [c], None, 1)
    with pytest.raises(TypeError):
        eng.sign_vote_sum([[x.long() for x in xs]], None, w, 1)
    for bad in (-1, 4, 1.0, True, None):
        with pytest.raises(ValueError, match="threshold"):
            eng.sign_vote_sum([xs], [c], w, bad)
    with pytest.raises(ValueError):
        eng.sign_vote_sum([xs], [c, c], w, 1)
    with pytest.raises(ValueError, match="center"):
        eng.sign_vote_sum([xs], [c.double()], w, 1)
    with pytest.raises(ValueError, match="center"):
        eng.sign_vote_sum([xs], [torch.zeros(7, device=DEV)], w, 1)
    with pytest.raises(ValueError):
        eng.sign_vote_sum([xs], [c.cpu()], w, 1)
    with pytest.raises(ValueError):
        eng.sign_vote_sum([xs], [c], w, 1, outs=[torch.zeros(7, device=DEV)])
    buf = torch.zeros(2, 4, 1024, device=DEV)
    c2 = torch.zeros(2048, device=DEV)
    with pytest.raises(ValueError):
        eng.sign_vote_sum_tiled(buf, [0, 1], c2, [1.0], 1)
    with pytest.raises(IndexError):
        eng.sign_vote_sum_tiled(buf, [0, 4], c2, [0.5, 0.5], 1)
    with pytest.raises(ValueError, match="threshold"):
        eng.sign_vote_sum_tiled(buf, [0, 1], c2, [0.5, 0.5], 3)
    with pytest.raises(ValueError, match="center"):
        eng.sign_vote_sum_tiled(buf, [0, 1], c2[:2047], [0.5, 0.5], 1)
    with pytest.raises(ValueError):
        eng.sign_vote_sum_tiled(buf, [0, 1], c2, [0.5, 0.5], 1, out=torch.zeros(7, device=DEV))


# ----------------------------------------------------------------------------- arena and defense, end to end
def _mixed_model(g):
    """Two float dtypes and an int64 counter: a bfloat16 Linear and a float32 BatchNorm."""
    m = torch.nn.Sequential(torch.nn.Linear(40, 130).to(torch.bfloat16), torch.nn.BatchNorm1d(130))
    with torch.no_grad():
        for v in m.state_dict().values():
            if v.dtype.is_floating_point:
                v.copy_(torch.randn(v.shape, generator=g))
            else:
                v.fill_(1000)
    return m


def _mixed_clients(g, model, k):
    ds = []
    for i in range(k):
        sd = OrderedDict()
        for key, v in model.state_dict().items():
            if v.dtype.is_floating_point:
                sd[key] = (v.float() + 0.05 * torch.randn(v.shape, generator=g)).to(v.dtype).to(DEV)
            else:
                sd[key] = torch.tensor(100 + 7 * i, dtype=torch.int64, device=DEV)
        ds.append(sd)
    return ds


def _through_server_aggregator(model, raw, **kw):
    from fedml_amd.core.security.fedml_defender import FedMLDefender
    from fedml_amd.ml.aggregator.default_aggregator import DefaultServerAggregator
    try:
        agg = DefaultServerAggregator(model, _cfg(enable_defense=True, defense_type="robust_lr", **kw))
        kept, _ = agg.on_before_aggregation(raw)
        assert len(kept) == len(raw) and all(a is b for (_, a), (_, b) in zip(kept, raw))
        out = agg.aggregate(kept)
        d = FedMLDefender.get_instance()
        return out, d.get_malicious_client_idxs(), d.defender.last_info
    finally:
        _reset_defender()


def _pack(arena, sd):
    packed = {dt: torch.zeros(n, dtype=dt, device=DEV) for dt, n in arena.layout.group_numel.items()}
    for key in arena.layout.keys:
        dt, off, _, n = arena.layout.where[key]
        packed[dt][off:off + n].copy_(sd[key].reshape(-1))
    return packed


def _restate_dicts(ds, cen, coef, threshold):
    """The restatement per dtype group: the group's float keys concatenated in dict order."""
    groups = OrderedDict()
    for key, v in ds[0].items():
        if v.dtype.is_floating_point:
            groups.setdefault(v.dtype, []).append(key)
    out, flipped = {}, 0
    for dt, keys in groups.items():
        x = torch.stack([torch.cat([d[key].reshape(-1).cpu() for key in keys]) for d in ds])
        c = None if cen is None else torch.cat([cen[key].reshape(-1).cpu() for key in keys])
        o, f = restate(x, c, coef, threshold)
        flipped += f
        pos = 0
        for key in keys:
            n = ds[0][key].numel()
            out[key] = o[pos:pos + n].view(ds[0][key].shape)
            pos += n
    return out, flipped


def test_every_route_gives_the_restatement(eng, monkeypatch):
    from fedml_amd.arena import ClientArena, resident_rows
    from fedml_amd.core.security.defense.robust_lr_defense import RobustLearningRateDefense
    from fedml_amd.ml.aggregator.agg_operator import FedMLAggOperator
    g = torch.Generator().manual_seed(27)
    k, eta, th = 5, 0.3, 2
    model = _mixed_model(g)
    glob = OrderedDict((key, v.clone()) for key, v in model.state_dict().items())
    ds = _mixed_clients(g, model, k)
    fk = [key for key, v in ds[0].items() if v.dtype.is_floating_point]
    assert {ds[0][key].dtype for key in fk} == {torch.bfloat16, torch.float32} and len(fk) < len(ds[0])
    counts = [int(v) for v in torch.randint(20, 600, (k,), generator=g)]
    total = float(sum(counts))
    coef = [eta * float(n) / total for n in counts]  # eta n_i / N
    raw = list(zip(counts, ds))
    elements = sum(ds[0][key].numel() for key in fk)
    ref, nref = _restate_dicts(ds, glob, coef, th)
    plain, nplain = _restate_dicts(ds, None, coef, th)
    assert 0 < nref < elements
    kw = dict(robust_lr_threshold=th, robust_lr_server_lr=eta)
    base = FedMLAggOperator.agg(_cfg(), raw)

    def check(out, want, info, count, keys=None):
        for key in keys or list(ds[0]):
            if ds[0][key].dtype == torch.int64:  # the base aggregation's value
                assert out[key].dtype == base[key].dtype and torch.equal(out[key].cpu(), base[key].cpu())
            else:
                assert out[key].shape == ds[0][key].shape and same_bits(out[key].cpu(), want[key]), key
        assert info == {"flipped": count, "elements": elements}

    # separate tensors, a CPU center
    d = RobustLearningRateDefense(_cfg(**kw))
    out = d.defend_on_aggregation(raw, FedMLAggOperator.agg, glob)
    assert list(out) == list(ds[0]) and d.get_malicious_client_idxs() == []
    check(out, ref, d.last_info, nref)
    assert all(torch.equal(v, model.state_dict()[key]) for key, v in glob.items())  # the center is only read
    # without a dict, and with robust_lr_center="none": the plain form
    check(d.defend_on_aggregation(raw, FedMLAggOperator.agg, None), plain, d.last_info, nplain)
    dn = RobustLearningRateDefense(_cfg(robust_lr_center="none", **kw))
    check(dn.defend_on_aggregation(raw, FedMLAggOperator.agg, glob), plain, dn.last_info, nplain)
    assert not all(same_bits(ref[key], plain[key]) for key in fk)
    # the full route: get_model_params() is the center
    out, bad, info = _through_server_aggregator(model, raw, **kw)
    assert bad == [] and list(out) == list(ds[0])
    check(out, ref, info, nref)
    out, _, info = _through_server_aggregator(model, raw, robust_lr_center="none", **kw)
    check(out, plain, info, nplain)
    # CPU dicts in, CPU tensors out
    cpu = d.defend_on_aggregation([(n, OrderedDict((key, v.cpu()) for key, v in sd.items())) for n, sd in raw],
                                  FedMLAggOperator.agg, glob)
    assert all(v.device.type == "cpu" for v in cpu.values())
    check(cpu, ref, d.last_info, nref)
    with pytest.raises(TypeError):  # an int64 key and nothing to aggregate it with
        d.defend_on_aggregation(raw, extra_auxiliary_info=glob)
    with pytest.raises(ValueError, match="exceeds"):
        RobustLearningRateDefense(_cfg(robust_lr_threshold=k + 1)).defend_on_aggregation(raw, FedMLAggOperator.agg, glob)
    for badc in (OrderedDict((key, t) for key, t in glob.items() if key != "0.weight"),
                 OrderedDict((key, t.float() if key == "0.weight" else t) for key, t in glob.items()),
                 OrderedDict((key, t.reshape(-1) if key == "0.weight" else t) for key, t in glob.items())):
        with pytest.raises(ValueError, match="center"):
            d.defend_on_aggregation(raw, FedMLAggOperator.agg, badc)
    # the arenas hold the float keys
    fds = [OrderedDict((key, sd[key]) for key in fk) for sd in ds]
    fglob = OrderedDict((key, glob[key].to(DEV)) for key in fk)
    ta = ClientArena.for_model(fds[0], k + 2, device=DEV, tiled=True)
    rows = [(5 * i + 3) % (k + 2) for i in range(k)]
    for r, sd in zip(rows, fds):
        ta.write(r, sd)
    for center, want, count in ((_pack(ta, fglob), ref, nref), (None, plain, nplain)):
        info = {}
        keep = None if center is None else {dt: t.clone() for dt, t in center.items()}
        out = ta.sign_vote_sum(counts, th, eta, center=center, clients=rows, info=info)
        assert list(out) == fk
        check(out, want, info, count, fk)
        assert keep is None or all(same_bits(center[dt], keep[dt]) for dt in keep)  # the center is only read
    with pytest.raises(ValueError, match="center"):
        ta.sign_vote_sum(counts, th, eta, center={torch.float32: torch.zeros(3, device=DEV)}, clients=rows)
    with pytest.raises(ValueError, match="threshold"):
        ta.sign_vote_sum(counts, k + 1, eta, clients=rows)
    # a client-major arena, driven directly and found by the defense through the adopted rows
    copies = [OrderedDict((key, v.clone()) for key, v in sd.items()) for sd in fds]
    ca = ClientArena.for_model(copies[0], k, device=DEV)
    for i, sd in enumerate(copies):
        ca.adopt(i, sd)
    info = {}
    check(ca.sign_vote_sum(counts, th, eta, center=_pack(ca, fglob), info=info), ref, info, nref, fk)
    assert resident_rows(copies) is not None
    calls = []
    real = ClientArena.sign_vote_sum
    monkeypatch.setattr(ClientArena, "sign_vote_sum", lambda self, *a, **kw_: calls.append(a) or real(self, *a, **kw_))
    for center, want, count in ((glob, ref, nref), (None, plain, nplain)):
        out = d.defend_on_aggregation(list(zip(counts, copies)), extra_auxiliary_info=center)
        check(out, want, d.last_info, count, fk)
    assert len(calls) == 2
    assert all(same_bits(a[key], b[key]) for a, b in zip(copies, fds) for key in fk)  # the inputs are only read
    assert all(torch.equal(v, model.state_dict()[key]) for key, v in glob.items())


# ----------------------------------------------------------------------------- the attack scenario
def test_backdoor_coordinates_move_against_the_attackers(eng):
    """2 of 10 clients add +delta on 64 coordinates where the honest updates are symmetric noise (five
    up, three down by construction: with the attackers net = +4); elsewhere all ten share a sign.
    threshold 8: the attacked coordinates are negated -- FedAvg would move them towards the attackers
    -- and the agreed ones are FedAvg's."""
    from fedml_amd.core.security.defense.robust_lr_defense import RobustLearningRateDefense
    g = torch.Generator().manual_seed(28)
    k, n, nb, delta, th = 10, 2048, 64, 2.0, 8
    glob = torch.randn(n, generator=g)
    common = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    upd = (0.05 + 0.1 * torch.rand(k, n, generator=g)) * common[None, :]  # agreed coordinates: one sign
    att = torch.randperm(n, generator=g)[:nb]
    noise = 0.05 + 0.1 * torch.rand(k, nb, generator=g)
    for j in range(nb):  # the eight honest clients: five up, three down, who is which at random
        s = torch.tensor([1.0] * 5 + [-1.0] * 3)[torch.randperm(8, generator=g)]
        noise[:8, j] *= s
    upd[:, att] = noise
    upd[8:, att] = delta  # the attackers
    x = glob[None, :] + upd
    counts = [100] * k
    coef = [1.0 * float(c) / float(sum(counts)) for c in counts]
    ref, nref = restate(x, glob, coef, th)
    # float64 numpy over the updates the float32 restatement saw
    u = (x - glob[None, :]).double().numpy()
    fedavg = u.mean(axis=0)
    moved = (ref - glob).double().numpy()
    attacked = np.zeros(n, dtype=bool)
    attacked[att.numpy()] = True
    assert nref == nb
    assert np.all(fedavg[attacked] > 0.3)  # FedAvg follows the attackers: 2 * delta / 10 = 0.4, noise < 0.15
    assert np.all(moved[attacked] < -0.3)  # the defense moves the other way
    np.testing.assert_allclose(moved[attacked], -fedavg[attacked], rtol=0, atol=1e-5)
    np.testing.assert_allclose(moved[~attacked], fedavg[~attacked], rtol=0, atol=1e-5)
    assert np.all(np.sign(moved[~attacked]) == common.numpy()[~attacked])
    d = RobustLearningRateDefense(_cfg(robust_lr_threshold=th))
    out = d.defend_on_aggregation([(c, OrderedDict(w=x[i].to(DEV))) for i, c in enumerate(counts)],
                                  extra_auxiliary_info=OrderedDict(w=glob.to(DEV)))
    assert same_bits(out["w"].cpu(), ref) and d.last_info == {"flipped": nb, "elements": n}
