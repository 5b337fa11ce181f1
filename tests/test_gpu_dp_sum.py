"""The fused clipped-sum-and-noise kernel (fa_centered_sum_noise, include/fedagg_dp.h) against
compositions of kernels the tree already tests, bit for bit: at scale 0 it is fa_sign_vote_sum at
threshold 0 (edge values included), at scale > 0 fa_add_noise applied to that result.  K below, at and
above the load group (8) and into a second partial group; sizes of one element, one slot, ragged slots
and an empty segment, aligned and offset by one element; with a center, without one, in place; flat
and tiled."""
from __future__ import annotations

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edgecases as E  # noqa: E402
from test_gpu_geometric_median import DEV, coefs, normal_data, same_bits, segments, tiled_buf  # noqa: E402

from fedml_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu

KS = [1, 7, 8, 9, 19]
ALL_DT = [torch.float32, torch.bfloat16, torch.float16, torch.float64]
MECHS = ["gaussian", "laplace"]
SEED, ROUND = 0xFEDCBA9876543210, 4


@pytest.fixture(scope="module")
def eng():
    from fedml_amd.engine import get_engine
    return get_engine(0)


def sizes_of(dt):
    el = N.TILE_BYTES // torch.empty((), dtype=dt).element_size()
    return [1, 5, 0, 1024, 1027, 3 * 1024 + 5, 2 * el + 5]


def centers(c, sizes, offset):
    return [col[0] for col in segments(c[None], sizes, offset)]


def same_noised(a, b, y, nan_rows):
    """a == b bit for bit.  ``nan_rows`` (the edge tables): where y is NaN both must be NaN and the
    bits are compared everywhere else.  y + t with one NaN returns that NaN, but the y the fused kernel
    holds is the outcome of its own chain of adds, and the tables have columns in which NaNs of both
    signs meet in one add: IEEE 754 (6.2.3) leaves which of two NaN operands propagates to the
    implementation, the hardware takes the first source, and the compiler may commute every add in
    every instantiation of the kernel.  (At scale 0 every element is compared, NaNs included.)"""
    if not nan_rows:
        return same_bits(a, b)
    nan = torch.isnan(y.cpu())
    a, b = a.cpu(), b.cpu()
    return bool(torch.isnan(a[nan]).all() and torch.isnan(b[nan]).all()) and same_bits(a[~nan], b[~nan])


def check(eng, x, c, sizes, offset, coef, what, nan_rows=False):
    """Every mechanism and scale 0 over one data set: with a center (when given), in place, without."""
    ids = list(range(10, 10 + len(sizes)))
    segs = segments(x, sizes, offset)
    for cen in ([None] if c is None else [None, c]):
        cens = None if cen is None else centers(cen, sizes, offset)
        y, _ = eng.sign_vote_sum(segs, cens, coef, 0)
        got0 = eng.centered_sum_noise(segs, cens, coef, "gaussian", 0.0, SEED, ROUND, ids)
        torch.cuda.synchronize()
        for s, (a, b) in enumerate(zip(got0, y)):
            assert same_bits(a, b), (what, "scale 0", cen is not None, s)
        for mech in MECHS:
            exp = eng.add_noise(y, mech, 0.3, SEED, ROUND, ids)
            got = eng.centered_sum_noise(segs, cens, coef, mech, 0.3, SEED, ROUND, ids)
            torch.cuda.synchronize()
            for s, (a, b) in enumerate(zip(got, exp)):
                assert same_noised(a, b, y[s], nan_rows), (what, mech, cen is not None, s)
            if cens is not None:  # d_out == d_center
                inpl = centers(cen, sizes, offset)
                eng.centered_sum_noise(segs, inpl, coef, mech, 0.3, SEED, ROUND, ids, outs=inpl)
                torch.cuda.synchronize()
                for s, (a, b) in enumerate(zip(inpl, exp)):
                    assert same_noised(a, b, y[s], nan_rows), (what, mech, "in place", s)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dt", ALL_DT, ids=str)
def test_fused_equals_the_composition(eng, dt, k):
    g = torch.Generator().manual_seed(900 + k)
    sizes = sizes_of(dt)
    for offset in (0, 1):
        x = normal_data(g, k, sum(sizes), dt)
        c = normal_data(g, 1, sum(sizes), dt)[0]
        check(eng, x, c, sizes, offset, coefs(g, k), f"normal k={k} {dt} offset={offset}")


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dt", ALL_DT, ids=str)
def test_edge_values(eng, dt, k):
    """Rows holding NaN, +-Inf, -0, the largest values and denormals (tests/edgecases.py); the center
    is client 0's row of another draw, so it holds them too."""
    el = N.TILE_BYTES // torch.empty((), dtype=dt).element_size()
    n = el + 2 * E.edge_columns(dt).numel() * 4 + 3
    x = torch.stack(E.clients(dt, k, n, 77 + k))
    c = E.clients(dt, max(k, 2), n, 5)[1]
    # 1.7 overflows the largest value, 0.0 meets Inf, the negative weight comes late
    coef = [0.155, 0.845, 0.3, 1.7, 0.0, 0.25, 0.125, 0.06, 0.5, 0.033, -0.25, 0.41, 0.077, 0.001, 0.999, 0.64, 0.02,
            0.5, 0.25][:k]
    for offset in (0, 1):
        check(eng, x, c, [n], offset, coef, f"edge k={k} {dt} offset={offset}", nan_rows=True)


@pytest.mark.parametrize("k", [1, 9])
@pytest.mark.parametrize("dt", ALL_DT, ids=str)
def test_tiled_equals_flat(eng, dt, k):
    g = torch.Generator().manual_seed(950 + k)
    el = N.TILE_BYTES // torch.empty((), dtype=dt).element_size()
    n = 3 * el + 17
    buf, rows, x, _ = tiled_buf(g, normal_data, k, k + 3, n, dt)
    c = normal_data(g, 1, n, dt)[0].to(DEV)
    coef = coefs(g, k)
    segs = segments(x, [n], 0)
    for cen in (None, c):
        for mech, scale in (("gaussian", 0.0), ("gaussian", 0.3), ("laplace", 0.3)):
            f, = eng.centered_sum_noise(segs, None if cen is None else [cen], coef, mech, scale, SEED, ROUND, [6])
            t = eng.centered_sum_noise_tiled(buf, rows, cen, coef, mech, scale, SEED, ROUND, 6, n=n)
            torch.cuda.synchronize()
            assert t.shape == (n,) and same_bits(t, f), (mech, scale, cen is not None)
    cc = c.clone()
    t = eng.centered_sum_noise_tiled(buf, rows, cc, coef, "laplace", 0.3, SEED, ROUND, 6, n=n, out=cc)
    torch.cuda.synchronize()
    assert same_bits(cc, f)
