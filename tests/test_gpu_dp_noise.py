"""The device noise generator (include/fedagg_dp.h) against the numpy restatement (tests/dpcases.py):
the words bit for bit (known answers, the 2^32 block carry, the anchor), the deviates within the
header's bound of a float64 evaluation from the same words, their rounding into every dtype, the
independence of the bits from alignment, layout and K, the moments, in place, and scale 0."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dpcases as D  # noqa: E402
import edgecases as E  # noqa: E402
from test_gpu_geometric_median import DEV, same_bits  # noqa: E402

from fedml_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu

MECHS = ["gaussian", "laplace"]
ALL_DT = [torch.float32, torch.bfloat16, torch.float16, torch.float64]
SIZES = [1, 5, 0, 1024, 1027, 3 * 1024 + 5]
IDS = [3, 0, 9, 1, 2, 0xFFFFFFFF]
SEED, ROUND = D.ANCHOR_SEED, D.ANCHOR_ROUND


@pytest.fixture(scope="module")
def eng():
    from fedml_amd.engine import get_engine
    return get_engine(0)


def dev_words(eng, seed, rnd, seg, first, nb):
    w = eng.noise_words(seed, rnd, seg, first, nb)
    torch.cuda.synchronize()
    return w.cpu().numpy().view(np.uint32)


def noise(eng, mech, scale, sizes, ids, dt=torch.float32, seed=SEED, rnd=ROUND, offset=0):
    """The noise itself (no input) into fresh segments; offset 1: views one element into a larger
    allocation (unaligned for every dtype)."""
    outs = [torch.full((n + offset,), 7.0, dtype=dt, device=DEV)[offset:] for n in sizes]
    eng.add_noise(None, mech, scale, seed, rnd, ids, outs=outs)
    torch.cuda.synchronize()
    return [o.cpu() for o in outs]


@pytest.mark.parametrize("counter,key,out", D.KAT)
def test_words_known_answers(eng, counter, key, out):
    seed, rnd, seg, first = D.kat_args(counter, key)
    assert tuple(int(x) for x in dev_words(eng, seed, rnd, seg, first, 1)[0]) == out


def test_words_carry_and_anchor(eng):
    first = 2 ** 32 - 2
    assert (dev_words(eng, SEED, 3, 7, first, 4) == D.words(SEED, 3, 7, first, 4)).all()
    assert (dev_words(eng, SEED, ROUND, D.ANCHOR_SEG, 0, 600) == D.words(SEED, ROUND, D.ANCHOR_SEG, 0, 600)).all()
    base = dev_words(eng, SEED, ROUND, 0, 0, 8)
    for other in (dev_words(eng, SEED ^ 1, ROUND, 0, 0, 8), dev_words(eng, SEED ^ (1 << 63), ROUND, 0, 0, 8),
                  dev_words(eng, SEED, ROUND + 1, 0, 0, 8), dev_words(eng, SEED, ROUND, 1, 0, 8)):
        assert (other != base).mean() > 0.9
    assert dev_words(eng, SEED, ROUND, 0, 5, 0).shape == (0, 4)


@pytest.mark.parametrize("mech", MECHS)
def test_deviates_within_the_headers_bound(eng, mech):
    got = noise(eng, mech, 1.0, SIZES, IDS)
    worst = 0.0
    for n, sid, t in zip(SIZES, IDS, got):
        ref = D.z64(mech, SEED, ROUND, sid, n)
        assert t.shape == (n,)
        if n:
            worst = max(worst, float(np.abs(t.double().numpy() - ref).max()))
    print(f"{mech}: max |t - z64| = {worst:.3e} (bound {N.NOISE_Z_ABS_ERR:.1e})")
    assert worst <= N.NOISE_Z_ABS_ERR


@pytest.mark.parametrize("scale", [1.0, 0.37])
@pytest.mark.parametrize("mech", MECHS)
def test_rounding_into_every_dtype(eng, mech, scale):
    """t = rnd((A)scale * (A)z): float64 widens the float32 z, the 16-bit types round the float32
    product once."""
    z = noise(eng, mech, 1.0, SIZES, IDS)
    for dt in ALL_DT:
        got = noise(eng, mech, scale, SIZES, IDS, dt)
        for a, zz in zip(got, z):
            ref = zz.double() * scale if dt == torch.float64 else (zz * torch.tensor(scale, dtype=torch.float32)).to(dt)
            assert same_bits(a, ref), (mech, dt)


@pytest.mark.parametrize("dt", ALL_DT, ids=str)
@pytest.mark.parametrize("mech", MECHS)
def test_bits_do_not_depend_on_the_path(eng, mech, dt):
    """Aligned (vector path) against a view offset by one element (element path); the fused sum over
    K = 1 and K = 9 all-zero clients, flat and tiled."""
    n, sid, scale = 4100, 5, 0.75
    a, = noise(eng, mech, scale, [n], [sid], dt)
    b, = noise(eng, mech, scale, [n], [sid], dt, offset=1)
    assert same_bits(a, b)
    El = N.TILE_BYTES // a.element_size()
    for k in (1, 9):
        zeros = [[torch.zeros(n, dtype=dt, device=DEV) for _ in range(k)]]
        f, = eng.centered_sum_noise(zeros, None, [1.0 / k] * k, mech, scale, SEED, ROUND, [sid])
        buf = torch.zeros(-(-n // El), k + 2, El, dtype=dt, device=DEV)
        t = eng.centered_sum_noise_tiled(buf, list(range(1, k + 1)), None, [1.0 / k] * k, mech, scale, SEED, ROUND,
                                         sid, n=n)
        torch.cuda.synchronize()
        assert same_bits(f, a) and same_bits(t, a), (k,)


@pytest.mark.parametrize("mech", MECHS)
def test_moments(eng, mech):
    z, = noise(eng, mech, 1.0, [1 << 20], [D.ANCHOR_SEG])
    z = z.double().numpy()
    assert np.abs(z).max() <= (5.77 if mech == "gaussian" else 15.95)
    for name, err, bound in D.moment_checks(mech, z):
        print(f"{mech} {name}: {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (mech, name, err, bound)


@pytest.mark.parametrize("dt", ALL_DT, ids=str)
def test_add_in_place_and_scale_zero(eng, dt):
    g = torch.Generator().manual_seed(11)
    xs = [torch.randn(n, generator=g, dtype=torch.float64).to(dt) for n in SIZES]
    for offset in (0, 1):
        def dev():
            return [torch.empty(x.numel() + offset, dtype=dt, device=DEV)[offset:].copy_(x) for x in xs]
        src = dev()
        out = eng.add_noise(src, "gaussian", 0.5, SEED, 2, IDS)
        same = dev()
        assert eng.add_noise(same, "gaussian", 0.5, SEED, 2, IDS, outs=same)[0] is same[0]
        t = noise(eng, "gaussian", 0.5, SIZES, IDS, dt, rnd=2, offset=offset)
        torch.cuda.synchronize()
        for x, s, o, i, tt in zip(xs, src, out, same, t):
            assert same_bits(s, x)  # the input is only read
            assert same_bits(o, x + tt) and same_bits(i, o)
    # scale 0: the input's bits, -0, NaN and denormals included
    tab = E.edge_columns(dt)
    for offset in (0, 1):
        src = torch.empty(tab.numel() + offset, dtype=dt, device=DEV)[offset:].copy_(tab)
        out, = eng.add_noise([src], "laplace", 0.0, SEED, 1, [0])
        eng.add_noise([src], "laplace", 0.0, SEED, 1, [0], outs=[src])
        zero, = noise(eng, "laplace", 0.0, [tab.numel()], [0], dt, offset=offset)
        torch.cuda.synchronize()
        assert same_bits(out, tab) and same_bits(src, tab)
        assert same_bits(zero, torch.zeros(tab.numel(), dtype=dt))
