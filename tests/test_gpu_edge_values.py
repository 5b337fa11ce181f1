"""The kernels of fedagg.hip on directed edge values (tests/edgecases.py): signed zeros, infinities,
NaN, the largest values, subnormals, accumulate ties, overflowing products, float16 / bfloat16 inputs
whose weighted product rounds differently once and twice, int64 values that float32 cannot hold,
wrapping int64 products and sums, counts of 2^24 and more.

Every entry is compared with the C oracle -- which tests/test_edge_values_cpu.py pins to the
reference's torch loop on these very tables -- bit for bit over every element: no tolerance, NaN
against NaN the only licence (NaN payloads are not part of the contract).  Sizes are two tiles of the
widest kernel shape plus a ragged tail; a view one element off alignment takes the whole tensor down
the scalar path; K = 1, 3, 9, 17 (17 passes one load group of U = 16 and enters the prefetch loop of
the double-buffered variants)."""
from __future__ import annotations

import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

import edgecases as E
from edgecases import MUL_N_DIV_N, MUL_W, SUM, assert_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = [MUL_W, MUL_N_DIV_N, SUM]
TILE_BYTES = 4096  # one arena tile


@pytest.fixture(scope="module")
def eng():
    from fedml_amd.engine import get_engine
    return get_engine(0)


def off_by_one(x):
    """A device copy of x one element past a 16-byte boundary."""
    base = torch.zeros(x.numel() + 8, dtype=x.dtype, device=DEV)
    view = base[1:1 + x.numel()]
    view.copy_(x)
    return view


@functools.lru_cache(maxsize=None)
def device_clients(dtype, K, aligned=True):
    """The clients of E.case(dtype, *, K) on the device (the modes share them); read only."""
    xs = E.case(dtype, SUM, K)[0]
    return [x.to(DEV) if aligned else off_by_one(x) for x in xs]


def arena(xs, capacity, rows):
    """Flat CPU tensors as a [tiles, capacity, E] tile-interleaved device group; client j -> row rows[j],
    the other rows and the padding hold 7 (nothing may read them into a result)."""
    dt, n = xs[0].dtype, xs[0].numel()
    El = TILE_BYTES // xs[0].element_size()
    nt = max(1, -(-n // El))
    buf = torch.full((nt, capacity, El), 7, dtype=dt)
    for j, x in enumerate(xs):
        flat = torch.full((nt * El,), 7, dtype=dt)
        flat[:n] = x
        buf[:, rows[j], :] = flat.view(nt, El)
    return buf.to(DEV)


def scattered(K):
    return [2 * (K - 1 - j) + 1 for j in range(K)], 2 * K + 1  # reverse order, every other row


# ------------------------------------------------------------------ fa_weighted_sum, every variant
@pytest.mark.parametrize("variant", range(9))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", E.DTYPES, ids=str)
def test_weighted_sum_every_variant(eng, dtype, mode, variant):
    try:
        eng.set_variant(variant)
        for K in E.KS:
            _, coef, div, exp = E.case(dtype, mode, K)
            for aligned in (True, False):
                got = eng.weighted_sum(device_clients(dtype, K, aligned), mode, coef, div)
                assert got.dtype == exp.dtype
                assert_bits(got, exp, f"variant {variant} K={K} {'aligned' if aligned else 'offset view'}", dtype)
    finally:
        eng.set_variant(0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", E.DTYPES, ids=str)
def test_weighted_sum_multi_segments(eng, dtype, mode):
    """One launch over an aligned segment, an offset view and a segment shorter than a tile."""
    from oracle import orc
    short_n = 3 * E.edge_columns(dtype).numel() + 2
    for K in E.KS:
        _, coef, div, exp = E.case(dtype, mode, K)
        short = E.clients(dtype, K, short_n, 400 + K)
        segs = [device_clients(dtype, K), device_clients(dtype, K, False), [x.to(DEV) for x in short]]
        outs = eng.weighted_sum_multi(segs, mode, coef, div)
        for s, e in enumerate([exp, exp, orc.weighted_sum(short, mode, coef, div)]):
            assert_bits(outs[s], e, f"K={K} segment {s}", dtype)


# ------------------------------------------------------------------ the tiled arena forms
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", E.DTYPES, ids=str)
def test_weighted_sum_tiled(eng, dtype, mode):
    """fa_weighted_sum_tiled and fa_weighted_sum_tiled_multi (two ranges, the second ragged), on the
    automatic shape, the four-slot shape and a double-buffered one."""
    El = TILE_BYTES // torch.empty(0, dtype=dtype).element_size()
    for K in E.KS:
        xs, coef, div, exp = E.case(dtype, mode, K)
        n = xs[0].numel()
        rows, cap = scattered(K)
        buf = arena(xs, cap, rows)
        for variant in (0, 6, 7):
            try:
                eng.set_variant(variant)
                got = eng.weighted_sum_tiled(buf, rows, mode, coef, div, n=n)
                ranges = [(0, 3 * El), (3 * El, n)]
                outs = [torch.empty(hi - lo, dtype=exp.dtype, device=DEV) for lo, hi in ranges]
                eng.weighted_sum_tiled_multi(buf, rows, mode, coef, div, ranges, outs)
            finally:
                eng.set_variant(0)
            assert_bits(got, exp, f"tiled K={K} variant {variant}", dtype)
            assert_bits(torch.cat(outs), exp, f"tiled_multi K={K} variant {variant}", dtype)


@pytest.mark.parametrize("layout", ["rows", "tiled"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", E.FLOAT_DTYPES, ids=str)
def test_weighted_sum_pair(eng, dtype, mode, layout):
    """A float table and the int64 table in one launch (the coefficients are the float type's)."""
    from oracle import orc
    for K in E.KS:
        xs, coef, div, exp = E.case(dtype, mode, K)
        cs = E.case(torch.int64, SUM, K)[0]
        exp_c = orc.weighted_sum(cs, mode, coef, div)
        rows, cap = scattered(K)
        if layout == "rows":
            bx = torch.full((cap, xs[0].numel()), 7, dtype=dtype)
            bc = torch.full((cap, cs[0].numel()), 7, dtype=torch.int64)
            for j, r in enumerate(rows):
                bx[r], bc[r] = xs[j], cs[j]
            got, got_c = eng.weighted_sum_pair(bx.to(DEV), bc.to(DEV), rows, mode, coef, div)
        else:
            got, got_c = eng.weighted_sum_pair(arena(xs, cap, rows), arena(cs, cap, rows), rows, mode, coef, div,
                                               n=xs[0].numel(), n_i64=cs[0].numel())
        assert got_c.dtype == exp_c.dtype
        assert_bits(got, exp, f"pair {layout} K={K} float group", dtype)
        assert_bits(got_c, exp_c, f"pair {layout} K={K} int64 group", torch.int64)


# ------------------------------------------------------------------ two-level sums
GROUP_PTR = [0, 4, 5, 13, 17]


@functools.lru_cache(maxsize=None)
def grouped_case(dtype, mode, gmode):
    """Clients, coefficients and the expectation formed from two levels of oracle calls."""
    from oracle import orc
    K = GROUP_PTR[-1]
    xs, coef, div, _ = E.case(dtype, mode, K)
    gcoef = [0.3, 1.7, 2.0, 0.01] if gmode == MUL_W else [11, 7, 3, 5]
    gdiv = [26.0, 26.0, 13.0, 7.0]
    terms = []
    for j, (a, b) in enumerate(zip(GROUP_PTR, GROUP_PTR[1:])):
        G = orc.weighted_sum(xs[a:b], mode, None if coef is None else coef[a:b], div)
        if gmode == MUL_W:
            G = orc.weighted_sum([G], MUL_W, [gcoef[j]])
        elif gmode == MUL_N_DIV_N:
            G = orc.weighted_sum([G], MUL_N_DIV_N, [gcoef[j]], gdiv[j])
        terms.append(G)
    return xs, coef, div, gcoef, gdiv, orc.weighted_sum(terms, SUM)


@pytest.mark.parametrize("mode,gmode", [(MUL_W, MUL_W), (MUL_W, MUL_N_DIV_N), (MUL_W, SUM), (SUM, SUM),
                                        (MUL_N_DIV_N, MUL_N_DIV_N)])
@pytest.mark.parametrize("dtype", E.FLOAT_DTYPES, ids=str)
def test_weighted_sum_grouped(eng, dtype, mode, gmode):
    xs, coef, div, gcoef, gdiv, exp = grouped_case(dtype, mode, gmode)
    K = len(xs)
    gc = gcoef if gmode != SUM else None
    gd = gdiv if gmode == MUL_N_DIV_N else None
    got = eng.weighted_sum_grouped(device_clients(dtype, K), mode, coef, div, GROUP_PTR, gmode, gc, gd)
    assert_bits(got, exp, "grouped", dtype)
    got = eng.weighted_sum_grouped(device_clients(dtype, K, False), mode, coef, div, GROUP_PTR, gmode, gc, gd)
    assert_bits(got, exp, "grouped, offset views", dtype)
    rows, cap = scattered(K)
    got = eng.weighted_sum_grouped_tiled(arena(xs, cap, rows), rows, mode, coef, div, GROUP_PTR, gmode, gc, gd,
                                         n=xs[0].numel())
    assert_bits(got, exp, "grouped_tiled", dtype)


# ------------------------------------------------------------------ the one-workgroup host round
@pytest.mark.parametrize("K", E.KS)
@pytest.mark.parametrize("mode", MODES)
def test_host_round_one_workgroup(mode, K):
    """CPU state_dicts of five edge tables through _host.small_host_round -> fa_weighted_sum_host
    (k_wsum_host1); with one client the float32 key is long enough for a second trip of the grid."""
    from fedml_amd import _host
    from fedml_amd.ml.aggregator import state_dict_agg as sda
    from oracle import orc
    names = {"w": torch.float32, "h": torch.bfloat16, "g": torch.float16, "d": torch.float64, "n": torch.int64}
    dicts = [OrderedDict() for _ in range(K)]
    for name, dt in names.items():
        n = 140_001 if (K == 1 and name == "w") else 8 * E.edge_columns(dt).numel() + 3
        for d, x in zip(dicts, E.clients(dt, K, n, 300 + K)):
            d[name] = x
    coef, div = E.coefficients(torch.float32, mode, K)
    coef = None if coef is None else [float(c) for c in coef]
    engine = sda.get_engine(None)
    fn, err, ctx = engine.host_round_abi()
    with engine.lock:
        got = _host.small_host_round(dicts, list(names), mode, coef, div, fn, err, ctx, 0, 4 << 20)
    assert got is not None and list(got) == list(names)
    for name, dt in names.items():
        exp = orc.weighted_sum([d[name] for d in dicts], mode, coef, div)
        assert got[name].device.type == "cpu" and got[name].dtype == exp.dtype
        assert_bits(got[name], exp, f"host round key {name}", dt)


# ------------------------------------------------------------------ mixing rows
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=str)
@pytest.mark.parametrize("name", list(E.mix_matrices()))
def test_mix(eng, name, dtype):
    """Both matrices on the banded kernel (the engine's default takes either) and on k_mix<4,3> (the
    band switched off), with and without the post-scale, aligned and off alignment."""
    from fedml_amd.engine import AggEngine
    xs, rp, cs, vs, post, exp, exp2 = E.mix_case(name, dtype)
    general = AggEngine(0)
    try:
        general.set_mix_band(False)
        for engine, kernel in ((eng, "band"), (general, "general")):
            for aligned in (True, False):
                dxs = [x.to(DEV) if aligned else off_by_one(x) for x in xs]
                for scale in (None, post):
                    outs, outs2 = engine.mix(dxs, rp, cs, vs, scale)
                    what = f"{name} {kernel} {'aligned' if aligned else 'offset'} {'post' if scale else 'plain'}"
                    for r in range(len(exp)):
                        assert_bits(outs[r], exp[r], f"{what} row {r}", dtype)
                        if scale:
                            assert_bits(outs2[r], exp2[r], f"{what} row {r} post-scaled", dtype)
    finally:
        general.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=str)
def test_pushsum_device_omega(eng, dtype):
    """fa_pushsum with omegas whose mixed value makes float32(1 / omega') subnormal, +Inf, NaN, -Inf
    and zero, against the float32 chain of refcases.oracle_pushsum."""
    from refcases import oracle_pushsum
    rp, cs, vs, num_in = E.PUSHSUM_ROWS
    rows, n = len(rp) - 1, E.mix_size(dtype)
    xs = E.clients(dtype, num_in, n, 500)
    omega = torch.tensor(E.PUSHSUM_OMEGA, dtype=torch.float32)
    ex = [torch.empty(n, dtype=dtype) for _ in range(rows)]
    ez = [torch.empty(n, dtype=dtype) for _ in range(rows)]
    eom = torch.empty(rows, dtype=torch.float32)
    with np.errstate(all="ignore"):
        oracle_pushsum(xs, rp, cs, vs, omega, ex, ez, eom)
    inv = (1.0 / eom.double()).float()
    assert 0 < float(inv[0]) < torch.finfo(torch.float32).tiny and float(inv[1]) == float("inf")
    assert bool(torch.isnan(inv[2])) and float(inv[4]) == float("-inf") and float(inv[5]) == 0.0
    outs, outs2, om = eng.pushsum([x.to(DEV) for x in xs], rp, cs, vs, omega.to(DEV))
    assert_bits(om, eom, "omega'")
    for r in range(rows):
        assert_bits(outs[r], ex[r], f"x' row {r}", dtype)
        assert_bits(outs2[r], ez[r], f"z row {r}", dtype)


# ------------------------------------------------------------------ the fused FedAvg + server step
@pytest.mark.parametrize("flags", list(E.SGD_FLAGS))
def test_fedavg_sgd(eng, flags):
    """fa_fedavg_sgd == the oracle's FedAvg then its torch.optim.SGD step: edge tables in the clients
    and the parameter at the first step, in the momentum buffer too at the later one."""
    from oracle import orc
    momentum, dampening, wd, nesterov = E.SGD_FLAGS[flags]
    n, K = E.size(torch.float32), E.STEP_K
    xs, coef, _, avg = E.case(torch.float32, MUL_W, K)
    p0, b0 = E.step_state(n)
    p_ref, b_ref = p0.clone(), torch.zeros(n)
    p_gpu, b_gpu = p0.to(DEV), torch.zeros(n, device=DEV)
    for step in range(2):
        if step == 1:
            b_ref.copy_(b0)
            b_gpu.copy_(b0)
        orc.sgd_apply(avg, p_ref, b_ref if momentum else None, 0.3, momentum, dampening, wd, nesterov, step == 0)
        eng.fedavg_sgd([device_clients(torch.float32, K)], coef, [p_gpu], [b_gpu] if momentum else None, 0.3,
                       momentum, dampening, wd, nesterov, first_step=(step == 0))
        assert_bits(p_gpu, p_ref, f"parameter, step {step}", torch.float32)
        if momentum:
            assert_bits(b_gpu, b_ref, f"momentum buffer, step {step}", torch.float32)


@pytest.mark.parametrize("momentum,wd", [(0.0, 0.0), (0.9, 0.0), (0.5, 1e-3)])
def test_fedavg_rmsprop(eng, momentum, wd):
    """fa_fedavg_rmsprop against the correctly rounded restatement of torch.optim.RMSprop
    (test_gpu_drivers._rmsprop_cr): bitwise wherever the restatement is not NaN, NaN where it is."""
    from test_gpu_drivers import _rmsprop_cr
    n, K, lr, alpha, eps = E.size(torch.float32), E.STEP_K, 0.01, 0.99, 1e-8
    xs, coef, _, avg = E.case(torch.float32, MUL_W, K)
    p0, b0 = E.step_state(n)
    p_ref, sq_ref, buf_ref = p0.clone(), torch.zeros(n), torch.zeros(n)
    p_gpu, sq_gpu, buf_gpu = p0.to(DEV), torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    for step in range(2):
        if step == 1:  # edge values in the state of the later step (a square average is not negative)
            sq_ref, buf_ref = b0.abs(), torch.roll(b0, 5)
            sq_gpu.copy_(sq_ref)
            buf_gpu.copy_(buf_ref)
        p_ref, sq_ref, buf_ref = _rmsprop_cr(p_ref, avg, sq_ref, buf_ref, lr, alpha, eps, wd, momentum)
        eng.fedavg_rmsprop([device_clients(torch.float32, K)], coef, [p_gpu], [sq_gpu],
                           [buf_gpu] if momentum else None, lr, alpha, eps, wd, momentum, first_step=(step == 0))
        assert_bits(p_gpu, p_ref, f"parameter, step {step}", torch.float32)
        assert_bits(sq_gpu, sq_ref, f"square average, step {step}", torch.float32)
        if momentum:
            assert_bits(buf_gpu, buf_ref, f"momentum buffer, step {step}", torch.float32)
