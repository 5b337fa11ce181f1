"""CPU only.  What tests/test_gpu_edge_values.py holds the HIP kernels against, pinned on the same
edge-value tables (tests/edgecases.py): the C oracle == the reference's literal torch loop for every
dtype x mode x K, == the host-resident twin of the kernels (host_sum.h); orc.mix == the per-operation
torch row loop; orc.sgd_apply == torch.optim.SGD.  Every comparison is bitwise (refcases.bits_equal:
NaN matches NaN, zero signs and infinities count).

The second half checks the tables themselves, on the reference's output alone: the cases still
produce a NaN from non-NaN inputs, infinities from finite inputs, subnormals, -0.0, both accumulate
ties and the double-rounding columns.  These are conditions on the inputs, so that a later edit of
the tables cannot empty the GPU test without a failure here."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import pytest
import torch

import edgecases as E
from edgecases import MUL_N_DIV_N, MUL_W, SUM, mismatches
from refcases import bits_equal, torch_mix_reference

MODES = [MUL_W, MUL_N_DIV_N, SUM]
BIG = 1 << 40


# ------------------------------------------------------------------ the helpers
def test_round_once_is_the_types_rounding():
    """round_once == numpy's float64 -> float16 and torch's float32 -> bfloat16 conversions."""
    g = np.random.default_rng(0)
    v = g.standard_normal(100_000) * np.exp2(g.integers(-30, 18, 100_000))
    with np.errstate(over="ignore"):
        assert np.array_equal(E.round_once(v, torch.float16), v.astype(np.float16).astype(np.float64))
    v32 = (v * 2.0 ** 100).astype(np.float32)
    v32 = np.concatenate([v32, (v * 2.0 ** -120).astype(np.float32)])
    exp = torch.from_numpy(v32).to(torch.bfloat16).double().numpy()
    assert np.array_equal(E.round_once(v32.astype(np.float64), torch.bfloat16), exp)


def test_double_rounding_search():
    """float16: float32(155 / 1000) times 1675, 1775, 1875 and 1975 rounds differently once and
    twice; torch (the reference) gives the twice-rounded value.  bfloat16: the searched pair has hits."""
    assert E.double_rounding_counts(torch.float16) == (155, 845)
    hits = E.double_rounding_inputs(torch.float16, np.float32(0.155))
    assert {1675.0, 1775.0, 1875.0, 1975.0} <= set(hits.tolist())
    for dt in (torch.float16, torch.bfloat16):
        c = np.float32(E.double_rounding_counts(dt)[0] / 1000)
        cols = torch.tensor(E.double_rounding_columns(dt), dtype=torch.float64).to(dt)
        assert cols.numel() >= 4 and set(cols.tolist()) <= set(E.double_rounding_inputs(dt, c).tolist())
        once, twice = E.product_roundings(cols, c)
        assert np.all(once != twice)
        assert np.array_equal((cols * float(c)).double().numpy(), twice)


@pytest.mark.parametrize("dtype", E.DTYPES, ids=str)
def test_table_holds_the_edges(dtype):
    tab = E.edge_columns(dtype)
    L = tab.numel()
    assert L % 2 == 1 and L % 3 and L % 17
    if dtype == torch.int64:
        want = [0, 1, -1, 2 ** 24 + 1, -(2 ** 24 + 1), 2 ** 24 + 3, 2 ** 53 + 1, 2 ** 62, 2 ** 63 - 1, -2 ** 63,
                2 ** 31, 123_456_789_012_345]
        assert set(want) <= set(tab.tolist())
        return
    fi = torch.finfo(dtype)
    d = tab.double()
    neg = torch.signbit(d)
    assert ((d == 0) & ~neg).any() and ((d == 0) & neg).any()
    assert (d == float("inf")).any() and (d == float("-inf")).any() and torch.isnan(d).any()
    assert (d == fi.max).any() and (d == -fi.max).any() and (d == fi.tiny).any()
    sub = d[(d.abs() > 0) & (d.abs() < fi.tiny)]
    assert (sub == fi.tiny * fi.eps).any() and sub.abs().unique().numel() >= 2
    p = 2.0 ** E._TIE_EXP[dtype]
    ties = E.tie_columns(dtype)
    assert float(d[ties["down"]]) == p and float(d[ties["up"]]) == p + 2
    assert (d == 1).any() and (d == 1 + fi.eps).any() and ((d - 1 / 3).abs() < fi.eps).any()
    if dtype == torch.float16:
        assert (d == 65504).sum() >= 2 and (d == 32768).any()
    if dtype == torch.bfloat16:
        assert (d > 3.2e38).any() and (d == 65536).any()
    # every table entry reaches every client (one holder per column in the odd repeats)
    n, K = E.size(dtype), 17
    j = torch.arange(n)
    odd = (j // L) % 2 == 1
    assert len({(int(a), int(b)) for a, b in zip((j % L)[odd], (j % K)[odd])}) == L * K


# ------------------------------------------------------------------ the references agree
@pytest.mark.parametrize("K", E.KS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", E.DTYPES, ids=str)
def test_oracle_equals_torch_chain(dtype, mode, K):
    xs, coef, div, exp = E.case(dtype, mode, K)
    ref = E.torch_chain(xs, mode, coef, div)
    assert exp.dtype == ref.dtype
    bad = mismatches(exp, ref)
    assert bad.numel() == 0, (bad.numel(), bad[:8].tolist())
    assert bits_equal(exp, ref)
    if exp.is_floating_point():
        assert torch.equal(torch.isnan(exp), torch.isnan(ref))


@pytest.mark.parametrize("K", E.KS)
@pytest.mark.parametrize("mode", MODES)
def test_host_twin_equals_oracle(mode, K):
    """host_sum.h (the CPU branch of the small host round) over a state_dict of all five tables."""
    from fedml_amd import _host
    names = {"w": torch.float32, "h": torch.bfloat16, "g": torch.float16, "d": torch.float64, "n": torch.int64}
    from oracle import orc
    dicts = [OrderedDict() for _ in range(K)]
    for name, dt in names.items():
        for d, x in zip(dicts, E.clients(dt, K, 8 * E.edge_columns(dt).numel() + 3, 300 + K)):
            d[name] = x
    # one coefficient list per round: float32's (float16's double-rounding pair has the same first weight)
    coef, div = E.coefficients(torch.float32, mode, K)
    exp = OrderedDict((name, orc.weighted_sum([d[name] for d in dicts], mode, coef, div)) for name in names)
    got = _host.small_host_round(dicts, list(names), mode, None if coef is None else [float(c) for c in coef], div,
                                 0, 0, 0, 0, BIG, cpu_max_bytes=BIG)
    assert got is not None and list(got) == list(names)
    for name in names:
        assert got[name].dtype == exp[name].dtype
        bad = mismatches(got[name], exp[name])
        assert bad.numel() == 0, (name, bad.numel(), bad[:8].tolist())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=str)
@pytest.mark.parametrize("name", list(E.mix_matrices()))
def test_oracle_mix_equals_torch_rows(name, dtype):
    xs, rp, cs, vs, post, exp, exp2 = E.mix_case(name, dtype)
    ref, ref2 = torch_mix_reference(xs, rp, cs, vs, post)
    for r, (a, b) in enumerate(zip(exp + exp2, ref + ref2)):
        assert bits_equal(a, b), (name, dtype, r, mismatches(a, b)[:8].tolist())
    rows = torch.stack([e.double() for e in exp + exp2])
    assert torch.isnan(rows).any() and torch.isinf(rows).any()
    assert ((rows == 0) & torch.signbit(rows)).any()


@pytest.mark.parametrize("flags", list(E.SGD_FLAGS))
def test_oracle_sgd_equals_torch_optimizer(flags):
    """orc.sgd_apply == torch.optim.SGD with edge values in the parameter, the averaged clients and
    (at the later step) the momentum buffer."""
    from oracle import orc
    momentum, dampening, wd, nesterov = E.SGD_FLAGS[flags]
    n = E.size(torch.float32)
    _, _, _, avg = E.case(torch.float32, MUL_W, E.STEP_K, n)
    p0, b0 = E.step_state(n)
    p_ref, b_ref = p0.clone(), torch.zeros(n)
    pt = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SGD([pt], lr=0.3, momentum=momentum, dampening=dampening, weight_decay=wd, nesterov=nesterov)
    for step in range(2):
        if step == 1 and momentum:
            b_ref.copy_(b0)
            opt.state[pt]["momentum_buffer"].copy_(b0)
        orc.sgd_apply(avg, p_ref, b_ref if momentum else None, 0.3, momentum, dampening, wd, nesterov, step == 0)
        pt.grad = pt.detach() - avg
        opt.step()
        assert bits_equal(pt.detach(), p_ref), (step, mismatches(pt.detach(), p_ref)[:8].tolist())
        if momentum:
            assert bits_equal(opt.state[pt]["momentum_buffer"], b_ref), step


# ------------------------------------------------------------------ the tables reach the edges
def census(xs, exp):
    """What the expected output of a float case holds, and how it got there."""
    x = torch.stack([t.double() for t in xs])
    e = exp.double()
    clean = ~torch.isnan(x).any(0)
    finite = torch.isfinite(x).all(0)
    tiny = torch.finfo(exp.dtype).tiny
    return {
        "nan_made": int((torch.isnan(e) & clean).sum()),
        "pinf_made": int(((e == float("inf")) & finite).sum()),
        "ninf_made": int(((e == float("-inf")) & finite).sum()),
        "subnormal": int(((e != 0) & (e.abs() < tiny)).sum()),
        "neg_zero": int(((e == 0) & torch.signbit(e)).sum()),
    }


@pytest.mark.parametrize("K", E.KS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", E.FLOAT_DTYPES, ids=str)
def test_cases_reach_the_edges(dtype, mode, K):
    """On the reference output alone.  Where a property cannot occur the reason is in the condition:
    one client cannot cancel (no NaN from Inf - Inf) and its weight 0.155 cannot overflow; from K = 17
    on the weighted form has a negative weight, so a column of -0.0 sums to +0.0."""
    xs, coef, div, exp = E.case(dtype, mode, K)
    c = census(xs, exp)
    if K >= 3:
        assert c["nan_made"] > 0, c
        assert c["pinf_made"] > 0 and c["ninf_made"] > 0, c
    if K == 1 and mode == MUL_N_DIV_N and dtype != torch.float64:
        assert c["pinf_made"] > 0 and c["ninf_made"] > 0, c  # max * 155 overflows before the divide
    assert c["subnormal"] > 0, c
    if not (mode == MUL_W and K == 17):
        assert c["neg_zero"] > 0, c
    if mode == SUM and K >= 3:
        tab = E.edge_columns(dtype)
        L = tab.numel()
        j = torch.arange(exp.numel())
        odd = (j // L) % 2 == 1
        p = 2.0 ** E._TIE_EXP[dtype]
        down = exp[odd & (j % L == E.tie_columns(dtype)["down"])].double()
        up = exp[odd & (j % L == E.tie_columns(dtype)["up"])].double()
        assert down.numel() > 0 and bool((down == p).all()), down      # 2^p + 1 -> 2^p, the even neighbour
        assert up.numel() > 0 and bool((up == p + 4).all()), up        # 2^p + 3 -> 2^p + 4
        if dtype == torch.float16:                                    # 65504 + 16: the tie below 2^16 -> Inf
            top = exp[odd & (j % L == 16)].double()
            assert top.numel() > 0 and bool((top == float("inf")).all())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=str)
def test_double_rounding_columns_reach_the_output(dtype):
    """MUL_W, one client: the output IS the rounded product.  At least 4 distinct inputs round
    differently once and twice, and the reference holds the twice-rounded value there."""
    xs, coef, _, exp = E.case(dtype, MUL_W, 1)
    once, twice = E.product_roundings(xs[0], np.float32(coef[0]))
    differ = (once != twice) & ~np.isnan(once)
    assert np.unique(xs[0].double().numpy()[differ]).size >= 4
    assert np.array_equal(exp.double().numpy()[differ], twice[differ])
    assert not np.array_equal(exp.double().numpy()[differ], once[differ])
    for K in E.KS[1:]:  # and with more clients there are columns where some product differs
        xs, coef, _, _ = E.case(dtype, MUL_W, K)
        assert int(E.double_rounding_column_mask(xs, coef, dtype).sum()) >= 4


def test_int64_cases_reach_the_edges():
    tab = E.edge_columns(torch.int64)
    inexact = [v for v in tab.tolist() if int(np.float32(v)) != v]
    assert len(inexact) >= 4                                     # int64 -> float32 rounds (2^24 + 1, 2^63 - 1, ...)
    assert float(np.float32(2 ** 24 + 1)) == 2.0 ** 24 and float(np.float32(2 ** 24 + 3)) == 2.0 ** 24 + 4
    for K in E.KS:
        xs, coef, _, _ = E.case(torch.int64, MUL_N_DIV_N, K)
        wraps = sum(int(not -2 ** 63 <= int(v) * int(c) < 2 ** 63) for x, c in zip(xs, coef) for v in x[:13].tolist())
        assert wraps > 0                                         # x * n wraps before the float divide
        assert (K < 3) == (max(coef) < 2 ** 24)                  # counts that float32 cannot hold
    xs, _, _, exp = E.case(torch.int64, SUM, 3)
    exact = [sum(int(x[j]) for x in xs) for j in range(13)]
    assert any(not -2 ** 63 <= v < 2 ** 63 for v in exact)       # the SUM wraps
    assert exp[:13].tolist() == [(v + 2 ** 63) % 2 ** 64 - 2 ** 63 for v in exact]


def test_restated_fma_is_exact():
    """test_gpu_drivers._fma32 (the fused multiply-adds of the RMSprop restatement that the GPU test
    compares with) == the C library's correctly rounded fmaf over every triple of float32 edge values;
    a product on a float32 tie with an addend far below it is where a plain float64 sum goes wrong."""
    import ctypes
    from test_gpu_drivers import _fma32
    libm = ctypes.CDLL("libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    vals = torch.cat([E.edge_columns(torch.float32), torch.tensor([10.0, -10.0, -0.01, 0.3, 0.1])])
    a, b, c = (t.reshape(-1).contiguous() for t in torch.meshgrid(vals, vals, vals, indexing="ij"))
    exp = torch.tensor([libm.fmaf(*t) for t in zip(a.tolist(), b.tolist(), c.tolist())], dtype=torch.float32)
    assert mismatches(_fma32(a, b, c), exp).numel() == 0
    plain = (a.double() * b.double() + c.double()).float()
    assert mismatches(plain, exp).numel() > 0  # the table holds such triples
