"""CPU side of the LCC decode cases (tests/lcccases.py): the numpy int64 reference == Python-int
arithmetic with the two's-complement wrap spelled out, and == the C oracle on every case of the
tiling grid, at the exactness limit, on the out-of-range inputs and on the adversarial ones; the
builders' own promises (stripes, the zero row, which (rows, k) straddle which constant, the moduli
at the float64 limit, the primes of the round trip); and the protocol round trip at 200 clients
through the oracle, so that nothing tests/test_gpu_lcc_decode.py asks of the HIP kernels rests on
an unchecked builder.  Every comparison is torch.equal on int64."""
from __future__ import annotations

import pytest
import torch

import lcccases as C

INT64 = (-2 ** 63, 2 ** 63 - 1)


def _orc(coef, F, p, n_out):
    from oracle import orc
    return orc.lcc_decode(coef, F, p, n_out)


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("p", [7, C.P15, C.P31, C.P61, C.P63])
def test_reference_equals_python_ints(p):
    """4 x 6 x 5 and smaller: in-range values, then the extremes of int64, so that single products and
    the running sum wrap (asserted), against _w64 on Python ints."""
    from fedml_amd.core.mpc.lightsecagg import _w64
    g = torch.Generator().manual_seed(p % 101)
    for rows, k, m in [(4, 6, 5), (1, 1, 1), (3, 2, 4)]:
        coef = torch.randint(0, p, (rows, k), generator=g, dtype=torch.int64)
        F = torch.randint(0, p, (k, m), generator=g, dtype=torch.int64)
        for extreme in (False, True):
            if extreme:
                F = C.adversarial(g, k * m, p).reshape(k, m)
                F[0, 0], F[k - 1, m - 1] = INT64
                coef[0, 0], coef[rows - 1, k - 1] = p - 1, -3
                wrapped = any(_w64(int(c) * int(f)) != int(c) * int(f) for c in coef[0].tolist() for f in F[:, 0].tolist())
                assert wrapped
            exp = torch.tensor(C.python_reference(coef.tolist(), F.tolist(), p), dtype=torch.int64).reshape(-1)
            assert torch.equal(C.reference(coef, F, p), exp), (p, rows, k, m, extreme)
            assert torch.equal(C.reference(coef, F, p, rows * m - 1), exp[:-1])
            assert bool((exp >= 0).all()) and bool((exp < p).all())


def test_reference_wraps_at_the_grid_primes():
    """What the grid's primes are for: no sum wraps at P15, every row with k >= 3 can at P31."""
    assert (C.P15 - 1) ** 2 * max(k for _, k in C.GRID) < 2 ** 53
    assert (C.P31 - 1) ** 2 * 3 >= 2 ** 63 > (C.P31 - 1) ** 2 * 2
    coef, F, ref = C.grid_case(9, 5, 257, C.P31)
    exact = [sum(int(c) * int(f) for c, f in zip(coef[8].tolist(), F[:, j].tolist())) for j in range(257)]
    assert max(exact) >= 2 ** 63  # the striped row's sums do wrap
    assert ref.reshape(9, 257)[8].tolist() != [e % C.P31 for e in exact]


@pytest.mark.parametrize("rows,k", C.GRID)
def test_grid_reference_equals_oracle(rows, k):
    for p in (C.P15, C.P31):
        for m in C.MS:
            coef, F, ref = C.grid_case(rows, k, m, p)
            assert coef.shape == (rows + C.EXTRA_ROWS, k) and F.shape == (k, m) and ref.numel() == rows * m
            full = _orc(coef, F, p, (rows + C.EXTRA_ROWS) * m)
            assert torch.equal(full[:rows * m], ref), (rows, k, m, p)
            assert torch.equal(full, C.reference(coef, F, p))
            for nrows, n_out in C.grid_runs(rows, m):
                assert torch.equal(_orc(coef[:nrows], F, p, n_out), ref[:n_out]), (rows, k, m, p, nrows, n_out)


# ------------------------------------------------------------------ the builders
def test_grid_straddles_the_constants():
    rows = {r for r, _ in C.GRID}
    ks = {k for _, k in C.GRID}
    assert {C.RB, C.RB + 1, C.RBF - 1, C.RBF, C.RBF + 1, 2 * C.RBF, 2 * C.RBF + 1} <= rows and 1 in rows
    assert {1, C.PF - 1, C.PF, C.PF + 1, C.LDS_I - 1, C.LDS_I, C.LDS_I + 1, C.LDS_I + C.PF - 1} <= ks
    assert {2 * C.LDS_I + 1, 300} <= ks and max(ks) > 2 * C.LDS_I  # a third LDS chunk
    assert len(C.GRID) == len(set(C.GRID)) == 25
    assert {1, C.BLOCK - 1, C.BLOCK, C.BLOCK + 1} <= set(C.MS) and max(C.MS) % C.BLOCK and max(C.MS) > 3 * C.BLOCK
    # the host case: a ragged last pass, a second chunk whose ring loads are clamped, a ragged block
    assert C.HOST_ROWS > C.RBF and C.HOST_ROWS % C.RBF and C.HOST_ROWS % C.RBF % C.RB == 0
    assert C.LDS_I < C.HOST_K < C.LDS_I + C.PF and C.HOST_M % C.BLOCK
    assert set(C.HOST_F_ROWS) == {0, C.LDS_I - 1, C.LDS_I, C.HOST_K - 1}
    assert set(C.HOST_F_COLS) == {0, 200, C.BLOCK - 1, C.BLOCK, C.HOST_M - 1} and 200 // 64 == 3
    assert (C.HOST_P - 1) ** 2 * C.HOST_K < 2 ** 53


@pytest.mark.parametrize("rows,k,m", [(1, 1, 1), (1, 3, 255), (9, 5, 257), (65, 257, 777)])
def test_grid_case_data(rows, k, m):
    for p in (C.P15, C.P31):
        coef, F, _ = C.grid_case(rows, k, m, p)
        for t in (coef, F):
            assert t.dtype == torch.int64 and int(t.min()) >= 0 and int(t.max()) == p - 1
        assert bool((coef[rows - 1] == p - 1).all()) and bool((coef[:rows, k - 1] == p - 1).all())
        zero = k // 2 if k >= 3 else None
        live = [i for i in range(k) if i != zero]
        assert bool((F[live, (m - 1) // 2] == p - 1).all())
        assert bool((F[k - 1] == p - 1).all())
        if zero is not None:
            assert bool((F[zero] == 0).all())
        again = C.striped(rows, k, m, p, seed=1000 * rows + k + 7 * m + p % 13)
        assert torch.equal(again[0], coef[:rows]) and torch.equal(again[1], F)  # deterministic


def test_grid_runs():
    assert C.grid_n_outs(33, 257) == [32 * 257 + 1, 33 * 257 - 5, 33 * 257]
    assert C.grid_n_outs(1, 1) == [1] and C.grid_n_outs(8, 1) == [3, 8]
    assert C.grid_runs(8, 1) == [(8, 3), (8, 8)]  # m <= 5: no extra coefficient rows
    runs = C.grid_runs(33, 257)
    assert len(runs) == 6 and {r for r, _ in runs} == {33, 35}
    for rows, m in [(33, 257), (65, 777), (1, 255)]:
        for _, n in C.grid_runs(rows, m):
            assert -(-n // m) == rows  # the host derives rows_needed = rows from every n_out


# ------------------------------------------------------------------ the exactness limit
def test_boundary_moduli():
    assert C.BOUNDARY_KS == (5, 129, 160, 300)
    for k in C.BOUNDARY_KS:
        p = C.p_hi(k)
        assert (p - 1) ** 2 * k < 2 ** 53 <= p ** 2 * k
        assert p == C.BOUNDARY_P_HI[k]
    assert [C.p_hi(k) for k in C.BOUNDARY_KS] == [42443373, 8356031, 7503000, 5479416]


@pytest.mark.parametrize("k", C.BOUNDARY_KS)
def test_boundary_reference(k):
    for p in (C.p_hi(k), C.p_hi(k) + 1):
        coef, F, ref = C.boundary_case(k, p, "full")
        assert coef.shape == (C.BOUNDARY_ROWS, k) and F.shape == (k, C.BOUNDARY_M)
        assert ref.tolist() == [k * (p - 1) ** 2 % p] * (C.BOUNDARY_ROWS * C.BOUNDARY_M)  # no wrap: < 2^54
        assert torch.equal(_orc(coef, F, p, ref.numel()), ref)
        coef, F, ref = C.boundary_case(k, p, "striped")
        assert int(coef.max()) == p - 1 == int(F.max()) and int(coef.min()) >= 0 and int(F.min()) >= 0
        cross = ref.reshape(C.BOUNDARY_ROWS, C.BOUNDARY_M)[C.BOUNDARY_ROWS - 1, (C.BOUNDARY_M - 1) // 2]
        assert int(cross) == k * (p - 1) ** 2 % p  # the full sum, among uniform data
        assert torch.equal(_orc(coef, F, p, ref.numel()), ref)


# ------------------------------------------------------------------ host path choice and redo
def test_host_case_bad_values_vs_oracle():
    coef, F, ref = C.host_case()
    coef = coef[:C.HOST_ROWS]
    assert set(C.HOST_BAD_F.values()) == {-5, C.HOST_P, C.HOST_P + 7, 2 ** 32 + 5, 2 ** 62 + 11, *INT64}
    assert 0 <= (2 ** 32 + 5) % 2 ** 32 < C.HOST_P  # a check of the low word alone would pass it
    assert all(not 0 <= v < C.HOST_P for v in C.HOST_BAD_F.values())
    pos = C.host_positions()
    assert len(pos) == 20
    vals = list(C.HOST_BAD_F.values())
    bad = C.with_entries(F, [(r, c, vals[i % len(vals)]) for i, (r, c) in enumerate(pos)])
    assert not torch.equal(bad, F) and int((bad != F).sum()) == 20
    exp = C.patched_reference(coef, bad, ref, C.HOST_P, C.HOST_F_COLS)
    assert torch.equal(exp, C.reference(coef, bad, C.HOST_P))
    assert torch.equal(exp, _orc(coef, bad, C.HOST_P, exp.numel()))
    assert not torch.equal(exp, ref)
    for v in C.HOST_BAD_COEF.values():
        assert not 0 <= v < C.HOST_P
        c2 = C.with_entries(coef, [(C.RBF, C.LDS_I, v)])
        assert torch.equal(C.reference(c2, F, C.HOST_P), _orc(c2, F, C.HOST_P, ref.numel()))


@pytest.mark.parametrize("p", [C.P61, C.P63])
def test_wrap_case_vs_oracle(p):
    coef, F, ref = C.wrap_case(p)
    assert coef.shape == (C.HOST_ROWS, C.HOST_K) and F.shape == (C.HOST_K, C.HOST_M)
    assert int(coef.min()) >= 0 and int(coef.max()) < p and int(coef.max()) > p // 2
    assert int(F.min()) == INT64[0] and int(F.max()) == INT64[1]
    assert torch.equal(ref, _orc(coef, F, p, ref.numel()))
    assert int(ref.min()) >= 0 and int(ref.max()) < p


def test_adversarial_is_deterministic():
    a = C.adversarial(torch.Generator().manual_seed(4), 4096, C.P15)
    b = C.adversarial(torch.Generator().manual_seed(4), 4096, C.P15)
    assert torch.equal(a, b)
    in_range = (a >= 0) & (a < C.P15)
    assert 0.2 < float(in_range.float().mean()) < 0.6 and bool((a < 0).any()) and bool((a >= 2 ** 62).any())


# ------------------------------------------------------------------ protocol round trip
def test_round_trip_primes():
    assert [p for p, _ in C.RT_CASES] == [C.P15, C.P27] and C.P27 == 2 ** 27 - 39
    assert C.is_prime(C.P15) and C.is_prime(C.P27)  # trial division
    assert not C.is_prime(2 ** 27 - 1) and not C.is_prime(1) and C.is_prime(2)
    assert (C.P15 - 1) ** 2 * C.RT_U < 2 ** 53                     # float64 path
    assert (C.P27 - 1) ** 2 * C.RT_U >= 2 ** 53                    # int64 path
    assert (C.P27 - 1) ** 2 * C.RT_N < 2 ** 63                     # and nothing wraps, encoding included
    assert C.RT_U > C.LDS_I and C.RT_U - C.RT_T > 2 * C.RBF        # two LDS chunks, three row passes


@pytest.mark.parametrize("p,m", C.RT_CASES)
def test_round_trip_through_the_oracle(p, m):
    from fedml_amd.core.mpc.lightsecagg import gen_Lagrange_coeffs
    X, F, survivors, alpha, beta = C.round_trip_case(p, m)
    assert X.shape == (C.RT_U, m) and F.shape == (C.RT_N, m)
    assert len(survivors) == len(set(survivors)) == C.RT_U and survivors != sorted(survivors)
    assert alpha.tolist() == list(range(1, C.RT_N + 1)) and beta.tolist() == list(range(C.RT_N + 1, C.RT_N + C.RT_U + 1))
    assert int(F.min()) >= 0 and int(F.max()) < p
    coef = torch.from_numpy(gen_Lagrange_coeffs(beta, alpha[survivors], p))
    assert coef.shape == (C.RT_U, C.RT_U) and int(coef.min()) >= 0 and int(coef.max()) < p
    n_out = (C.RT_U - C.RT_T) * m
    got = _orc(coef, F[survivors].contiguous(), p, n_out)
    assert torch.equal(got, X[:C.RT_U - C.RT_T].reshape(-1))
    assert torch.equal(C.reference(coef, F[survivors].contiguous(), p), X.reshape(-1))  # all U pieces come back
