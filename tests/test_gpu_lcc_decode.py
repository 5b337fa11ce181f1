"""LightSecAgg's mask decoding (fa_lcc_decode, fedml_amd/csrc/finite.hip) at large cohorts and at the
float64 exactness limit, bit for bit.

The cases of tests/lcccases.py against np.mod(coef.dot(F), p) on numpy int64 (pinned to Python ints
and to the C oracle by tests/test_lcc_cases_cpu.py); every comparison is torch.equal on int64.

* The tiling grid: (rows_needed, k) around k_lcc_decode's register block (kRB = 8) and
  k_lcc_decode_f64's row pass (kRBF = 32), prefetch ring (kPF = 4) and LDS chunk (kLdsI = 128), up to
  three passes and three chunks; 1 .. 777 columns; n_out that ends a row early or one entry in; more
  coefficient rows than needed.  Each on the float64 path, on the int64 path forced by variant 1, and
  on the int64 path at p = 2^31 - 1 where the sums wrap.
* The exactness limit: the last modulus the host may send to float64 at k = 5, 129, 160, 300 and the
  first it may not, with every product (p - 1)^2.
* The host's choice of path: out-of-range F values around the chunk and block edges (the redo of
  single blocks), out-of-range coefficients in needed and in unneeded rows, redo flags from one call
  not leaking into the next, and moduli near 2^63 on adversarial F.
* Memory discipline through the C ABI: nothing written outside out[:n_out], F untouched, 8-byte
  aligned buffers, the same bits twice.
* The protocol at 200 clients, 160 survivors: decoding the shares of known pieces gives the pieces
  back, through LCC_decoding_with_points and through LightSecAggAggregator.

Broken on purpose in a scratch build, k_lcc_decode_f64 fails these tests (LightSecAgg):
the pass offset of the staged coefficients dropped, the chunk base dropped from the ring's row
index, the host's float64 limit raised to <= 2^54.  The first two fail the grid's float64 runs with
a second pass / a second chunk and everything built on the host case; the last fails
test_exactness_boundary at k = 5 and 129, where p_hi is odd (at the even p_hi of k = 160 and 300
every product is a multiple of 64 and float64 stays exact past 2^53).  None of the three fails an
LCC test of test_gpu_finite.py."""
from __future__ import annotations

import types

import pytest
import torch

import lcccases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def eng():
    from fedml_amd.engine import get_engine
    return get_engine(0)


def _decode(eng, coef, F_dev, p, n_out, variant=0):
    if not variant:
        return eng.lcc_decode(coef.tolist(), F_dev, p, n_out).cpu()
    try:
        eng.set_variant(variant)
        return eng.lcc_decode(coef.tolist(), F_dev, p, n_out).cpu()
    finally:
        eng.set_variant(0)


# ----------------------------------------------------------------------------- 1. the tiling grid
@pytest.mark.parametrize("way", ["f64", "forced_i64", "i64_wrap"])
@pytest.mark.parametrize("rows,k", C.GRID)
def test_tiling_grid(eng, rows, k, way):
    p = C.P31 if way == "i64_wrap" else C.P15
    variant = 1 if way == "forced_i64" else 0
    for m in C.MS:
        coef, F, ref = C.grid_case(rows, k, m, p)
        F_dev = F.to(DEV)
        for nrows, n_out in C.grid_runs(rows, m):
            got = _decode(eng, coef[:nrows], F_dev, p, n_out, variant)
            assert torch.equal(got, ref[:n_out]), (rows, k, m, way, nrows, n_out)


# ----------------------------------------------------------------------------- 2. the exactness limit
@pytest.mark.parametrize("kind", ["full", "striped"])
@pytest.mark.parametrize("k", C.BOUNDARY_KS)
def test_exactness_boundary(eng, k, kind):
    """p_hi: the largest sums float64 is trusted with, 2^53 - k (p - 1)^2 < 2 k (p - 1); p_hi + 1: the
    host must not take float64 any more.  Variant 1 gives the same bits at p_hi."""
    p_hi = C.p_hi(k)
    for p in (p_hi, p_hi + 1):
        coef, F, ref = C.boundary_case(k, p, kind)
        F_dev = F.to(DEV)
        got = _decode(eng, coef, F_dev, p, ref.numel())
        assert torch.equal(got, ref), (k, kind, p)
        if p == p_hi:
            forced = _decode(eng, coef, F_dev, p, ref.numel(), variant=1)
            assert torch.equal(forced, got) and torch.equal(forced, ref), (k, kind, p)


# ----------------------------------------------------------------------------- 3. path choice and redo
def _bad_f(which):
    """Entries (row, col, value) per F: one value at one position at a time, or all seven dealt over
    the twenty positions at once."""
    pos = C.host_positions()
    if which == "all":
        vals = list(C.HOST_BAD_F.values())
        return [[(r, c, vals[i % len(vals)]) for i, (r, c) in enumerate(pos)]]
    return [[(r, c, C.HOST_BAD_F[which])] for r, c in pos]


@pytest.mark.parametrize("which", list(C.HOST_BAD_F) + ["all"])
def test_out_of_range_f(eng, which):
    coef, F, ref = C.host_case()
    coef = coef[:C.HOST_ROWS]
    for entries in _bad_f(which):
        bad = C.with_entries(F, entries)
        exp = C.patched_reference(coef, bad, ref, C.HOST_P, [c for _, c, _ in entries])
        got = _decode(eng, coef, bad.to(DEV), C.HOST_P, exp.numel())
        assert torch.equal(got, exp), (which, entries if len(entries) == 1 else "all")
    # a shorter n_out: the bad columns' last rows are not stored by either kernel
    entries = _bad_f("all")[0]
    bad = C.with_entries(F, entries)
    exp = C.patched_reference(coef, bad, ref, C.HOST_P, C.HOST_F_COLS)
    n_out = (C.HOST_ROWS - 1) * C.HOST_M + 201
    assert torch.equal(_decode(eng, coef, bad.to(DEV), C.HOST_P, n_out), exp[:n_out])


def test_redo_flags_are_fresh_on_every_call(eng):
    """bad then clean, clean then bad, on one engine: a flag left over would hand a clean block to the
    int64 kernel (harmless) -- a flag not raised again would leave float64's result for a bad one."""
    coef, F, ref = C.host_case()
    coef = coef[:C.HOST_ROWS]
    entries = [(C.LDS_I, 200, -5), (0, C.HOST_M - 1, 2 ** 32 + 5)]
    bad = C.with_entries(F, entries)
    bad_ref = C.patched_reference(coef, bad, ref, C.HOST_P, [200, C.HOST_M - 1])
    F_dev, bad_dev = F.to(DEV), bad.to(DEV)
    n = ref.numel()
    for order in ("bad_clean", "clean_bad", "bad_bad_clean_clean"):
        for step in order.split("_"):
            got = _decode(eng, coef, bad_dev if step == "bad" else F_dev, C.HOST_P, n)
            assert torch.equal(got, bad_ref if step == "bad" else ref), (order, step)


@pytest.mark.parametrize("which", list(C.HOST_BAD_COEF))
def test_out_of_range_coefficients(eng, which):
    v = C.HOST_BAD_COEF[which]
    coef_x, F, ref = C.host_case()  # HOST_ROWS + EXTRA_ROWS coefficient rows
    F_dev = F.to(DEV)
    rows = C.HOST_ROWS
    # in a needed row: the first, around the pass edge, the last; around the chunk edge
    for j, i in [(0, 0), (C.RBF - 1, C.LDS_I - 1), (C.RBF, C.LDS_I), (rows - 1, C.HOST_K - 1)]:
        bad = C.with_entries(coef_x[:rows], [(j, i, v)])
        exp = C.reference(bad, F, C.HOST_P)
        assert torch.equal(_decode(eng, bad, F_dev, C.HOST_P, exp.numel()), exp), (which, j, i)
    # in a row at or past rows_needed: ignored -- the reference's prefix, and what a zeroed row gives
    for n_out, j in [(rows * C.HOST_M, rows), (rows * C.HOST_M - 5, rows + 1),
                     (C.RBF * C.HOST_M + 1, C.RBF + 1), ((C.RBF + 1) * C.HOST_M, rows - 1)]:
        assert j >= -(-n_out // C.HOST_M)
        bad = C.with_entries(coef_x, [(j, C.LDS_I, v)])
        zeroed = bad.clone()
        zeroed[j] = 0
        got = _decode(eng, bad, F_dev, C.HOST_P, n_out)
        assert torch.equal(got, ref[:n_out]), (which, n_out, j)
        assert torch.equal(got, _decode(eng, zeroed, F_dev, C.HOST_P, n_out)), (which, n_out, j)


@pytest.mark.parametrize("p", [C.P61, C.P63])
def test_int64_wrap_on_large_moduli(eng, p):
    coef, F, ref = C.wrap_case(p)
    F_dev = F.to(DEV)
    for n_out in (ref.numel(), ref.numel() - C.HOST_M + 1):
        assert torch.equal(_decode(eng, coef, F_dev, p, n_out), ref[:n_out]), (p, n_out)


# ----------------------------------------------------------------------------- 4. memory discipline
SENTINEL = -0x5A5A5A5A5A5A5A5B


@pytest.mark.parametrize("p", [C.P15, C.P31], ids=["f64", "i64"])
@pytest.mark.parametrize("out_offset", [0, 1])
def test_c_abi_memory_discipline(eng, p, out_offset):
    """fa_lcc_decode itself: out[:n_out] written and nothing else, F read and not written, buffers
    that are 8-byte aligned only, the same bits twice."""
    from fedml_amd import _native as N
    rows, k, m = 65, 257, 777
    coef, F, ref = C.grid_case(rows, k, m, p)
    coef = coef[:rows].contiguous()
    n_out = rows * m - 5
    f_buf = torch.full((k * m + 3,), SENTINEL, dtype=torch.int64, device=DEV)
    f_view = f_buf[1:1 + k * m]
    f_view.copy_(F.reshape(-1))
    assert f_view.data_ptr() % 16 == 8
    f_before = f_buf.clone()
    results = []
    for _ in range(2):
        o_buf = torch.full((out_offset + n_out + 64,), SENTINEL, dtype=torch.int64, device=DEV)
        out = o_buf[out_offset:]
        assert out.data_ptr() % 16 == 8 * out_offset
        rc = N.lib().fa_lcc_decode(eng._ctx, rows, k, m, N.i64_array(coef.reshape(-1).tolist()), f_view.data_ptr(),
                                   p, n_out, out.data_ptr(), eng._stream(None))
        N.check(rc, "fa_lcc_decode")
        torch.cuda.synchronize()
        host = o_buf.cpu()
        assert bool((host[:out_offset] == SENTINEL).all()), "written before out"
        assert bool((host[out_offset + n_out:] == SENTINEL).all()), "written past n_out"
        assert torch.equal(host[out_offset:out_offset + n_out], ref[:n_out])
        assert torch.equal(f_buf, f_before), "F changed"
        results.append(host)
    assert torch.equal(results[0], results[1])


# ----------------------------------------------------------------------------- 5. protocol round trip
class _Trainer:
    def get_model_params(self):
        return {}

    def set_model_params(self, p):
        pass


@pytest.mark.parametrize("p,m", C.RT_CASES)
def test_round_trip_large_cohort(eng, p, m):
    """The shares of known pieces, decoded from 160 of 200 clients, are the pieces: a property of the
    protocol, independent of the oracle.  p = 2^15 - 19: float64, two LDS chunks, three row passes;
    p = 2^27 - 39: int64, nothing wraps."""
    from fedml_amd.core.mpc import lightsecagg as lsa
    from fedml_amd.cross_silo.lightsecagg import LightSecAggAggregator
    X, F, survivors, alpha, beta = C.round_trip_case(p, m)
    keep = C.RT_U - C.RT_T
    want = X[:keep].reshape(-1)
    got = lsa.LCC_decoding_with_points(F[survivors].to(DEV), alpha[survivors], beta, p, n_out=keep * m)
    assert got.is_cuda and torch.equal(got.cpu(), want)

    args = types.SimpleNamespace(prime_number=p, precision_parameter=8)
    agg = LightSecAggAggregator(None, None, 0, {}, {}, {}, C.RT_N, DEV, args, _Trainer())
    agg.targeted_number_active_clients, agg.privacy_guarantee = C.RT_U, C.RT_T
    agg.total_dimension = keep * m - 37  # rounded up to keep * m again
    for i in survivors:
        agg.add_local_aggregate_encoded_mask(i, F[i].tolist())
    mask = agg.aggregate_mask_reconstruction(survivors)
    assert tuple(mask.shape) == (keep * m, 1) and torch.equal(mask.reshape(-1).cpu(), want)
