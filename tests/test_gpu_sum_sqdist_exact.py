"""The fused sum-and-distance pass (fedml_amd/csrc/wsum_dist.hip: the geometric median's and centered
clipping's device work) at hundreds of per-chunk rows, exactly.

One workgroup owns one chunk and writes a row of 2K float64 partial sums; k_wsd_reduce adds the rows
split 64 ways, eight rows of a split per pass of an unrolled loop and the rest in a tail loop.  The
unrolled loop needs more than 448 rows before its first split enters it; the older tests
(test_gpu_geometric_median.py, test_gpu_centered_clipping.py) produce about ten.  The row counts here:

    449   the first split alone enters the unrolled loop
    512   every split, one unrolled pass, no tail
    513   one tail step
    1061  two unrolled passes and ragged tails

as single segments of (P - 1) chunks and 37 elements, plus a model-like dozen of segments (an empty
one, several below one chunk) whose rows total more than 1,024.

The tables of tests/chunkcases.py (small integers, coefficients m_i / 256 -- m_i / 16 for the 16-bit
types) make every step exact, so every comparison is bit equality: out with the exact rational value
and (plain mode) with weighted_sum_multi's MUL_W sum, the 2K sums with the int64 reference, in all
three modes (plain, centred with coefficients, distance-only), through the register kernel, the
generic kernel (K = 33, other dtypes, FA_WSD_REG=0, unaligned pointers) and both tiled entries.  The
one-hot rows -- client i non-zero in one chunk only, dealt from rows 0, 63, 64, 447, 448, 449, 511,
512, 513 and the last -- show a lost or doubled row as a wrong ss_i."""
from __future__ import annotations

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chunkcases as C  # noqa: E402
from test_gpu_geometric_median import DEV, bits, tiled_buf  # noqa: E402

pytestmark = pytest.mark.gpu


def _id(v):
    return str(v).replace("torch.", "")


@pytest.fixture(scope="module")
def eng():
    from fedml_amd.engine import get_engine
    return get_engine(0)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def call(eng, mode, segs, cens, coef):
    """(outs or None, stats) of one pass in ``mode``."""
    if mode == "plain":
        return eng.weighted_sum_sqdist(segs, coef)
    return eng.centered_sum_sqdist(segs, cens, coef if mode == "center" else None)


def check(eng, x, cen, dt, k, sizes, aligned, what, modes=C.WSD_MODES):
    """Every mode over the int8 host table x [k, n] and centre [n] placed on the device in ``dt``: out
    and the stats bit for bit the integer reference's, twice; inputs and centre only read."""
    from fedml_amd.engine import MUL_W
    den = C.WSD_DENOM[dt]
    m, coef = C.wsd_coef(k, dt)
    x, cen = x.to(DEV), cen.to(DEV)
    xb, segs = C.place(x, sizes, aligned, dt)
    cb, cs = C.place(cen[None], sizes, aligned, dt)
    cens = [col[0] for col in cs]
    keep_c = cb.clone()
    checksum = xb.view(torch.uint8).sum(dtype=torch.int64)
    for mode in modes:
        O, D2, SS = C.wsd_reference(x, cen, m, den, mode)
        exp = C.wsd_expected_stats(D2, SS, den)
        outs, stats = call(eng, mode, segs, cens, coef)
        again, stats2 = call(eng, mode, segs, cens, coef)
        torch.cuda.synchronize()
        got = stats.cpu()
        bad = (got.view(torch.int64) != exp.view(torch.int64)).nonzero()
        assert not bad.numel(), (what, mode, [("d2" if r == 0 else "ss", i, got[r, i].item(), exp[r, i].item())
                                              for r, i in bad[:8].tolist()])
        assert torch.equal(stats2.view(torch.int64), stats.view(torch.int64)), (what, mode)
        if mode == "dist":
            assert outs is None
        else:
            out = torch.cat([o.reshape(-1) for o in outs])
            want = (O.double() / den).to(dt)
            assert torch.equal(want.double() * den, O.double())  # the exact rational value
            assert same(out, want), (what, mode, "out")
            assert same(torch.cat([o.reshape(-1) for o in again]), want), (what, mode, "second call")
            if mode == "plain":
                ws = eng.weighted_sum_multi(segs, MUL_W, coef)
                assert same(torch.cat([o.reshape(-1) for o in ws]), want), (what, "weighted_sum_multi")
        assert same(cb, keep_c), (what, mode, "the centre was written")
    assert int(xb.view(torch.uint8).sum(dtype=torch.int64)) == int(checksum), (what, "an input was written")


def onehot_rounds(k, rows):
    """The named rows dealt to k clients, as many rounds as it takes to use every row once."""
    return [[rows[(r + i) % len(rows)] for i in range(k)] for r in range(0, len(rows), k)]


@pytest.mark.parametrize("dt,k,P", C.WSD_CASES, ids=_id)
def test_single_segment_rows_exact(eng, dt, k, P, monkeypatch):
    """One segment of P chunks (the last one ragged): the dense table in all three modes -- for K = 3
    also one element past alignment (every chunk on the element path) and, float32, with FA_WSD_REG=0
    (the generic kernel; the variable is read per call) -- and one-hot rows in plain mode."""
    n = C.wsd_single(P, dt)
    assert C.wsd_chunks([n], k, dt) == P
    steps = C.wsd_reduce_steps(P)
    print(f"{dt} K={k}: n={n} rows={P}; k_wsd_reduce (unrolled passes, tail steps): first split {steps[0]}, "
          f"last split {steps[1]}")
    x, cen = C.wsd_tables(k, n, C.WSD_MAG[dt])
    what = f"{dt} K={k} rows={P}"
    check(eng, x, cen, dt, k, [n], True, what)
    if k == C.WSD_OFFSET_K:
        check(eng, x, cen, dt, k, [n], False, what + " offset")
        if dt == torch.float32:
            monkeypatch.setenv("FA_WSD_REG", "0")
            check(eng, x, cen, dt, k, [n], True, what + " FA_WSD_REG=0")
            monkeypatch.delenv("FA_WSD_REG")
    for rows in onehot_rounds(k, C.wsd_named_rows(P)):
        print(f"{what}: one-hot rows {rows[:12]}")
        check(eng, C.wsd_onehot_rows(x, [n], dt, rows), cen, dt, k, [n], True, f"{what} one-hot rows {rows[:12]}",
              modes=("plain",))


@pytest.mark.parametrize("dt,k", [(C.F32, 3), (C.F32, 33), (C.BF16, 3), (C.F64, 3)], ids=_id)
def test_model_layout_rows_exact(eng, dt, k):
    """A dozen segments, an empty one and several below one chunk among them, more than 1,024 rows
    in all: find_seg, ragged chunks inside the row order, aligned and one element past alignment."""
    sizes = C.wsd_model_sizes(dt)
    rows = C.wsd_chunks(sizes, k, dt)
    print(f"{dt} K={k}: segments {sizes} rows={rows}; k_wsd_reduce steps {C.wsd_reduce_steps(rows)}")
    assert rows > 1024
    x, cen = C.wsd_tables(k, sum(sizes), C.WSD_MAG[dt])
    for aligned in (True, False):
        check(eng, x, cen, dt, k, sizes, aligned, f"{dt} K={k} model aligned={aligned}")


@pytest.mark.parametrize("dt,k", [(C.F32, 3), (C.BF16, 3)], ids=_id)
def test_tiled_entries_rows_exact(eng, dt, k):
    """fa_weighted_sum_sqdist_tiled and fa_centered_sum_sqdist_tiled (with coefficients and
    distance-only) at 513 rows, non-consecutive rows of an arena of capacity K + 3."""
    P = 513
    n = C.wsd_single(P, dt)
    den, mag = C.WSD_DENOM[dt], C.WSD_MAG[dt]
    m, coef = C.wsd_coef(k, dt)
    g = torch.Generator().manual_seed(9400 + k)
    ints = lambda g_, k_, n_, dt_: torch.randint(-mag, mag + 1, (k_, n_), generator=g_).to(dt_)  # noqa: E731
    buf, rows, xt, _ = tiled_buf(g, ints, k, k + 3, n, dt)
    print(f"tiled {dt} K={k}: n={n} rows={P} arena rows {rows}")
    before = buf.clone()
    x, cen = xt.to(torch.int8).to(DEV), ints(g, 1, n, torch.int8)[0].to(DEV)
    cd = cen.to(dt)
    for mode in C.WSD_MODES:
        O, D2, SS = C.wsd_reference(x, cen, m, den, mode)
        exp = C.wsd_expected_stats(D2, SS, den)
        if mode == "plain":
            out, stats = eng.weighted_sum_sqdist_tiled(buf, rows, coef, n=n)
        else:
            out, stats = eng.centered_sum_sqdist_tiled(buf, rows, cd, coef if mode == "center" else None, n=n)
        torch.cuda.synchronize()
        assert torch.equal(stats.cpu().view(torch.int64), exp.view(torch.int64)), (dt, k, mode)
        if mode == "dist":
            assert out is None
        else:
            assert same(out, (O.double() / den).to(dt)), (dt, k, mode)
        assert same(buf, before) and same(cd, cen.to(dt)), (dt, k, mode)


def test_same_call_same_bits_when_the_sums_round(eng):
    """The dense table with coefficients that are not dyadic, so every sum rounds and the order of the
    1,061 rows shows: two calls, one bit pattern."""
    k, dt = 32, torch.float32
    n = C.wsd_single(1061, dt)
    x, cen = C.wsd_tables(k, n, C.WSD_MAG[dt])
    coef = [(i + 1) / (k * (k + 1) / 2) for i in range(k)]
    _, segs = C.place(x.to(DEV), [n], True, dt)
    segs[0][0].mul_(0.37)
    runs = [eng.weighted_sum_sqdist(segs, coef) for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(runs[0][1].view(torch.int64), runs[1][1].view(torch.int64))
    assert same(runs[0][0][0], runs[1][0][0])
    assert bool(torch.isfinite(runs[0][1]).all()) and bool((runs[0][1] > 0).all())
