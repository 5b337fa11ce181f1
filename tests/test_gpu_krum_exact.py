"""Krum's pairwise squared distances (fedml_amd/csrc/robust.hip) past one chunk per workgroup, exactly.

The tables of tests/krumcases.py (integers in [-15, 15], dense or one-hot on the layout's boundaries,
times powers of two) make every form of the kernels exact by arithmetic, so every comparison here is
bit equality with the float64 reference, plus symmetry and a zero diagonal.  The sizes are the
smallest at which a workgroup of the direct kernels (k_pairdist_lane, k_pairdist, k_pairdist_f64) and
of the Gram kernels (the LDS-DMA ring, the f32-input and the bf16x3 forms) runs four or five chunks:
the second LDS buffer, the prefetch of chunk + 2, the pointer reload when a workgroup's run crosses a
segment boundary, the float32-run accounting across chunks and the within-block phase's run all take
part, aligned and one element past alignment, on one segment and on a model-like dozen.  The chunk
size of the direct kernels is read from the library (krumcases.probe_pe), not written down here.

One comparison is not bitwise: the float32 run length (test_direct_run_length) asserts the bound the
header's contract implies, |D - exact| <= 64.  Nothing else carries a tolerance: the Gram forms are
exact on these tables too (the matrix cores' float32 accumulation keeps integer sums below 2^24
exact, observed on every form), so no Gram comparison falls back to the header's error model.

Kernels broken on purpose in a scratch build -- the segment pointer never reloaded (direct or Gram),
the second LDS buffer never written, the float32 run never flushed inside the chunk loop -- fail
these tests; the three direct breaks pass every pairwise test of test_gpu_robust.py (Krum).

Not reached: the non-default A/B forms (FA_GRAM3=0, FA_GRAM_GLDS=0, FA_PAIR_NPL=8, FA_PAIR_PF=1,
FA_PAIR_BLOCKS, FA_GRAM_BLOCKS).  The library reads those variables once per process, so each needs a
child process per case; setting them from a test of this process would change nothing."""
from __future__ import annotations

import pytest
import torch

import krumcases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

DIRECT_KS = [2, 3, 4, 5, 8, 16, 17, 32, 33, 64, 65, 96, 97, 100, 128]
HALF_KS = [8, 32, 40, 72, 96, 100, 128]
F64_KS = [2, 23, 128]
GRAM_KS = [5, 16, 32, 33, 64, 65, 96, 97, 128]
BLOCK_KS = [130, 200]
RUN_KS = [8, 32, 64, 100, 128]
POISON_KS = [5, 32, 33, 97, 128]


@pytest.fixture(scope="module")
def eng():
    from fedml_amd.engine import get_engine
    return get_engine(0)


def _layouts(n, chunk):
    return {"single": [n], "model": C.model_sizes(n, chunk)}


def _direct(eng, segs, dtype=torch.float32):
    D = eng._pairwise_launch(segs, None, dtype, form="direct")
    assert eng.last_pair_form == "direct"
    return D


def _scaled_runs(run, buf, exp, what, scales):
    """run() on the placed buffer times 2^s, in place (exact both ways), for every s."""
    for s in scales:
        buf.mul_(2.0 ** s)
        try:
            C.assert_exact(run(), C.scaled(exp, s), f"{what} times 2^{s}")
        finally:
            buf.mul_(2.0 ** -s)


@pytest.mark.parametrize("K", DIRECT_KS)
def test_direct_exact(eng, K):
    """form="direct", float32 differences: no tiles (K <= 4), the lane kernel, each KPAD, padded
    clients, both thread caps; dense and one-hot tables on both layouts, aligned and offset; the dense
    table times 2^50 and 2^-55."""
    pe = C.probe_pe(K)
    n = C.total(pe)
    dense = C.dense_table(K, n).to(DEV)
    exp = C.dense_reference(K, n)
    for name, sizes in _layouts(n, pe).items():
        pos = C.boundary_positions(sizes, pe, C.PAIR_BLOCKS, K)
        onehot = C.onehot_table(K, n, pos, DEV)
        for aligned in (True, False):
            what = f"direct K={K} pe={pe} {name} {'aligned' if aligned else 'offset'}"
            buf, segs = C.place(dense, sizes, aligned)
            C.assert_exact(_direct(eng, segs), exp, f"{what} dense")
            if aligned:
                _scaled_runs(lambda: _direct(eng, segs), buf, exp, f"{what} dense", C.SCALES[torch.float32])
            del buf, segs
            buf, segs = C.place(onehot, sizes, aligned)
            C.assert_exact(_direct(eng, segs), C.onehot_expected(K), f"{what} one-hot", pos)
            del buf, segs


@pytest.mark.parametrize("K", HALF_KS)
def test_direct_half_differences_exact(eng, K):
    """bfloat16 / float16 differences (the only Krum path of half models) on both layouts: the dense
    table and its scalings -- 2^50 and 2^-55 for bfloat16, 2^11 (the largest difference 61,440) and
    2^-24 (float16 subnormal differences) for float16."""
    pe = C.probe_pe(K)
    n = C.total(pe)
    dense = C.dense_table(K, n).to(DEV)
    exp = C.dense_reference(K, n)
    for name, sizes in _layouts(n, pe).items():
        buf, segs = C.place(dense, sizes, True)
        for dt in (torch.bfloat16, torch.float16):
            what = f"direct {dt} K={K} pe={pe} {name}"
            C.assert_exact(_direct(eng, segs, dt), exp, what)
            _scaled_runs(lambda: _direct(eng, segs, dt), buf, exp, what, C.SCALES[dt])
        del buf, segs


@pytest.mark.parametrize("K", F64_KS)
def test_direct_f64_exact(eng, K):
    """k_pairdist_f64 (32-coordinate chunks, up to 32 pairs per thread) on float64 integer tables cut
    like a model, aligned and offset, and times 2^-300."""
    n = C.total(C.F64_CHUNK)
    dense = C.dense_table(K, n).to(DEV)
    exp = C.dense_reference(K, n)
    sizes = C.model_sizes(n, C.F64_CHUNK)
    pos = C.boundary_positions(sizes, C.F64_CHUNK, C.PAIR_BLOCKS, K)
    for aligned in (True, False):
        what = f"float64 K={K} {'aligned' if aligned else 'offset'}"
        buf, segs = C.place(dense, sizes, aligned, torch.float64)
        C.assert_exact(eng.pairwise_sqdist(segs, diff_dtype=torch.float64), exp, what)
        _scaled_runs(lambda: eng.pairwise_sqdist(segs, diff_dtype=torch.float64), buf, exp, what,
                     C.SCALES[torch.float64])
        del buf, segs
        _, segs = C.place(C.onehot_table(K, n, pos, DEV), sizes, aligned, torch.float64)
        C.assert_exact(eng.pairwise_sqdist(segs, diff_dtype=torch.float64), C.onehot_expected(K),
                       f"{what} one-hot", pos)
        del segs


@pytest.mark.parametrize("K", GRAM_KS)
def test_gram_exact(eng, K, monkeypatch):
    """form="gram" (no guard): the ring (K <= 32, aligned), the register-staged f32 form (K <= 32,
    offset) and the bf16x3 forms (K > 32), with segment changes inside a workgroup's run and unaligned
    loads in steady state; then the default path (the guarded Gram form or the direct kernels it hands
    over to) on the same dense data: exact whichever form the guard keeps."""
    monkeypatch.setenv("FEDML_AMD_KRUM_STICKY", "0")  # this call's own guard, not a previous call's
    n = C.total(C.GRAM_CHUNK, C.GRAM_BLOCKS)
    dense = C.dense_table(K, n).to(DEV)
    exp = C.dense_reference(K, n)
    gram = lambda segs: eng._pairwise_launch(segs, form="gram")
    for name, sizes in _layouts(n, C.GRAM_CHUNK).items():
        pos = C.boundary_positions(sizes, C.GRAM_CHUNK, C.GRAM_BLOCKS, K)
        onehot = C.onehot_table(K, n, pos, DEV)
        for aligned in (True, False):
            what = f"K={K} {name} {'aligned' if aligned else 'offset'}"
            _, segs = C.place(onehot, sizes, aligned)
            C.assert_exact(gram(segs), C.onehot_expected(K), f"gram {what} one-hot", pos)
            del segs
            buf, segs = C.place(dense, sizes, aligned)
            C.assert_exact(gram(segs), exp, f"gram {what} dense")
            assert eng.last_pair_form == "gram"
            if aligned:
                _scaled_runs(lambda: gram(segs), buf, exp, f"gram {what} dense", C.SCALES[torch.float32])
            D = eng.pairwise_sqdist(segs)
            form = eng.last_pair_form
            C.assert_exact(D, exp, f"default path ({form}) {what} dense")
            del buf, segs


@pytest.mark.parametrize("K", BLOCK_KS)
def test_more_than_128_clients_exact(eng, K, monkeypatch):
    """K > 128 (the engine's 64-client block pairs): three segments, offset views, float32, bfloat16
    and float64 differences; every entry against the reference."""
    monkeypatch.setenv("FEDML_AMD_KRUM_STICKY", "0")
    chunk = C.probe_pe(128)
    n = C.total(chunk, per_group=2)
    dense = C.dense_table(K, n).to(DEV)
    exp = C.dense_reference(K, n)
    sizes = C.three_sizes(n, chunk)
    for dt in (torch.float32, torch.bfloat16, torch.float64):
        _, segs = C.place(dense, sizes, False, torch.float64 if dt == torch.float64 else torch.float32)
        C.assert_exact(eng.pairwise_sqdist(segs, diff_dtype=dt), exp, f"K={K} {dt} three offset segments")
        del segs


@pytest.mark.parametrize("K", RUN_KS)
def test_direct_run_length(eng, K):
    """The header's float32 runs of at most 64 coordinates, summed in float64.  Client 0 holds 4096 at
    coordinate 0 and 1 elsewhere, the others zero: D_0j = 2^24 + n - 1 exactly.  Inside the run that
    holds the 2^24 term each of at most 64 additions can err by at most 1 (half an ulp there); every
    other run is exact.  So |D_0j - exact| <= 64 -- derived from the contract, not measured; a kernel
    whose runs grow across chunks loses a few hundred.  All other pairs are exactly 0."""
    n = C.total(C.probe_pe(K))
    x = torch.zeros((K, -(-n // 4) * 4), device=DEV)[:, :n]  # 16-byte aligned rows
    x[0] = 1.0
    x[0, 0] = 4096.0
    D = _direct(eng, [list(x)]).cpu()
    exact = float(2 ** 24 + n - 1)
    err = (D[0, 1:] - exact).abs()
    print(f"K={K} n={n}: largest |D_0j - exact| = {float(err.max())}")
    assert float(err.max()) <= C.KPE, (K, [(j + 1, float(e)) for j, e in enumerate(err) if e > C.KPE][:8])
    assert torch.equal(D[0], D[:, 0]) and float(D[0, 0]) == 0.0
    assert bool((D[1:, 1:] == 0).all())


@pytest.mark.parametrize("K", POISON_KS)
def test_direct_non_finite_inputs(eng, K, monkeypatch):
    """One non-finite value taints its client's row and column only.  Each poison (krumcases.poisons)
    alone, at coordinate 0, at the last coordinate of the ragged tail and at the first coordinate of a
    workgroup's third chunk; float32, bfloat16 and float16 differences through form="direct", and
    float32 through the default path (which must hand over to the direct kernels).  Entries between
    finite clients: the bits of the same call with the poison replaced by 0.  Poisoned rows and columns:
    the class float64 arithmetic gives -- Inf against finite +Inf, Inf against Inf or anything against
    NaN NaN."""
    monkeypatch.setenv("FEDML_AMD_KRUM_STICKY", "0")
    pe = C.probe_pe(K)
    n = C.total(pe)
    buf, segs = C.place(C.dense_table(K, n).to(DEV), [n], True)
    chunks, ranges = C.chunk_map([n], pe, C.PAIR_BLOCKS)
    third = chunks[ranges[len(ranges) // 2][0] + 2][0]
    runs = [(str(dt), lambda dt=dt: _direct(eng, segs, dt)) for dt in (torch.float32, torch.bfloat16, torch.float16)]
    runs.append(("default path", lambda: eng.pairwise_sqdist(segs)))
    for p in (0, n - 1, third):
        for name, poison in C.poisons(K).items():
            rows = [i for i, _ in poison]
            keep = buf[rows, p].clone()
            nan, inf = C.poison_classes(K, poison)
            fin = ~(nan | inf)
            try:
                for what, run in runs:
                    buf[rows, p] = 0.0
                    base = run().cpu()
                    assert bool(torch.isfinite(base).all())
                    buf[rows, p] = torch.tensor([v for _, v in poison], device=DEV)
                    D = run().cpu()
                    where = f"K={K} {what} {name} at coordinate {p}"
                    if what == "default path":
                        assert eng.last_pair_form == "direct", where
                    assert torch.equal(torch.isnan(D), nan) and torch.equal(torch.isposinf(D), inf), where
                    assert torch.equal(D[fin].view(torch.int64), base[fin].view(torch.int64)), where
            finally:
                buf[rows, p] = keep


@pytest.mark.parametrize("K", [32, 128])
def test_deterministic(eng, K):
    """The model-like layout called twice gives the same bits, direct and Gram -- on the dense table
    times 0.37, so that the sums round and their order shows."""
    pe = C.probe_pe(K)
    for chunk, form in ((pe, "direct"), (C.GRAM_CHUNK, "gram")):
        n = C.total(chunk)
        buf, segs = C.place(C.dense_table(K, n).to(DEV), C.model_sizes(n, chunk), True)
        buf.mul_(0.37)
        a = eng._pairwise_launch(segs, form=form).cpu()
        b = eng._pairwise_launch(segs, form=form).cpu()
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)), (K, form)
        del segs
