"""CPU side of the exact tables of tests/chunkcases.py: the restated layout facts against the library's
host-only probes (dot_plan for every K, the sum-and-distance row count); every table in every dtype
restated per op with torch CPU ops in the storage dtype equals the integer reference bit for bit, so
the tables are exact by construction and not by luck; the run-length table tells a float32 run of
more than 64 coordinates from one within the rule; and every layout the GPU tests run
(tests/test_gpu_pairwise_dot_exact.py, tests/test_gpu_sum_sqdist_exact.py) really reaches the code
it is meant for, by chunk_map."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import chunkcases as C

ALL_DT = [torch.float32, torch.bfloat16, torch.float16, torch.float64]
SMALL_N = 1237
INT_VIEW = {2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t):
    return t.contiguous().view(INT_VIEW[t.element_size()])


def widen(t, dt, s=0):
    """An integer table times 2^s in the storage dtype, checked to be representable."""
    out = (t.double() * 2.0 ** s).to(dt)
    assert torch.equal(out.double() * 2.0 ** -s, t.double()), (dt, s)
    return out


# ------------------------------------------------------------------ the restated layout facts
def test_dot_plan_equals_the_library_probe():
    """float64 has the smallest chunk of the four dtypes at every K, and the library's block count
    gives exactly the restated pe there; the other dtypes' pe share the restated formula."""
    for k in range(1, 129):
        plans = {dt: C.dot_plan(k, dt) for dt in ALL_DT}
        pe64 = plans[torch.float64]["pe"]
        assert pe64 == min(p["pe"] for p in plans.values()), k
        assert C.probe_min_pe(k) == pe64, (k, pe64)
        for n in (1, pe64, pe64 + 1, 7 * pe64 + 3, 1023 * pe64 + 1, 10 ** 7):
            assert C.dot_blocks(k, n) == min(-(-n // pe64), C.DOT_BLOCKS), (k, n)
        for p in plans.values():
            assert p["pe"] & (p["pe"] - 1) == 0 and 2 <= p["pe"] <= 256 and p["cemax"] <= C.KPE
            assert p["ntiles"] * p["esplit"] <= p["nthreads"] <= 576


def test_dot_plan_known_values():
    """The float32 chunk sizes and flush cadences derived from pairdot.hip's dot_plan."""
    got = {k: (C.dot_plan(k, torch.float32)["pe"], C.flush_every(k, torch.float32))
           for k in (3, 8, 9, 31, 32, 33, 64, 65, 88, 89, 97, 128)}
    assert got == {3: (256, 16), 8: (256, 16), 9: (128, 16), 31: (64, 6), 32: (64, 6), 33: (32, 9), 64: (32, 5),
                   65: (32, 5), 88: (32, 4), 89: (16, 4), 97: (16, 4), 128: (32, 2)}
    assert all(C.dot_plan(k, torch.float32)["esplit"] == 1 for k in range(89, 129))
    assert C.dot_plan(88, torch.float32)["esplit"] == 2


def test_wsd_chunks_equals_the_library_probe():
    """The probe counts float64 chunks of 2,048 elements; a float32 chunk holds twice, a 16-bit chunk
    four times as many (one chunk is four 4-KiB slots in every dtype)."""
    sizes = [5000, 0, 3, 2048, 2049, 8191, 8192, 8193, 123457]
    for k in (1, 3, 33):
        assert C.wsd_chunks(sizes, k, torch.float64) == sum(-(-s // 2048) for s in sizes)
        assert C.wsd_chunks(sizes, k, torch.float32) == C.wsd_rows_probe([-(-s // 2) for s in sizes], k)
        assert C.wsd_chunks(sizes, k, torch.bfloat16) == C.wsd_rows_probe([-(-s // 4) for s in sizes], k)
        assert C.wsd_chunks(sizes, k, torch.float16) == C.wsd_chunks(sizes, k, torch.bfloat16)


# ------------------------------------------------------------------ pairwise dot: the tables are exact
def run_rule_gram(y):
    """G of the documented order on the CPU: products and runs of <= 64 coordinates in float32 (float64
    for float64 storage), the runs added in float64."""
    k, n = y.shape
    if y.dtype == torch.float64:
        return y @ y.T
    yf = torch.zeros(k, -(-n // C.KPE) * C.KPE)
    yf[:, :n] = y.float()
    G = torch.empty(k, k, dtype=torch.float64)
    for i in range(k):
        prod = (yf[i][None, :] * yf).view(k, -1, C.KPE)
        runs = torch.zeros(prod.shape[:2])
        for e in range(C.KPE):  # sequential float32 adds, as a lane makes them
            runs = runs + prod[:, :, e]
        G[i] = runs.double().sum(1)
    return G


@pytest.mark.parametrize("dt", ALL_DT, ids=str)
@pytest.mark.parametrize("k", [3, 9])
def test_dot_integer_tables_are_exact(dt, k):
    x, c, h = C.dot_tables(k, SMALL_N)
    assert int(x.min()) == -C.MAG and int(x.max()) == C.MAG and bool((x == 0).any())
    for s in (0,) + C.SCALES[dt]:
        xs, cs, hs = widen(x, dt, s), widen(c, dt, s), widen(h, dt, s)
        for cen, hist in C.MODES:
            y, G = C.dot_reference(k, SMALL_N, cen, hist)
            u = xs - cs[None, :] if cen else xs          # one rounding per op, in the storage dtype
            got = hs + u if hist else u
            assert torch.equal(bits(got), bits(widen(y, dt, s))), (dt, k, s, cen, hist)
            Gs = G * 2.0 ** (2 * s)
            assert bool(torch.isfinite(Gs).all()) and bool((Gs.diagonal() > 0).all())
            C.assert_gram_exact(run_rule_gram(got), Gs, f"restated {dt} k={k} s={s} {cen} {hist}")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=str)
def test_dot_onehot_table_is_exact(dt):
    k, pe = 33, C.dot_plan(33, dt)["pe"]
    sizes = C.model_sizes(C.total(pe, 64, 4), pe)
    pos = C.boundary_positions(sizes, pe, 64, k)
    t = widen(C.onehot_table(k, sum(sizes), pos), dt)
    C.assert_gram_exact(run_rule_gram(t), C.onehot_gram(k), f"one-hot {dt}", pos)
    assert bool((C.onehot_gram(k).diagonal() > 0).all()) and int((C.onehot_gram(k) != 0).sum()) == k


# ------------------------------------------------------------------ the run-length table discriminates
def test_run_length_values():
    assert C.RUN_PRODUCT == 2 ** 18 + 1 == 262145
    for dt in (torch.float32, torch.float16):
        t = C.run_table(5, 7, dt)
        assert t.double().tolist() == [[545.0 if i % 2 == 0 else 481.0] * 7 for i in range(5)]
    assert float(torch.tensor(545.0).to(torch.bfloat16)) != 545.0  # why bfloat16 is left out
    # no pair of bfloat16 integers (8 significant bits) has the product 2^18 + 1 = 5 * 13 * 37 * 109
    eight_bits = lambda v: v >> max(0, v.bit_length() - 8) << max(0, v.bit_length() - 8) == v  # noqa: E731
    divisors = [d for d in range(1, C.RUN_PRODUCT + 1) if C.RUN_PRODUCT % d == 0]
    assert not [d for d in divisors if eight_bits(d) and eight_bits(C.RUN_PRODUCT // d)]


def test_run_length_table_tells_runs_past_64():
    """A sequential float32 sum of L copies of 262,145 is exact if and only if L <= 64."""
    s = C.f32_run_sums(1024)
    exact = np.arange(1025, dtype=np.float64) * C.RUN_PRODUCT
    assert np.array_equal(s[:65].astype(np.float64), exact[:65])
    assert not (s[65:].astype(np.float64) == exact[65:]).any()


@pytest.mark.parametrize("dt,k", C.DOT_RUN_CASES, ids=str)
def test_run_length_cases_tell_one_missed_flush(dt, k):
    """At the sizes the GPU test uses: runs within the rule give n * 262,145 exactly, and the concrete
    cadence of a kernel that misses every other flush (2 * flush_every chunks of cemax coordinates per
    run), or never flushes inside a workgroup's run, does not."""
    plan, fe = C.dot_plan(k, dt), C.flush_every(k, dt)
    assert fe * plan["cemax"] <= C.KPE < (fe + 1) * plan["cemax"]
    (name, sizes, flags), = C.dot_case_layouts(dt, k, "run")
    n = sum(sizes)
    exact = float(n * C.RUN_PRODUCT)
    assert n * C.RUN_PRODUCT < 2 ** 53
    for run in (1, plan["cemax"], fe * plan["cemax"], C.KPE):
        assert C.run_rule_sum(n, run) == exact, (k, run)
    facts = C.layout_facts(sizes, plan["pe"])
    missed = 2 * fe * plan["cemax"]
    for run in (missed, C.KPE + 1, facts["min"] * plan["cemax"], facts["max"] * plan["cemax"]):
        assert run > C.KPE and C.run_rule_sum(n, run) != exact, (k, run)


# ------------------------------------------------------------------ pairwise dot: the GPU layouts
@pytest.mark.parametrize("kind,dt,k", [(kind, dt, k) for kind, cases in (
    ("exact", C.DOT_EXACT_CASES), ("onehot", C.DOT_ONEHOT_CASES), ("run", C.DOT_RUN_CASES),
    ("two", [C.DOT_TWO_CALLS])) for dt, k in cases], ids=str)
def test_dot_gpu_layouts_reach_the_code(kind, dt, k):
    """Every flat layout of every GPU case: more than 1,024 chunks, a workgroup with >= 3 chunks
    (>= flush_every + 1 for the run-length cases), a workgroup whose run crosses a segment boundary,
    and one whose run steps from a ragged chunk (element path) into a whole one."""
    plan = C.dot_plan(k, dt)
    for name, sizes, flags in C.dot_case_layouts(dt, k, kind):
        f = C.layout_facts(sizes, plan["pe"])
        assert f["nchunks"] > C.DOT_BLOCKS and (0 in sizes or k > 33), (name, f)
        need = C.flush_every(k, dt) + 1 if kind == "run" else 3
        assert f["min"] >= need and f["max"] == f["min"] + 1, (name, f)
        assert f["cross"] >= 1 and f["ragged_to_whole"] >= 1, (name, f)
        assert len(flags) == len(sizes)
        if name == "mixed":
            odd = flags.index(False)
            assert flags.count(False) == 1 and 0 < odd < len(sizes) - 1 and sizes[odd] > 0
            assert sizes[odd - 1] > 0 or sizes[odd - 2] > 0
        if kind == "onehot":
            pos = C.boundary_positions(sizes, plan["pe"], C.DOT_BLOCKS, k)
            chunks, ranges = C.chunk_map(sizes, plan["pe"], C.DOT_BLOCKS)
            inner = {chunks[c][0] for a, b in ranges for c in range(a + 1, b)}
            assert len(set(pos)) == k and set(pos) & inner, (name, k)
        # held in device memory: inputs, a copy, history, expected history -- far below 1 GB
        assert 4 * k * sum(sizes) * C.ELEM[dt] < 2 ** 29


@pytest.mark.parametrize("dt,k", C.DOT_TILED_CASES, ids=str)
def test_dot_tiled_sizes(dt, k):
    pe = C.dot_plan(k, dt)["pe"]
    f = C.layout_facts([C.total(pe)], pe)
    assert f["nchunks"] > C.DOT_BLOCKS and f["min"] >= 4
    assert (4096 // C.ELEM[dt]) % pe == 0  # a chunk never straddles a tile


# ------------------------------------------------------------------ sum and distance
@pytest.mark.parametrize("dt,k", [(dt, k) for dt in ALL_DT for k in (3, 16, 33) if k <= C.WSD_DENOM[dt]], ids=str)
def test_wsd_tables_are_exact(dt, k):
    """The per-op restatement in the storage dtype gives the exact rational out and the exact sums, in
    all three modes, on the dense table and on one-hot rows."""
    den, mag, ch = C.WSD_DENOM[dt], C.WSD_MAG[dt], C.WSD_CHUNK[dt]
    sizes = [2 * ch + C.TAIL]
    x, cen = C.wsd_tables(k, sum(sizes), mag)
    assert int(x.min()) == -mag and int(x.max()) == mag
    m, coef = C.wsd_coef(k, dt)
    assert sum(coef) == 1.0 and all(float(torch.tensor(v).to(dt)) == v for v in coef)
    onehot = C.wsd_onehot_rows(x, sizes, dt, [i % 3 for i in range(k)])
    for table in (x, onehot):
        for mode in C.WSD_MODES:
            O, D2, SS = C.wsd_reference(table, cen, m, den, mode)
            out, stats = C.wsd_restate(widen(table, dt), widen(cen, dt), coef, mode)
            if mode != "dist":
                assert torch.equal(bits(out), bits((O.double() / den).to(dt))), (dt, k, mode)
                assert torch.equal(out.double() * den, O.double())  # the exact rational value
            assert torch.equal(stats.view(torch.int64), C.wsd_expected_stats(D2, SS, den).view(torch.int64)), (dt, k, mode)
    O, D2, SS = C.wsd_reference(onehot, cen, m, den, "plain")
    lo = [C.chunk_map(sizes, ch, 1 << 40)[0][i % 3] for i in range(k)]
    assert SS.tolist() == [int((onehot[i, a:a + b].long() ** 2).sum()) for i, (a, b) in enumerate(lo)]
    assert all(int(onehot[i].long().abs().sum()) == int(onehot[i, a:a + b].long().abs().sum()) > 0
               for i, (a, b) in enumerate(lo))


def test_wsd_gpu_layouts_have_the_named_rows():
    """The row counts the GPU test names, and what each makes k_wsd_reduce do: (unrolled passes, tail
    steps) of the first and of the last of the 64 splits."""
    assert {p: C.wsd_reduce_steps(p) for p in C.WSD_ROWS} == {
        449: ((1, 0), (0, 7)),    # the first split alone enters the unrolled loop
        512: ((1, 0), (1, 0)),    # every split one unrolled pass, no tail
        513: ((1, 1), (1, 0)),    # one tail step
        1061: ((2, 1), (2, 0))}   # two unrolled passes, ragged tails
    assert C.wsd_reduce_steps(20001 // 4096 + 1) == ((0, 1), (0, 0))  # the older tests: no pass, one step
    for dt, k, p in C.WSD_CASES:
        n = C.wsd_single(p, dt)
        assert C.wsd_chunks([n], k, dt) == p and n % C.WSD_CHUNK[dt] == C.TAIL and n < 2 ** 23
        assert k * n * C.ELEM[dt] + k * n < 2 ** 30 * 0.75  # the placed inputs and the int8 table
        rows = C.wsd_named_rows(p)
        assert rows[0] == 0 and rows[-1] == p - 1 and set(rows) <= set(C.WSD_NAMED_ROWS) | {p - 1}
        assert len(rows) >= 5 and (p < 514 or set(C.WSD_NAMED_ROWS) <= set(rows))
    for dt in ALL_DT:
        sizes = C.wsd_model_sizes(dt)
        assert C.wsd_chunks(sizes, 3, dt) > 1024 and 0 in sizes
        assert sum(0 < s < C.WSD_CHUNK[dt] for s in sizes) >= 4
    assert C.wsd_chunks(C.wsd_model_sizes(torch.float64), 3, torch.float64) == \
        sum(-(-s // 2048) for s in C.wsd_model_sizes(torch.float64))
