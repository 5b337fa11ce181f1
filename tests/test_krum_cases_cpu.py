"""CPU side of the exact Krum tables (tests/krumcases.py): the float64 Gram-form reference == the C
oracle, bit for bit, on a small n for every table kind (dense, one-hot, every power-of-two scaling,
the rounded-difference oracle for bfloat16 / float16); the tables' preconditions (magnitudes, distinct
one-hot positions on the layout's boundaries, scaled values inside the normal range); the layouts
(segments whose boundaries fall inside a workgroup's run, four or five chunks per workgroup); and the
probe that reads the direct kernels' chunk size from the library.  tests/test_gpu_krum_exact.py runs
the HIP kernels over the same tables."""
from __future__ import annotations

import pytest
import torch

import krumcases as C

KS = [2, 8, 16, 32, 33, 64, 96, 100, 128]
SMALL_N = 301  # sums stay far below 2^24, so the oracle's rounded-difference sums are exact too


def _orc(rows, dtype):
    from oracle import orc
    if dtype == torch.float32:
        return orc.pairwise_sqdist(rows)
    return orc.pairwise_sqdist_rt(rows, dtype)


def _tables(K):
    pos = C.boundary_positions([SMALL_N], 16, 4, K)
    return {"dense": C.dense_table(K, SMALL_N), "onehot": C.onehot_table(K, SMALL_N, pos)}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=str)
@pytest.mark.parametrize("K", [2, 5, 23])
def test_reference_equals_oracle(K, dtype):
    for kind, table in _tables(K).items():
        ref = C.reference(table)
        if kind == "onehot":
            C.assert_exact(ref, C.onehot_expected(K), f"one-hot closed form K={K}")
        for s in (0,) + C.SCALES[dtype]:
            rows = [r.float() * 2.0 ** s for r in table]
            assert all(bool(torch.isfinite(r).all()) for r in rows)
            C.assert_exact(_orc(rows, dtype), C.scaled(ref, s), f"{kind} K={K} {dtype} s={s}")


@pytest.mark.parametrize("K", [2, 5, 23])
def test_reference_equals_float64_loop(K):
    """float64 tables (k_pairdist_f64's inputs) against the plain loop sum((x_i - x_j)^2), at 2^-300 too."""
    for kind, table in _tables(K).items():
        ref = C.reference(table)
        for s in (0,) + C.SCALES[torch.float64]:
            x = table.double() * 2.0 ** s
            loop = torch.stack([torch.stack([((x[i] - x[j]) ** 2).sum() for j in range(K)]) for i in range(K)])
            C.assert_exact(loop, C.scaled(ref, s), f"{kind} K={K} float64 s={s}")


def test_table_preconditions():
    t = C.dense_table(7, 5000)
    assert t.dtype == torch.int8 and int(t.min()) == -C.MAG and int(t.max()) == C.MAG
    assert (2 * C.MAG) ** 2 * C.RUN < 2 ** 24 and (2 * C.MAG) ** 2 * C.KPE < 2 ** 24
    with pytest.raises(AssertionError):
        C.check_exact(torch.full((2, 3), 128, dtype=torch.int16))  # (2 * 128)^2 * 256 = 2^24
    assert torch.equal(C.dense_table(7, 5000), t)  # seeded
    with pytest.raises(AssertionError):
        C.onehot_table(3, 10, [1, 1, 2])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, torch.float64], ids=str)
def test_scaled_cases_stay_in_range(dtype):
    """Every scaled difference is representable in the difference dtype and every square and run sum is
    a normal, finite number of the accumulating type (float32; float64 for float64 models)."""
    acc = torch.float64 if dtype == torch.float64 else torch.float32
    fi = torch.finfo(acc)
    for s in C.SCALES[dtype]:
        d = torch.arange(1, 2 * C.MAG + 1, dtype=torch.float64) * 2.0 ** s
        assert torch.equal(d.to(dtype).double(), d), (dtype, s)            # differences representable
        lo, hi = float(d[0]) ** 2, float(d[-1]) ** 2 * C.RUN
        assert fi.tiny <= lo and hi <= fi.max, (dtype, s, lo, hi)          # squares and runs normal
        assert float(torch.tensor(lo, dtype=acc)) == lo
    if dtype in (torch.float32, torch.bfloat16):
        assert 2.0 ** -110 <= (2.0 ** -55) ** 2 and (2 * C.MAG * 2.0 ** 50) ** 2 * C.RUN <= 2.0 ** 118


def test_poison_classes_equal_oracle():
    from oracle import orc
    K = 6
    for name, poison in C.poisons(K).items():
        x = C.dense_table(K, 40).float()
        for i, v in poison:
            x[i, 11] = v
        ref = orc.pairwise_sqdist(list(x))
        nan, inf = C.poison_classes(K, poison)
        assert torch.equal(torch.isnan(ref), nan) and torch.equal(torch.isposinf(ref), inf), name
        hit = {i for i, _ in poison}
        for i in range(K):
            for j in range(K):
                if i != j:
                    assert bool(nan[i, j] | inf[i, j]) == (i in hit or j in hit), (name, i, j)


# ------------------------------------------------------------------ the chunk probe and the layouts
@pytest.mark.parametrize("K", KS)
def test_pe_probe(K):
    pe = C.probe_pe(K)
    assert 16 <= pe <= 1024
    for n in (1, pe, pe + 1, 2 * pe, 2 * pe + 1, 7 * pe + 3, 1023 * pe + 1, C.total(pe), 10 ** 8):
        assert C.direct_chunks(K, n) == min(-(-n // pe), C.PAIR_BLOCKS), (K, pe, n)


def test_pe_known_values():
    """pair_split's chunk sizes as the kernel file documents them."""
    assert [C.probe_pe(K) for K in (8, 16, 100, 128)] == [128, 256, 144, 128]


def _chunks(K):
    return sorted({C.probe_pe(K), C.GRAM_CHUNK, C.F64_CHUNK})


@pytest.mark.parametrize("K", KS)
def test_layouts(K):
    for chunk in _chunks(K):
        n = C.total(chunk)
        single, model = [n], C.model_sizes(n, chunk)
        assert sum(model) == n and 0 in model and 1 in model and 5 in model and 3 * chunk in model
        assert 10 <= len(model) <= 14 and sorted(model)[-2] > 100 * chunk
        i = model.index(chunk // 2 + 3)  # shorter than a chunk, between two large pieces
        assert model[i - 1] > 100 * chunk and model[i + 1] > 100 * chunk
        for sizes in (single, model):
            chunks, ranges = C.chunk_map(sizes, chunk, C.PAIR_BLOCKS)
            assert len(ranges) == C.PAIR_BLOCKS and ranges[0][0] == 0 and ranges[-1][1] == len(chunks)
            per = [b - a for a, b in ranges]
            assert min(per) >= 4 and max(per) <= 5                      # past one chunk per workgroup
            assert sum(c[1] for c in chunks) == n and chunks[-1][1] != chunk  # a ragged tail
            if chunk == C.probe_pe(K):
                assert len(chunks) > C.direct_chunks(K, n) - 1
        # segment changes strictly inside a workgroup's run: into large pieces and into tiny ones
        chunks, ranges = C.chunk_map(model, chunk, C.PAIR_BLOCKS)
        seg = [C.segment_of(model, c[0]) for c in chunks]
        inside = {seg[c] for a, b in ranges for c in range(a + 1, b) if seg[c] != seg[c - 1]}
        assert len(inside) >= 5, inside
        assert any(model[s] > 100 * chunk for s in inside) and any(model[s] < chunk for s in inside), inside


@pytest.mark.parametrize("K", [2, 5, 33, 128])
def test_onehot_positions(K):
    for chunk in _chunks(K):
        n = C.total(chunk)
        for sizes in ([n], C.model_sizes(n, chunk)):
            pos = C.boundary_positions(sizes, chunk, C.PAIR_BLOCKS, K)
            assert len(pos) == K and len(set(pos)) == K and min(pos) >= 0 and max(pos) < n
            chunks, ranges = C.chunk_map(sizes, chunk, C.PAIR_BLOCKS)
            starts = {c[0] for c in chunks}
            ends = {c[0] + c[1] - 1 for c in chunks}
            assert all(p in starts or p in ends for p in pos)            # boundaries only
            if K == 128:
                second = {chunks[a + 1][0] for a, b in ranges}
                third = {chunks[a + 2][0] for a, b in ranges}
                assert 0 in pos and n - 1 in pos and set(pos) & second and set(pos) & third
                off = 0
                for s in sizes:
                    if s:
                        assert off in pos and off + s - 1 in pos
                    off += s
    # the small client counts together still reach the chunk boundaries inside a run
    n = C.total(128)
    sizes = C.model_sizes(n, 128)
    chunks, ranges = C.chunk_map(sizes, 128, C.PAIR_BLOCKS)
    inner = {chunks[c][0] for a, b in ranges for c in range(a + 1, b)}
    for K in (2, 3, 4, 5):
        assert set(C.boundary_positions(sizes, 128, C.PAIR_BLOCKS, K)) & inner, K


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize("aligned", [True, False])
def test_place(aligned, dtype):
    """The segments' views hold the table, start on (or one element past) a 16-byte boundary, and the
    gaps between them hold NaN."""
    table = C.dense_table(3, 700)
    sizes = C.model_sizes(700, 8)
    buf, segs = C.place(table, sizes, aligned, dtype)
    es = buf.element_size()
    assert buf.data_ptr() % 16 == 0 and buf.stride(0) * es % 16 == 0
    used = torch.zeros_like(buf, dtype=torch.bool)
    for i in range(3):
        assert torch.equal(torch.cat([seg[i] for seg in segs]), table[i].to(dtype))
        for seg in segs:
            if seg[i].numel() == 0:
                continue
            assert seg[i].is_contiguous() and seg[i].data_ptr() % 16 == (0 if aligned else es)
            lo = (seg[i].data_ptr() - buf.data_ptr()) // es - i * buf.stride(0)
            used[i, lo:lo + seg[i].numel()] = True
    assert bool(torch.isnan(buf[~used]).all()) and not bool(torch.isnan(buf[used]).any())
    assert int((~used).sum()) >= 3 * (len(sizes) - 1 if not aligned else 1)
