"""GPU parity of the coordinate-wise mean around the median (fa_coord_mean_around_median,
include/fedagg_robust.h; Bulyan's second stage): bit for bit, no element left out, against a CPU
reference that follows the contract's five steps -- sort the column (NaN last, -0.0 below +0.0), take
the lower median m = s[(K-1)/2], measure dist(v) = |v - m| in float64 (0 where v == m, +inf for NaN),
count lo = lomin + #{r in [lomin, lomax): dist(s[r]) > dist(s[r + keep])}, sum ranks lo .. lo+keep-1
in order in float64 from the first, divide, round once per format -- on the one-lane buckets
B = 8 .. 40, 56 and 64 and the two-lane ones N = 36, 48, 52 and 64 in float32 (16-bit types: K = 3, 6,
32, 40, 96), both sides of the one-lane / two-lane and two-lane / generic boundaries, all dtypes, ragged
and unaligned segments, the tiled and the client-major arena, hand-made columns with stated results, and
against the trimmed mean where the two operators coincide.  Both ends of EVERY bucket, in every dtype
and on inputs whose sums depend on their order, are tests/test_gpu_column_buckets.py's.

The reference (tests/trimcases.py) sorts with ``numpy.sort`` and repairs the order of -0.0 and +0.0, which
``numpy.sort`` leaves unspecified (``_order_zeros``).

Two data recipes.  "light" is the trimmed-mean test's (5 % each of -0.0 and +0.0, 2 % half-integer
ties, 0.1 % NaN, 1 % +-inf); it almost never makes a median infinite.  "heavy" rewrites the columns
e with e % 16 in 0..4: more than half the clients +inf / -inf / NaN (some with the sign bit set), all
values equal, two distinct values -- the columns on which the ``v == m`` rule, the restricted range of
step 4 and the NaN fall-back can go wrong on every path.
"""
from __future__ import annotations

import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

from trimcases import _column_data, _heavy, _keeps, _mam, _sorted_columns, assert_same, mam_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def eng():
    from fedml_amd.engine import get_engine
    return get_engine(0)


# the reference, the two data recipes and _keeps: tests/trimcases.py


@functools.lru_cache(maxsize=3)
def _case(seed, k, n, dtype, recipe):
    """(client tensors on the device, their sorted columns): computed once per case, shared by its keeps."""
    g = torch.Generator().manual_seed(seed)
    xs = _column_data(g, k, n, dtype, 0.05)
    if recipe == "heavy":
        xs = _heavy(g, xs)
    return [x.to(DEV) for x in xs], _sorted_columns(xs), xs


def test_heavy_recipe_has_what_it_promises():
    _, s, xs = _case(33, 33, 20001, torch.float32, "heavy")
    h = 16
    assert bool(np.isposinf(s[h, 0::16]).all()) and bool(np.isneginf(s[h, 1::16]).all())
    assert bool(np.isnan(s[h, 2::16]).all())
    assert bool((s[0, 3::16] == s[-1, 3::16]).all())
    a = torch.stack(xs)
    assert bool((a.view(torch.int32) == -4194304).any())
    assert int(np.isfinite(s[h]).sum()) > 12000


# ----------------------------------------------------------------------------- 1. float32, K across the buckets
F32_K = [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 24, 25, 32, 33, 40, 56, 57, 63, 64, 65, 72, 96, 100, 127, 128, 129, 150]


@pytest.mark.parametrize("recipe", ["light", "heavy"])
@pytest.mark.parametrize("k,keep", [(k, c) for k in F32_K for c in _keeps(k)])
def test_mean_around_median_f32(eng, k, keep, recipe):
    n = 3000 if k > 128 else 20001
    dev, s, _ = _case(k, k, n, torch.float32, recipe)
    got = eng.coord_mean_around_median([dev], keep)[0]
    assert_same(got, _mam(s, keep, torch.float32), f"K={k} keep={keep} {recipe}")


# ----------------------------------------------------------------------------- 2. dtypes
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float64])
@pytest.mark.parametrize("k,keep", [(k, c) for k in [3, 6, 32, 40, 96] for c in _keeps(k)])
def test_mean_around_median_dtypes(eng, dtype, k, keep):
    dev, s, _ = _case(100 + k, k, 5003, dtype, "heavy")
    got = eng.coord_mean_around_median([dev], keep)[0]
    assert_same(got, _mam(s, keep, dtype), f"{dtype} K={k} keep={keep}")


# ----------------------------------------------------------------------------- 3. ragged, unaligned
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("k", [2, 8, 17, 33, 65])
def test_mean_around_median_ragged_segments(eng, dtype, k, offset):
    """Six segments in one call, every client tensor and every output a view at an element offset."""
    keep = k - 2 * (k // 5)
    sizes = [1, 2, 3, 257, 4096, 3001]
    g = torch.Generator().manual_seed(300 + k)
    segs_cpu = [_heavy(g, _column_data(g, k, n, dtype, zeros=0.1)) for n in sizes]
    view = lambda t: torch.cat([t.new_zeros(offset), t]).to(DEV)[offset:]  # noqa: E731
    segs = [[view(x) for x in col] for col in segs_cpu]
    outs = [torch.zeros(n + offset, dtype=dtype, device=DEV)[offset:] for n in sizes]
    res = eng.coord_mean_around_median(segs, keep, outs=outs)
    for s, (col, o) in enumerate(zip(segs_cpu, res)):
        assert o.data_ptr() == outs[s].data_ptr()
        assert_same(o, mam_ref(col, keep), f"segment {s} K={k}")


# ----------------------------------------------------------------------------- 4. tiled == flat == reference
def _tiled_rows(xs, dtype, cap_extra=2):
    from fedml_amd.arena import ArenaLayout, ClientArena
    n = xs[0].numel()
    arena = ClientArena(ArenaLayout([("w", (n,), dtype)]), len(xs) + cap_extra, device=DEV, tiled=True)
    rows = list(range(cap_extra, cap_extra + len(xs)))
    for r, x in zip(rows, xs):
        arena.write(r, {"w": x.to(DEV)})
    return arena, rows


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("k", [5, 33, 64, 100, 128])
def test_mean_around_median_tiled_equals_flat(eng, dtype, k):
    keep = k - 2 * (k // 5)
    per_tile = 4096 // (4 if dtype == torch.float32 else 2)
    n = 2 * per_tile + 777
    g = torch.Generator().manual_seed(400 + k)
    xs = _heavy(g, _column_data(g, k, n, dtype, zeros=0.15))
    arena, rows = _tiled_rows(xs, dtype)
    exp = mam_ref(xs, keep)
    assert_same(eng.coord_mean_around_median_tiled(arena.bufs[dtype], rows, keep, n=n), exp, "tiled")
    assert_same(eng.coord_mean_around_median([[x.to(DEV) for x in xs]], keep)[0], exp, "flat")
    assert_same(arena.mean_around_median(keep, rows)["w"], exp, "ClientArena(tiled=True)")
    # a row subset in non-ascending order: the kernel reads only those rows, in place
    perm = torch.randperm(k, generator=g).tolist()[:max(1, k - 2)]
    if perm == sorted(perm):
        perm.reverse()
    ks = min(keep, len(perm))
    exp = mam_ref([xs[i] for i in perm], ks)
    assert_same(arena.mean_around_median(ks, [rows[i] for i in perm])["w"], exp, "tiled subset")
    assert_same(eng.coord_mean_around_median([[xs[i].to(DEV) for i in perm]], ks)[0], exp, "flat subset")


# ----------------------------------------------------------------------------- 5. client-major arena
def test_client_major_arena_per_key(eng):
    from fedml_amd.arena import ArenaLayout, ClientArena
    g = torch.Generator().manual_seed(12)
    shapes = [("conv.weight", (16, 3, 3, 3), torch.float32), ("conv.bias", (16,), torch.float32),
              ("emb.weight", (37, 29), torch.bfloat16), ("fc.weight", (10, 300), torch.float32),
              ("emb.scale", (29,), torch.bfloat16)]
    K, keep = 12, 4
    ds = [OrderedDict((k, _column_data(g, 1, int(np.prod(s)), dt)[0].view(s)) for k, s, dt in shapes) for _ in range(K)]
    arena = ClientArena(ArenaLayout(shapes), K + 1, device=DEV, tiled=False)
    for i, d in enumerate(ds):
        arena.write(i + 1, OrderedDict((k, v.to(DEV)) for k, v in d.items()))
    rows = [5, 1, 12, 3, 2, 4, 9, 8, 7]  # a subset, not ascending
    out = arena.mean_around_median(keep, rows)
    assert list(out) == [k for k, _, _ in shapes]
    for k, s, dt in shapes:
        assert out[k].shape == torch.Size(s) and out[k].dtype == dt
        assert_same(out[k].reshape(-1), mam_ref([ds[r - 1][k].reshape(-1) for r in rows], keep), k)


# ----------------------------------------------------------------------------- 6. hand-made columns
_NAN, _INF = float("nan"), float("inf")
HAND = [
    ([0, 1, 2, 3, 4], 2, 1.5),  # the tie goes left
    ([0, 1, 2, 3, 4], 3, 2.0),
    ([0, 1, 2, 3, 4], 4, 1.5),
    ([0, 0, 0, 0, 10], 3, 0.0),
    ([-1e30, 1e-30, 1e30], 3, 0.0),  # in rank order only
    ([-0.0, -0.0, 0.0], 1, -0.0),
    ([1, 2, 3, 4, _INF, _INF, _INF, _INF, _INF], 2, _INF),
    ([-_INF, 0, 1, 2, _INF], 3, 1.0),
    ([-_INF, 0, 1, 2, _INF], 5, _NAN),
    ([1, 2, 3, _NAN, _NAN], 2, 2.5),
    ([1, 2, 3, _NAN, _NAN], 3, 2.0),
    ([1, 2, 3, _NAN, _NAN], 4, _NAN),
    ([1, _NAN, _NAN], 1, _NAN),
    ([1, _NAN, _NAN], 2, _NAN),
    ([1, _NAN, _NAN], 3, _NAN),
]


@pytest.mark.parametrize("col,keep,expected", HAND)
def test_hand_made_columns(eng, col, keep, expected):
    k = len(col)
    reps = 70  # more than one wave; every replica has the clients in another rotation
    m = torch.tensor([[col[(i + r) % k] for r in range(reps)] for i in range(k)], dtype=torch.float32)
    got = eng.coord_mean_around_median([[m[i].contiguous().to(DEV) for i in range(k)]], keep)[0].cpu()
    exp = torch.full((reps,), expected, dtype=torch.float32)
    assert_same(got, exp, f"{col} keep={keep}")
    assert_same(mam_ref([m[i].contiguous() for i in range(k)], keep), exp, "the reference itself")


# ----------------------------------------------------------------------------- 7. against the trimmed mean
@pytest.mark.parametrize("k", [5, 33, 64, 65, 127])
def test_keep_all_is_the_trimmed_mean_with_trim_0(eng, k):
    dev, _, _ = _case(600 + k, k, 20001, torch.float32, "heavy")
    assert_same(eng.coord_mean_around_median([dev], k)[0], eng.coord_trimmed_mean([dev], 0)[0], f"K={k}")


@pytest.mark.parametrize("k", [5, 33, 65, 127])
def test_keep_one_on_odd_k_is_the_full_trim(eng, k):
    dev, _, _ = _case(600 + k, k, 20001, torch.float32, "heavy")
    assert_same(eng.coord_mean_around_median([dev], 1)[0], eng.coord_trimmed_mean([dev], (k - 1) // 2)[0], f"K={k}")


# ----------------------------------------------------------------------------- 8. errors
def test_mean_around_median_errors(eng):
    from fedml_amd import _native as N
    K, n = 6, 100
    xs = [torch.randn(n, device=DEV) for _ in range(K)]
    for bad in (0, K + 1, -1, 1.5):
        with pytest.raises(ValueError):
            eng.coord_mean_around_median([xs], bad)
    with pytest.raises(TypeError):
        eng.coord_mean_around_median([[x.to(torch.int64) for x in xs]], 1)
    arena, rows = _tiled_rows([x.cpu() for x in xs], torch.float32)
    for bad in (0, K + 1):
        with pytest.raises(ValueError):
            eng.coord_mean_around_median_tiled(arena.bufs[torch.float32], rows, bad, n=n)
        with pytest.raises(ValueError):
            arena.mean_around_median(bad, rows)
    out = torch.full((n,), 7.0, device=DEV)
    L = N.lib()
    ptrs, outp = N.ptr_array([x.data_ptr() for x in xs]), N.ptr_array([out.data_ptr()])
    for bad in (0, K + 1):
        rc = L.fa_coord_mean_around_median(eng._ctx, N.F32, 1, N.i64_array([n]), K, bad, ptrs, outp, None)
        assert rc == N.FA_ERR_INVALID and b"keep" in L.fa_last_error()
        assert b"fa_coord_mean_around_median:" in L.fa_last_error()
        rc = L.fa_coord_mean_around_median_tiled(eng._ctx, N.F32, 1, N.i64_array([n]), K, bad, ptrs, 4096, outp, None)
        assert rc == N.FA_ERR_INVALID and b"keep" in L.fa_last_error()
        assert b"fa_coord_mean_around_median_tiled:" in L.fa_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing was launched
