"""CPU check of tests/trimcases.py: the trimmed-mean and mean-around-the-median references on
hand-computed columns with stated float64 results, the bucket list, and the condition that makes
``cancel_columns`` worth running -- on a stated share of its columns the output bits depend on the
order of the float64 sum.  That condition is a property of the inputs, not a tolerance: every GPU
comparison on them is bit for bit (tests/test_gpu_column_buckets.py)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from trimcases import (_mam, _sorted_columns, _walk, _window, bucket_ks, cancel_columns, mam_ref, order_share,
                       trimmed_mean_ref)

NAN, INF = float("nan"), float("inf")
H = 1.5 * 2.0 ** 60  # a float32 value; float64 values in [2^60, 2^61) are 256 apart


def _cols(col, dtype=torch.float32):
    """One column as K one-element client tensors."""
    return [torch.tensor([v], dtype=dtype) for v in col]


def _bits(t):
    return int(t.view(torch.int32 if t.dtype == torch.float32 else torch.int64))


# ----------------------------------------------------------------------------- the references, by hand
TRIMMED = [
    # column, b, the float64 quotient
    ([5.0, -1.0, 3.0, 100.0, -50.0], 1, 7.0 / 3.0),        # -1 + 3 + 5
    ([5.0, -1.0, 3.0, 100.0, -50.0], 0, 57.0 / 5.0),
    ([5.0, -1.0, 3.0, 100.0, -50.0], 2, 3.0),
    ([1.0, NAN, 2.0], 1, 2.0),                               # NaN is the largest: 1, 2, NaN
    ([1.0, NAN, 2.0], 0, NAN),
    ([-INF, 4.0, INF, 6.0], 1, 5.0),
    ([-INF, 4.0, INF, 6.0], 0, NAN),                         # -inf + inf
    ([-0.0, 0.0, -0.0], 1, -0.0),                            # -0, -0, +0: rank 1 is -0
    ([0.0, -0.0, 0.0], 1, 0.0),                              # -0, +0, +0
    ([0.0, -0.0, 0.0, -0.0], 0, 0.0),                        # -0 + -0 + 0 + 0
    ([1e30, 1e-30, -1e30], 0, 0.0),                          # -1e30 + 1e-30 = -1e30, + 1e30 = 0
    # -H + 160 = -(H - 256) (96 from it, 160 from -H), + 160 = -(H - 416) -> -(H - 512), + H = 512
    ([H, 160.0, -H, 160.0], 0, 128.0),
    # -H + 100 = -H three times over, + H = 0
    ([100.0, H, 100.0, -H, 100.0], 0, 0.0),
]


@pytest.mark.parametrize("col,b,q", TRIMMED)
def test_trimmed_mean_reference_by_hand(col, b, q):
    got = trimmed_mean_ref(_cols(col), b)
    exp = torch.tensor([q], dtype=torch.float64).to(torch.float32)
    assert got.dtype == torch.float32
    assert bool(torch.isnan(got)) == bool(torch.isnan(exp))
    if q == q:
        assert _bits(got) == _bits(exp), (col, b, got.item())
    got64 = trimmed_mean_ref(_cols(col, torch.float64), b)  # float32 values: the same float64 sum
    assert got64.dtype == torch.float64 and (_bits(got64) == _bits(torch.tensor([q], dtype=torch.float64)) or q != q)


def test_rank_order_and_halves_order_give_different_bits():
    """[-H, 100, 100, 100, H], H = 1.5 * 2^60.  Rank order: -H + 100 = -H (100 < 128) three times, + H = 0,
    so the mean is 0.0 (0x00000000).  Two halves, ranks 0-1 and 2-4: -H + 100 = -H, and 100 + 100 + 100 =
    300, + H = H + 256; together 256, so the mean is 51.2 (float32 0x424CCCCD).  The contract is the
    first."""
    s = _sorted_columns(_cols([100.0, H, 100.0, -H, 100.0]))
    assert s[:, 0].tolist() == [-H, 100.0, 100.0, 100.0, H]
    assert ((-H + 100.0) + 100.0 + 100.0) + H == 0.0 and (-H + 100.0) + ((100.0 + 100.0) + 100.0 + H) == 256.0
    assert _bits(_walk(s, 0, torch.float32)) == 0x00000000
    assert _bits(torch.tensor([256.0 / 5.0], dtype=torch.float64).to(torch.float32)) == 0x424CCCCD
    assert order_share(s, 0, 5, torch.float32) == 1.0
    assert order_share(s, 0, 5, torch.float64) == 1.0
    assert order_share(s, 1, 4, torch.float32) == 0.0  # 100 + 100 + 100 either way
    # four clients: one small value per half, rounded the same way next to -H and next to +H
    s = _sorted_columns(_cols([H, 160.0, -H, 160.0]))
    assert order_share(s, 0, 4, torch.float32) == 0.0
    # and a column of small values: exact in any order
    s = _sorted_columns(_cols([0.1, -2.5, 3.25, 7.0, -1.0]))
    assert order_share(s, 0, 5, torch.float32) == 0.0


MAM = [
    # column, keep, the float64 quotient (tests/test_gpu_mean_around_median.py runs these on the device too)
    ([0, 1, 2, 3, 4], 2, 1.5),                # the tie goes left
    ([0, 1, 2, 3, 4], 3, 2.0),
    ([0, 0, 0, 0, 10], 3, 0.0),
    ([-1e30, 1e-30, 1e30], 3, 0.0),           # in rank order only
    ([-0.0, -0.0, 0.0], 1, -0.0),
    ([-INF, 0, 1, 2, INF], 3, 1.0),
    ([-INF, 0, 1, 2, INF], 5, NAN),
    ([1, 2, 3, NAN, NAN], 2, 2.5),
    ([1, NAN, NAN], 1, NAN),
    # -H + 160 = -(H - 256); + 160 = -(H - 416) -> -(H - 512); + 170 = -(H - 682) -> -(H - 768); + H = 768
    ([H, 160.0, -H, 160.0, 170.0], 5, 768.0 / 5.0),
    ([1.0, 2.0, 10.0, 11.0, 12.0, 13.0, 30.0], 3, 11.0),  # m = 11: 10, 11, 12
]


@pytest.mark.parametrize("col,keep,q", MAM)
def test_mean_around_median_reference_by_hand(col, keep, q):
    got = mam_ref(_cols([float(v) for v in col]), keep)
    exp = torch.tensor([q], dtype=torch.float64).to(torch.float32)
    assert bool(torch.isnan(got)) == bool(torch.isnan(exp))
    if q == q:
        assert _bits(got) == _bits(exp), (col, keep, got.item())


def test_window_by_hand():
    s = _sorted_columns(_cols([1.0, 2.0, 10.0, 11.0, 12.0, 13.0, 30.0]))
    m, lo = _window(s, 3)
    assert m.tolist() == [11.0] and lo.tolist() == [2]
    m, lo = _window(s, 4)  # 10 .. 13: dist(2) = 9 > dist(13) = 2 moves the start to 2
    assert lo.tolist() == [2]
    m, lo = _window(s, 7)
    assert lo.tolist() == [0]


# ----------------------------------------------------------------------------- the buckets
def test_bucket_ks():
    ks = bucket_ks()
    assert len(ks) == 32 and ks == sorted(set(ks)) and ks[0] == 1 and ks[-1] == 128
    assert [(k + 7) // 8 for k in ks] == [q for q in range(1, 17) for _ in range(2)]
    assert all(k % 8 in (0, 1) for k in ks)


# ----------------------------------------------------------------------------- cancel_columns
N = 4099
KS = [8, 16, 33, 64, 65, 100, 128]
DTYPES = [torch.float32, torch.float64, torch.bfloat16, torch.float16]


def _sorted_case(k, dtype):
    return _sorted_columns(cancel_columns(k, N, dtype, 7000 + k))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 3, 8, 33, 128])
def test_cancel_columns_shape(dtype, k):
    xs = cancel_columns(k, 257, dtype, 5)
    assert len(xs) == k and all(x.shape == (257,) and x.dtype == dtype and x.is_contiguous() for x in xs)
    again = cancel_columns(k, 257, dtype, 5)
    assert all(torch.equal(a, b) for a, b in zip(xs, again))
    m = torch.stack(xs).to(torch.float64)
    assert bool(torch.isfinite(m).all())
    p = k // 4
    big = 16.0 if dtype == torch.float16 else 2.0 ** 40
    s = m.sort(dim=0).values
    if p:
        assert bool((s[:p] == -s.flip(0)[:p]).all())  # -H is exact: the extremes mirror each other
        assert bool((s[:p] <= -big).all())
        if k >= 8:  # shuffled per column: no client holds one sign of H throughout
            assert all(bool((row <= -big).any()) and bool((row >= big).any()) for row in m)
    assert bool((s[p:k - p].abs() < 2.0 ** 14).all())  # randn 2^10: six sigma


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("k", KS)
def test_trimmed_sums_depend_on_their_order(dtype, k):
    """Measured (n = 4099): float32 0.216 (K = 8, b = 0) .. 0.84, float64 0.252 (K = 8, b = 1) .. 0.93."""
    s = _sorted_case(k, dtype)
    for b in sorted({0, 1, k // 10}):
        share = order_share(s, b, k - b, dtype)
        assert share >= 0.15, (k, b, share)


@pytest.mark.parametrize("k", [k for k in KS if k >= 16])
def test_trimmed_sums_depend_on_their_order_bf16(k):
    """b = 0 only: with 8 significant bits the larger trims fall to 0.03 .. 0.3.  Measured: 0.26
    (K = 16) .. 0.84."""
    s = _sorted_case(k, torch.bfloat16)
    share = order_share(s, 0, k, torch.bfloat16)
    assert share >= 0.15, (k, share)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("k", KS)
def test_window_sums_depend_on_their_order(dtype, k):
    """keep = K - 2 (K // 5), on the window the reference picks (it is the centred one: the +-H mirror
    each other around a small median).  Measured: 0.252 (K = 8) .. 0.91."""
    s = _sorted_case(k, dtype)
    keep = k - 2 * (k // 5)
    _, lo = _window(s, keep)
    share = order_share(s, lo, lo + keep, dtype)
    assert share >= 0.15, (k, keep, share)
    assert np.isfinite(_mam(s, keep, dtype).numpy()).all()


@pytest.mark.parametrize("k", KS)
def test_float16_sums_are_exact_in_any_order(k):
    """float16 values are multiples of 2^-24 below 2^16, so a float64 sum of 128 of them (47 bits) is
    exact whatever its order: no recipe can make float16 order-sensitive, and none is asked to."""
    s = _sorted_case(k, torch.float16)
    for b in sorted({0, 1, k // 10}):
        assert order_share(s, b, k - b, torch.float16) == 0.0
