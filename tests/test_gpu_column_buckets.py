"""GPU parity of EVERY shipped instantiation of the column-sort kernels (fedml_amd/csrc/trimmed.hip,
median.hip), bit for bit against the CPU references of tests/trimcases.py and the C oracle.

The kernels are one template instantiation per bucket of clients, B = K rounded up to 8: one lane per
column on MidNet<B> / SortNet<B> for B = 8 .. 64 (the median also a FULL variant for K == B, and up to
B = 128 when forced), two lanes per column on SortNet<N> + BitonicLo / Hi<N> for N = B / 2 = 36 .. 64.
``bucket_ks()`` is both ends of every bucket: K = 8Q (no sentinel; FULL) and K = 8Q - 7 (seven), so each
instantiation runs, in float32, bfloat16 and float16; float64 (the rank kernels) at K = 9, 65, 129.

n = 773 columns: a one-lane workgroup owns 256 columns and a two-lane one 128, so three or six full
tiles and a ragged one.  The tiled addressing does not depend on the bucket and stays with the older
files.

Two kinds of data.  ``cancel_columns`` makes the float64 sum's ORDER matter -- the contract sums in rank
order from the first kept value, which the two-lane kernels keep by handing a running float64 from the
lower lane to the upper one -- and where tests/test_trim_cases_cpu.py pins that condition it is asserted
here too, on these very columns, before the comparison: a kernel that added its lanes' partial sums, or
started from +0.0, fails.  Its reference must be finite, so the fast path and not the in-order fall-back
produced the result.  The older files' "light" and "heavy" recipes bring zeros of both signs, ties, NaN
and infinities to every bucket, and ``_special_columns`` subnormals, +-max and odd NaNs to the trimmed
kernels (a flushing min / max or float32 -> float64 convert changes those bits).
"""
from __future__ import annotations

import pytest
import torch

from trimcases import (_column_data, _heavy, _keeps, _mam, _sorted_columns, _special_columns, _walk, _window,
                       assert_same, bucket_ks, cancel_columns, order_share)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 773
SHARE = 0.15
DT3 = [torch.float32, torch.bfloat16, torch.float16]
F64_K = [9, 65, 129]
INT_VIEW = {8: torch.int64, 4: torch.int32, 2: torch.int16}


@pytest.fixture(scope="module")
def eng():
    from fedml_amd.engine import get_engine
    return get_engine(0)


def _dev(xs):
    """The clients as rows of one device buffer (one copy), every row 4-byte aligned."""
    k, n = len(xs), xs[0].numel()
    buf = torch.zeros(k, n + (n & 1), dtype=xs[0].dtype)
    buf[:, :n] = torch.stack(xs)
    d = buf.to(DEV)
    return [d[i, :n] for i in range(k)]


def _data(recipe, k, dtype):
    if recipe == "cancel":
        return cancel_columns(k, N, dtype, 7000 + k)
    g = torch.Generator().manual_seed(k)
    xs = _column_data(g, k, N, dtype, 0.05)
    return _heavy(g, xs) if recipe == "heavy" else xs


def _trims(k):
    return sorted({b for b in (0, 1, k // 10, (k - 1) // 2) if 2 * b < k})


def _trim_order_matters(dtype, k, b):
    """The cases whose order share tests/test_trim_cases_cpu.py pins (float16 sums are exact)."""
    if dtype in (torch.float32, torch.float64):
        return k >= 8 and b in (0, 1, k // 10)
    return dtype == torch.bfloat16 and k >= 16 and b == 0


def _check_trimmed(eng, dtype, k, recipe):
    xs = _data(recipe, k, dtype)
    s, dev = _sorted_columns(xs), _dev(xs)
    for b in _trims(k):
        exp = _walk(s, b, dtype)
        if recipe == "cancel":
            assert bool(torch.isfinite(exp).all()), (k, b)
            if _trim_order_matters(dtype, k, b):
                share = order_share(s, b, k - b, dtype)
                assert share >= SHARE, (k, b, share)
        assert_same(eng.coord_trimmed_mean([dev], b)[0], exp, f"{dtype} K={k} b={b} {recipe}")


def _check_mam(eng, dtype, k, recipe):
    xs = _data(recipe, k, dtype)
    s, dev = _sorted_columns(xs), _dev(xs)
    for keep in _keeps(k):
        exp = _mam(s, keep, dtype)
        if recipe == "cancel":
            assert bool(torch.isfinite(exp).all()), (k, keep)
            if dtype in (torch.float32, torch.float64) and k >= 8 and keep == k - 2 * (k // 5):
                _, lo = _window(s, keep)
                share = order_share(s, lo, lo + keep, dtype)
                assert share >= SHARE, (k, keep, share)
        assert_same(eng.coord_mean_around_median([dev], keep)[0], exp, f"{dtype} K={k} keep={keep} {recipe}")


# ----------------------------------------------------------------------------- 1. trimmed mean
@pytest.mark.parametrize("recipe", ["cancel", "light"])
@pytest.mark.parametrize("k", bucket_ks())
@pytest.mark.parametrize("dtype", DT3)
def test_trimmed_mean_every_bucket(eng, dtype, k, recipe):
    _check_trimmed(eng, dtype, k, recipe)


@pytest.mark.parametrize("recipe", ["cancel", "light"])
@pytest.mark.parametrize("k", F64_K)
def test_trimmed_mean_f64(eng, k, recipe):
    _check_trimmed(eng, torch.float64, k, recipe)


# ----------------------------------------------------------------------------- 2. mean around the median
@pytest.mark.parametrize("recipe", ["cancel", "heavy"])
@pytest.mark.parametrize("k", bucket_ks())
@pytest.mark.parametrize("dtype", DT3)
def test_mean_around_median_every_bucket(eng, dtype, k, recipe):
    _check_mam(eng, dtype, k, recipe)


@pytest.mark.parametrize("recipe", ["cancel", "heavy"])
@pytest.mark.parametrize("k", F64_K)
def test_mean_around_median_f64(eng, k, recipe):
    _check_mam(eng, torch.float64, k, recipe)


# ----------------------------------------------------------------------------- 3. median
def _check_median(eng, dtype, k):
    """A selection: the result is one of the inputs, the first NaN included, so plain bit equality."""
    from oracle import orc
    xs = _data("light", k, dtype)
    got, exp = eng.coord_median([_dev(xs)])[0].cpu(), orc.coord_median(xs)
    assert_same(got, exp, f"{dtype} K={k}")
    iv = INT_VIEW[got.element_size()]
    assert torch.equal(got.view(iv), exp.view(iv)), f"{dtype} K={k}: NaN bits"


@pytest.mark.parametrize("k", bucket_ks())
def test_median_one_lane_f32(eng, k, monkeypatch):
    """k_median_off<B>, FULL and not, for all of B = 8 .. 128."""
    monkeypatch.setenv("FA_MEDIAN_LANES", "1")
    _check_median(eng, torch.float32, k)


@pytest.mark.parametrize("k", [k for k in bucket_ks() if k > 64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_median_two_lanes(eng, dtype, k, monkeypatch):
    """k_median_2l<N>, FULL and not, N = 36 .. 64."""
    monkeypatch.setenv("FA_MEDIAN_LANES", "2")
    _check_median(eng, dtype, k)


@pytest.mark.parametrize("k", [k for k in bucket_ks() if k <= 64])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_median_packed_16bit(eng, dtype, k):
    """k_median_pk<B>: 4-byte aligned 16-bit columns, two per lane; the odd 773rd column alone."""
    xs = _dev(_data("light", k, dtype))
    assert all(x.data_ptr() % 4 == 0 for x in xs)
    _check_median(eng, dtype, k)


@pytest.mark.parametrize("k", F64_K)
def test_median_f64(eng, k):
    _check_median(eng, torch.float64, k)


# ----------------------------------------------------------------------------- 4. special bit patterns
@pytest.mark.parametrize("k", [7, 64, 100])
@pytest.mark.parametrize("dtype", DT3)
def test_trimmed_kernels_on_special_values(eng, dtype, k):
    """Subnormals of both signs, +-max, +-0, +-inf, signalling and negative NaNs through the full sorts,
    the mergers, the float32 -> float64 converts and the stores of both trimmed kernels."""
    xs = _special_columns(torch.Generator().manual_seed(1000 + k), k, N, dtype)
    s, dev = _sorted_columns(xs), _dev(xs)
    sub = torch.stack(xs).to(torch.float32)
    assert bool(((sub != 0) & (sub.abs() < torch.finfo(dtype).tiny)).any())
    assert k < 64 or bool(torch.isnan(sub).any())  # about 0.05 % of the values
    for b in (0, 2):
        assert_same(eng.coord_trimmed_mean([dev], b)[0], _walk(s, b, dtype), f"{dtype} K={k} b={b}")
    for keep in (3, k - 2):
        assert_same(eng.coord_mean_around_median([dev], keep)[0], _mam(s, keep, dtype), f"{dtype} K={k} keep={keep}")
