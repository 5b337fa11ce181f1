"""The numpy restatement of the rotation contract (tests/rhtcases.py) against an independent reference:
on integer tables every partial sum is an integer below 2^24, so no add rounds, the stage order cannot
matter, and the staged float32 butterflies must equal the float64 product with the explicit Hadamard
matrix bit for bit; and the inverse undoes the forward within one rounding per stage and scale."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rhtcases as R  # noqa: E402

SEED, ROUND, SEG = 0x0123456789ABCDEF, 7, 3


def int_table(rng, n):
    return rng.integers(-1024, 1025, n).astype(np.float32)


@pytest.mark.parametrize("b", range(5, 14))
def test_stages_equal_the_hadamard_matrix_on_integers(b):
    B = 1 << b
    x = int_table(np.random.default_rng(b), 2 * B)
    i = np.arange(B)
    pop = np.zeros((B, B), np.int64)
    for p in range(b):
        pop += ((i[:, None] & i[None, :]) >> p) & 1
    H = (1 - 2 * (pop & 1)).astype(np.float64)  # Sylvester order: H[i, j] = (-1)^popcount(i & j)
    exp = (x.astype(np.float64).reshape(2, B) @ H).reshape(-1)
    assert np.abs(exp).max() < 2 ** 24 and 1024 * B <= 2 ** 24  # the bound on every partial sum
    got = R.stages(x, b)
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), exp)


def test_signs_take_the_stream_bit_by_bit():
    from dpcases import words
    s = R.signs(SEED, ROUND, SEG, 300)
    w = words(SEED, ROUND, SEG, 0, 3)
    for e in (0, 1, 31, 32, 127, 128, 299):
        assert s[e] == ((int(w[e >> 7, (e >> 5) & 3]) >> (e & 31)) & 1) << 31
    assert 100 < np.count_nonzero(s) < 200


@pytest.mark.parametrize("b", range(5, 14))
def test_inverse_undoes_forward(b):
    rng = np.random.default_rng(100 + b)
    n = 3 * (1 << b) + 17
    x = (rng.standard_normal(n) * np.exp(3 * rng.standard_normal(n))).astype(np.float32)
    y = R.forward(x, b, SEED, ROUND, SEG)
    assert y.size == 4 << b
    back = R.inverse(y, n, b, SEED, ROUND, SEG).astype(np.float64)
    err = np.linalg.norm(back - x) / np.linalg.norm(x)
    print(f"b={b}: normwise relative error {err:.3g}, bound {(2 * b + 2) * 2.0 ** -24:.3g}")
    assert err <= (2 * b + 2) * 2.0 ** -24  # one rounding per stage and scale, in each direction
