"""Inputs for LightSecAgg's mask decoding (fa_lcc_decode, fedml_amd/csrc/finite.hip) and the plain
reference they are held against.  No tests here: tests/test_lcc_cases_cpu.py pins the reference to
Python-int arithmetic and to the C oracle and checks the builders themselves,
tests/test_gpu_lcc_decode.py runs the HIP kernels over the same cases.  Everything is built in code
from fixed seeds, on the CPU.

The reference is the reference implementation's own expression on numpy int64,
np.mod(coef.dot(F), p).reshape(-1)[:n_out]: its two's-complement wrap on * and + is the contract, so
every comparison is torch.equal on int64 and nothing carries a tolerance.

The shapes are chosen around the kernels' constants.  k_lcc_decode_f64 walks the output rows in
passes of RBF = 32 (kRBF), stages coefficients in LDS chunks of LDS_I = 128 rows of F (kLdsI) and
prefetches F through a ring of PF = 4 rows (kPF); k_lcc_decode works in register blocks of RB = 8
rows (kRB); both give one column to each of BLOCK = 256 threads.  Whoever changes one of those
constants moves GRID, MS and the positions of HOST_* with it."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

RB, RBF, PF, LDS_I, BLOCK = 8, 32, 4, 128, 256

P15 = 2 ** 15 - 19   # float64 path for every k of the grid: (p - 1)^2 * 300 < 2^39
P31 = 2 ** 31 - 1    # int64 path: (p - 1)^2 is just under 2^62, so sums of three or more products wrap
P27 = 2 ** 27 - 39   # a prime past the float64 limit at k = 160 whose sums of 200 products do not wrap
P61 = 2 ** 61 - 1
P63 = 2 ** 63 - 25

# (rows_needed, k): around the register block (8), the row pass (32), the ring (4) and the LDS chunk (128)
GRID = ([(1, k) for k in (1, 3, 4, 5)] +
        [(r, k) for r in (8, 9, 31, 32, 33) for k in (5, 128)] +
        [(r, k) for r in (64, 65) for k in (127, 128, 129, 131)] +
        [(33, 160), (65, 257), (40, 300)])
# columns: one, around one workgroup, three full workgroups and a ragged fourth
MS = (1, 255, 256, 257, 777)
EXTRA_ROWS = 2       # coefficient rows past rows_needed in the `rows > rows_needed` runs

BOUNDARY_KS = (5, 129, 160, 300)
BOUNDARY_P_HI = {5: 42443373, 129: 8356031, 160: 7503000, 300: 5479416}
BOUNDARY_ROWS, BOUNDARY_M = 33, 257

# host path choice and redo: three row passes (the last of 8 rows), two LDS chunks (128 + 3 rows of F,
# so the ring's loads are clamped in the second), three full workgroups and a ragged fourth
HOST_P, HOST_ROWS, HOST_K, HOST_M = P15, 40, 131, 777
HOST_BAD_F = {"neg": -5, "p": HOST_P, "p_plus_7": HOST_P + 7, "low_word_in_range": 2 ** 32 + 5,
              "2_62": 2 ** 62 + 11, "int64_min": -2 ** 63, "int64_max": 2 ** 63 - 1}
HOST_F_ROWS = (0, 127, 128, 130)          # first row, last of chunk 0, first of chunk 1, the clamped tail
HOST_F_COLS = (0, 200, 255, 256, 776)     # 200: wave 3 of block 0 alone; 776: the column dead lanes re-read
HOST_BAD_COEF = {"neg": -1, "p": HOST_P, "p_plus_3": HOST_P + 3}

# protocol round trip: N clients, U survivors needed, T colluders tolerated
RT_N, RT_U, RT_T = 200, 160, 80
RT_CASES = ((P15, 300), (P27, 64))        # (p, m): float64 path, two chunks, three passes / int64 path


# ------------------------------------------------------------------ the reference
def reference(coef: torch.Tensor, F: torch.Tensor, p: int, n_out: int | None = None) -> torch.Tensor:
    """np.mod(coef.dot(F), p).reshape(-1)[:n_out] on numpy int64 (wrapping * and +)."""
    c, f = coef.numpy(), F.numpy()
    assert c.dtype == np.int64 and f.dtype == np.int64
    with np.errstate(over="ignore"):
        out = np.mod(c.dot(f), np.int64(p)).reshape(-1)
    return torch.from_numpy(out if n_out is None else out[:n_out].copy())


def python_reference(coef, F, p: int) -> list:
    """The same product on Python ints, every * and + wrapped by lightsecagg._w64; rows of lists."""
    from fedml_amd.core.mpc.lightsecagg import _w64
    rows, k, m = len(coef), len(F), len(F[0])
    out = []
    for j in range(rows):
        row = []
        for c in range(m):
            acc = 0
            for i in range(k):
                acc = _w64(acc + _w64(int(coef[j][i]) * int(F[i][c])))
            row.append(acc % p)
        out.append(row)
    return out


# ------------------------------------------------------------------ the tiling grid
def _uniform(g, shape, p):
    return torch.randint(0, p, shape, generator=g, dtype=torch.int64)


def striped(rows: int, k: int, m: int, p: int, seed: int, zero_row: bool = True):
    """(coef rows x k, F k x m), uniform in [0, p).  The last row and the last column of coef and the
    last row and the middle column of F hold p - 1, so one output entry sums k products of (p - 1)^2
    less the zero row's; with k >= 3 and zero_row the middle row of F is all zero."""
    g = torch.Generator().manual_seed(seed)
    coef, F = _uniform(g, (rows, k), p), _uniform(g, (k, m), p)
    coef[rows - 1, :] = p - 1
    coef[:, k - 1] = p - 1
    F[k - 1, :] = p - 1
    F[:, (m - 1) // 2] = p - 1
    if zero_row and k >= 3:
        F[k // 2, :] = 0
    return coef, F


@functools.lru_cache(maxsize=None)
def grid_case(rows: int, k: int, m: int, p: int):
    """(coef, F, ref) of one grid point; coef has EXTRA_ROWS uniform rows past ``rows`` (coef[:rows] is
    the plain case) and ref is the full rows * m product of coef[:rows].  Shared: never written to."""
    coef, F = striped(rows, k, m, p, seed=1000 * rows + k + 7 * m + p % 13)
    g = torch.Generator().manual_seed(rows + k + m)
    coef = torch.cat([coef, _uniform(g, (EXTRA_ROWS, k), p)])
    return coef, F, reference(coef[:rows], F, p)


def grid_n_outs(rows: int, m: int) -> list:
    """Everything, five entries short, and a last row of one entry (all need ``rows`` rows unless m < 5)."""
    return sorted({n for n in (rows * m, rows * m - 5, (rows - 1) * m + 1) if n > 0})


def grid_runs(rows: int, m: int) -> list:
    """(coefficient rows passed, n_out) of every run of one grid point."""
    runs = [(rows, n) for n in grid_n_outs(rows, m)]
    if m > 5:
        runs += [(rows + EXTRA_ROWS, n) for n in grid_n_outs(rows, m)]
    return runs


# ------------------------------------------------------------------ the exactness limit
def p_hi(k: int) -> int:
    """The largest modulus with (p - 1)^2 * k < 2^53: the last one the host sends to float64."""
    return math.isqrt((2 ** 53 - 1) // k) + 1


@functools.lru_cache(maxsize=None)
def boundary_case(k: int, p: int, kind: str):
    """(coef, F, ref) at BOUNDARY_ROWS x k x BOUNDARY_M.  "full": every entry p - 1, so every output is
    k (p - 1)^2 mod p; "striped": uniform with the stripes of striped() and no zero row, so the
    entry where they cross is the same full sum."""
    if kind == "full":
        coef = torch.full((BOUNDARY_ROWS, k), p - 1, dtype=torch.int64)
        F = torch.full((k, BOUNDARY_M), p - 1, dtype=torch.int64)
    else:
        coef, F = striped(BOUNDARY_ROWS, k, BOUNDARY_M, p, seed=k, zero_row=False)
    return coef, F, reference(coef, F, p)


# ------------------------------------------------------------------ host path choice and redo
@functools.lru_cache(maxsize=None)
def host_case():
    """(coef, F, ref) at HOST_ROWS x HOST_K x HOST_M, clean; coef carries EXTRA_ROWS more rows."""
    return grid_case(HOST_ROWS, HOST_K, HOST_M, HOST_P)


def with_entries(t: torch.Tensor, entries) -> torch.Tensor:
    """A copy of t with t[r, c] = v for every (r, c, v)."""
    t = t.clone()
    for r, c, v in entries:
        t[r, c] = v
    return t


def patched_reference(coef: torch.Tensor, F: torch.Tensor, ref: torch.Tensor, p: int, cols) -> torch.Tensor:
    """reference(coef, F, p) given ref = reference(coef, F', p) where F' differs from F in ``cols`` only."""
    cols = sorted(set(cols))
    out = ref.clone().reshape(coef.shape[0], F.shape[1])
    out[:, cols] = reference(coef, F[:, cols].contiguous(), p).reshape(coef.shape[0], len(cols))
    return out.reshape(-1)


def host_positions() -> list:
    return [(r, c) for r in HOST_F_ROWS for c in HOST_F_COLS]


def adversarial(g, n, p):
    """n int64 values: in range, negated, huge of either sign, INT64_MAX, INT64_MIN and in range + p."""
    v = torch.randint(0, p, (n,), generator=g, dtype=torch.int64)
    sel = torch.randint(0, 8, (n,), generator=g)
    big = torch.randint(-2 ** 62, 2 ** 62, (n,), generator=g, dtype=torch.int64) * 2
    v = torch.where(sel == 1, -v, v)
    v = torch.where(sel == 2, big, v)
    v = torch.where(sel == 3, torch.full_like(v, 2 ** 63 - 1), v)
    v = torch.where(sel == 4, torch.full_like(v, -2 ** 63), v)
    v = torch.where(sel == 5, v + p, v)
    return v


@functools.lru_cache(maxsize=None)
def wrap_case(p: int):
    """(coef, F, ref) at the host shape: coefficients uniform in [0, p), F adversarial."""
    g = torch.Generator().manual_seed(p % 1009)
    coef = _uniform(g, (HOST_ROWS, HOST_K), p)
    F = adversarial(g, HOST_K * HOST_M, p).reshape(HOST_K, HOST_M)
    return coef, F, reference(coef, F, p)


# ------------------------------------------------------------------ protocol round trip
def is_prime(p: int) -> bool:
    return p >= 2 and all(p % d for d in range(2, math.isqrt(p) + 1))


@functools.lru_cache(maxsize=None)
def round_trip_case(p: int, m: int):
    """LightSecAgg's encoding at RT_N clients.  Returns (X, F, survivors, alpha, beta): X the RT_U x m
    pieces (uniform in [0, p)), F = np.mod(W.dot(X), p) the RT_N x m shares with W the Lagrange
    coefficients from beta = N+1 .. N+U to alpha = 1 .. N, and RT_U survivors from a seeded
    permutation.  Decoding F[survivors] from alpha[survivors] back to beta gives X; the first
    RT_U - RT_T rows are the aggregate mask."""
    from fedml_amd.core.mpc.lightsecagg import gen_Lagrange_coeffs
    g = torch.Generator().manual_seed(p % 997 + m)
    alpha, beta = np.arange(RT_N) + 1, np.arange(RT_U) + RT_N + 1
    X = _uniform(g, (RT_U, m), p)
    W = gen_Lagrange_coeffs(alpha, beta, p)
    F = reference(torch.from_numpy(W), X, p).reshape(RT_N, m)
    survivors = torch.randperm(RT_N, generator=g)[:RT_U].tolist()  # in the permutation's order
    return X, F, survivors, alpha, beta
