"""Directed edge-value inputs for the ordered-sum, mixing and fused-step kernels of fedagg.hip, and
the plain torch loop they are held against.  No tests here: tests/test_edge_values_cpu.py pins the
C oracle to the torch loop on these tables and checks the tables themselves,
tests/test_gpu_edge_values.py runs the HIP kernels over the same tables.

Everything is built in code (no fixture files).  The tables hold what random data almost never
does: signed zeros, infinities, NaN, the largest and the smallest values, subnormals, sums that land
on a rounding tie, products that overflow, and -- for the 16-bit types -- inputs whose product with
a float32 weight rounds differently when it is rounded once (exact product -> 16 bit) and twice
(exact product -> float32 -> 16 bit, what the reference does)."""
from __future__ import annotations

import functools

import numpy as np
import torch

MUL_W, MUL_N_DIV_N, SUM = 0, 1, 2
FLOAT_DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.float64]
DTYPES = FLOAT_DTYPES + [torch.int64]
KS = [1, 3, 9, 17]

# (significand bits, smallest normal exponent, largest exponent) of the storage types
_FMT = {torch.float16: (11, -14, 15), torch.bfloat16: (8, -126, 127), torch.float32: (24, -126, 127)}
# accumulate ties: 2^p + 1 lies half way between two neighbours of the type
_TIE_EXP = {torch.bfloat16: 8, torch.float16: 11, torch.float32: 24, torch.float64: 53}


def round_once(v, dtype) -> np.ndarray:
    """float64 values rounded ONCE to ``dtype`` (round to nearest even, gradual underflow, overflow
    to infinity), returned as float64.  Scaling by a power of two is exact, so rint does the rounding."""
    p, emin, emax = _FMT[dtype]
    v = np.asarray(v, dtype=np.float64)
    out = v.copy()
    fin = np.isfinite(v) & (v != 0)
    _, e = np.frexp(v[fin])  # the leading bit has exponent e - 1
    q = np.ldexp(1.0, np.maximum(e - 1, emin) - (p - 1))
    r = np.rint(v[fin] / q) * q
    out[fin] = np.where(np.abs(r) >= np.ldexp(1.0, emax + 1), np.copysign(np.inf, r), r)
    return out


def product_roundings(x16: torch.Tensor, coef32) -> tuple:
    """(once, twice) for x * coef32: the exact product (at most 11 + 24 significand bits, so float64
    holds it) rounded to x's 16-bit type directly, and via float32.  float64 arrays."""
    with np.errstate(over="ignore", invalid="ignore"):
        exact = x16.double().numpy() * np.float64(np.float32(coef32))
        via32 = exact.astype(np.float32).astype(np.float64)
    return round_once(exact, x16.dtype), round_once(via32, x16.dtype)


def double_rounding_inputs(dtype16, coef32) -> torch.Tensor:
    """Every finite value of the 16-bit type whose product with the float32 ``coef32`` rounds
    differently once and twice (both results finite), ascending by bit pattern."""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    x = bits.view(dtype16)
    x = x[torch.isfinite(x)]
    once, twice = product_roundings(x, coef32)
    hit = (once != twice) & np.isfinite(once) & np.isfinite(twice)
    return x[torch.from_numpy(hit)]


# count pairs (n_0, n_1) of N = 1000 searched for the weight of client 0
_DR_CANDIDATES = [(155, 845), (175, 825), (225, 775), (275, 725)]


@functools.lru_cache(maxsize=None)
def double_rounding_counts(dtype16) -> tuple:
    """The counts whose first weight float32(n_0 / 1000) the double-rounding columns are built for:
    (155, 845) for float16 (1675, 1775, 1875 and 1975 differ); for bfloat16 the candidate pair with
    the most double-rounding inputs in one binade, (225, 775)."""
    if dtype16 == torch.float16:
        return _DR_CANDIDATES[0]
    p = _FMT[dtype16][0]
    binade = torch.arange(1 << (p - 1), 1 << p, dtype=torch.float32).to(dtype16)
    best, best_hits = None, -1
    for pair in _DR_CANDIDATES:
        once, twice = product_roundings(binade, np.float32(pair[0] / 1000))
        hits = int((once != twice).sum())
        if hits > best_hits:
            best, best_hits = pair, hits
    return best


@functools.lru_cache(maxsize=None)
def double_rounding_columns(dtype16) -> tuple:
    """The double-rounding inputs of one binade for client 0's weight, scaled over a few exponents
    (kept only where the scaled value is still one), as Python floats."""
    p = _FMT[dtype16][0]
    c = np.float32(double_rounding_counts(dtype16)[0] / 1000)
    binade = torch.arange(1 << (p - 1), 1 << p, dtype=torch.float32).to(dtype16)
    once, twice = product_roundings(binade, c)
    base = binade[torch.from_numpy(once != twice)].double()
    vals = []
    for s in (0, -6, 4):
        x = (base * 2.0 ** s).to(dtype16)
        o, t = product_roundings(x, c)
        vals += [float(v) for v, keep in zip(x, (o != t) & np.isfinite(o) & np.isfinite(t)) if keep]
    return tuple(vals)


def _float_table(dtype):
    """(values, partners): partners[j] is what ONE other client holds against values[j] (the rest hold
    zero) where the pair, not the value alone, is the edge."""
    fi = torch.finfo(dtype)
    tie = 2.0 ** _TIE_EXP[dtype]
    inf, nan = float("inf"), float("nan")
    vals = [0.0, -0.0, inf, -inf, nan, fi.max, -fi.max, fi.tiny, fi.tiny * fi.eps, fi.tiny * 0.75,
            -fi.tiny * fi.eps, 1.0, 1.0 + fi.eps, 1.0 / 3.0, tie, tie + 2.0]
    partners = {14: 1.0, 15: 1.0}  # 2^p + 1 -> 2^p (down to even), 2^p + 3 -> 2^p + 4 (up to even)
    if dtype == torch.float16:
        partners[len(vals)] = 16.0  # 65504 + 16 = 65520: the tie between the largest value and 2^16 -> Inf
        vals += [65504.0, 32768.0, 60000.0]
    if dtype == torch.bfloat16:
        vals += [65504.0, 65520.0, 3.3e38, 1.7e38]  # 2 x 1.7e38 and 1.7 x 3.3e38 overflow the type
    if dtype in _FMT and dtype != torch.float32:
        vals += list(double_rounding_columns(dtype))
    filler = iter([2.0, -1.5, 0.1, -3.0, 0.75])
    # odd: every value meets every lane of a 16-byte vector and both halves of a packed word; no
    # multiple of 3 or 17: with one holder per column (clients()) every client holds every value
    while len(vals) % 2 == 0 or len(vals) % 3 == 0 or len(vals) % 17 == 0:
        vals.append(next(filler))
    return vals, partners


_INT64_TABLE = [0, 1, -1, 2 ** 24 + 1, -(2 ** 24 + 1), 2 ** 24 + 3, 2 ** 53 + 1, 2 ** 62, 2 ** 63 - 1, -2 ** 63,
                2 ** 31, 123_456_789_012_345, -(2 ** 62)]


def edge_columns(dtype) -> torch.Tensor:
    """The 1-D table of edge values of a storage type (odd length)."""
    if dtype == torch.int64:
        t = torch.tensor(_INT64_TABLE, dtype=torch.int64)
    else:
        t = torch.tensor(_float_table(dtype)[0], dtype=torch.float64).to(dtype)
    assert t.numel() % 2 == 1
    return t


def tie_columns(dtype) -> dict:
    """Table indices of the accumulate ties: 'down' (2^p against 1) and 'up' (2^p + 2 against 1)."""
    return {"down": 14, "up": 15}


def clients(dtype, K: int, n: int, seed: int) -> list:
    """K CPU tensors of n elements over the repeated table; column j holds table entry j % L in
    repeat j // L.
      repeat % 4 == 0: every client holds the entry (all-NaN, all -0.0, all-max columns);
      repeat % 4 == 2: every client holds it, odd clients negated (Inf - Inf, max - max, -0 + +0);
      odd repeats:     only client j % K holds it, the others hold randn / 8 -- the entry comes first,
                       in the middle and last, so it meets the -0.0 start and the guarded last load
                       group.  Where a pair is the edge (an accumulate tie), client (j + 1) % K holds
                       the partner and the rest hold +0.0, which leaves the pair's sum alone.
    int64: client i is the table rolled by i."""
    tab = edge_columns(dtype)
    L = tab.numel()
    j = torch.arange(n)
    if dtype == torch.int64:
        return [tab[(j + i) % L].clone() for i in range(K)]
    g = torch.Generator().manual_seed(seed)
    base, rep = tab[j % L], j // L
    partners = _float_table(dtype)[1]
    partner = torch.zeros(n, dtype=dtype)
    paired = torch.zeros(n, dtype=torch.bool)
    for idx, val in partners.items():
        partner[j % L == idx] = val
        paired |= j % L == idx
    xs = []
    for i in range(K):
        noise = (torch.randn(n, generator=g, dtype=torch.float64) / 8).to(dtype)
        other = torch.where(paired, torch.where((j + 1) % K == i, partner, torch.zeros(n, dtype=dtype)), noise)
        x = torch.where(rep % 2 == 1, torch.where(j % K == i, base, other), base)
        if i % 2 == 1:
            x = torch.where(rep % 4 == 2, -x, x)
        xs.append(x.contiguous())
    return xs


# weights in thousandths; the first two are the 16-bit type's double-rounding pair.  1.7 overflows the
# largest value, 0.0 meets Inf (0 * Inf), the negative weight comes late so that K <= 9 keeps -0.0 sums
_MILLI = [155, 845, 300, 1700, 0, 250, 125, 60, 500, 33, -250, 410, 77, 1, 999, 640, 20]
# client counts of the (x * n) / N form: two are inexact in float32 (>= 2^24)
_COUNTS = [155, 845, 2 ** 24 + 1, 7, 2 ** 25 + 3, 300, 61, 1700, 500, 33, 250, 410, 77, 1, 999, 640, 20]


def coefficients(dtype, mode: int, K: int) -> tuple:
    """(coef, divisor) of a case: weights w_i (MUL_W), integer counts n_i and N = sum (MUL_N_DIV_N)."""
    if mode == SUM:
        return None, 1.0
    if mode == MUL_N_DIV_N:
        return list(_COUNTS[:K]), float(sum(_COUNTS[:K]))
    milli = list(_MILLI)
    if dtype in (torch.float16, torch.bfloat16):
        milli[:2] = double_rounding_counts(dtype)
    return [m / 1000 for m in milli[:K]], 1.0


def torch_chain(xs, mode: int, coef=None, divisor=1.0) -> torch.Tensor:
    """The reference's literal loop on CPU tensors: acc = x_0 * c_0, acc = acc + x_i * c_i
    (agg_operator.py:35-54); x * n / N with the integer n_i and N (FedAVGAggregator.py:99-116);
    a plain + for SUM.  torch does the promotion (int64 * float -> float32) and the rounding."""
    acc = None
    for i, x in enumerate(xs):
        if mode == MUL_W:
            t = x * float(coef[i])
        elif mode == MUL_N_DIV_N:
            t = x * int(coef[i]) / divisor
        else:
            t = x.clone()
        acc = t if acc is None else acc + t
    return acc


def vec_elems(dtype) -> int:
    return 16 // torch.empty(0, dtype=dtype).element_size()


def size(dtype) -> int:
    """Two tiles of the widest kernel shape (256 lanes x one 16-byte vector x S = 4) plus a ragged
    tail: the smallest n at which every variant runs its vector path twice and its scalar path."""
    return 2 * 256 * vec_elems(dtype) * 4 + 37


@functools.lru_cache(maxsize=None)
def case(dtype, mode: int, K: int, n: int = 0, seed: int = 0) -> tuple:
    """(clients, coef, divisor, C oracle's result) of one weighted-sum case; computed once, shared by
    the tests, never written."""
    from oracle import orc
    xs = clients(dtype, K, n or size(dtype), seed or 100 + K)
    coef, div = coefficients(dtype, mode, K)
    return xs, coef, div, orc.weighted_sum(xs, mode, coef, div)


def double_rounding_column_mask(xs, coef, dtype16) -> torch.Tensor:
    """Columns in which some client's product x_i * float32(w_i) rounds differently once and twice."""
    mask = np.zeros(xs[0].numel(), dtype=bool)
    for x, c in zip(xs, coef):
        once, twice = product_roundings(x, np.float32(c))
        mask |= (once != twice) & ~(np.isnan(once) & np.isnan(twice))
    return torch.from_numpy(mask)


# ------------------------------------------------------------------ mixing rows
def mix_size(dtype) -> int:
    """Two tiles of the mixing kernels (256 lanes x one 16-byte vector) plus a ragged tail."""
    return 2 * 256 * vec_elems(dtype) + 37


def mix_matrices() -> dict:
    """name -> (row_ptr, cols, vals, num_in, post_scale).  A dense 3 x 3 matrix (k_mix<4,3>; the banded
    kernel takes it too, three inputs always fit the band) and a ring of five (k_mix_band); weights of
    zero, above one and below zero; post-scales that overflow, cancel and flip the sign."""
    dense = [[0.5, 0.25, 0.25], [0.155, 0.845, 0.0], [1.7, -0.25, 0.3]]
    out = {"dense3": ([0, 3, 6, 9], [0, 1, 2] * 3, [v for row in dense for v in row], 3, [0.5, 1.7, 0.0])}
    ring = [[1 / 3, 1 / 3, 1 / 3], [0.155, 0.845, 0.0], [0.5, 1.7, 0.3], [0.25, 0.5, 0.25], [1.0, -0.25, 0.125]]
    cols = [c % 5 for r in range(5) for c in (r, r - 1, r + 1)]
    out["ring5"] = ([0, 3, 6, 9, 12, 15], cols, [v for row in ring for v in row], 5, [0.5, 1.7, 0.0, -0.25, 1 / 3])
    return out


@functools.lru_cache(maxsize=None)
def mix_case(name: str, dtype) -> tuple:
    """(inputs, row_ptr, cols, vals, post_scale, oracle rows, oracle post-scaled rows); computed once."""
    from oracle import orc
    rp, cs, vs, num_in, post = mix_matrices()[name]
    xs = clients(dtype, num_in, mix_size(dtype), 200 + num_in)
    exp, exp2 = orc.mix(xs, rp, cs, vs, post_scale=post)
    return xs, rp, cs, vs, post, exp, exp2


# PushSum weights whose mixed omega' makes float32(1 / omega') subnormal (row 0), +Inf (row 1: omega' =
# +0), NaN (row 2: Inf - Inf), ordinary (row 3), -Inf (row 4: omega' = -0) and zero (row 5: overflow)
PUSHSUM_OMEGA = [3e38, 0.0, 0.0, float("inf"), float("-inf"), 1.5]
PUSHSUM_ROWS = ([0, 2, 4, 6, 8, 9, 11], [0, 1, 1, 2, 3, 4, 5, 2, 1, 0, 0],
                [0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, -0.5, 0.9, 0.9], 6)


# ------------------------------------------------------------------ the fused FedAvg + server step
SGD_FLAGS = {  # momentum, dampening, weight_decay, nesterov
    "momentum": (0.9, 0.0, 0.0, False), "nesterov_wd": (0.9, 0.0, 0.001, True),
    "dampening": (0.5, 0.1, 0.01, False), "none": (0.0, 0.0, 0.0, False),
}
STEP_K = 9


def step_state(n: int) -> tuple:
    """(parameter, state buffer) of n float32 elements over the edge table: with the clients' column
    j % L the parameter holds entry (j // L) % L, so every pair of entries meets once n >= L * L; the
    buffer walks the table at a third pace."""
    tab = edge_columns(torch.float32)
    L = tab.numel()
    j = torch.arange(n)
    return tab[(j // L) % L].clone(), tab[(2 * j + j // (L * L)) % L].clone()


# ------------------------------------------------------------------ reporting
def mismatches(got: torch.Tensor, exp: torch.Tensor) -> torch.Tensor:
    """Indices where two same-dtype tensors differ bitwise; NaN against NaN is no difference."""
    got, exp = got.detach().cpu().reshape(-1), exp.detach().cpu().reshape(-1)
    assert got.dtype == exp.dtype and got.numel() == exp.numel(), (got.dtype, exp.dtype, got.numel(), exp.numel())
    if not got.is_floating_point():
        return torch.nonzero(got != exp).reshape(-1)
    same = (got.view(torch.uint8) == exp.view(torch.uint8)).view(got.numel(), -1).all(1)
    return torch.nonzero(~(same | (torch.isnan(got) & torch.isnan(exp)))).reshape(-1)


def assert_bits(got, exp, what, table_dtype=None):
    """Every element compared; a failure names the first columns, their table entries and both values."""
    bad = mismatches(got, exp)
    if bad.numel():
        got, exp = got.detach().cpu().reshape(-1), exp.detach().cpu().reshape(-1)
        lines = []
        for j in bad[:8].tolist():
            entry = ""
            if table_dtype is not None:
                tab = edge_columns(table_dtype)
                entry = f" entry {j % tab.numel()} ({tab[j % tab.numel()].item()!r}, repeat {j // tab.numel()})"
            lines.append(f"column {j}{entry}: got {got[j].item()!r} expected {exp[j].item()!r}")
        raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} elements differ\n  " + "\n  ".join(lines))
