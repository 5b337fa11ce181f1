"""Directed edge-value inputs for the sign-vote weighted sum (fa_sign_vote_sum, the robust learning
rate) and a float64 restatement of its contract (include/fedagg_robust.h).  No tests here and nothing
native at import: tests/test_vote_cases_cpu.py checks the tables and pins the per-op restatement of
tests/test_gpu_robust_lr.py (``parts``, ``finish``) to the one below on them;
tests/test_gpu_robust_lr_edges.py runs the HIP kernel over the same tables.

Two tables per storage type and client count K, each (x [K, n], center [n], coef) with
n = 2 slots + 37 elements (two whole slots on the 16-byte vector path and a ragged one on the element
path):
  crossed(dt, K)   edgecases.clients with the MUL_W coefficients (0.0 and 1.7 among them); the center
                   walks the type's edge table at a second pace in half the repeats and holds ordinary
                   values in the other half;
  directed(dt, K)  named hand-built columns: the vote is taken from sign(rnd(x - c)) in the storage
                   type, so a subnormal difference must vote, an overflowing one votes with its sign,
                   Inf - Inf and a NaN center abstain."""
from __future__ import annotations

import functools

import numpy as np
import torch

import edgecases

KS = [3, 9]
TILE_BYTES = 4096  # FA_TILE_BYTES
OP = {torch.float32: torch.float32, torch.bfloat16: torch.float32, torch.float16: torch.float32,
      torch.float64: torch.float64}


def slot_elems(dt):
    return TILE_BYTES // torch.empty((), dtype=dt).element_size()


def size(dt):
    return 2 * slot_elems(dt) + 37


def third(k):
    return max(1, round(0.8 * k ** 0.5))


def coefficients(dt, K):
    return edgecases.coefficients(dt, edgecases.MUL_W, K)[0]


# ------------------------------------------------------------------ crossed
def ordinary_center(dt, n):
    """Columns whose center is ordinary: the first five repeats of every ten, so each of the four kinds
    of repeat of edgecases.clients meets an edge center and an ordinary one, and an entry that comes
    back a repeat later comes back on another lane of the 16-byte vector."""
    L = edgecases.edge_columns(dt).numel()
    return (torch.arange(n) // L) % 10 < 5


@functools.lru_cache(maxsize=None)
def crossed(dt, K):
    tab = edgecases.edge_columns(dt)
    L, n = tab.numel(), size(dt)
    j = torch.arange(n)
    x = torch.stack(edgecases.clients(dt, K, n, 5100 + K))
    g = torch.Generator().manual_seed(5200 + K)
    plain = (torch.randn(n, generator=g, dtype=torch.float64) / 8).to(dt)
    # the second pace: against the clients' entry j % L the center holds entry 2 j % L
    c = torch.where(ordinary_center(dt, n), plain, tab[(2 * j) % L])
    return x.contiguous(), c.contiguous(), coefficients(dt, K)


# ------------------------------------------------------------------ directed
def directed_columns(dt):
    """(name, center, what the even clients hold, what the odd clients hold): x is given directly, so
    u = rnd(x - c).  With an odd K the even clients are one more than the odd ones."""
    fi = torch.finfo(dt)
    sub = fi.tiny * fi.eps  # the smallest subnormal
    tie = 2.0 ** edgecases._TIE_EXP[dt]
    inf, nan = float("inf"), float("nan")
    cols = [
        ("x - c subnormal, positive", fi.tiny, fi.tiny + sub, fi.tiny),
        ("x - c subnormal, negative", fi.tiny + sub, fi.tiny, fi.tiny + sub),
        ("x - c subnormal, both signs", fi.tiny, fi.tiny + sub, fi.tiny - sub),
        ("x - c overflows: max - (-max) = +Inf", -fi.max, fi.max, -fi.max),
        ("x - c overflows: -max - max = -Inf", fi.max, -fi.max, fi.max),
        ("Inf - Inf: NaN", inf, inf, 1.0),
        ("x - c on a rounding tie, down to even", -1.0, tie, -1.0),
        ("x - c on a rounding tie, up to even", -1.0, tie + 2.0, -1.0),
        ("c = NaN", nan, 1.0, -1.0),
        ("c = +Inf, finite x", inf, 1.0, fi.max),
        ("c = -Inf, finite x", -inf, 1.0, -fi.max),
        ("u c overflows with the 1.7 weight (K = 9)", 0.0, fi.max, -fi.max),
        ("ordinary", 0.5, 0.75, 0.25),
    ]
    assert len(cols) % 2 == 1  # an odd period: every column meets every lane of a 16-byte vector
    return cols


@functools.lru_cache(maxsize=None)
def directed(dt, K):
    cols = directed_columns(dt)
    j = torch.arange(size(dt)) % len(cols)
    c, even, odd = (torch.tensor([col[i] for col in cols], dtype=torch.float64).to(dt)[j] for i in (1, 2, 3))
    x = torch.stack([even if i % 2 == 0 else odd for i in range(K)])
    return x.contiguous(), c.contiguous(), coefficients(dt, K)


TABLES = {"crossed": crossed, "directed": directed}


def column_name(table, dt, j):
    if table == "directed":
        cols = directed_columns(dt)
        return cols[j % len(cols)][0]
    tab = edgecases.edge_columns(dt)
    L = tab.numel()
    where = "ordinary" if bool(ordinary_center(dt, j + 1)[j]) else f"entry {(2 * j) % L} ({tab[(2 * j) % L].item()!r})"
    return f"clients entry {j % L} ({tab[j % L].item()!r}, repeat {j // L}), center {where}"


def assert_out(got, exp, table, dt, what):
    """edgecases.assert_bits with the table's own name of every differing column."""
    bad = edgecases.mismatches(got, exp)
    if bad.numel():
        got, exp = got.detach().cpu().reshape(-1), exp.reshape(-1)
        lines = [f"column {j} [{column_name(table, dt, j)}]: got {got[j].item()!r} expected {exp[j].item()!r}"
                 for j in bad[:8].tolist()]
        raise AssertionError(f"{table} {dt}, {what}: {bad.numel()} of {got.numel()} elements differ\n  " + "\n  ".join(lines))


# ------------------------------------------------------------------ the float64 restatement
def _rnd(v, dt):
    """A float64 array rounded to the storage type the way the kernel's op type does: for the 16-bit
    types to float32 first (the op is a float32 op) and then to the type; as float64."""
    if dt == torch.float64:
        return np.asarray(v, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)
    return v if dt == torch.float32 else edgecases.round_once(v, dt)


def restate64(x, c, coef, dt):
    """(acc, net) of the contract in numpy float64 per-op math, every op rounded to the storage type:
    u_i = rnd(x_i - c) (x_i without a center), the vote sign(u_i) from two comparisons, t_i =
    rnd(u_i * (A)coef_i) with A the op type, the ordered sum acc = rnd(acc + t_i).  For float64 storage
    the ops are numpy's own."""
    with np.errstate(all="ignore"):
        X = x.double().numpy()
        C = None if c is None else c.double().numpy()
        acc, net = None, np.zeros(X.shape[1], dtype=np.int64)
        for i in range(X.shape[0]):
            u = X[i] if C is None else _rnd(X[i] - C, dt)
            net += np.where(u > 0, 1, 0) - np.where(u < 0, 1, 0)
            cf = np.float64(coef[i]) if OP[dt] == torch.float64 else np.float64(np.float32(coef[i]))
            t = _rnd(u * cf, dt)
            acc = t if acc is None else _rnd(acc + t, dt)
        return acc, net


def finish64(acc, net, c, threshold, dt):
    """(out, flipped, the flip mask): acc negated where |net| < threshold, then rnd(c + acc)."""
    with np.errstate(all="ignore"):
        flip = np.abs(net) < threshold
        acc = np.where(flip, -acc, acc)
        out = acc if c is None else _rnd(c.double().numpy() + acc, dt)
        return torch.from_numpy(out).to(dt), int(flip.sum()), torch.from_numpy(flip)
