"""Directed edge-value inputs for the adaptive FedOpt server steps (fa_fedavg_adaptive: FedAdam, FedYogi,
FedAdagrad) and the two plain restatements of the contract in include/fedagg.h they are held against.
No tests here and nothing native at import: tests/test_adapt_cases_cpu.py pins ``restate`` (torch CPU
float32 ops) to ``restate64`` (numpy float64, rounded to float32 after every op) on these tables and
checks that the tables hold what they claim; tests/test_gpu_fedopt_adaptive_edges.py runs the HIP
kernel over the same tables.

Three tables, all float32, each a function returning (x [K, n], coef, p, m, v):
  crossed(K)  the edge table of tests/edgecases.py in the clients, the parameter and both moments, every
              (client entry, v entry) and every (p entry, v entry) pair present;
  wide(seed)  sign x mantissa x 2^e with e uniform over the whole exponent range of v and m: the data
              that tells a correctly rounded sqrt and division from their fast approximations and
              from a build that flushes float32 denormals;
  directed()  named hand-built columns, K = 1 with coefficient 1, so g = p - x.
Every table is at least 2 E + 37 elements long (E = 1024, a workgroup's slot): two whole slots on the
16-byte vector path and a ragged one on the element path."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import edgecases

ADAM, YOGI, ADAGRAD = 0, 1, 2  # FA_ADAPT_* (include/fedagg.h)
RULES = {"adam": ADAM, "yogi": YOGI, "adagrad": ADAGRAD}
E = 1024  # FA_TILE_BYTES / 4
MIN_N = 2 * E + 37
LR = 2.0 ** -4  # exact, so the directed tie column can be built
BETA2 = 0.99
EPSES = (1e-3, 0.0)
STEPS = ((0.0, False, 1), (1e-3, True, 2), (0.0, True, 10 ** 6))  # weight decay, bias correction, step
ROUNDS = 2
_F = torch.finfo(torch.float32)


# ------------------------------------------------------------------ the two restatements
def f32(x):
    """A host scalar cast double -> float once."""
    return torch.tensor(float(x), dtype=torch.float64).float()


def weighted_avg(x, coef):
    """fa_weighted_sum's FA_MODE_MUL_W arithmetic: clients in order, t_i = rnd(x_i * (float)coef_i)."""
    cf = torch.tensor(list(coef), dtype=torch.float64).float()
    avg = None
    for i in range(x.shape[0]):
        t = x[i] * cf[i]
        avg = t if avg is None else avg + t
    return avg


def restate(x, coef, p, m, v, rule, lr, beta1, beta2, eps, wd=0.0, bias=False, step=1, trace=None):
    """One round of the contract in include/fedagg.h with torch CPU float32 ops, one op per line:
    x [k, n], p, m (None exactly when beta1 == 0) and v [n].  Returns the new (p, m, v).  ``trace``: a
    dict that receives the intermediates (g, g2, the v read, Yogi's d and s, num, root, den, q)."""
    v_in = v
    d = s = None
    avg = weighted_avg(x, coef)
    g = p - avg
    if wd != 0:
        pw = p * f32(wd)
        g = g + pw
    g2 = g * g
    if rule == ADAM:
        a = v * f32(beta2)
        b = g2 * f32(1 - beta2)
        v = a + b
    elif rule == YOGI:
        d = v - g2
        s = (d > 0).float() - (d < 0).float()  # a NaN: neither comparison holds
        t = f32(1 - beta2) * g2
        t = t * s
        v = v - t
    else:
        v = v + g2
    if beta1 != 0:
        a = m * f32(beta1)
        b = g * f32(1 - beta1)
        m = a + b
        num = m
    else:
        num = g
    c2 = f32(math.sqrt(1 - beta2 ** step)) if bias else f32(1.0)
    step_size = f32(lr / (1 - beta1 ** step) if bias else lr)
    root = v.double().sqrt().float()
    den = root / c2
    den = den + f32(eps)
    q = num / den
    if trace is not None:
        trace.update(g=g, g2=g2, v_in=v_in, d=d, s=s, v=v, m=m, num=num, root=root, den=den, q=q)
    q = step_size * q
    p = p - q
    return p, m, v


def _rnd(a):
    """float64 -> the nearest float32 (ties to even, gradual underflow, overflow to Inf), as float64."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _scalar(x):
    return np.float64(np.float32(float(x)))


def restate64(x, coef, p, m, v, rule, lr, beta1, beta2, eps, wd=0.0, bias=False, step=1):
    """The same contract restated on its own in numpy float64, rounded to float32 after every single op
    (the square root included), host scalars cast double -> float once.  A float64 op on float32
    operands followed by the rounding to float32 is the correctly rounded float32 op: products are
    exact in float64, and for +, -, / and sqrt 53 >= 2 * 24 + 2 bits make the second rounding
    innocuous (fewer bits are kept in the subnormal range, which only widens the margin)."""
    with np.errstate(all="ignore"):
        X, P, V = x.double().numpy(), p.double().numpy(), v.double().numpy()
        M = None if m is None else m.double().numpy()
        avg = None
        for i in range(X.shape[0]):
            t = _rnd(X[i] * _scalar(coef[i]))
            avg = t if avg is None else _rnd(avg + t)
        g = _rnd(P - avg)
        if wd != 0:
            g = _rnd(g + _rnd(P * _scalar(wd)))
        g2 = _rnd(g * g)
        if rule == ADAM:
            V = _rnd(_rnd(V * _scalar(beta2)) + _rnd(g2 * _scalar(1 - beta2)))
        elif rule == YOGI:
            d = _rnd(V - g2)
            s = np.where(d > 0, 1.0, 0.0) - np.where(d < 0, 1.0, 0.0)
            V = _rnd(V - _rnd(_rnd(_scalar(1 - beta2) * g2) * s))
        else:
            V = _rnd(V + g2)
        if beta1 != 0:
            M = _rnd(_rnd(M * _scalar(beta1)) + _rnd(g * _scalar(1 - beta1)))
            num = M
        else:
            num = g
        c2 = _scalar(math.sqrt(1 - beta2 ** step)) if bias else np.float64(1.0)
        step_size = _scalar(lr / (1 - beta1 ** step) if bias else lr)
        den = _rnd(_rnd(_rnd(np.sqrt(V)) / c2) + _scalar(eps))
        P = _rnd(P - _rnd(step_size * _rnd(num / den)))

        def back(a):
            return None if a is None else torch.from_numpy(a.astype(np.float32))
        return back(P), back(M), back(V)


# ------------------------------------------------------------------ configurations
def configs(rule=None, eps=None):
    """(rule name, momentum, eps, weight decay, bias correction, step, beta2): rule x momentum x eps x
    STEPS at beta2 = 0.99, and one Adam case with beta2 = 0."""
    out = [(r, mom, e, wd, bias, step, BETA2) for r in RULES for mom in (True, False) for e in EPSES
           for wd, bias, step in STEPS]
    out.append(("adam", True, EPSES[0], 0.0, False, 1, 0.0))
    return [c for c in out if (rule is None or c[0] == rule) and (eps is None or c[2] == eps)]


def describe(cfg):
    rule, mom, eps, wd, bias, step, beta2 = cfg
    return f"{rule} momentum={mom} eps={eps} wd={wd} bias={bias} step={step} beta2={beta2}"


def run(fn, table, cfg, trace=None):
    """ROUNDS consecutive rounds of ``fn`` (restate or restate64) over a table: [(p, m, v)] per round,
    the step advancing by one, the clients the same.  ``trace``: the first round's intermediates."""
    rule, mom, eps, wd, bias, step, beta2 = cfg
    x, coef, p, m, v = table
    m = m if mom else None
    out = []
    for r in range(ROUNDS):
        kw = dict(trace=trace) if (trace is not None and r == 0) else {}
        p, m, v = fn(x, coef, p, m, v, RULES[rule], LR, 0.9 if mom else 0.0, beta2, eps, wd, bias, step + r, **kw)
        out.append((p, m, v))
    return out


# ------------------------------------------------------------------ crossed
CROSSED_K = 9


def v_entries():
    """What v walks in ``crossed``: the float32 edge table and five more entries."""
    extra = torch.tensor([-_F.tiny * _F.eps, -1.0, 2.0 ** -149, 2.0 ** -100, 2.0 ** 100], dtype=torch.float64).float()
    return torch.cat([edgecases.edge_columns(torch.float32), extra])


def crossed_index(n=None):
    """(client entry, p entry, m entry, v entry, repeat) of every column of ``crossed``.  With L = 19
    entries the clients walk the table column by column (an odd period: every entry meets every lane
    of a 16-byte vector), p every L columns, v every L * L columns -- so inside one block of L * L
    columns every (client, p) pair meets one v entry, and over the 24 blocks every (client, v) and every
    (p, v) pair occurs -- and m at the third pace of edgecases.step_state."""
    L = edgecases.edge_columns(torch.float32).numel()
    LV = v_entries().numel()
    n = n or L * L * LV
    j = torch.arange(n)
    return j % L, (j // L) % L, (2 * j + j // (L * L)) % L, (j // (L * L)) % LV, j // L


@functools.lru_cache(maxsize=None)
def crossed(K=CROSSED_K):
    """edgecases.clients with the MUL_W coefficients (0.0 and 1.7 among them) against p, m and v walking
    the edge table.  Where every client holds the same entry (the even repeats of edgecases.clients) and
    the weighted average is NaN or Inf -- the entries NaN and +-Inf, and +-FLT_MAX, which the 1.7 weight
    takes to Inf -- p ends as NaN whatever the state holds.  Eight in nine of those columns are thinned
    out: every client holds randn / 8 there instead.  The even repeats 0, 18, 36, ... keep them, plain
    and with the odd clients negated by turns."""
    tab = edgecases.edge_columns(torch.float32)
    ci, pi, mi, vi, rep = crossed_index()
    n = ci.numel()
    assert n >= MIN_N
    xs = torch.stack(edgecases.clients(torch.float32, K, n, 4100 + K))
    coef, _ = edgecases.coefficients(torch.float32, edgecases.MUL_W, K)
    thin = (rep % 2 == 0) & ~torch.isfinite(weighted_avg(xs, coef)) & ((rep // 2) % 9 != 0)
    g = torch.Generator().manual_seed(4200 + K)
    noise = (torch.randn(K, n, generator=g, dtype=torch.float64) / 8).float()
    xs = torch.where(thin[None, :], noise, xs).contiguous()
    return xs, coef, tab[pi].clone(), tab[mi].clone(), v_entries()[vi].clone()


def crossed_entry(j):
    ci, pi, mi, vi, rep = (int(t[j]) for t in crossed_index())
    tab, vt = edgecases.edge_columns(torch.float32), v_entries()
    return (f"clients entry {ci} ({tab[ci].item()!r}, repeat {rep}), p entry {pi} ({tab[pi].item()!r}), "
            f"m entry {mi} ({tab[mi].item()!r}), v entry {vi} ({vt[vi].item()!r})")


# ------------------------------------------------------------------ wide
WIDE_K = 9
WIDE_N = 4 * E + 37


def _spread(g, n, lo, hi, signed=True):
    """sign x (1 + 23 uniform bits) x 2^e, e uniform over the integers lo .. hi, rounded to float32
    (below 2^-126 onto the subnormal grid)."""
    e = torch.randint(lo, hi + 1, (n,), generator=g)
    mant = 1.0 + torch.randint(0, 1 << 23, (n,), generator=g).double() / (1 << 23)
    val = torch.ldexp(mant, e)
    if signed:
        val = val * (1 - 2 * torch.randint(0, 2, (n,), generator=g)).double()
    return val.float()


@functools.lru_cache(maxsize=None)
def wide(seed=4300):
    """v >= 0 and m over 2^-149 .. 2^127, p and x over 2^-75 .. 2^64, so g^2 spans subnormal to overflow;
    in the last quarter of the columns x is p with its last four bits changed, so g is a few ulps of p
    and exact.  Client j % 9 holds x and the others +0.0, every coefficient 1.0: avg == x."""
    g = torch.Generator().manual_seed(seed)
    n = WIDE_N
    p = _spread(g, n, -75, 64)
    x = _spread(g, n, -75, 64)
    m = _spread(g, n, -149, 127)
    v = _spread(g, n, -149, 127, signed=False)
    close = torch.arange(n) >= n - n // 4
    near = (p.view(torch.int32) ^ torch.randint(1, 16, (n,), generator=g, dtype=torch.int32)).view(torch.float32)
    x = torch.where(close, near, x)
    j = torch.arange(n)
    xs = torch.stack([torch.where(j % WIDE_K == i, x, torch.zeros(n)) for i in range(WIDE_K)]).contiguous()
    return xs, [1.0] * WIDE_K, p, m, v


# ------------------------------------------------------------------ directed
_MAX, _TINY = _F.max, _F.tiny
_INF = float("inf")
# name, p, x, m, v: K = 1 with coefficient 1, so g = p - x.  A column that may end as NaN says so.
DIRECTED = [
    ("g2 subnormal", 1.2345678 * 2.0 ** -70, 0.0, 2.0 ** -72, 2.0 ** -130),
    ("g2 overflows from a finite g", 3e19, -1e19, 1.0, 1.0),
    ("v = 2^-149", 2.0 ** -80, 0.0, 2.0 ** -80, 2.0 ** -149),
    ("v = +0.0, g != 0", 2.0 ** -80, 0.0, 2.0 ** -80, 0.0),
    ("v = -0.0, g != 0", 2.0 ** -80, 0.0, 2.0 ** -80, -0.0),
    ("v = -tiny eps: sqrt NaN", 2.0 ** -80, 0.0, 2.0 ** -80, -_TINY * _F.eps),
    ("v = +Inf, finite g: NaN at beta2 = 0 (Inf 0)", 1.0, 0.5, 0.25, _INF),
    ("v = +Inf, g2 = +Inf: yogi NaN", 3e19, -1e19, 1.0, _INF),
    ("yogi v == g2, large v", 2.0 ** 42, 2.0 ** 40, 2.0 ** 30, 9 * 2.0 ** 80),
    ("quotient overflows at eps > 0: num near FLT_MAX over den near 1e-3", 2.0 ** -80, 0.0, _MAX, 0.0),
    ("quotient subnormal and inexact: num subnormal over den > 1", 1.37 * 2.0 ** -130, 0.0, 1.1 * 2.0 ** -130, 9.0),
    ("m subnormal times beta1", 1.0, 1.0, 1.3 * 2.0 ** -127, 1.0),
    ("p = FLT_MAX: p wd + g overflows, NaN with weight decay", _MAX, 0.0, 0.0, 1.0),
    ("adagrad, eps = 0, no momentum: p - q a rounding tie", 2.0 ** 19 + 2.0 ** -4, 2.0 ** 19 + 2.0 ** -4 - 1.0, 0.0, 3.0),
    ("ordinary", -2.0, 0.75, 0.1, 0.0625),
]
assert len(DIRECTED) % 2 == 1  # an odd period: every column meets every lane of a 16-byte vector


def directed_names():
    return [c[0] for c in DIRECTED]


@functools.lru_cache(maxsize=None)
def directed():
    L = len(DIRECTED)
    j = torch.arange(MIN_N) % L
    col = [torch.tensor([c[i] for c in DIRECTED], dtype=torch.float64).float()[j].clone() for i in (1, 2, 3, 4)]
    return col[1][None, :].contiguous(), [1.0], col[0], col[2], col[3]


TABLES = {"crossed": crossed, "wide": wide, "directed": directed}


def column_name(table, j):
    if table == "directed":
        return DIRECTED[j % len(DIRECTED)][0]
    if table == "crossed":
        return crossed_entry(j)
    return "random column"


@functools.lru_cache(maxsize=None)
def reference(table, cfg):
    """``restate``'s (p, m, v) after each round of one table and configuration; computed once, shared by
    the tests, never written."""
    return run(restate, TABLES[table](), cfg)


def assert_state(got, exp, table, cfg, what):
    """edgecases.assert_bits with the table's own name of every differing column."""
    bad = edgecases.mismatches(got, exp)
    if bad.numel():
        got, exp = got.detach().cpu().reshape(-1), exp.reshape(-1)
        lines = [f"column {j} [{column_name(table, j)}]: got {got[j].item()!r} expected {exp[j].item()!r}"
                 for j in bad[:8].tolist()]
        raise AssertionError(f"{table}, {describe(cfg)}, {what}: {bad.numel()} of {got.numel()} elements differ\n  "
                             + "\n  ".join(lines))


# ------------------------------------------------------------------ what the tables hold
def subnormal(a):
    return (a != 0) & (a.abs() < _TINY)


CATEGORIES = ["g2 subnormal", "g2 Inf from a finite g", "v' subnormal", "v < 0", "quotient subnormal",
              "quotient Inf from finite num and den, eps > 0", "den == +-0", "m' subnormal", "yogi s == 0, d not NaN"]


def categories(table, rule):
    """name -> bool mask over the table's columns, from ``restate``'s intermediates in the first round
    with momentum, no weight decay and no bias correction: at eps = 1e-3, and "den == +-0" at eps = 0.
    The Yogi category is None for the other rules."""
    t, t0 = {}, {}
    run(restate, table, (rule, True, EPSES[0], 0.0, False, 1, BETA2), trace=t)
    run(restate, table, (rule, True, 0.0, 0.0, False, 1, BETA2), trace=t0)
    fin = torch.isfinite
    return {
        "g2 subnormal": subnormal(t["g2"]),
        "g2 Inf from a finite g": torch.isinf(t["g2"]) & fin(t["g"]),
        "v' subnormal": subnormal(t["v"]),
        "v < 0": t["v_in"] < 0,
        "quotient subnormal": subnormal(t["q"]),
        "quotient Inf from finite num and den, eps > 0": torch.isinf(t["q"]) & fin(t["num"]) & fin(t["den"]) & (t["den"] != 0),
        "den == +-0": t0["den"] == 0,
        "m' subnormal": subnormal(t["m"]),
        "yogi s == 0, d not NaN": ((t["s"] == 0) & ~torch.isnan(t["d"])) if rule == "yogi" else None,
    }
