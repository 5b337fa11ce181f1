"""tests/adaptcases.py on the CPU: the two restatements of fa_fedavg_adaptive's contract agree bit for
bit on every table, configuration and round, and the tables hold what they claim.

``restate`` (torch float32 ops) against ``restate64`` (numpy float64, rounded to float32 after every
op): 0 differing elements in p, m and v over crossed, wide and directed, all 37 configurations, both
rounds.

Columns per category (adaptcases.categories: the first round with momentum, no weight decay, no bias
correction, eps = 1e-3, "den == +-0" at eps = 0), adam / yogi / adagrad:
                                                   crossed (8,664)      wide (4,133)
  g2 subnormal                                     0 / 0 / 0            110 / 110 / 110
  g2 Inf from a finite g                           1072 / 1072 / 1072   54 / 54 / 54
  v' subnormal                                     108 / 90 / 90        26 / 26 / 18
  v < 0                                            2166 / 2166 / 2166   0 / 0 / 0
  quotient subnormal                               31 / 31 / 31         3 / 3 / 3
  quotient Inf from finite num and den, eps > 0    209 / 209 / 119      18 / 18 / 16
  den == +-0                                       36 / 36 / 36         0 / 0 / 0
  m' subnormal                                     98 / 98 / 98         0 / 0 / 0
  yogi s == 0, d not NaN                           - / 42 / -           - / 0 / -
Share of columns whose reference p is NaN after the first round, the smallest and the largest over the
37 configurations: crossed 0.364 (adagrad, no momentum, no weight decay) to 0.497 (yogi, momentum,
weight decay: p = +-FLT_MAX overflows p wd + g), and up to 0.599 after the second round; wide 0.000 in
every configuration, and 0.028 at most after the second round (a p that overflowed to Inf in the first
gives Inf - Inf there); directed only the columns whose name says NaN."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import adaptcases as A
import edgecases

TINY = torch.finfo(torch.float32).tiny


def signbit(t):
    return bool(torch.signbit(t))


# ------------------------------------------------------------------ the two restatements
@pytest.mark.parametrize("table", list(A.TABLES))
def test_restatements_agree_bit_for_bit(table):
    """A difference means one of the two is wrong.  restate64 is not built on restate: numpy against
    torch, float64 ops rounded once against float32 ops, two np.where against two casts for the sign."""
    tab = A.TABLES[table]()
    for cfg in A.configs():
        got, exp = A.reference(table, cfg), A.run(A.restate64, tab, cfg)
        for r in range(A.ROUNDS):
            for name, a, b in zip("pmv", got[r], exp[r]):
                assert (a is None) == (b is None) == (name == "m" and not cfg[1])
                if a is not None:
                    A.assert_state(a, b, table, cfg, f"{name}, round {r}, restate against restate64")


def test_wide_tells_a_square_root_one_ulp_off():
    """The data has teeth: a square root one ulp above the correctly rounded one (what an approximate
    sqrt gives) changes p in more than a fifth of the wide table's columns."""
    x, coef, p, m, v = A.wide()
    t = {}
    ref = A.restate(x, coef, p, m, v, A.ADAM, A.LR, 0.9, A.BETA2, 1e-3, trace=t)
    den = torch.nextafter(t["root"], torch.tensor(float("inf"))) + A.f32(1e-3)
    p_off = p - A.f32(A.LR) * (t["num"] / den)
    share = edgecases.mismatches(p_off, ref[0]).numel() / p.numel()
    print(f"a root one ulp off changes p in {share:.3f} of wide")
    assert share > 0.2


# ------------------------------------------------------------------ the tables
def test_tables_are_laid_out_as_claimed():
    tab, vt = edgecases.edge_columns(torch.float32), A.v_entries()
    L, LV = tab.numel(), vt.numel()
    assert L % 2 == 1 and len(A.DIRECTED) % 2 == 1
    for want in (-TINY * 2.0 ** -23, -1.0, 2.0 ** -149, 2.0 ** -100, 2.0 ** 100):
        assert bool((vt == want).any()), want
    for name, fn in A.TABLES.items():
        x, coef, p, m, v = fn()
        n = p.numel()
        assert n >= A.MIN_N and x.shape == (len(coef), n) and m.shape == v.shape == p.shape == (n,)
        assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (x, p, m, v))
    # crossed: every (client entry, v entry) and every (p entry, v entry) pair, each on every lane
    ci, pi, mi, vi, rep = A.crossed_index()
    lane = torch.arange(ci.numel()) % 4
    for a in (ci, pi):
        seen = torch.zeros(L, LV, 4, dtype=torch.bool)
        seen[a, vi, lane] = True
        assert bool(seen.all())
    for idx, size in ((ci, L), (pi, L), (mi, L), (vi, LV)):
        seen = torch.zeros(size, 4, dtype=torch.bool)
        seen[idx, lane] = True
        assert bool(seen.all())
    # the thinning keeps columns in which every client holds the same NaN, +Inf, -Inf, plain and negated
    x, coef = A.crossed()[:2]
    for k in range(L):
        if not bool(torch.isfinite(tab[k])):
            same = (ci == k) & (rep % 2 == 0) & ~torch.isfinite(x).any(0)
            assert {0, 2} <= set((rep[same] % 4).tolist()), k
            assert bool((~torch.isfinite(x[:, same])).all())
    assert edgecases.coefficients(torch.float32, edgecases.MUL_W, A.CROSSED_K)[0] == coef and 0.0 in coef and 1.7 in coef
    # wide: avg == x, and the close block's g is exact and tiny
    x, coef, p, m, v = A.wide()
    n = p.numel()
    xx = x.sum(0)
    assert A.weighted_avg(x, coef).equal(xx) and bool((v >= 0).all()) and int((x != 0).sum(0).max()) == 1
    close = torch.arange(n) >= n - n // 4
    g = (p.double() - xx.double())[close]
    assert bool((g != 0).all()) and bool((g.float().double() == g).all())
    assert bool((g.abs() <= 15 * 2.0 ** -23 * p[close].abs().double() * 1.0000001).all())
    for t, lo, hi in ((v, -149, 127), (m, -149, 127), (p, -75, 64)):
        e = torch.frexp(t[t != 0].double())[1] - 1
        assert int(e.min()) <= lo + 4 and int(e.max()) >= hi - 4 and int(e.min()) >= lo - 1 and int(e.max()) <= hi
    # directed: tiled with its odd period, every column on every lane
    x, coef, p, m, v = A.directed()
    Ld = len(A.DIRECTED)
    assert coef == [1.0] and p.numel() >= 4 * Ld
    for j, (_, pj, xj, mj, vj) in enumerate(A.DIRECTED):
        for t, want in ((p, pj), (x[0], xj), (m, mj), (v, vj)):
            w = torch.tensor(want, dtype=torch.float64).float()
            got = t[j::Ld].contiguous()
            assert edgecases.mismatches(got, w.expand(got.numel()).contiguous()).numel() == 0


def test_categories_are_reached_on_every_lane():
    """Each category at least 4 times in crossed and wide together; the counts are printed."""
    for rule in A.RULES:
        cats = {name: A.categories(A.TABLES[name](), rule) for name in ("crossed", "wide")}
        for cat in A.CATEGORIES:
            counts = [None if cats[t][cat] is None else int(cats[t][cat].sum()) for t in ("crossed", "wide")]
            print(f"{rule:8s} {cat:48s} crossed {counts[0]} wide {counts[1]}")
            if counts[0] is not None:
                assert sum(counts) >= 4, (rule, cat, counts)
    assert A.categories(A.wide(), "yogi")["g2 subnormal"].sum() >= 4  # crossed has none: wide is what reaches it


def test_share_of_nan_parameters():
    """After the first round the reference p is NaN in at most half of crossed, in at most 5 % of wide,
    and in directed only where the column's name says so -- in every configuration."""
    names = A.directed_names()
    shares = {"crossed": [], "wide": []}
    for cfg in A.configs():
        for table in A.TABLES:
            first, second = (r[0].isnan() for r in A.reference(table, cfg))
            if table == "directed":
                bad = sorted({names[j % len(names)] for j in torch.nonzero(first).reshape(-1).tolist()})
                assert all("NaN" in name for name in bad), (A.describe(cfg), bad)
            else:
                share = float(first.float().mean())
                shares[table].append(share)
                print(f"{table:8s} {A.describe(cfg):70s} NaN share {share:.3f}, after the second round "
                      f"{float(second.float().mean()):.3f}")
                assert share <= (0.5 if table == "crossed" else 0.05), (table, A.describe(cfg), share)
    for table, s in shares.items():
        print(f"{table}: NaN share {min(s):.3f} .. {max(s):.3f}")


def _trace(rule, mom=True, eps=1e-3, wd=0.0, bias=False, step=1):
    t = {}
    out = A.run(A.restate, A.directed(), (rule, mom, eps, wd, bias, step, A.BETA2), trace=t)
    t["p"] = out[0][0]
    return t


def test_directed_columns_hit_their_category():
    col = {name: j for j, name in enumerate(A.directed_names())}
    x, _, p0, m0, v0 = A.directed()
    for rule in A.RULES:
        cats = A.categories(A.directed(), rule)
        t, t0 = _trace(rule), _trace(rule, eps=0.0)
        for name, cat in (("g2 subnormal", "g2 subnormal"),
                          ("g2 overflows from a finite g", "g2 Inf from a finite g"),
                          ("v = 2^-149", "v' subnormal"),
                          ("v = -tiny eps: sqrt NaN", "v < 0"),
                          ("quotient overflows at eps > 0: num near FLT_MAX over den near 1e-3",
                           "quotient Inf from finite num and den, eps > 0"),
                          ("quotient subnormal and inexact: num subnormal over den > 1", "quotient subnormal"),
                          ("m subnormal times beta1", "m' subnormal"),
                          ("v = +0.0, g != 0", "den == +-0"), ("v = -0.0, g != 0", "den == +-0")):
            assert bool(cats[cat][col[name]]), (rule, name)
        j = col["v = 2^-149"]
        assert float(v0[j]) == 2.0 ** -149 and float(t["root"][j]) == float(np.float32(2.0 ** -74.5))
        j = col["v = -tiny eps: sqrt NaN"]
        assert bool(t["root"][j].isnan()) and bool(t["p"][j].isnan())
        j = col["quotient subnormal and inexact: num subnormal over den > 1"]
        assert float(t["den"][j]) > 1 and float(t["q"][j].double() * t["den"][j].double()) != float(t["num"][j])
        j = col["quotient overflows at eps > 0: num near FLT_MAX over den near 1e-3"]
        assert float(t["num"][j]) > 0.89 * A._MAX and 0.9e-3 < float(t["den"][j]) < 1.1e-3
        j = col["m subnormal times beta1"]
        assert 0 < float(m0[j]) < TINY and float(t["g"][j]) == 0
        # v = +-0.0 at eps = 0: Yogi keeps the -0.0 (s == 0), Adam and Adagrad add g2 = +0 to it; the
        # root of -0.0 is -0.0, but den = rnd(root / c2 + (float)eps) adds +0.0, and -0 + +0 = +0 in
        # round-to-nearest: den is +0.0 in both columns and the infinite quotient has num's sign in both
        jp, jn = col["v = +0.0, g != 0"], col["v = -0.0, g != 0"]
        assert float(t0["g"][jn]) != 0 and signbit(v0[jn]) and not signbit(v0[jp])
        assert signbit(t0["v"][jn]) == signbit(t0["root"][jn]) == (rule == "yogi")
        for j in (jp, jn):
            assert float(t0["den"][j]) == 0 and not signbit(t0["den"][j]) and float(t0["q"][j]) == float("inf")
        j = col["v = +Inf, finite g: NaN at beta2 = 0 (Inf 0)"]
        assert float(t["v"][j]) == float("inf") and float(t["q"][j]) == 0 and float(t["p"][j]) == float(p0[j])
        j = col["p = FLT_MAX: p wd + g overflows, NaN with weight decay"]
        w = _trace(rule, wd=1e-3, bias=True, step=2)
        assert float(p0[j]) == A._MAX and float(t["g"][j]) == A._MAX and float(w["g"][j]) == float("inf")
        assert bool(w["p"][j].isnan()) and not bool(t["p"][j].isnan())
    y = _trace("yogi")
    j = col["v = +Inf, finite g: NaN at beta2 = 0 (Inf 0)"]
    assert float(y["d"][j]) == float("inf") and float(y["s"][j]) == 1
    j = col["v = +Inf, g2 = +Inf: yogi NaN"]
    assert bool(y["d"][j].isnan()) and float(y["s"][j]) == 0 and bool(y["v"][j].isnan()) and bool(y["p"][j].isnan())
    assert float(_trace("adam")["p"][j]) == float(p0[j])  # Adam: v stays Inf, the quotient is 0
    j = col["yogi v == g2, large v"]
    assert float(y["g2"][j]) == float(v0[j]) == 9 * 2.0 ** 80 and float(y["d"][j]) == 0 and float(y["s"][j]) == 0
    assert float(y["v"][j]) == float(v0[j])
    # the tie: p - step_size q lies half way between two float32 neighbours and goes to the even one
    j = col["adagrad, eps = 0, no momentum: p - q a rounding tie"]
    a = _trace("adagrad", mom=False, eps=0.0)
    assert float(a["q"][j]) == 0.5
    sq = float(A.f32(A.LR)) * 0.5
    assert float(np.float32(sq)) == sq  # the scaled quotient is exact in float32
    exact = float(p0[j]) - sq  # exact in float64
    lo, hi = float(np.nextafter(np.float32(p0[j]), np.float32(0))), float(p0[j])
    if exact - lo == hi - exact:
        assert float(a["p"][j]) in (lo, hi) and (np.float32(a["p"][j]).view(np.uint32) & 1) == 0
    else:
        pytest.fail(f"p - q is no tie: {lo!r} < {exact!r} < {hi!r}")
