"""tests/votecases.py on the CPU: the per-op restatement of fa_sign_vote_sum's contract that the GPU
tests compare with (``parts`` and ``finish`` of tests/test_gpu_robust_lr.py: torch CPU ops in the
storage type) reproduces in float64 per-op math rounded to the storage type -- the net vote by value,
out bit for bit, the count of negated elements by value -- and the tables hold what they claim."""
from __future__ import annotations

import pytest
import torch

import edgecases
import votecases as V
from test_gpu_robust_lr import finish, parts

DTYPES = edgecases.FLOAT_DTYPES


def cases():
    for table in V.TABLES:
        for K in V.KS:
            yield table, K


@pytest.mark.parametrize("dt", DTYPES, ids=str)
def test_restatement_reproduces_in_float64(dt):
    for table, K in cases():
        x, c, coef = V.TABLES[table](dt, K)
        for cen in (c, None):
            what = f"K={K} center={cen is not None}"
            acc, net = parts(x, cen, coef)
            acc64, net64 = V.restate64(x, cen, coef, dt)
            assert torch.equal(net, torch.from_numpy(net64)), (table, dt, what)
            V.assert_out(acc, torch.from_numpy(acc64).to(dt), table, dt, what + " acc")
            for th in sorted({1, V.third(K)}):
                out, flipped, mask = finish(acc, net, cen, th)
                out64, flipped64, mask64 = V.finish64(acc64, net64, cen, th, dt)
                V.assert_out(out, out64, table, dt, f"{what} threshold={th} out")
                assert flipped == flipped64 and torch.equal(mask, mask64)
                print(f"{table} {dt} {what} threshold={th}: {flipped / x.shape[1]:.3f} of the elements negated, "
                      f"{float(out.isnan().float().mean()):.3f} NaN")


@pytest.mark.parametrize("dt", DTYPES, ids=str)
def test_crossed_is_laid_out_as_claimed(dt):
    tab = edgecases.edge_columns(dt)
    L = tab.numel()
    assert L % 2 == 1
    for K in V.KS:
        x, c, coef = V.crossed(dt, K)
        n = V.size(dt)
        assert x.shape == (K, n) and c.shape == (n,) and x.dtype == c.dtype == dt and n == 2 * V.slot_elems(dt) + 37
        assert coef == edgecases.coefficients(dt, edgecases.MUL_W, K)[0] and (K < 9 or (0.0 in coef and 1.7 in coef))
        assert torch.equal(torch.stack(edgecases.clients(dt, K, n, 5100 + K)).view(torch.uint8), x.view(torch.uint8))
        plain = V.ordinary_center(dt, n)
        assert 0.5 <= float(plain.float().mean()) <= 0.55
        assert bool(torch.isfinite(c[plain]).all()) and bool((c[plain].abs().float() < 1).all())
        # where it is not ordinary the center walks the table: every entry, each on every lane
        j = torch.nonzero(~plain).reshape(-1)
        idx = (2 * j) % L
        assert edgecases.mismatches(c[j].contiguous(), tab[idx].contiguous()).numel() == 0
        seen = torch.zeros(L, edgecases.vec_elems(dt), dtype=torch.bool)
        seen[idx, j % edgecases.vec_elems(dt)] = True
        assert bool(seen.all())
        kinds = torch.zeros(4, 2, dtype=torch.bool)  # each kind of repeat meets both kinds of center
        kinds[(torch.arange(n) // L) % 4, plain.long()] = True
        assert bool(kinds.all())


@pytest.mark.parametrize("dt", DTYPES, ids=str)
def test_directed_columns_are_what_their_names_say(dt):
    fi = torch.finfo(dt)
    inf = float("inf")
    names = [col[0] for col in V.directed_columns(dt)]
    col = {name: j for j, name in enumerate(names)}
    for K in V.KS:
        x, c, coef = V.directed(dt, K)
        assert x.shape[1] == V.size(dt) >= edgecases.vec_elems(dt) * len(names)
        for j, (_, cv, even, odd) in enumerate(V.directed_columns(dt)):  # nothing was rounded away
            for got, want in ((c[j], cv), (x[0, j], even), (x[1, j], odd)):
                assert float(got) == want or (want != want and bool(got.isnan())), (names[j], float(got), want)
        u = x - c[None, :]  # the storage type's own subtraction
        _, net = parts(x, c, coef)
        up, down = (K + 1) // 2, K // 2  # the even clients and the odd ones

        def sub(t):
            return bool(((t != 0) & (t.abs().double() < fi.tiny)).all())
        j = col["x - c subnormal, positive"]
        assert sub(u[0::2, j]) and bool((u[0::2, j] > 0).all()) and bool((u[1::2, j] == 0).all()) and int(net[j]) == up
        j = col["x - c subnormal, negative"]
        assert sub(u[0::2, j]) and bool((u[0::2, j] < 0).all()) and int(net[j]) == -up
        j = col["x - c subnormal, both signs"]
        assert sub(u[:, j]) and int(net[j]) == up - down
        j = col["x - c overflows: max - (-max) = +Inf"]
        assert bool(torch.isfinite(x[:, j]).all()) and float(u[0, j]) == inf and float(u[1, j]) == 0 and int(net[j]) == up
        j = col["x - c overflows: -max - max = -Inf"]
        assert float(u[0, j]) == -inf and int(net[j]) == -up
        j = col["Inf - Inf: NaN"]
        assert bool(u[0::2, j].isnan().all()) and float(u[1, j]) == -inf and int(net[j]) == -down
        tie = 2.0 ** edgecases._TIE_EXP[dt]
        j = col["x - c on a rounding tie, down to even"]
        assert float(x[0, j]) == tie and float(c[j]) == -1.0 and float(u[0, j]) == tie  # tie + 1 -> tie
        j = col["x - c on a rounding tie, up to even"]
        assert float(x[0, j]) == tie + 2 and float(u[0, j]) == tie + 4  # tie + 3 -> tie + 4
        j = col["c = NaN"]
        assert bool(u[:, j].isnan().all()) and int(net[j]) == 0
        j = col["c = +Inf, finite x"]
        assert bool(torch.isfinite(x[:, j]).all()) and bool((u[:, j] == -inf).all()) and int(net[j]) == -K
        j = col["c = -Inf, finite x"]
        assert bool((u[:, j] == inf).all()) and int(net[j]) == K
        j = col["u c overflows with the 1.7 weight (K = 9)"]
        acc, _ = parts(x, c, coef)
        assert bool(torch.isfinite(u[:, j]).all()) and (float(acc[j]) == -inf) == (K == 9) and int(net[j]) == up - down
        # a flushed subnormal difference would abstain and the column would be negated at threshold 1
        for name in ("x - c subnormal, positive", "x - c subnormal, negative", "x - c subnormal, both signs"):
            assert abs(int(net[col[name]])) >= 1
