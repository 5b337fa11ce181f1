"""fa_sign_vote_sum on the directed edge tables of tests/votecases.py: the vote is sign(rnd(x - c)) in
the storage type, so a subnormal difference must vote (a flushed one would abstain), a difference that
overflows the type votes with its sign, Inf - Inf and a NaN center abstain, a 16-bit difference on a
rounding tie and a product that overflows go into the sum as the reference rounds them.

out is compared bit for bit (no tolerance, NaN against NaN the only licence) and the count of negated
elements by value with ``parts`` and ``finish`` of tests/test_gpu_robust_lr.py -- which
tests/test_vote_cases_cpu.py pins to a float64 restatement on these very tables.  Every table is two
whole slots (the 16-byte vector path) and a ragged one (the element path); at element offset 1 every
slot takes the element path."""
from __future__ import annotations

import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edgecases  # noqa: E402
import votecases as V  # noqa: E402
from test_gpu_geometric_median import DEV, segments  # noqa: E402
from test_gpu_robust_lr import finish, parts, slot_elems, third  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from fedml_amd.engine import get_engine
    return get_engine(0)


@functools.lru_cache(maxsize=None)
def reference(table, dt, K, centered):
    """(acc, net) of the restatement; computed once, shared by the thresholds and offsets."""
    x, c, coef = V.TABLES[table](dt, K)
    return parts(x, c if centered else None, coef)


def test_the_tables_are_the_kernel_s():
    assert all(V.slot_elems(dt) == slot_elems(dt) for dt in edgecases.FLOAT_DTYPES)
    assert all(V.third(k) == third(k) for k in range(1, 200))


@pytest.mark.parametrize("K", V.KS)
@pytest.mark.parametrize("dt", edgecases.FLOAT_DTYPES, ids=str)
def test_edge_tables(eng, dt, K):
    for table in V.TABLES:
        x, c, coef = V.TABLES[table](dt, K)
        n = x.shape[1]
        assert n == 2 * slot_elems(dt) + 37
        for offset in (0, 1):
            segs = segments(x, [n], offset)
            for centered in (True, False):
                acc, net = reference(table, dt, K, centered)
                cen = c if centered else None
                for th in sorted({1, third(K)}):
                    what = f"K={K} center={centered} threshold={th} offset={offset}"
                    ref, nref, mask = finish(acc, net, cen, th)
                    cens = [segments(c[None], [n], offset)[0][0]] if centered else None
                    outs, flipped = eng.sign_vote_sum(segs, cens, coef, th)
                    print(f"{table} {dt} {what}: the restatement negates {float(mask.float().mean()):.3f} of the "
                          f"elements, {float(ref.isnan().float().mean()):.3f} of out are NaN")
                    V.assert_out(outs[0], ref, table, dt, what)
                    assert int(flipped.item()) == nref, (table, dt, what, int(flipped.item()), nref)
                    if centered:
                        edgecases.assert_bits(cens[0], c, f"{table} {dt} {what}: the center after the run")  # only read
                        same, flipped = eng.sign_vote_sum(segs, cens, coef, th, outs=cens)  # out over the center
                        assert same[0].data_ptr() == cens[0].data_ptr()
                        V.assert_out(cens[0], ref, table, dt, what + ", in place")
                        assert int(flipped.item()) == nref, (table, dt, what, "in place")
            back = torch.stack(list(segs[0])).cpu()
            edgecases.assert_bits(back, x, f"{table} {dt} K={K} offset={offset}: the clients after the runs")  # only read
