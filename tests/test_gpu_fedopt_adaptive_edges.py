"""fa_fedavg_adaptive on the directed edge tables of tests/adaptcases.py: subnormal, overflowing,
negative, infinite and -0.0 second moments, subnormal first moments and quotients, Yogi's sign at Inf,
and v and den spread over the whole exponent range -- the data on which a correctly rounded sqrt and
division differ from their fast approximations and from flushed float32 denormals.

Two rounds in place per table, configuration and layout; p, m and v after each round are compared with
adaptcases.restate -- which tests/test_adapt_cases_cpu.py pins to an independent float64 restatement on
these very tables -- bit for bit over every element: no tolerance, NaN against NaN the only licence.
Every table is two whole slots and more (the 16-byte vector path) and a ragged last slot (the element
path); at element offset 1, and with v alone unaligned, every slot takes the element path."""
from __future__ import annotations

import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptcases as A  # noqa: E402
from edgecases import assert_bits  # noqa: E402
from test_gpu_edge_values import arena, scattered  # noqa: E402
from test_gpu_fedopt_adaptive import gather, guards_intact, place  # noqa: E402
from test_gpu_geometric_median import DEV, segments  # noqa: E402

from fedml_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu

# name: element offset of the clients, the parameter, m, v
LAYOUTS = {"aligned": (0, 0, 0, 0), "offset 1": (1, 1, 1, 1), "v unaligned": (0, 0, 0, 1)}


@pytest.fixture(scope="module")
def eng():
    from fedml_amd.engine import get_engine
    return get_engine(0)


def test_the_tables_are_the_kernel_s():
    assert (A.ADAM, A.YOGI, A.ADAGRAD) == (N.ADAPT_ADAM, N.ADAPT_YOGI, N.ADAPT_ADAGRAD) and A.E == N.TILE_BYTES // 4


@functools.lru_cache(maxsize=None)
def device_clients(table, offset):
    """One segment of the table's clients on the device (the configurations share it); read only."""
    return segments(A.TABLES[table]()[0], [A.TABLES[table]()[2].numel()], offset)


def run_table(eng, table, cfg, layout):
    rule, mom, eps, wd, bias, step, beta2 = cfg
    x, coef, p, m, v = A.TABLES[table]()
    n = p.numel()
    oc, op, om, ov = LAYOUTS[layout]
    ref = A.reference(table, cfg)
    (dp, bp), (dv, bv) = place(p, [n], op), place(v, [n], ov)
    dm, bm = place(m, [n], om) if mom else (None, [])
    for r in range(A.ROUNDS):
        eng.fedavg_adaptive(device_clients(table, oc), coef, dp, dm, dv, A.RULES[rule], A.LR, 0.9 if mom else 0.0, beta2,
                            eps, weight_decay=wd, bias_correction=bias, step=step + r)
        for name, got, exp in (("p", dp, ref[r][0]), ("m", dm, ref[r][1]), ("v", dv, ref[r][2])):
            if got is not None:
                A.assert_state(gather(got), exp, table, cfg, f"{layout}, {name} after round {r}")
    assert guards_intact(bp, [n], op) and guards_intact(bv, [n], ov) and guards_intact(bm, [n], om), (table, cfg, layout)


@pytest.mark.parametrize("eps", A.EPSES)
@pytest.mark.parametrize("rule", list(A.RULES))
def test_two_rounds_equal_the_restatement(eng, rule, eps):
    """Momentum x (weight decay, bias correction, step) at beta2 = 0.99 -- and Adam once more at
    beta2 = 0 -- over every table and layout."""
    cfgs = A.configs(rule, eps)
    assert len(cfgs) == 6 + (rule == "adam" and eps == A.EPSES[0])
    for table in A.TABLES:
        for cfg in cfgs:
            for layout in LAYOUTS:
                run_table(eng, table, cfg, layout)
        x = A.TABLES[table]()[0]
        for offset in (0, 1):
            back = torch.stack([t for t in device_clients(table, offset)[0]]).cpu()
            assert_bits(back, x, f"{table}: the clients at offset {offset} after the runs")  # only read


@pytest.mark.parametrize("rule", list(A.RULES))
def test_crossed_through_the_tiled_entry(eng, rule):
    """fa_fedavg_adaptive_tiled over a tile-interleaved buffer whose rows are out of order and every
    other one; the other rows and the padding hold 7."""
    cfg = (rule, True, 1e-3, 1e-3, True, 2, A.BETA2)
    x, coef, p, m, v = A.crossed()
    rows, cap = scattered(x.shape[0])
    buf = arena(list(x), cap, rows)
    keep = buf.clone()
    ref = A.reference("crossed", cfg)
    dp, dm, dv = p.to(DEV), m.to(DEV), v.to(DEV)
    for r in range(A.ROUNDS):
        eng.fedavg_adaptive_tiled(buf, rows, coef, dp, dm, dv, A.RULES[rule], A.LR, 0.9, A.BETA2, 1e-3,
                                  weight_decay=1e-3, bias_correction=True, step=2 + r)
        for name, got, exp in (("p", dp, ref[r][0]), ("m", dm, ref[r][1]), ("v", dv, ref[r][2])):
            A.assert_state(got.cpu(), exp, "crossed", cfg, f"tiled, {name} after round {r}")
    assert_bits(buf, keep, "the arena after the runs")  # only read
