"""FoolsGold end to end on the device: the sybil scenario through ``DefaultServerAggregator`` +
``FedMLDefender``, the all-honest identity, the memory across rounds and ``reset()``, the arena-resident
route against the dict route, and the center.

The scenario is the one ``foolsgold_weights`` is pinned on (tests/test_fools_gold_cpu.py): P = 4096, six
honest clients with independent normal updates, three sybils whose updates are one direction t plus
5 % noise.  Around the right center the sybils' pairwise cosine is 0.9975 and everyone else's is ~0, so
the weights are [1] * 6 + [0] * 3 with a wide margin on either side."""
from __future__ import annotations

import os
import sys
import types
from collections import OrderedDict

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_geometric_median import DEV, _cfg, _reset_defender, same_bits  # noqa: E402

from fedml_amd.foolsgold import foolsgold_weights, largest_similarity  # noqa: E402

pytestmark = pytest.mark.gpu

P = 4096
COUNTS = [120, 75, 300, 41, 99, 230, 150, 150, 150]


class TinyModel(torch.nn.Module):
    """One weight vector and a BatchNorm-like int64 counter."""

    def __init__(self, w=None):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(P) if w is None else w.clone(), requires_grad=False)
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.int64))


def scenario(seed=0, honest_scale=1.0, spread=True):
    """[9, P] float32 updates: six honest clients, then three sybils (``spread`` False: the sybils send
    independent directions, i.e. nobody colludes)."""
    rng = np.random.default_rng(seed)
    honest = honest_scale * rng.standard_normal((6, P))
    t = rng.standard_normal(P)
    sybils = np.stack([t + 0.05 * rng.standard_normal(P) for _ in range(3)]) if spread else rng.standard_normal((3, P))
    return torch.from_numpy(np.concatenate([honest, sybils])).float()


def dicts(x, device=DEV):
    return [OrderedDict([("w", x[i].to(device)), ("num_batches_tracked", torch.tensor(10 + i, device=device))])
            for i in range(x.shape[0])]


def serve(model, raw, **kw):
    """(kept, kept positions, aggregate, malicious positions, last_info) through the server's hooks."""
    from fedml_amd.core.security.fedml_defender import FedMLDefender
    from fedml_amd.ml.aggregator.default_aggregator import DefaultServerAggregator
    try:
        agg = DefaultServerAggregator(model, _cfg(enable_defense=True, defense_type="fools_gold", **kw))
        kept, idxs = agg.on_before_aggregation(raw)
        out = agg.aggregate(kept)
        d = FedMLDefender.get_instance()
        return kept, idxs, out, d.get_malicious_client_idxs(), d.defender.last_info
    finally:
        _reset_defender()


def test_sybils_are_dropped_and_the_aggregate_is_the_honest_fedavg():
    from fedml_amd.ml.aggregator.agg_operator import FedMLAggOperator
    raw = list(zip(COUNTS, dicts(scenario())))
    kept, idxs, out, bad, info = serve(TinyModel(), raw)
    assert bad == [6, 7, 8] and idxs == [0, 1, 2, 3, 4, 5]
    assert len(kept) == 6 and all(a[0] == b[0] and a[1] is b[1] for a, b in zip(kept, raw[:6]))
    assert info["weights"] == [1.0] * 6 + [0.0] * 3
    assert min(info["max_cs"][6:]) > 0.99 > 0.1 > max(info["max_cs"][:6])
    want = FedMLAggOperator.agg(_cfg(), raw[:6])
    assert list(out) == list(want) and all(same_bits(out[key], want[key]) for key in want)
    undefended = FedMLAggOperator.agg(_cfg(), raw)
    assert not same_bits(out["w"], undefended["w"])  # the sybils would have moved the model


def test_all_honest_returns_the_list_as_it_came():
    from fedml_amd.core.security.defense.fools_gold_defense import FoolsGoldDefense
    raw = list(zip(COUNTS, dicts(scenario(spread=False))))
    kept, idxs, _, bad, info = serve(TinyModel(), raw)
    assert bad == [] and idxs == list(range(9)) and info["weights"] == [1.0] * 9
    assert len(kept) == 9 and all(a[0] is b[0] and a[1] is b[1] for a, b in zip(kept, raw))  # counts and objects
    one = FoolsGoldDefense(types.SimpleNamespace()).defend_before_aggregation(raw[:1], None)  # K = 1
    assert len(one) == 1 and one[0][0] is raw[0][0] and one[0][1] is raw[0][1]


def test_memory_softens_a_first_coincidence_and_reset_forgets():
    """Round A: the three sybils send DIFFERENT random directions; round B: one direction.  Their
    histories A + B are then at cosine ~0.5, their round-B updates alone at ~0.9975: with memory they
    are suspected less in B than without (the CPU restatement gives weights ~0.5 against 0)."""
    from fedml_amd.core.security.defense.fools_gold_defense import FoolsGoldDefense
    xa, xb = scenario(1, spread=False), scenario(2)
    ra, rb = list(zip(COUNTS, dicts(xa))), list(zip(COUNTS, dicts(xb)))
    mem = FoolsGoldDefense(types.SimpleNamespace(fools_gold_use_memory=True))
    nomem = FoolsGoldDefense(types.SimpleNamespace(fools_gold_use_memory=False))
    for d in (mem, nomem):
        assert len(d.defend_before_aggregation(ra, None)) == 9 and d.get_malicious_client_idxs() == []
    with_memory = mem.defend_before_aggregation(rb, None)
    cs_mem, w_mem = mem.last_info["max_cs"], mem.last_info["weights"]
    assert len(nomem.defend_before_aggregation(rb, None)) == 6
    cs_no, w_no = nomem.last_info["max_cs"], nomem.last_info["weights"]
    for s in (6, 7, 8):
        assert max(cs_mem[:6]) < cs_mem[s] < cs_no[s]  # suspected, but less than without the memory
        assert w_no[s] == 0 < w_mem[s] < 1
    assert w_mem[:6] == w_no[:6] == [1.0] * 6
    # the down-weighted sybils stay in the list with n_i * w_i, a float
    assert [n for n, _ in with_memory] == COUNTS[:6] + [COUNTS[s] * w_mem[s] for s in (6, 7, 8)]
    # the CPU restatement of both
    ya, yb = xa.double().numpy(), xb.double().numpy()
    for got, y in ((w_mem, ya + yb), (w_no, yb)):
        assert got == pytest.approx(foolsgold_weights(y @ y.T)[0], abs=1e-4)
    mem.reset()
    mem.defend_before_aggregation(rb, None)  # B alone: what the defense without memory saw
    assert mem.last_info == nomem.last_info and mem.get_malicious_client_idxs() == [6, 7, 8]


def test_arena_route_equals_dict_route(monkeypatch):
    """Float keys of two dtypes, resident in a client-major arena (found through the adopted rows)
    against plain device dicts and CPU dicts: the same weights, the same aggregate bits."""
    from fedml_amd.arena import ClientArena, resident_rows
    from fedml_amd.core.security.defense.fools_gold_defense import FoolsGoldDefense
    from fedml_amd.ml.aggregator.agg_operator import FedMLAggOperator
    x = scenario(3)
    plain = [OrderedDict([("a.weight", x[i, :1000].to(DEV)), ("b.weight", x[i, 1000:].bfloat16().to(DEV)),
                          ("a.bias", x[i, 5:8].clone().to(DEV))]) for i in range(9)]
    center = OrderedDict((key, (0.01 * torch.ones_like(v)).cpu()) for key, v in plain[0].items())
    copies = [OrderedDict((key, v.clone()) for key, v in sd.items()) for sd in plain]
    arena = ClientArena.for_model(copies[0], 9, device=DEV)
    for i, sd in enumerate(copies):
        arena.adopt(i, sd)
    assert resident_rows(copies) is not None
    calls = []
    real = ClientArena.pairwise_dot
    monkeypatch.setattr(ClientArena, "pairwise_dot", lambda self, *a, **kw: calls.append(kw) or real(self, *a, **kw))
    cpu = [OrderedDict((key, v.cpu()) for key, v in sd.items()) for sd in plain]
    results = []
    for ds in (plain, copies, cpu):
        d = FoolsGoldDefense(types.SimpleNamespace())
        for _ in range(2):  # two rounds on the memory
            kept = d.defend_before_aggregation(list(zip(COUNTS, ds)), center)
        assert d.get_malicious_client_idxs() == [6, 7, 8]
        assert len(kept) == 6 and all(a[1] is b for a, b in zip(kept, ds))
        results.append((d.last_info, FedMLAggOperator.agg(_cfg(), kept)))
    assert len(calls) == 2 and all(kw["hists"] is not None and kw["center"] is not None for kw in calls)
    (i0, o0) = results[0]
    for info, out in results[1:]:
        assert info["weights"] == i0["weights"] == [1.0] * 6 + [0.0] * 3
        assert info["max_cs"] == pytest.approx(i0["max_cs"], abs=1e-5)  # the sums' orders differ, within the bound
        assert all(same_bits(out[key].cpu(), o0[key].cpu()) for key in o0)
    assert all(v.device.type == "cpu" for v in results[2][1].values())  # CPU dicts in, CPU tensors out
    assert all(same_bits(a[key], b[key]) for a, b in zip(copies, plain) for key in a)  # the inputs are only read
    # the memory was built for one route: the other one is refused until reset()
    d = FoolsGoldDefense(types.SimpleNamespace())
    d.defend_before_aggregation(list(zip(COUNTS, plain)), center)
    with pytest.raises(ValueError, match=r"reset\(\)"):
        d.defend_before_aggregation(list(zip(COUNTS, copies)), center)
    d.reset()
    d.defend_before_aggregation(list(zip(COUNTS, copies)), center)


def test_center_global_finds_the_sybils_and_none_punishes_the_honest():
    """The clients send MODELS: a common center (3 per coordinate) plus updates, the honest clients'
    small (0.02 per coordinate), the sybils' as in the scenario.  Around the global model the weights
    are [1] * 6 + [0] * 3.  Decided from the CPU restatement (float64 Gram of the stored float32
    models): with "none" the common center makes everyone look alike -- 1 - cs is ~4e-5 among the honest
    clients and ~2.5e-4 among the sybils, an order above the Gram bound of 4e-6 -- so the honest
    clients, whose small updates leave them MOST alike, are the ones weighted 0 and the sybils are
    kept: the weights differ, [0] * 6 + [1] * 3, and no all-zero error is raised."""
    rng = np.random.default_rng(7)
    c = torch.from_numpy(3.0 * rng.standard_normal(P)).float()
    models = c[None, :] + scenario(0, honest_scale=0.02)
    md = models.double().numpy()
    ud = (models - c[None, :]).double().numpy()
    want_global, want_none = foolsgold_weights(ud @ ud.T)[0], foolsgold_weights(md @ md.T)[0]
    assert want_global == [1.0] * 6 + [0.0] * 3 and want_none == [0.0] * 6 + [1.0] * 3
    raw = list(zip(COUNTS, dicts(models)))
    _, idxs, _, bad, info = serve(TinyModel(c), raw, fools_gold_center="global")
    assert bad == [6, 7, 8] and idxs == [0, 1, 2, 3, 4, 5] and info["weights"] == want_global
    kept, _, _, bad, info = serve(TinyModel(c), raw, fools_gold_center="none")
    assert bad == [0, 1, 2, 3, 4, 5] and info["weights"] == want_none
    assert len(kept) == 3 and all(a[1] is b[1] for a, b in zip(kept, raw[6:]))
    want_cs = largest_similarity(foolsgold_weights(md @ md.T)[1])
    assert [1 - v for v in info["max_cs"]] == pytest.approx([1 - v for v in want_cs], abs=1e-5)
