"""Device-free checks of FoolsGold's plumbing: the C entries reject a NULL context with an error code,
the symbols are exported and declared, FedMLDefender builds the defense for its type and serves it
before aggregation, the defense validates its config, ``foolsgold_weights`` is the documented formula,
and the memory's guard and ``reset()`` work (with the engine call stubbed)."""
from __future__ import annotations

import ctypes
import math
import types
from collections import OrderedDict

import numpy as np
import pytest
import torch

from fedml_amd import _native as N
from fedml_amd.foolsgold import foolsgold_weights, largest_similarity


def test_null_ctx_returns_invalid():
    L = N.lib()
    rc = L.fa_pairwise_dot(None, N.F32, 1, None, 4, None, None, None, None, None, 0, None)
    assert rc == N.FA_ERR_INVALID and b"fa_pairwise_dot: ctx" in L.fa_last_error()
    for stride in (4096, 0):  # the context is checked before the tile stride
        rc = L.fa_pairwise_dot_tiled(None, N.F32, 1, None, 4, None, stride, None, None, None, None, 0, None)
        assert rc == N.FA_ERR_INVALID and b"fa_pairwise_dot_tiled: ctx" in L.fa_last_error()


def test_symbols_are_declared_and_exported():
    raw = ctypes.CDLL(N.LIB_PATH)  # the built library itself, not the declared binding
    for name in ("fa_pairwise_dot", "fa_pairwise_dot_tiled", "fa_pairwise_dot_scratch_bytes"):
        assert name in N.EXPORTED_SYMBOLS
        assert hasattr(raw, name)
    assert len(N.lib().fa_pairwise_dot.argtypes) == 12
    assert len(N.lib().fa_pairwise_dot_tiled.argtypes) == 13
    assert N.lib().fa_abi_version() == 3 and N.ABI_VERSION == 3


def test_scratch_bytes_host_only():
    L = N.lib()
    nm = N.i64_array([0, 5, 1000])
    assert L.fa_pairwise_dot_scratch_bytes(3, nm, 0) == 0 and L.fa_pairwise_dot_scratch_bytes(3, nm, 129) == 0
    for k in (1, 4, 33, 128):
        need = L.fa_pairwise_dot_scratch_bytes(3, nm, k)
        assert need > 0 and need % (8 * (k * (k + 1) // 2)) == 0  # whole workgroups' upper triangles


def test_defender_builds_the_defense():
    from fedml_amd.core.security.constants import DEFENSE_FOOLS_GOLD
    from fedml_amd.core.security.defense.fools_gold_defense import FoolsGoldDefense
    from fedml_amd.core.security.fedml_defender import FedMLDefender
    assert DEFENSE_FOOLS_GOLD == "fools_gold"
    d = FedMLDefender.get_instance()
    try:
        d.init(types.SimpleNamespace(enable_defense=True, defense_type="fools_gold"))
        assert type(d.defender) is FoolsGoldDefense
        assert (d.defender.use_memory, d.defender.confidence, d.defender.center) == (True, 1.0, "global")  # defaults
        assert d.is_defense_before_aggregation()
        assert not d.is_defense_on_aggregation() and not d.is_defense_after_aggregation()
        assert d.get_malicious_client_idxs() == []
        d.init(types.SimpleNamespace(enable_defense=True, defense_type="fools_gold", fools_gold_use_memory=False,
                                     fools_gold_confidence=2, fools_gold_center="none"))
        assert (d.defender.use_memory, d.defender.confidence, d.defender.center) == (False, 2.0, "none")
        with pytest.raises(NotImplementedError, match="fools_gold") as e:  # the reference's name: unserved
            d.init(types.SimpleNamespace(enable_defense=True, defense_type="foolsgold"))
        for served in ("krum", "multikrum", "trimmed_mean", "wise_median", "coordinate_trimmed_mean",
                       "geometric_median", "centered_clipping", "bulyan", "robust_lr", "fools_gold"):
            assert served in str(e.value)
    finally:
        d.init(types.SimpleNamespace())
    assert not d.is_defense_enabled()


@pytest.mark.parametrize("cfg", [dict(fools_gold_use_memory=1), dict(fools_gold_use_memory=0),
                                 dict(fools_gold_use_memory="True"), dict(fools_gold_use_memory=None),
                                 dict(fools_gold_confidence=0.0), dict(fools_gold_confidence=-1e-6),
                                 dict(fools_gold_confidence=float("nan")), dict(fools_gold_confidence=float("inf")),
                                 dict(fools_gold_confidence="1"), dict(fools_gold_confidence=True),
                                 dict(fools_gold_confidence=None), dict(fools_gold_center="mean"),
                                 dict(fools_gold_center=None), dict(fools_gold_center=0),
                                 dict(fools_gold_center=["none"])], ids=str)
def test_defense_rejects_bad_config(cfg):
    from fedml_amd.core.security.defense.fools_gold_defense import FoolsGoldDefense
    with pytest.raises(ValueError, match=next(iter(cfg))):
        FoolsGoldDefense(types.SimpleNamespace(**cfg))


def sybil_gram():
    """The issue's scenario: six honest random vectors, three sybils around one direction; G in float64."""
    rng = np.random.default_rng(0)
    P = 4096
    honest = rng.standard_normal((6, P))
    t = rng.standard_normal(P)
    sybils = np.stack([t + 0.05 * rng.standard_normal(P) for _ in range(3)])
    x = np.concatenate([honest, sybils])
    return x @ x.T


def test_weights_on_the_stated_cases():
    assert foolsgold_weights(np.eye(4))[0] == [1, 1, 1, 1]
    assert foolsgold_weights([[1, 1], [1, 1]])[0] == [0, 0]
    assert foolsgold_weights([[1]])[0] == [1]
    assert foolsgold_weights([[0, 0], [0, 1]])[0] == [1, 1]
    w, cs = foolsgold_weights(sybil_gram())
    assert w == [1] * 6 + [0] * 3
    assert min(largest_similarity(cs)[6:]) > 0.99 > 0.1 > max(largest_similarity(cs)[:6])
    assert foolsgold_weights(torch.eye(3, dtype=torch.float64))[0] == [1, 1, 1]  # tensors are accepted
    with pytest.raises(ValueError, match="square"):
        foolsgold_weights([[1, 0]])


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_void_client_is_dropped_and_leaves_the_rest_alone(bad):
    G = sybil_gram()
    w_ref, cs_ref = foolsgold_weights(G)
    n = len(G)
    H = np.zeros((n + 1, n + 1))
    keep = [0, 1, 2, 4, 5, 6, 7, 8, 9]  # the void client sits at position 3
    H[np.ix_(keep, keep)] = G
    H[3, :] = H[:, 3] = float("nan")  # its row and column are tainted ...
    H[3, 3] = bad                      # ... and its norm is not finite
    w, cs = foolsgold_weights(H)
    assert w[3] == 0 and [w[i] for i in keep] == w_ref
    assert cs[3] == [0.0] * (n + 1) and [cs[i][3] for i in range(n + 1)] == [0.0] * (n + 1)
    assert [[cs[i][j] for j in keep] for i in keep] == cs_ref
    # a finite norm with a non-finite product against a finite client is void too
    H2 = np.array([[1.0, 0.0, bad], [0.0, 1.0, 0.0], [bad, 0.0, 1.0]])
    assert foolsgold_weights(H2)[0] == [0, 1, 0]


def test_a_silent_client_gets_weight_one_with_cs_zero():
    G = np.zeros((4, 4))
    G[1:, 1:] = [[1, 1, 0], [1, 1, 0], [0, 0, 1]]  # clients 1 and 2 are one direction, client 0 has sent nothing
    w, cs = foolsgold_weights(G)
    assert w == [1, 0, 0, 1]
    assert cs[0] == [0.0] * 4 and [cs[i][0] for i in range(4)] == [0.0] * 4


def test_confidence_scales_the_logit():
    # unit vectors: 0 and 1 at cosine c, both orthogonal to 2.  v = (c, c, 0), no pardoning applies to
    # the pair (0, 1); a = (1 - c, 1 - c, 1), m = 1, so w_0 = w_1 = conf * (ln((1 - c) / c) + 0.5)
    c = 0.6
    G = [[1, c, 0], [c, 1, 0], [0, 0, 1]]
    for conf in (1.0, 0.5, 2.0):
        w, cs = foolsgold_weights(G, conf)
        x = (1 - cs[0][1]) / 1.0
        want = conf * (math.log(x / (1 - x)) + 0.5)
        assert 0 < want < 1
        assert w[2] == 1 and w[0] == w[1] == pytest.approx(want, rel=1e-15)
    assert foolsgold_weights(G, 0.5)[0][0] == pytest.approx(0.5 * foolsgold_weights(G, 1.0)[0][0], rel=1e-12)


def test_pardoning_spares_the_honest_client_that_resembles_a_sybil():
    # sybils 0, 1 at cosine 0.99; honest client 2 at cosine 0.7 to both; honest client 3 orthogonal
    G = np.array([[1, 0.99, 0.7, 0], [0.99, 1, 0.7, 0], [0.7, 0.7, 1, 0], [0, 0, 0, 1.0]])
    w, cs = foolsgold_weights(G)
    assert cs[2][0] == pytest.approx(0.7 * 0.7 / 0.99) and cs[0][2] == 0.7  # only the honest side is pardoned
    assert w[0] == w[1] == 0 and w[2] > w[0] and w[3] == 1
    # without the pardoning client 2's a = 1 - 0.7 would give ln(0.3 / 0.7) + 0.5 < 0, i.e. weight 0 too
    assert math.log(0.3 / 0.7) + 0.5 < 0
    assert w[2] == pytest.approx(math.log((1 - 0.49 / 0.99) / (0.49 / 0.99)) + 0.5) and 0 < w[2] < 1


def _updates(k, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(10 + i, OrderedDict([("w", torch.randn(8, generator=g)),
                                  ("bn.running_mean", torch.randn(8, generator=g)),
                                  ("bn.num_batches_tracked", torch.tensor(3))])) for i in range(k)]


def test_memory_guard_and_reset_with_a_stubbed_engine_call():
    from fedml_amd.core.security.defense.fools_gold_defense import FoolsGoldDefense
    d = FoolsGoldDefense(types.SimpleNamespace())
    calls = []

    def gram(grads, keys, cen):
        calls.append((len(grads), list(keys), cen))
        return torch.eye(len(grads), dtype=torch.float64)
    d._gram = gram
    raw = _updates(4)
    out = d.defend_before_aggregation(raw, None)
    assert out == raw and all(a[1] is b[1] for a, b in zip(out, raw))  # nobody suspected: the list as it came
    assert calls[-1][:2] == (4, ["w"]) and calls[-1][2] is None  # BatchNorm statistics and counters stay out
    assert d.get_malicious_client_idxs() == [] and d.last_info["weights"] == [1.0] * 4
    d.defend_before_aggregation(_updates(4, seed=1), None)
    for changed in (_updates(5), [(n, OrderedDict(w=g["w"][:4])) for n, g in _updates(4)],
                    [(n, OrderedDict(w=g["w"].double())) for n, g in _updates(4)],
                    [(n, OrderedDict(v=g["w"])) for n, g in _updates(4)]):
        with pytest.raises(ValueError, match=r"reset\(\)"):
            d.defend_before_aggregation(changed, None)
    assert len(calls) == 2  # the guard comes before the device work
    d.reset()
    assert len(d.defend_before_aggregation(_updates(5), None)) == 5
    # without memory nothing is remembered, so nothing can change
    d2 = FoolsGoldDefense(types.SimpleNamespace(fools_gold_use_memory=False))
    d2._gram = gram
    d2.defend_before_aggregation(_updates(4), None)
    assert len(d2.defend_before_aggregation(_updates(5), None)) == 5


def test_weights_become_counts_and_all_zero_is_an_error():
    from fedml_amd.core.security.defense.fools_gold_defense import FoolsGoldDefense
    d = FoolsGoldDefense(types.SimpleNamespace(fools_gold_center="global"))
    c = 0.6
    d._gram = lambda grads, keys, cen: torch.tensor([[1, c, 0], [c, 1, 0], [0, 0, 1]], dtype=torch.float64)
    raw = _updates(3)
    out = d.defend_before_aggregation(raw, {"w": torch.zeros(8)})
    w = math.log(0.4 / 0.6) + 0.5
    assert [n for n, _ in out] == [10 * w, 11 * w, 12] and isinstance(out[2][0], int)
    assert d.last_info["max_cs"] == [c, c, 0.0]
    with pytest.raises(ValueError, match="center lacks key 'w'"):
        d.defend_before_aggregation(raw, {"v": torch.zeros(8)})
    with pytest.raises(ValueError, match="center's key 'w' differs"):
        d.defend_before_aggregation(raw, {"w": torch.zeros(4)})
    d._gram = lambda grads, keys, cen: torch.ones((3, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match="fools_gold: every client was weighted 0"):
        d.defend_before_aggregation(raw, None)
    assert d.get_malicious_client_idxs() == [0, 1, 2]
    d._gram = lambda grads, keys, cen: torch.tensor([[1, 1, 0], [1, 1, 0], [0, 0, 1]], dtype=torch.float64)
    out = d.defend_before_aggregation(raw, None)
    assert [n for n, _ in out] == [12] and out[0][1] is raw[2][1] and d.get_malicious_client_idxs() == [0, 1]
    with pytest.raises(ValueError, match="no client"):
        d.defend_before_aggregation([], None)
    with pytest.raises(ValueError, match="no floating-point weight key"):
        d.defend_before_aggregation([(1, OrderedDict(n=torch.tensor(1)))], None)
