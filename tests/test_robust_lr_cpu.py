"""Device-free checks of the robust learning rate's plumbing: the C entries reject a NULL context with
an error code, the symbols are exported and declared, FedMLDefender builds the defense for its type
and serves it on aggregation, the defense validates its config, and the coefficients are the
documented formula."""
from __future__ import annotations

import ctypes
import types

import pytest

from fedml_amd import _native as N


def test_null_ctx_returns_invalid():
    L = N.lib()
    rc = L.fa_sign_vote_sum(None, N.F32, 1, None, 4, None, None, None, 1, None, None, None)
    assert rc == N.FA_ERR_INVALID and b"fa_sign_vote_sum: ctx" in L.fa_last_error()
    for stride in (4096, 0):  # the context is checked before the tile stride
        rc = L.fa_sign_vote_sum_tiled(None, N.F32, 1, None, 4, None, stride, None, None, 1, None, None, None)
        assert rc == N.FA_ERR_INVALID and b"fa_sign_vote_sum_tiled: ctx" in L.fa_last_error()


def test_symbols_are_declared_and_exported():
    raw = ctypes.CDLL(N.LIB_PATH)  # the built library itself, not the declared binding
    for name in ("fa_sign_vote_sum", "fa_sign_vote_sum_tiled"):
        assert name in N.EXPORTED_SYMBOLS
        assert hasattr(raw, name)
        fn = getattr(N.lib(), name)
        assert fn.argtypes is not None and len(fn.argtypes) == (13 if name.endswith("_tiled") else 12)
    assert N.lib().fa_abi_version() == 3 and N.ABI_VERSION == 3


def test_defender_builds_the_defense():
    from fedml_amd.core.security.constants import DEFENSE_ROBUST_LR
    from fedml_amd.core.security.defense.robust_lr_defense import RobustLearningRateDefense
    from fedml_amd.core.security.fedml_defender import FedMLDefender
    assert DEFENSE_ROBUST_LR == "robust_lr"
    d = FedMLDefender.get_instance()
    try:
        d.init(types.SimpleNamespace(enable_defense=True, defense_type="robust_lr", robust_lr_threshold=4))
        assert type(d.defender) is RobustLearningRateDefense
        assert (d.defender.threshold, d.defender.server_lr, d.defender.center) == (4, 1.0, "global")  # the defaults
        assert d.is_defense_on_aggregation()
        assert not d.is_defense_before_aggregation() and not d.is_defense_after_aggregation()
        assert d.get_malicious_client_idxs() == []
        d.init(types.SimpleNamespace(enable_defense=True, defense_type="robust_lr", robust_lr_threshold=0,
                                     robust_lr_server_lr=2, robust_lr_center="none"))
        assert (d.defender.threshold, d.defender.server_lr, d.defender.center) == (0, 2.0, "none")
        with pytest.raises(ValueError, match="robust_lr_threshold"):  # required
            d.init(types.SimpleNamespace(enable_defense=True, defense_type="robust_lr"))
        with pytest.raises(NotImplementedError, match="robust_lr") as e:  # the reference's name: unserved
            d.init(types.SimpleNamespace(enable_defense=True, defense_type="robust_learning_rate"))
        for served in ("krum", "multikrum", "trimmed_mean", "wise_median", "coordinate_trimmed_mean",
                       "geometric_median", "centered_clipping", "bulyan", "robust_lr"):
            assert served in str(e.value)
    finally:
        d.init(types.SimpleNamespace())
    assert not d.is_defense_enabled()


@pytest.mark.parametrize("cfg", [dict(), dict(robust_lr_threshold=-1), dict(robust_lr_threshold=1.5),
                                 dict(robust_lr_threshold=2.0), dict(robust_lr_threshold="3"),
                                 dict(robust_lr_threshold=True), dict(robust_lr_threshold=None),
                                 dict(robust_lr_server_lr=0.0), dict(robust_lr_server_lr=-1e-6),
                                 dict(robust_lr_server_lr=float("nan")), dict(robust_lr_server_lr=float("inf")),
                                 dict(robust_lr_server_lr="1"), dict(robust_lr_server_lr=True),
                                 dict(robust_lr_server_lr=None), dict(robust_lr_center="mean"),
                                 dict(robust_lr_center=None), dict(robust_lr_center=0), dict(robust_lr_center=["none"])],
                         ids=str)
def test_defense_rejects_bad_config(cfg):
    from fedml_amd.core.security.defense.robust_lr_defense import RobustLearningRateDefense
    name = next(iter(cfg), "robust_lr_threshold")
    full = dict(cfg) if name == "robust_lr_threshold" else dict(robust_lr_threshold=2, **cfg)
    with pytest.raises(ValueError, match=name):
        RobustLearningRateDefense(types.SimpleNamespace(**full))


def test_threshold_above_the_client_count_is_rejected_at_aggregation():
    from collections import OrderedDict

    import torch

    from fedml_amd.core.security.defense.robust_lr_defense import RobustLearningRateDefense
    d = RobustLearningRateDefense(types.SimpleNamespace(robust_lr_threshold=3))
    raw = [(1, OrderedDict(w=torch.zeros(4))), (2, OrderedDict(w=torch.ones(4)))]
    with pytest.raises(ValueError, match="robust_lr_threshold 3 exceeds"):
        d.defend_on_aggregation(raw)
    with pytest.raises(ValueError, match="no client"):
        d.defend_on_aggregation([])


def test_coefficients_are_the_formula():
    from fedml_amd.arena import sign_vote_coef
    counts = [17, 301, 44.0, 5]
    for lr in (1.0, 0.5, 0.3):
        total = sum(float(c) for c in counts)
        assert sign_vote_coef(counts, lr) == [lr * float(c) / total for c in counts]
    for bad in ([1, 0], [1, -2], [1, float("nan")], [1, float("inf")]):
        with pytest.raises(ValueError, match="weight"):
            sign_vote_coef(bad, 1.0)
    for bad in (0, -1.0, float("nan"), float("inf"), True, "1"):
        with pytest.raises(ValueError, match="server_lr"):
            sign_vote_coef([1, 2], bad)
