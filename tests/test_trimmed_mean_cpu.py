"""Device-free checks of the coordinate-wise trimmed mean's plumbing: the two C entries reject a NULL
context with an error code, FedMLDefender builds the new defense for its type (and still the
reference's client-level trim for ``trimmed_mean``), and the defense rejects an invalid beta before
anything touches a device."""
from __future__ import annotations

import types
from collections import OrderedDict

import pytest
import torch

from fedml_amd import _native as N


def test_null_ctx_returns_invalid():
    L = N.lib()
    rc = L.fa_coord_trimmed_mean(None, N.F32, 1, None, 4, 1, None, None, None)
    assert rc == N.FA_ERR_INVALID and b"ctx" in L.fa_last_error()
    rc = L.fa_coord_trimmed_mean_tiled(None, N.F32, 1, None, 4, 1, None, 4096, None, None)
    assert rc == N.FA_ERR_INVALID and b"ctx" in L.fa_last_error()
    rc = L.fa_coord_trimmed_mean_tiled(None, N.F32, 1, None, 4, 1, None, 0, None, None)
    assert rc == N.FA_ERR_INVALID and b"ctx" in L.fa_last_error()
    # the median's entries share the driver: the context is checked before tile_stride there too
    rc = L.fa_coord_median(None, N.F32, 1, None, 4, None, None, None)
    assert rc == N.FA_ERR_INVALID and b"ctx" in L.fa_last_error()
    rc = L.fa_coord_median_tiled(None, N.F32, 1, None, 4, None, 4096, None, None)
    assert rc == N.FA_ERR_INVALID and b"ctx" in L.fa_last_error()
    rc = L.fa_coord_median_tiled(None, N.F32, 1, None, 4, None, 0, None, None)
    assert rc == N.FA_ERR_INVALID and b"ctx" in L.fa_last_error()


def test_symbols_are_declared_and_exported():
    for name in ("fa_coord_trimmed_mean", "fa_coord_trimmed_mean_tiled"):
        assert name in N.EXPORTED_SYMBOLS
        assert hasattr(N.lib(), name)
    assert N.lib().fa_abi_version() == 3


def test_defender_builds_the_new_defense():
    from fedml_amd.core.security.constants import DEFENSE_COORD_TRIMMED_MEAN
    from fedml_amd.core.security.defense.coordinate_trimmed_mean_defense import CoordinateTrimmedMeanDefense
    from fedml_amd.core.security.defense.coordinate_wise_trimmed_mean_defense import CoordinateWiseTrimmedMeanDefense
    from fedml_amd.core.security.fedml_defender import FedMLDefender
    assert DEFENSE_COORD_TRIMMED_MEAN == "coordinate_trimmed_mean"
    d = FedMLDefender.get_instance()
    try:
        d.init(types.SimpleNamespace(enable_defense=True, defense_type="coordinate_trimmed_mean", beta=0.1))
        assert type(d.defender) is CoordinateTrimmedMeanDefense
        assert d.is_defense_on_aggregation() and not d.is_defense_before_aggregation()
        assert not d.is_defense_after_aggregation()
        d.init(types.SimpleNamespace(enable_defense=True, defense_type="trimmed_mean", beta=0.1))
        assert type(d.defender) is CoordinateWiseTrimmedMeanDefense
        assert d.is_defense_before_aggregation() and not d.is_defense_on_aggregation()
        with pytest.raises(NotImplementedError, match="coordinate_trimmed_mean"):
            d.init(types.SimpleNamespace(enable_defense=True, defense_type="no_such_defense"))
    finally:
        d.init(types.SimpleNamespace())
    assert not d.is_defense_enabled()


def _dicts(k):
    return [(1.0, OrderedDict(w=torch.full((3,), float(i)))) for i in range(k)]


def test_defense_rejects_invalid_beta():
    from fedml_amd.core.security.defense.coordinate_trimmed_mean_defense import CoordinateTrimmedMeanDefense
    with pytest.raises(ValueError):
        CoordinateTrimmedMeanDefense(types.SimpleNamespace(beta=-0.1))
    half = CoordinateTrimmedMeanDefense(types.SimpleNamespace(beta=0.5))
    for k in (2, 4, 10):  # b = K / 2 leaves nothing: rejected before any tensor is looked at
        with pytest.raises(ValueError):
            half.defend_on_aggregation(_dicts(k))
    assert half.trim_count(9) == 4  # odd K: the median
    assert CoordinateTrimmedMeanDefense(types.SimpleNamespace(beta=0.2)).trim_count(10) == 2
    assert CoordinateTrimmedMeanDefense(types.SimpleNamespace(beta=0.0)).trim_count(1) == 0
    with pytest.raises(ValueError):
        CoordinateTrimmedMeanDefense(types.SimpleNamespace(beta=0.7)).trim_count(10)
