"""Device-free checks of Bulyan's plumbing: the two C entries of the mean around the median reject a
NULL context with an error code, the symbols are exported under ABI version 3, FedMLDefender builds
BulyanDefense for ``"bulyan"`` (on aggregation only), the defense rejects too few clients before it
looks at a tensor, and ``bulyan_select`` (fedml_amd/bulyan.py) agrees with a brute force written
here on random, tied, non-finite and planted distance matrices."""
from __future__ import annotations

import math
import random
import types
from collections import OrderedDict

import pytest

from fedml_amd import _native as N


def test_null_ctx_returns_invalid():
    L = N.lib()
    rc = L.fa_coord_mean_around_median(None, N.F32, 1, None, 4, 1, None, None, None)
    assert rc == N.FA_ERR_INVALID and b"ctx" in L.fa_last_error()
    rc = L.fa_coord_mean_around_median_tiled(None, N.F32, 1, None, 4, 1, None, 4096, None, None)
    assert rc == N.FA_ERR_INVALID and b"ctx" in L.fa_last_error()
    rc = L.fa_coord_mean_around_median_tiled(None, N.F32, 1, None, 4, 1, None, 0, None, None)
    assert rc == N.FA_ERR_INVALID and b"ctx" in L.fa_last_error()


def test_symbols_are_declared_and_exported():
    for name in ("fa_coord_mean_around_median", "fa_coord_mean_around_median_tiled"):
        assert name in N.EXPORTED_SYMBOLS
        assert hasattr(N.lib(), name)
    assert N.lib().fa_abi_version() == 3


def test_defender_builds_the_defense():
    from fedml_amd.core.security.constants import DEFENSE_BULYAN
    from fedml_amd.core.security.defense.bulyan_defense import BulyanDefense
    from fedml_amd.core.security.fedml_defender import FedMLDefender
    assert DEFENSE_BULYAN == "bulyan"
    d = FedMLDefender.get_instance()
    try:
        d.init(types.SimpleNamespace(enable_defense=True, defense_type="bulyan", byzantine_client_num=1))
        assert type(d.defender) is BulyanDefense
        assert d.is_defense_on_aggregation() and not d.is_defense_before_aggregation()
        assert not d.is_defense_after_aggregation()
        assert d.get_malicious_client_idxs() == []
        with pytest.raises(NotImplementedError, match="bulyan"):
            d.init(types.SimpleNamespace(enable_defense=True, defense_type="no_such_defense"))
    finally:
        d.init(types.SimpleNamespace())
    assert not d.is_defense_enabled() and d.defender is None


class _Untouchable(OrderedDict):
    """A client dict that fails the test when anything reads it."""

    def __getitem__(self, k):
        raise AssertionError("the defense looked at a tensor")

    def items(self):
        raise AssertionError("the defense looked at a tensor")

    keys = values = __iter__ = items


def test_defense_rejects_too_few_clients():
    from fedml_amd.core.security.defense.bulyan_defense import BulyanDefense
    for f, k in ((1, 6), (2, 10), (3, 14), (-1, 9)):  # K = 4f + 2, and f = -1
        d = BulyanDefense(types.SimpleNamespace(byzantine_client_num=f))
        with pytest.raises(ValueError):
            d.defend_on_aggregation([(1.0, _Untouchable()) for _ in range(k)])
    assert BulyanDefense(types.SimpleNamespace(byzantine_client_num=2)).check(11) == 2


# ----------------------------------------------------------------------------- bulyan_select
def _brute(D, f):
    """Independent of bulyan_select's code: sets, explicit minima, math.fsum-free ascending sums."""
    K = len(D)
    clean = [[D[i][j] if math.isfinite(D[i][j]) else math.inf for j in range(K)] for i in range(K)]
    left, chosen = set(range(K)), []
    while len(chosen) < K - 2 * f:
        n = len(left)
        nn = min(n - 1, max(1, n - f - 2))
        scores = {}
        for i in left:
            ds = [clean[i][j] for j in left if j != i]
            total = 0.0
            for _ in range(nn):
                v = min(ds)
                ds.remove(v)
                total = total + v
            scores[i] = total
        lowest = min(scores.values())
        pick = min(i for i in left if scores[i] == lowest)
        left.discard(pick)
        chosen.append(pick)
    return chosen


def _sym(rng, K, ties):
    D = [[0.0] * K for _ in range(K)]
    for i in range(K):
        for j in range(i + 1, K):
            D[i][j] = D[j][i] = float(rng.randint(1, 6)) if ties else rng.random() * 10.0
    return D


def test_select_matches_brute_force_on_random_matrices():
    from fedml_amd.bulyan import bulyan_select
    rng = random.Random(5)
    n = 0
    for K in range(3, 13):
        for f in range(0, (K - 3) // 4 + 1):
            for rep in range(12):
                D = _sym(rng, K, ties=rep % 2 == 1)
                got = bulyan_select(D, f)
                assert got == _brute(D, f), (K, f, rep)
                assert len(got) == K - 2 * f and len(set(got)) == len(got)
                n += 1
    assert n >= 200  # 18 (K, f) pairs x 12
    for K, f in ((6, 1), (10, 2), (5, -1)):
        with pytest.raises(ValueError):
            bulyan_select(_sym(rng, K, False), f)


def test_select_all_equal_takes_clients_in_order():
    from fedml_amd.bulyan import bulyan_select
    for K, f in ((7, 1), (11, 2), (12, 0)):
        D = [[0.0 if i == j else 3.0 for j in range(K)] for i in range(K)]
        assert bulyan_select(D, f) == list(range(K - 2 * f))


def test_select_puts_a_non_finite_client_last_or_nowhere():
    from fedml_amd.bulyan import bulyan_select
    rng = random.Random(9)
    # f = 0 chooses everyone; its last step has two clients left at distance +inf from each other, a
    # tie that the lower index wins -- so there the non-finite client has the highest index
    for K, f, bad, val in ((9, 0, 8, math.nan), (9, 1, 0, math.inf), (11, 2, 10, math.nan), (11, 2, 3, math.nan),
                           (7, 0, 6, -math.inf)):
        D = _sym(rng, K, False)
        for j in range(K):
            if j != bad:
                D[bad][j] = D[j][bad] = val
        got = bulyan_select(D, f)
        assert got == _brute(D, f)
        if f == 0:
            assert got[-1] == bad
        else:
            assert bad not in got


def test_select_leaves_out_two_planted_far_clients():
    from fedml_amd.bulyan import bulyan_select
    K, f = 11, 2
    rng = random.Random(3)
    pts = [[rng.gauss(0.0, 1.0) for _ in range(16)] for _ in range(K)]
    for far in (3, 8):
        pts[far] = [50.0 + far + v for v in pts[far]]
    D = [[sum((a - b) ** 2 for a, b in zip(pts[i], pts[j])) for j in range(K)] for i in range(K)]
    got = bulyan_select(D, f)
    assert len(got) == 7 and 3 not in got and 8 not in got
    assert got == _brute(D, f)
