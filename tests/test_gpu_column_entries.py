"""Argument checks of the four per-column C entries (fa_coord_median[_tiled], fa_coord_trimmed_mean
[_tiled]; include/fedagg_robust.h) on a live context: they share one host path
(fedml_amd/csrc/median_host.h), so every entry rejects the same bad inputs with the same codes, and
the message names the entry that was called.  Nothing is launched."""
from __future__ import annotations

import pytest
import torch

from fedml_amd import _native as N

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K, NUMEL = 3, 8
ENTRIES = ["fa_coord_median", "fa_coord_median_tiled", "fa_coord_trimmed_mean", "fa_coord_trimmed_mean_tiled"]


@pytest.fixture(scope="module")
def eng():
    from fedml_amd.engine import get_engine
    return get_engine(0)


@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_rejects_bad_arguments(eng, entry):
    L = N.lib()
    tiled, trimmed = entry.endswith("_tiled"), "trimmed" in entry
    xs = [torch.zeros(NUMEL, device=DEV) for _ in range(K)]
    out = torch.full((NUMEL,), 7.0, device=DEV)
    good = [x.data_ptr() for x in xs]

    def call(dtype=N.F32, numel=NUMEL, k=K, ptrs=good, tile_stride=N.TILE_BYTES):
        args = [eng._ctx, dtype, 1, N.i64_array([numel]), k]
        args += [1] if trimmed else []
        args += [N.ptr_array(ptrs)]
        args += [tile_stride] if tiled else []
        args += [N.ptr_array([out.data_ptr()]), None]
        return getattr(L, entry)(*args), L.fa_last_error()

    def named(err):
        return err.startswith(entry.encode() + b":")

    rc, err = call(dtype=N.I64)
    assert rc == N.FA_ERR_DTYPE and named(err), err
    if tiled:
        rc, err = call(tile_stride=1000)
        assert rc == N.FA_ERR_INVALID and b"tile_stride" in err and named(err), err
    rc, err = call(ptrs=[good[0], None, good[2]])
    assert rc == N.FA_ERR_INVALID and b"input NULL" in err and named(err), err
    rc, err = call(numel=-NUMEL)
    assert rc == N.FA_ERR_INVALID and named(err), err
    rc, err = call(k=0)
    assert rc == N.FA_ERR_INVALID and named(err), err
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing was launched
