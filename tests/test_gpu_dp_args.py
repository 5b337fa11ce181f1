"""The native DP entries' argument checks (include/fedagg_dp.h), in their stated order: every call fails
at a check that precedes any HIP call, so nothing is launched."""
from __future__ import annotations

import pytest

from fedml_amd import _native as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from fedml_amd.engine import get_engine
    return get_engine(0)._ctx


def test_argument_checks_in_the_stated_order(ctx):
    """Every call fails at a check that precedes any HIP call; each later argument is also invalid, so
    the message names the first one in the header's order."""
    L = N.lib()
    one, ids, p, coef = N.i64_array([4]), N.u32_array([0]), N.ptr_array([16]), N.f64_array([1.0])
    nullp = N.ptr_array([None])
    inf, nan = float("inf"), float("nan")

    def err(rc, code, text):
        assert rc == code, (rc, L.fa_last_error())
        assert text.encode() in L.fa_last_error(), L.fa_last_error()

    # fa_noise_words: nblocks / the range, then the pointer
    err(L.fa_noise_words(ctx, 0, 0, 0, 0, -1, None, None), N.FA_ERR_INVALID, "nblocks")
    err(L.fa_noise_words(ctx, 0, 0, 0, 2 ** 64 - 1, 2, None, None), N.FA_ERR_INVALID, "nblocks")
    err(L.fa_noise_words(ctx, 0, 0, 0, 0, 1, None, None), N.FA_ERR_INVALID, "d_out_u32")
    err(L.fa_noise_words(ctx, 0, 0, 0, 0, 1, 8, None), N.FA_ERR_INVALID, "d_out_u32")
    assert L.fa_noise_words(ctx, 0, 0, 0, 5, 0, None, None) == N.FA_OK
    # fa_add_noise: the segment arguments, mech, scale, seg_id, dtype, pointers
    err(L.fa_add_noise(ctx, N.I64, 9, -1.0, 0, 0, 0, one, None, None, nullp, None), N.FA_ERR_INVALID, "invalid arguments")
    err(L.fa_add_noise(ctx, N.I64, 9, -1.0, 0, 0, 1, None, None, None, nullp, None), N.FA_ERR_INVALID, "invalid arguments")
    err(L.fa_add_noise(ctx, N.I64, 9, -1.0, 0, 0, 1, one, None, None, None, None), N.FA_ERR_INVALID, "invalid arguments")
    err(L.fa_add_noise(ctx, N.I64, 9, -1.0, 0, 0, 1, one, None, None, nullp, None), N.FA_ERR_INVALID, "mech")
    for bad in (-1.0, inf, nan):
        err(L.fa_add_noise(ctx, N.I64, 1, bad, 0, 0, 1, one, None, None, nullp, None), N.FA_ERR_INVALID, "scale")
    err(L.fa_add_noise(ctx, N.I64, 1, 1.0, 0, 0, 1, one, None, None, nullp, None), N.FA_ERR_INVALID, "seg_id")
    for scale in (1.0, 0.0):
        err(L.fa_add_noise(ctx, N.I64, 1, scale, 0, 0, 1, one, ids, None, nullp, None), N.FA_ERR_DTYPE, "dtype")
        err(L.fa_add_noise(ctx, N.F32, 1, scale, 0, 0, 1, N.i64_array([-1]), ids, None, nullp, None), N.FA_ERR_INVALID,
            "negative")
        err(L.fa_add_noise(ctx, N.F32, 1, scale, 0, 0, 1, one, ids, None, nullp, None), N.FA_ERR_INVALID, "output NULL")
        err(L.fa_add_noise(ctx, N.F32, 1, scale, 0, 0, 1, one, ids, nullp, p, None), N.FA_ERR_INVALID, "input NULL")
        assert L.fa_add_noise(ctx, N.F32, 1, scale, 0, 0, 1, N.i64_array([0]), ids, None, nullp, None) == N.FA_OK
    # the fused entries: k / segments, coef, mech, scale, seg_id, dtype, tile_stride's multiple, pointers
    for tiled in (False, True):
        def call(dtype, nseg, numel, k, d_in, stride, cen, cf, mech, scale, sid, d_out):
            if tiled:
                return L.fa_centered_sum_noise_tiled(ctx, dtype, nseg, numel, k, d_in, stride, cen, cf, mech, scale, 0, 0,
                                                     sid, d_out, None)
            return L.fa_centered_sum_noise(ctx, dtype, nseg, numel, k, d_in, cen, cf, mech, scale, 0, 0, sid, d_out, None)
        if tiled:
            err(call(N.I64, 0, None, 0, None, 0, None, None, 9, nan, None, None), N.FA_ERR_INVALID, "tile_stride must be > 0")
        err(call(N.I64, 1, one, 0, p, 100, None, None, 9, nan, None, nullp), N.FA_ERR_INVALID, "invalid arguments")
        err(call(N.I64, 1, one, 1, p, 100, None, None, 9, nan, None, nullp), N.FA_ERR_INVALID, "coef")
        err(call(N.I64, 1, one, 1, p, 100, None, coef, 9, nan, None, nullp), N.FA_ERR_INVALID, "mech")
        err(call(N.I64, 1, one, 1, p, 100, None, coef, 0, nan, None, nullp), N.FA_ERR_INVALID, "scale")
        err(call(N.I64, 1, one, 1, p, 100, None, coef, 0, 1.0, None, nullp), N.FA_ERR_INVALID, "seg_id")
        err(call(N.I64, 1, one, 1, p, 100, None, coef, 0, 1.0, ids, nullp), N.FA_ERR_DTYPE, "dtype")
        if tiled:
            err(call(N.F32, 1, one, 1, p, 100, None, coef, 0, 1.0, ids, nullp), N.FA_ERR_INVALID, "multiple")
        err(call(N.F32, 1, one, 1, p, 4096, nullp, coef, 0, 1.0, ids, nullp), N.FA_ERR_INVALID, "center NULL")
        err(call(N.F32, 1, one, 1, p, 4096, None, coef, 0, 1.0, ids, nullp), N.FA_ERR_INVALID, "output NULL")
        err(call(N.F32, 1, one, 1, nullp, 4096, None, coef, 0, 1.0, ids, p), N.FA_ERR_INVALID, "input NULL")
        assert call(N.F32, 1, N.i64_array([0]), 1, nullp, 4096, None, coef, 0, 1.0, ids, nullp) == N.FA_OK
