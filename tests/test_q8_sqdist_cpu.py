"""fa_weighted_sum_sqdist_q8 / fa_centered_sum_sqdist_q8 (include/fedagg_quant_dist.h) without a device: the
exported symbols, the scratch size and the argument checks, which run before any HIP call in the header's
order, so fake tables reach them."""
from __future__ import annotations

import ctypes

import pytest

from fedml_amd import _native as N

NUMEL = [100, 5000]  # 1 + 2 slots of 4096 elements


def call(centered, **kw):
    L = N.lib()
    a = dict(ctx=ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p), nseg=2, numel=N.i64_array(NUMEL), k=2,
             block=128, q=N.ptr_array([0x10001 + 0x2000 * i for i in range(4)]),
             scale=N.ptr_array([0x80000 + 0x100 * i for i in range(4)]), center=N.ptr_array([0x500000, 0x600000]),
             coef=N.f64_array([0.5, 0.5]), out=N.ptr_array([0x100000, 0x110000]), stats=0x300000, scratch=0x400000,
             bytes=1 << 20)
    a.update(kw)
    head = (a["ctx"], a["nseg"], a["numel"], a["k"], a["block"], a["q"], a["scale"])
    tail = (a["coef"], a["out"], a["stats"], a["scratch"], a["bytes"], None)
    rc = L.fa_centered_sum_sqdist_q8(*head, a["center"], *tail) if centered else L.fa_weighted_sum_sqdist_q8(*head, *tail)
    return rc, L.fa_last_error().decode()


def test_symbols_and_scratch_size():
    L = N.lib()
    assert all(hasattr(L, s) and getattr(L, s).argtypes for s in N.Q8_DIST_SYMBOLS)
    nm = N.i64_array(NUMEL)
    assert L.fa_weighted_sum_sqdist_q8_scratch_bytes(2, nm, 5) == 3 * 2 * 5 * 8
    assert L.fa_weighted_sum_sqdist_q8_scratch_bytes(2, nm, 0) == 0 == L.fa_weighted_sum_sqdist_q8_scratch_bytes(0, nm, 5)


@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("kw,word", [
    (dict(ctx=None, block=8, k=0), "ctx"), (dict(block=8, k=0), "block"), (dict(block=48, q=None), "block"),
    (dict(k=0, q=None), "num_segments"), (dict(numel=None), "table"), (dict(q=None), "table"),
    (dict(scale=None, stats=None), "table"), (dict(numel=N.i64_array([100, -1])), "negative"),
    (dict(q=N.ptr_array([0x10001, 0x10002, 0, 0x10004]), stats=None), "segment 1 client 0: q"),
    (dict(scale=N.ptr_array([0x80000, 0x80100, 0x80200, 0x80302]), stats=None), "segment 1 client 1: scale"),
    (dict(stats=None, scratch=None), "d_stats"), (dict(scratch=None), "scratch"), (dict(bytes=3 * 4 * 8 - 1), "scratch")])
def test_rejected_before_any_hip_call(centered, kw, word):
    rc, msg = call(centered, **kw)
    assert rc == N.FA_ERR_INVALID and word in msg, msg


def test_the_entries_own_tables_in_order():
    rc, msg = call(False, coef=None, out=N.ptr_array([0x100000, 0x110002]))
    assert rc == N.FA_ERR_INVALID and "coef" in msg
    rc, msg = call(False, out=N.ptr_array([0x100000, 0x110002]), stats=None)
    assert rc == N.FA_ERR_INVALID and "segment 1: output" in msg
    rc, msg = call(True, out=None, center=None)  # with coef an output table is required, before the center
    assert rc == N.FA_ERR_INVALID and "table" in msg
    for bad in (None, N.ptr_array([0x500000, 0]), N.ptr_array([0x500000, 0x600002])):  # NULL, or unaligned
        rc, msg = call(True, center=bad, stats=None, scratch=None)
        assert rc == N.FA_ERR_INVALID and "center" in msg, msg
    # distance-only: coef NULL, the output table is not looked at; an empty segment's center is not either
    rc, msg = call(True, coef=None, out=None, stats=None)
    assert rc == N.FA_ERR_INVALID and "d_stats" in msg
    rc, msg = call(True, coef=None, out=None, numel=N.i64_array([100, 0]), center=N.ptr_array([0x500000, 2]), bytes=31)
    assert rc == N.FA_ERR_INVALID and "scratch" in msg
