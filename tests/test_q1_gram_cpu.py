"""fa_pairwise_gram_q1's argument checks (include/fedagg_sign_gram.h): they run before any HIP call, in the
header's order, so fake tables reach them without a device."""
from __future__ import annotations

import ctypes

import pytest

from fedml_amd import _native as N

NUMEL = [100, 5000]  # 1 + 5 units of 1024: 2 workgroups


def call(**kw):
    L = N.lib()
    k = kw.get("k", 2)
    a = dict(ctx=ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p), nseg=2, numel=N.i64_array(NUMEL), k=k,
             block=128, bits=N.ptr_array([0x10000 + 0x2000 * i for i in range(2 * max(k, 1))]),
             scale=N.ptr_array([0x80000 + 0x100 * i for i in range(2 * max(k, 1))]), gram=0x200000, dist=0x300000,
             scratch=0x400000, bytes=1 << 30)
    a.update(kw)
    rc = L.fa_pairwise_gram_q1(a["ctx"], a["nseg"], a["numel"], a["k"], a["block"], a["bits"], a["scale"], a["gram"],
                               a["dist"], a["scratch"], a["bytes"], None)
    return rc, L.fa_last_error().decode()


def test_symbols_and_scratch_size():
    L = N.lib()
    assert all(hasattr(L, s) for s in N.Q1_GRAM_SYMBOLS)
    assert (N.Q1_GRAM_UNIT, N.Q1_GRAM_MIN_UNITS, N.Q1_GRAM_MAX_K) == (1024, 4, 128)
    nm = N.i64_array(NUMEL)  # k = 33: 2 tiles of 32 = 4 of 16, 10 slabs per workgroup
    assert L.fa_pairwise_gram_q1_scratch_bytes(2, nm, 33) == 8 * (2 * 10 * 256 + 33 * 33)
    assert L.fa_pairwise_gram_q1_scratch_bytes(2, nm, 0) == 0 == L.fa_pairwise_gram_q1_scratch_bytes(2, nm, 129)


@pytest.mark.parametrize("kw,word", [
    (dict(ctx=None, block=16, k=0), "ctx"), (dict(block=16, k=0), "block"), (dict(block=96), "block"),
    (dict(block=2048), "block"), (dict(k=0, bits=None), "k"), (dict(k=129), "k"), (dict(nseg=0), "num_segments"),
    (dict(numel=None), "table"), (dict(bits=None), "table"), (dict(scale=None), "table"), (dict(dist=None), "table"),
    (dict(numel=N.i64_array([100, -1])), "negative"),
    (dict(bits=N.ptr_array([0x10000, 0x12000, 0, 0x16000])), "segment 1 client 0: bits"),
    (dict(bits=N.ptr_array([0x10000, 0x12000, 0x14002, 0x16000])), "segment 1 client 0: bits"),
    (dict(scale=N.ptr_array([0x80000, 0x80100, 0x80200, 0x80302])), "segment 1 client 1: scale"),
    (dict(scratch=None), "scratch"), (dict(bytes=8 * (2 * 3 * 256 + 4) - 1), "scratch")])
def test_rejected_before_any_hip_call(kw, word):
    rc, msg = call(**kw)
    assert rc == N.FA_ERR_INVALID and word in msg, msg
