"""The mixing / gossip kernels (k_mix, k_mix_band, k_pushsum_omega behind fa_mix, fa_mix_tiled and
fa_pushsum) against the C oracle on irregular gossip matrices: rows of different degree in one row
group, largest degree exactly 4, ragged last passes of dense rows, unaligned views, sizes of exactly
two tiles and of less than one, tiled arenas of different strides, special values, the FA_BAND_VAR
forms of the banded kernel, argument checks and zero-element tensors.

Every output is a view into a sentinel-filled buffer; whatever lies outside the views must still hold
the sentinel after the call.  tests/test_mix_cpu.py shows that the oracle is a reference on these
matrices."""
from __future__ import annotations

import functools
import math
import os
import subprocess
import sys
from collections import OrderedDict

import pytest
import torch

from fedml_amd import _native as N
from refcases import (MIX_SENTINEL, bits_equal, guarded_views, guards_intact, mix_inputs, mix_matrices,
                      mix_post_scale, mix_tile, oracle_pushsum)

gpu = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
MATS = mix_matrices()

# The kernel every matrix is meant for: (engine default, banded kernel switched off).
EXPECTED_KERNEL = {
    "ring3": ("band", "k_mix<4,3>"),
    "ring5": ("band", "k_mix<4,3>"),
    "ring8": ("band", "k_mix<4,3>"),
    "ring37": ("band", "k_mix<4,3>"),
    "chain9": ("band", "k_mix<4,3>"),
    "isolated9": ("band", "k_mix<4,3>"),
    "star3": ("band", "k_mix<4,3>"),
    "ring11_permuted": ("k_mix<4,3>", "k_mix<4,3>"),
    "balanced_tree7": ("k_mix<4,3>", "k_mix<4,3>"),
    "undirected_tree7": ("k_mix<4,4>", "k_mix<4,4>"),
    "undirected_tree10": ("k_mix<4,4>", "k_mix<4,4>"),
    "complete4_dense": ("k_mix<4,4>", "k_mix<4,4>"),
    "star9": ("k_mix<2,8>", "k_mix<2,8>"),
    "star12": ("k_mix<2,8>", "k_mix<2,8>"),
    "torus9": ("k_mix<2,8>", "k_mix<2,8>"),
    "random8": ("k_mix<2,8>", "k_mix<2,8>"),
    "random12": ("k_mix<2,8>", "k_mix<2,8>"),
    "complete11_dense": ("k_mix<2,8>", "k_mix<2,8>"),
    "complete9_gossip": ("k_mix<2,8>", "k_mix<2,8>"),
    # its three rows over four inputs happen to fit the band at offset 1, so the default engine runs
    # it on k_mix_band; the band-off test takes it to k_mix<2,8> (degrees 4, 1, 10)
    "handmade": ("band", "k_mix<2,8>"),
}
BAND_ELIGIBLE = [k for k, v in EXPECTED_KERNEL.items() if v[0] == "band"]
EXPECTED_DEGREES = {
    "chain9": [2, 3, 3, 3, 3, 3, 3, 3, 2], "isolated9": [1] * 9, "star3": [3, 2, 2],
    "balanced_tree7": [1, 2, 2, 2, 2, 2, 2], "undirected_tree7": [3, 4, 4, 2, 2, 2, 2],
    "undirected_tree10": [3, 4, 4, 4, 3, 2, 2, 2, 2, 2], "complete4_dense": [4] * 4,
    "star9": [9] + [2] * 8, "star12": [12] + [2] * 11, "torus9": [5] * 9, "complete11_dense": [11] * 11,
    "complete9_gossip": [9] * 9, "handmade": [4, 1, 10],
}


# ------------------------------------------------------------------ the dispatch of mix_impl, restated
def band_offset(row_ptr, cols, num_in):
    """fedagg.hip band_offset: the offset `off` for which every entry of row r is input
    (r + off + {-1, 0, 1}) mod num_in, or None."""
    rows = len(row_ptr) - 1
    if rows <= 0 or num_in < 3 or row_ptr[1] <= row_ptr[0]:
        return None
    c0 = cols[row_ptr[0]]
    for d in (-1, 0, 1):
        off = (c0 - d) % num_in
        if all((cols[j] - (r + off) + 1) % num_in <= 2
               for r in range(rows) for j in range(row_ptr[r], row_ptr[r + 1])):
            return off
    return None


def expected_kernel(row_ptr, cols, num_in, band=True):
    """The kernel mix_impl launches for aligned tensors."""
    if band and band_offset(row_ptr, cols, num_in) is not None:
        return "band"
    maxdeg = max(b - a for a, b in zip(row_ptr, row_ptr[1:]))
    return "k_mix<4,3>" if maxdeg <= 3 else "k_mix<4,4>" if maxdeg <= 4 else "k_mix<2,8>"


@pytest.mark.parametrize("name", list(MATS))
def test_matrix_reaches_its_kernel(name):
    """CPU only: every matrix of the table still lands on the kernel it is meant for."""
    rp, cs, vs, num_in = MATS[name]
    assert (expected_kernel(rp, cs, num_in), expected_kernel(rp, cs, num_in, band=False)) == EXPECTED_KERNEL[name]
    deg = [b - a for a, b in zip(rp, rp[1:])]
    if name in EXPECTED_DEGREES:
        assert deg == EXPECTED_DEGREES[name]
    elif name.startswith("ring"):
        assert set(deg) == {3}
    else:  # the golden random graphs
        assert min(deg) == 2 and max(deg) == 7 - (name == "random8")
    assert len(vs) == len(cs) == rp[-1] and all(0 <= c < num_in for c in cs)


def test_table_is_complete():
    assert set(MATS) == set(EXPECTED_KERNEL)
    # the permuted ring splits into row groups of 4 + 4 + 3, the dense rows into passes of 8 + 3 and 8 + 1
    assert len(MATS["ring11_permuted"][0]) - 1 == 11
    hand = MATS["handmade"]
    assert hand[1] == [2, 0, 2, 1, 1, 0, 3, 3, 3, 3, 3, 3, 3, 3, 0] and hand[3] == 4
    assert {0.0, -0.75, 0.1} <= set(hand[2])
    torus = MATS["torus9"]
    assert sum(v == 0.0 for v in torus[2]) == 6  # the reference's diagonal slip: rows 3..8 weigh themselves 0


# ------------------------------------------------------------------ shared pieces
@pytest.fixture(scope="module")
def eng():
    from fedml_amd.engine import get_engine
    return get_engine(0)


def sizes(dtype):
    t = mix_tile(dtype)
    return [3 * t + 17, 2 * t, 5]


@functools.lru_cache(maxsize=None)
def reference(name, dtype, n, special, seed=1):
    """(inputs, oracle rows, oracle post-scaled rows) of one case, computed once and never written."""
    from oracle import orc
    rp, cs, vs, num_in = MATS[name]
    xs = mix_inputs(dtype, num_in, n, seed, special)
    exp, exp2 = orc.mix(xs, rp, cs, vs, post_scale=mix_post_scale(len(rp) - 1))
    return xs, exp, exp2


def to_device(x, shift=0):
    """A device copy of x: a fresh (16-byte aligned) tensor, or a view `shift` elements into one."""
    if not shift:
        return x.to(DEV)
    base = torch.zeros(x.numel() + 8, dtype=x.dtype, device=DEV)
    view = base[shift:shift + x.numel()]
    view.copy_(x)
    return view


def _int_view(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def check_negative_zeros(name, got, exp):
    """Elements 0 and 1 of a row that starts with input 0 (-0.0 there) at a positive weight: where the
    oracle holds a zero, the same zero, sign included, compared as bit patterns."""
    rp, cs, vs, _ = MATS[name]
    seen = 0
    for r in range(len(rp) - 1):
        if cs[rp[r]] != 0 or not vs[rp[r]] > 0:
            continue
        e, g = exp[r][:2], got[r][:2].cpu()
        for i in range(2):
            if float(e[i]) == 0.0:
                assert int(_int_view(g)[i]) == int(_int_view(e)[i]), (name, r, i, float(g[i]), float(e[i]))
                seen += math.copysign(1.0, float(e[i])) < 0
        if all(v > 0 for v in vs[rp[r]:rp[r + 1]]):  # -0.0 * w summed with -0.0 * w': the oracle keeps the sign
            assert float(e[1]) == 0.0 and math.copysign(1.0, float(e[1])) < 0, (name, r)
    return seen


def run_flat(engine, name, dtype, n, special, post, in_shifts=None, out_shifts=None, out2_shifts=None):
    """One fa_mix call on guarded outputs == the oracle; returns the number of -0.0 outputs checked."""
    rp, cs, vs, num_in = MATS[name]
    rows = len(rp) - 1
    xs, exp, exp2 = reference(name, dtype, n, special)
    dxs = [to_device(x, in_shifts[i] if in_shifts else 0) for i, x in enumerate(xs)]
    buf, outs, starts = guarded_views(dtype, n, rows, out_shifts)
    buf2 = outs2 = starts2 = None
    if post:
        buf2, outs2, starts2 = guarded_views(dtype, n, rows, out2_shifts)
    engine.mix(dxs, rp, cs, vs, mix_post_scale(rows) if post else None, outs, outs2)
    torch.cuda.synchronize()
    what = (name, dtype, n, "special" if special else "finite", "post" if post else "plain")
    for r in range(rows):
        assert bits_equal(outs[r], exp[r]), what + (r,)
        if post:
            assert bits_equal(outs2[r], exp2[r]), what + (r, "out2")
    assert guards_intact(buf, starts, n), what
    if post:
        assert guards_intact(buf2, starts2, n), what
    for x, d in zip(xs, dxs):
        assert bits_equal(d, x), what  # inputs untouched
    return check_negative_zeros(name, outs, exp) if special else 0


def run_all_sizes(engine, name, dtype):
    t = mix_tile(dtype)
    seen = 0
    for n in sizes(dtype):
        for post in (False, True):
            run_flat(engine, name, dtype, n, False, post)
            if n == 3 * t + 17:
                seen += run_flat(engine, name, dtype, n, True, post)
    rp, cs, vs, _ = MATS[name]
    if any(cs[rp[r]] == 0 and all(v > 0 for v in vs[rp[r]:rp[r + 1]]) for r in range(len(rp) - 1)):
        assert seen > 0, name


# ------------------------------------------------------------------ 1, 2: every matrix against the oracle
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("name", list(MATS))
def test_mix_irregular_vs_oracle(eng, name, dtype):
    run_all_sizes(eng, name, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_mix_band_off_vs_oracle(dtype):
    """The band-eligible matrices on the general kernel: k_mix<4,3> on rows of 1, 2 and 3 entries, and
    k_mix<2,8> on the hand-made rows of 4, 1 and 10."""
    from fedml_amd.engine import AggEngine
    engine = AggEngine(0)
    try:
        engine.set_mix_band(False)
        for name in BAND_ELIGIBLE:
            run_all_sizes(engine, name, dtype)
    finally:
        engine.close()


# ------------------------------------------------------------------ 3: tensors that are not 16-byte aligned
@gpu
@pytest.mark.parametrize("variant", ["all_inputs", "input1", "output2", "out2_row0"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
@pytest.mark.parametrize("name", ["ring8", "star9", "undirected_tree10"])
def test_mix_unaligned_views(eng, name, dtype, variant):
    """One view that starts one element into its allocation sends every tile through the scalar loop."""
    rp, _, _, num_in = MATS[name]
    rows = len(rp) - 1
    one = lambda count, i: [int(k == i) for k in range(count)]  # noqa: E731
    kw = {"all_inputs": dict(in_shifts=[1] * num_in), "input1": dict(in_shifts=one(num_in, 1)),
          "output2": dict(out_shifts=one(rows, 2)), "out2_row0": dict(out2_shifts=one(rows, 0))}[variant]
    t = mix_tile(dtype)
    for n in (3 * t + 17, 5):
        for post in ((True,) if variant == "out2_row0" else (False, True)):
            run_flat(eng, name, dtype, n, False, post, **kw)
        run_flat(eng, name, dtype, n, True, True, **kw)


# ------------------------------------------------------------------ 4: tiled arenas against the oracle
def scattered_rows(count, cap):
    """`count` distinct rows of an arena of capacity `cap`, neither contiguous nor ascending."""
    step = next(s for s in (3, 5, 7, 2) if math.gcd(s, cap) == 1)
    rows = [(step * k + 1) % cap for k in range(count)]
    assert len(set(rows)) == count and rows != sorted(rows)
    return rows


def arena(xs, cap, rows, n, fill):
    e = N.TILE_BYTES // xs[0].element_size()
    nt = max(1, -(-n // e))
    buf = torch.full((nt, cap, e), fill, dtype=xs[0].dtype)
    for j, x in enumerate(xs):
        flat = torch.full((nt * e,), fill, dtype=x.dtype)
        flat[:n] = x
        buf[:, rows[j], :] = flat.view(nt, e)
    return buf


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=str)
@pytest.mark.parametrize("name", ["ring8", "chain9", "ring11_permuted", "undirected_tree10", "star9"])
def test_mix_tiled_vs_oracle(eng, name, dtype):
    """fa_mix_tiled with an input tile stride (capacity num_in + 1) different from the outputs'
    (capacity num_in + 3): rows == the oracle, everything else in the output arenas untouched."""
    rp, cs, vs, num_in = MATS[name]
    rows = len(rp) - 1
    in_rows, out_rows = scattered_rows(num_in, num_in + 1), scattered_rows(rows, num_in + 3)
    for n in sizes(dtype):
        xs, exp, exp2 = reference(name, dtype, n, False)
        buf = arena(xs, num_in + 1, in_rows, n, float("nan")).to(DEV)
        e, nt = buf.shape[2], buf.shape[0]
        used = torch.zeros(nt * e, dtype=torch.bool)
        used[:n] = True
        keep = torch.ones((nt, num_in + 3, e), dtype=torch.bool)
        for r in out_rows:
            keep[:, r, :] = ~used.view(nt, e)
        for post in (False, True):
            obuf = torch.full((nt, num_in + 3, e), MIX_SENTINEL, dtype=dtype, device=DEV)
            obuf2 = torch.full_like(obuf, MIX_SENTINEL) if post else None
            eng.mix_tiled(buf, in_rows, rp, cs, vs, obuf, out_rows, mix_post_scale(rows) if post else None, obuf2, n=n)
            torch.cuda.synchronize()
            for o, ex in ((obuf, exp), (obuf2, exp2)) if post else ((obuf, exp),):
                o = o.cpu()
                for r in range(rows):
                    assert bits_equal(o[:, out_rows[r], :].reshape(-1)[:n], ex[r]), (name, dtype, n, post, r)
                assert bool((o[keep] == MIX_SENTINEL).all()), (name, dtype, n, post)


# ------------------------------------------------------------------ 5: the FA_BAND_VAR forms of k_mix_band
BAND_VAR_CASES = [(name, dt, tiles, post) for name in ("ring37", "chain9", "ring5")
                  for dt in (torch.float32, torch.bfloat16) for tiles in (10, 3) for post in (False, True)]

_BAND_VAR_SCRIPT = r"""
import sys, torch
root = sys.argv[1]
sys.path[:0] = [root, root + "/tests", root + "/tests/golden"]
from refcases import guarded_views, guards_intact, mix_inputs, mix_matrices, mix_post_scale, mix_tile
from fedml_amd.engine import get_engine
eng = get_engine(0)
mats = mix_matrices()
res = {}
for name in ("ring37", "chain9", "ring5"):
    rp, cs, vs, num_in = mats[name]
    rows = len(rp) - 1
    for dt in (torch.float32, torch.bfloat16):
        for tiles in (10, 3):
            n = tiles * mix_tile(dt) + 17
            xs = [x.cuda() for x in mix_inputs(dt, num_in, n, 23, tiles == 3)]
            for post in (False, True):
                buf, outs, starts = guarded_views(dt, n, rows)
                buf2, outs2, starts2 = guarded_views(dt, n, rows) if post else (None, None, None)
                eng.mix(xs, rp, cs, vs, mix_post_scale(rows) if post else None, outs, outs2)
                torch.cuda.synchronize()
                ok = guards_intact(buf, starts, n) and (not post or guards_intact(buf2, starts2, n))
                res["%s|%s|%d|%d" % (name, dt, tiles, post)] = {
                    "outs": [o.cpu() for o in outs], "outs2": [o.cpu() for o in outs2 or []], "guards": ok}
torch.save(res, sys.argv[2])
"""


@gpu
@pytest.mark.parametrize("band_var", [0, 2, 3, 4])
def test_band_var_forms_vs_oracle(tmp_path, band_var):
    """FA_BAND_VAR (read once per process, so one child each): 0 cached loads, 2 and 3 the XCD tile map,
    4 groups of 16 rows.  11 tiles (the XCD map with a remainder) and 4 tiles (fewer than XCDs); the
    smaller size carries the special values."""
    path = str(tmp_path / "out.pt")
    env = dict(os.environ, FA_BAND_VAR=str(band_var))
    subprocess.run([sys.executable, "-c", _BAND_VAR_SCRIPT, ROOT, path], env=env, check=True, timeout=120)
    res = torch.load(path, weights_only=True)
    assert len(res) == len(BAND_VAR_CASES)
    for name, dt, tiles, post in BAND_VAR_CASES:
        got = res["%s|%s|%d|%d" % (name, dt, tiles, post)]
        n = tiles * mix_tile(dt) + 17
        _, exp, exp2 = reference(name, dt, n, tiles == 3, 23)
        assert got["guards"], (name, dt, tiles, post)
        assert len(got["outs"]) == len(exp) and len(got["outs2"]) == (len(exp2) if post else 0)
        for r, (a, b) in enumerate(zip(got["outs"] + got["outs2"], exp + exp2)):
            assert bits_equal(a, b), (band_var, name, dt, tiles, post, r)


# ------------------------------------------------------------------ 6: PushSum with the weights on the device
@functools.lru_cache(maxsize=None)
def pushsum_matrix(name):
    if name != "ring300":
        return MATS[name]
    from fedml_amd.core.distributed.topology.topology_manager import SymmetricTopologyManager, gossip_rows
    m = SymmetricTopologyManager(300, 2)
    m.generate_topology()
    return gossip_rows(m.topology) + (300,)


def pushsum_reference(name, dtype, n, seed=41):
    rp, cs, vs, num_in = pushsum_matrix(name)
    rows = len(rp) - 1
    xs = mix_inputs(dtype, num_in, n, seed, False)
    omega = torch.rand(num_in, generator=torch.Generator().manual_seed(seed), dtype=torch.float32) * 1.5 + 0.5
    ex = [torch.empty(n, dtype=dtype) for _ in range(rows)]
    ez = [torch.empty(n, dtype=dtype) for _ in range(rows)]
    eom = torch.empty(rows, dtype=torch.float32)
    oracle_pushsum(xs, rp, cs, vs, omega, ex, ez, eom)
    return xs, omega, ex, ez, eom


@gpu
@pytest.mark.parametrize("name,dtype,size", [("star9", torch.float32, "3T+17"), ("star9", torch.bfloat16, "5"),
                                             ("random12", torch.float32, "5"), ("random12", torch.bfloat16, "3T+17"),
                                             ("random12", torch.float16, "2T"), ("ring300", torch.float32, "5")],
                         ids=str)
def test_pushsum_device_vs_float32_chain(eng, name, dtype, size):
    """engine.pushsum: omega' the row's ordered float32 chain (a row of 9 entries; 300 rows = two
    k_pushsum_omega workgroups), x' the mixing rows, z = x' * float32(1 / omega'), bit for bit."""
    t = mix_tile(dtype)
    n = {"3T+17": 3 * t + 17, "2T": 2 * t, "5": 5}[size]
    rp, cs, vs, num_in = pushsum_matrix(name)
    rows = len(rp) - 1
    xs, omega, ex, ez, eom = pushsum_reference(name, dtype, n)
    buf, outs, starts = guarded_views(dtype, n, rows)
    buf2, outs2, starts2 = guarded_views(dtype, n, rows)
    obuf, (om_out,), ostarts = guarded_views(torch.float32, rows, 1)
    eng.pushsum([x.to(DEV) for x in xs], rp, cs, vs, omega.to(DEV), outs, outs2, om_out)
    torch.cuda.synchronize()
    assert bits_equal(om_out, eom)
    for r in range(rows):
        assert bits_equal(outs[r], ex[r]), r
        assert bits_equal(outs2[r], ez[r]), r
    assert guards_intact(buf, starts, n) and guards_intact(buf2, starts2, n) and guards_intact(obuf, ostarts, rows)


# ------------------------------------------------------------------ 7: argument checks of the raw entries
@gpu
def test_mix_entries_reject_bad_arguments(eng):
    """fa_mix / fa_mix_tiled / fa_pushsum return the documented code for every bad argument and launch
    nothing; a good call afterwards writes the oracle's rows."""
    from oracle import orc
    L = N.lib()
    n, num_in, rows = 8, 3, 2
    g = torch.Generator().manual_seed(9)
    hx = [torch.randn(n + 4, generator=g) for _ in range(num_in)]
    xs = [x.to(DEV) for x in hx]
    out = torch.full((rows, n), MIX_SENTINEL, device=DEV)
    out2 = torch.full((rows, n), MIX_SENTINEL, device=DEV)
    om_in = torch.ones(num_in, device=DEV)
    om_out = torch.full((rows,), MIX_SENTINEL, device=DEV)
    ins, outs, outs2 = [x.data_ptr() for x in xs], [o.data_ptr() for o in out], [o.data_ptr() for o in out2]
    csr = dict(rp=[0, 2, 3], cs=[0, 1, 2], vs=[0.5, 0.25, 2.0])
    post = [1.0, 0.5]

    def mix(dtype=N.F32, rows=rows, rp=csr["rp"], cs=csr["cs"], ins=ins, outs=outs, post=None, outs2=None,
            strides=None):
        a = [eng._ctx, dtype, n, rows, N.i32_array(rp), N.i32_array(cs), N.f64_array(csr["vs"]), num_in,
             N.ptr_array(ins)]
        a += [strides[0]] if strides else []
        a += [N.ptr_array(outs)]
        a += [strides[1]] if strides else []
        a += [N.f64_array(post) if post else None, N.ptr_array(outs2) if outs2 else None, None]
        return (L.fa_mix_tiled if strides else L.fa_mix)(*a), L.fa_last_error()

    def pushsum(omega_out):
        rc = L.fa_pushsum(eng._ctx, N.F32, n, rows, N.i32_array(csr["rp"]), N.i32_array(csr["cs"]),
                          N.f64_array(csr["vs"]), num_in, N.ptr_array(ins), om_in.data_ptr(), N.ptr_array(outs),
                          N.ptr_array(outs2), omega_out, None)
        return rc, L.fa_last_error()

    tile = (N.TILE_BYTES, N.TILE_BYTES)
    bad = [
        (mix(dtype=N.F64), N.FA_ERR_DTYPE, b"dtype"),
        (mix(rows=0), N.FA_ERR_INVALID, b"invalid arguments"),
        (mix(rp=[1, 2, 3]), N.FA_ERR_INVALID, b"row_ptr[0]"),
        (mix(rp=[0, 3, 3]), N.FA_ERR_INVALID, b"row 1 is empty"),
        (mix(cs=[0, num_in, 2]), N.FA_ERR_INVALID, b"col 3 out of range"),
        (mix(cs=[0, 1, -1]), N.FA_ERR_INVALID, b"col -1 out of range"),
        (mix(outs=[outs[0], None]), N.FA_ERR_INVALID, b"row 1 output NULL"),
        (mix(post=post), N.FA_ERR_INVALID, b"post_scale without d_out2"),
        (mix(strides=(0, N.TILE_BYTES)), N.FA_ERR_INVALID, b"tile strides"),
        (mix(strides=(N.TILE_BYTES, 1000)), N.FA_ERR_INVALID, b"tile strides"),
        (mix(ins=[ins[0], ins[1] + 4, ins[2]], strides=tile), N.FA_ERR_INVALID, b"16-byte aligned"),
        (pushsum(None), N.FA_ERR_INVALID, b"fa_pushsum"),
    ]
    for i, ((rc, err), code, text) in enumerate(bad):
        assert rc == code and text in err, (i, rc, err)
    torch.cuda.synchronize()
    for t in (out, out2, om_out):
        assert bool((t == MIX_SENTINEL).all())  # nothing was launched

    rc, err = mix(post=post, outs2=outs2)
    assert rc == N.FA_OK, err
    exp, exp2 = orc.mix([x[:n].contiguous() for x in hx], csr["rp"], csr["cs"], csr["vs"], post_scale=post)
    for r in range(rows):
        assert bits_equal(out[r], exp[r]) and bits_equal(out2[r], exp2[r])


# ------------------------------------------------------------------ 8: zero-element tensors
@gpu
def test_mix_empty_tensors(eng):
    """n == 0: an empty tensor's pointer is NULL; the mixing entries accept that, return empty rows,
    still compute PushSum's omega', and still reject a bad CSR."""
    rp, cs, vs, num_in = MATS["star9"]
    rows = len(rp) - 1
    xs = [torch.empty(0, device=DEV) for _ in range(num_in)]
    assert xs[0].data_ptr() == 0
    o, o2 = eng.mix(xs, rp, cs, vs)
    assert len(o) == rows and all(t.numel() == 0 for t in o) and o2 is None
    o, o2 = eng.mix(xs, rp, cs, vs, mix_post_scale(rows))
    assert len(o) == len(o2) == rows and all(t.numel() == 0 for t in o + o2)
    _, omega, _, _, eom = pushsum_reference("star9", torch.float32, 0)
    o, o2, om = eng.pushsum(xs, rp, cs, vs, omega.to(DEV))
    torch.cuda.synchronize()
    assert len(o) == len(o2) == rows and all(t.numel() == 0 for t in o + o2)
    assert bits_equal(om, eom)
    with pytest.raises(N.FedAggNativeError, match="is empty"):
        eng.mix(xs, [0, 0] + rp[2:], cs, vs)
    with pytest.raises(N.FedAggNativeError, match="out of range"):
        eng.mix(xs, rp, [num_in] + cs[1:], vs)
    with pytest.raises(N.FedAggNativeError, match="dtype"):
        eng.mix([x.double() for x in xs], rp, cs, vs)


def _state_dicts(num_in, seed):
    g = torch.Generator().manual_seed(seed)
    spec = [("w", (33, 7), torch.float32), ("none", (0,), torch.float32), ("h", (2049,), torch.bfloat16),
            ("none2d", (0, 5), torch.float16), ("b", (5,), torch.float32)]
    return [OrderedDict((k, torch.randn(shape, generator=g, dtype=torch.float64).to(dt).to(DEV))
                        for k, shape, dt in spec) for _ in range(num_in)]


def _check_rows(got, dicts, exp_of, what):
    for k, v in dicts[0].items():
        exp = exp_of([d[k].cpu().reshape(-1) for d in dicts])
        for r, row in enumerate(got):
            assert list(row) == list(dicts[0])
            assert row[k].shape == v.shape and row[k].dtype == v.dtype, (what, k, r)
            assert bits_equal(row[k].reshape(-1), exp[r]), (what, k, r)


@gpu
def test_state_dicts_with_zero_element_keys(eng):
    """state_dict_agg.mix, dsgd_step and pushsum_step (host and device weights) on models that hold
    zero-element keys among ordinary ones: the empty keys come back empty, the others == the oracle."""
    from oracle import orc
    from fedml_amd.core.distributed.topology.topology_manager import gossip_rows, overlay_star
    from fedml_amd.ml.aggregator.state_dict_agg import mix
    from fedml_amd.simulation.sp.decentralized import dsgd_step, pushsum_step
    W = overlay_star(9)
    rp, cs, vs = gossip_rows(W)
    rows = len(rp) - 1
    post = mix_post_scale(rows)
    dicts = _state_dicts(9, 3)

    got, got2 = mix(dicts, rp, cs, vs, post)
    _check_rows(got, dicts, lambda xs: orc.mix(xs, rp, cs, vs)[0], "mix")
    _check_rows(got2, dicts, lambda xs: orc.mix(xs, rp, cs, vs, post_scale=post)[1], "mix post")

    _check_rows(dsgd_step(dicts, W), dicts, lambda xs: orc.mix(xs, rp, cs, vs)[0], "dsgd")

    omegas = [1.0 + 0.125 * i for i in range(9)]
    x, z, om = pushsum_step(dicts, W, omegas)
    _check_rows(x, dicts, lambda xs: orc.mix(xs, rp, cs, vs)[0], "pushsum x")
    _check_rows(z, dicts, lambda xs: orc.mix(xs, rp, cs, vs, post_scale=[1.0 / o for o in om])[1], "pushsum z")

    def device_step(xs, which):
        n = xs[0].numel()
        ex = [torch.empty(n, dtype=xs[0].dtype) for _ in range(rows)]
        ez = [torch.empty(n, dtype=xs[0].dtype) for _ in range(rows)]
        eom = torch.empty(rows, dtype=torch.float32)
        oracle_pushsum(xs, rp, cs, vs, torch.tensor(omegas, dtype=torch.float32), ex, ez, eom)
        return (ex, ez, eom)[which]

    x, z, om = pushsum_step(dicts, W, torch.tensor(omegas, dtype=torch.float32, device=DEV))
    _check_rows(x, dicts, lambda xs: device_step(xs, 0), "pushsum device x")
    _check_rows(z, dicts, lambda xs: device_step(xs, 1), "pushsum device z")
    assert bits_equal(om, device_step([torch.empty(0)] * 9, 2))
