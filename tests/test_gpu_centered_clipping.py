"""Centered clipping on the device: the fused pass fa_centered_sum_sqdist (out bit for bit the per-op
restatement below; the 2K sums within 1e-6 relative of float64 numpy over the returned out), its
distance-only mode, the in-place update, the tiled entry, special values, determinism, and the
defense built on it -- replayed pass by pass, checked against the all-float64 algorithm and the step
bound, and taken through every route (separate tensors, client-major and tiled arenas,
ServerAggregator + FedMLDefender with the global model as the center).

Shapes, data and the stats check are the geometric median tests' (test_gpu_geometric_median.py): a
workgroup chunk is 4096 float32 / 8192 16-bit / 2048 float64 elements; float32 with K <= 32 takes the
single-read register kernel on whole aligned chunks (one instance per K rounded up to 8), every other
K and dtype, ragged and unaligned chunks the generic kernel, whose second walk sums 128 clients per
LDS block."""
from __future__ import annotations

import math
import os
import sys
import types
from collections import OrderedDict

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_geometric_median import (DEV, SEGS, SINGLE, TOL, _cfg, _model_dicts, _reset_defender,  # noqa: E402
                                       check_stats, cluster_data, coefs, normal_data, same_bits, segments,
                                       tiled_buf)

from fedml_amd import _native as N  # noqa: E402
from fedml_amd.cclip import cclip_scales  # noqa: E402

pytestmark = pytest.mark.gpu

F32_K = [1, 2, 8, 12, 17, 32, 33, 65, 129, 150]  # 8, 12, 17, 32: the four register instances
OTHER_K = [3, 40]
OTHER_DT = [torch.bfloat16, torch.float16, torch.float64]
OP = {torch.float32: torch.float32, torch.bfloat16: torch.float32, torch.float16: torch.float32,
      torch.float64: torch.float64}


@pytest.fixture(scope="module")
def eng():
    from fedml_amd.engine import get_engine
    return get_engine(0)


def restate(x, c, coef):
    """The contract of one pass, per op, with torch CPU ops in the storage dtype: x [k, n], c [n].
    Differences and sums are the dtype's own ops (float32 math rounded once for the 16-bit types); the
    product is op-type math with the coefficient cast to the op type, rounded once."""
    dt, a = x.dtype, OP[x.dtype]
    cf = torch.tensor(list(coef), dtype=torch.float64).to(a)
    acc = None
    for i in range(x.shape[0]):
        u = x[i] - c
        t = (u.to(a) * cf[i]).to(dt)
        acc = t if acc is None else acc + t
    return c + acc


def dist2(x, c):
    return ((x.double().numpy() - c.double().numpy()[None, :]) ** 2).sum(axis=1)


def regimes(g, x, c):
    """(name, coef): no client clipped (the weights), every client clipped (radius half the smallest
    distance; a client AT the center cannot be clipped and keeps its weight)."""
    w = coefs(g, x.shape[0])
    r = np.sqrt(dist2(x, c))
    pos = r[r > 0]
    tau = 0.5 * float(pos.min()) if len(pos) else 1.0
    return [("none", w), ("all", [wi * min(1.0, tau / ri) if ri > 0 else wi for wi, ri in zip(w, r)])]


def centered_cluster(g, k, n, dt):
    x = cluster_data(g, k, n, dt)
    c = (50.0 + 1e-3 * torch.randn(n, generator=g, dtype=torch.float64)).to(dt)  # inside the cluster
    return x, c


def normal_pair(g, k, n, dt):
    return normal_data(g, k, n, dt), normal_data(g, 1, n, dt)[0]


def run_flat(eng, x, c, sizes, offset, coef, what, inplace=False):
    segs = segments(x, sizes, offset)
    cens = [col[0] for col in segments(c[None], sizes, offset)]
    outs, stats = eng.centered_sum_sqdist(segs, cens, coef, outs=cens if inplace else None)
    torch.cuda.synchronize()
    out = torch.cat([o.reshape(-1) for o in outs]).cpu()
    assert same_bits(out, restate(x, c, coef)), what
    check_stats(stats, x, out, what)
    return out, stats


def _flat_cases(eng, k, dt, seed):
    g = torch.Generator().manual_seed(seed)
    for make in (normal_pair, centered_cluster):
        for sizes, offsets in ((SEGS, (0, 1)), ([SINGLE], (0,))):
            for offset in offsets:
                x, c = make(g, k, sum(sizes), dt)
                for name, coef in regimes(g, x, c):
                    run_flat(eng, x, c, sizes, offset, coef,
                             f"{make.__name__} k={k} {dt} n={sum(sizes)} offset={offset} clipped={name}")


@pytest.mark.parametrize("k", F32_K)
def test_fused_pass_f32(eng, k):
    _flat_cases(eng, k, torch.float32, 1100 + k)


@pytest.mark.parametrize("k", OTHER_K)
@pytest.mark.parametrize("dt", OTHER_DT, ids=str)
def test_fused_pass_dtypes(eng, dt, k):
    _flat_cases(eng, k, dt, 1200 + k)


# ----------------------------------------------------------------------------- distance-only, in place
def _raw(eng, entry, dt, sizes, k, in_ptrs, cen_ptrs, coef, out_ptrs, stats_ptr, scratch, sbytes,
         tile_stride=N.TILE_BYTES, d_center=True):
    from fedml_amd.engine import DTYPE_CODE
    L = N.lib()
    args = [eng._ctx, DTYPE_CODE[dt] if isinstance(dt, torch.dtype) else dt, len(sizes), N.i64_array(sizes), k,
            N.ptr_array(in_ptrs)]
    args += [tile_stride] if entry.endswith("_tiled") else []
    args += [N.ptr_array(cen_ptrs) if d_center else None, None if coef is None else N.f64_array(coef),
             None if out_ptrs is None else N.ptr_array(out_ptrs), stats_ptr, scratch, sbytes, None]
    return getattr(L, entry)(*args), L.fa_last_error()


@pytest.mark.parametrize("dt,k", [(torch.float32, 8), (torch.float32, 17), (torch.float32, 40), (torch.float32, 129),
                                  (torch.bfloat16, 3), (torch.float16, 40), (torch.float64, 3)], ids=str)
def test_distance_only(eng, dt, k):
    g = torch.Generator().manual_seed(1300 + k)
    L = N.lib()
    for make in (normal_pair, centered_cluster):
        for sizes, offset in ((SEGS, 0), (SEGS, 1), ([SINGLE], 0)):
            what = f"dist {make.__name__} k={k} {dt} n={sum(sizes)} offset={offset}"
            x, c = make(g, k, sum(sizes), dt)
            segs = segments(x, sizes, offset)
            cens = [col[0] for col in segments(c[None], sizes, offset)]
            outs, stats = eng.centered_sum_sqdist(segs, cens, None)
            assert outs is None
            check_stats(stats, x, c, what)  # against the center itself
            assert same_bits(torch.cat(cens), c)
            # the C entry: a sentinel-filled out is not written, and d_out may be NULL
            guard = [torch.full((n,), 7.0, dtype=dt, device=DEV) for n in sizes]
            need = L.fa_weighted_sum_sqdist_scratch_bytes(len(sizes), N.i64_array(sizes), k)
            scratch = torch.zeros(need, dtype=torch.uint8, device=DEV)
            for out_ptrs in ([t.data_ptr() for t in guard], None):
                st = torch.full((2, k), 7.0, dtype=torch.float64, device=DEV)
                rc, err = _raw(eng, "fa_centered_sum_sqdist", dt, sizes, k, [t.data_ptr() for col in segs for t in col],
                               [t.data_ptr() for t in cens], None, out_ptrs, st.data_ptr(), scratch.data_ptr(), need)
                assert rc == N.FA_OK, err
                torch.cuda.synchronize()
                assert torch.equal(st.view(torch.int64), stats.view(torch.int64)), what
            assert all(bool((t == 7.0).all()) for t in guard), what


@pytest.mark.parametrize("dt,k", [(torch.float32, 8), (torch.float32, 40), (torch.bfloat16, 3)], ids=str)
def test_in_place_equals_separate_buffers(eng, dt, k):
    """d_out == d_center: the register form (float32, K = 8, whole aligned chunks) and the generic one."""
    g = torch.Generator().manual_seed(1400 + k)
    for sizes, offset in ((SEGS, 0), (SEGS, 1), ([SINGLE], 0)):
        x, c = normal_pair(g, k, sum(sizes), dt)
        coef = regimes(g, x, c)[1][1]
        sep, st_sep = run_flat(eng, x, c, sizes, offset, coef, f"separate k={k} {dt}")
        inp, st_inp = run_flat(eng, x, c, sizes, offset, coef, f"in place k={k} {dt}", inplace=True)
        assert same_bits(sep, inp)
        assert torch.equal(st_sep.view(torch.int64), st_inp.view(torch.int64))


@pytest.mark.parametrize("tiles", [3, 9], ids=["3E+17", "9E+17"])
@pytest.mark.parametrize("dt,k", [(torch.float32, 3), (torch.float32, 32), (torch.float32, 129),
                                  (torch.bfloat16, 40)], ids=str)
def test_tiled_equals_flat(eng, dt, k, tiles):
    g = torch.Generator().manual_seed(1500 + k + tiles)
    for make in (normal_data, cluster_data):
        E = N.TILE_BYTES // torch.empty((), dtype=dt).element_size()
        n = tiles * E + 17
        buf, rows, x, _ = tiled_buf(g, make, k, k + 3, n, dt)
        c = x[0].clone() if make is cluster_data else normal_data(g, 1, n, dt)[0]
        x = x.contiguous()
        for name, coef in regimes(g, x, c):
            what = f"{make.__name__} k={k} {dt} n={n} clipped={name}"
            cd = c.to(DEV)
            out_t, stats_t = eng.centered_sum_sqdist_tiled(buf, rows, cd, coef, n=n)
            out_f, _ = run_flat(eng, x, c, [n], 0, coef, "flat " + what)
            torch.cuda.synchronize()
            assert out_t.shape == (n,) and same_bits(out_t.cpu(), out_f)
            check_stats(stats_t, x, out_t, "tiled " + what)
            assert same_bits(cd.cpu(), c)  # the center is only read
            none, stats_d = eng.centered_sum_sqdist_tiled(buf, rows, cd, None, n=n)
            assert none is None
            check_stats(stats_d, x, c, "tiled dist " + what)
            out_i, stats_i = eng.centered_sum_sqdist_tiled(buf, rows, cd, coef, n=n, out=cd)  # in place
            assert out_i.data_ptr() == cd.data_ptr() and same_bits(cd.cpu(), out_f)
            assert torch.equal(stats_i.view(torch.int64), stats_t.view(torch.int64))


MIXED = [0, 5, 0, 4097]


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=str)
def test_empty_segments_among_full_ones(eng, dt, offset):
    """The host path leaves empty segments out of the segment table: the kept segments' centers must
    be the ones the kernel finds at their table index."""
    g = torch.Generator().manual_seed(1600 + offset)
    x, c = normal_pair(g, 3, sum(MIXED), dt)
    coef = coefs(g, 3)
    run_flat(eng, x, c, MIXED, offset, coef, f"mixed {dt} offset={offset}")
    segs = segments(x, MIXED, offset)
    cens = [col[0] for col in segments(c[None], MIXED, offset)]
    check_stats(eng.centered_sum_sqdist(segs, cens, None)[1], x, c, f"mixed dist {dt} offset={offset}")
    # all segments empty: the stats are zeroed
    empty = [[torch.empty(0, dtype=dt, device=DEV) for _ in range(3)] for _ in range(2)]
    for cf in (coef, None):
        _, st = eng.centered_sum_sqdist(empty, [torch.empty(0, dtype=dt, device=DEV)] * 2, cf)
        assert bool((st == 0.0).all())


def test_single_client_at_the_center(eng):
    g = torch.Generator().manual_seed(15)
    for dt in (torch.float32, torch.bfloat16, torch.float16, torch.float64):
        x = normal_data(g, 1, SINGLE, dt)
        segs = segments(x, [SINGLE], 0)
        outs, stats = eng.centered_sum_sqdist(segs, [segs[0][0].clone()], [1.0])
        assert torch.equal(outs[0].cpu(), x[0])  # out == x (a -0.0 comes back as +0.0: -0 + (+0))
        s = stats.cpu()
        assert s[0, 0].item() == 0.0 and math.copysign(1.0, s[0, 0].item()) == 1.0
        check_stats(stats, x, outs[0], f"k=1 {dt}")


def test_same_call_gives_the_same_bits(eng):
    g = torch.Generator().manual_seed(16)
    for k in (17, 33):
        x, c = normal_pair(g, k, sum(SEGS) + SINGLE, torch.float32)
        segs = segments(x, SEGS + [SINGLE], 0)
        cens = [col[0] for col in segments(c[None], SEGS + [SINGLE], 0)]
        coef = coefs(g, k)
        for cf in (coef, None):
            runs = [eng.centered_sum_sqdist(segs, cens, cf) for _ in range(3)]
            torch.cuda.synchronize()
            for outs, stats in runs[1:]:
                assert torch.equal(stats.view(torch.int64), runs[0][1].view(torch.int64))
                assert cf is None or all(same_bits(a, b) for a, b in zip(outs, runs[0][0]))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float64], ids=str)
def test_special_values(eng, dt):
    g = torch.Generator().manual_seed(17)
    k = 9
    x, c = normal_pair(g, k, sum(SEGS), dt)
    coef = coefs(g, k)
    # a NaN in the center: NaN out there, every distance NaN
    cn = c.clone()
    cn[300] = float("nan")
    segs = segments(x, SEGS, 0)
    outs, stats = eng.centered_sum_sqdist(segs, [col[0] for col in segments(cn[None], SEGS, 0)], coef)
    out, ref = torch.cat(outs).cpu(), restate(x, cn, coef)
    assert bool(out[300].isnan()) and int(out.isnan().sum()) == 1 and torch.equal(out.isnan(), ref.isnan())
    keep = ~out.isnan()
    assert same_bits(out[keep], ref[keep])
    s = stats.cpu().numpy()
    assert np.all(np.isnan(s[0])) and np.all(np.isfinite(s[1]))
    s = eng.centered_sum_sqdist(segs, [col[0] for col in segments(cn[None], SEGS, 0)], None)[1].cpu().numpy()
    assert np.all(np.isnan(s[0])) and np.all(np.isfinite(s[1]))
    # a client with an Inf: its ss and d2 are not finite; with coefficient 0 the Inf still gives NaN
    xi = x.clone()
    xi[6, 5000] = float("inf")
    segs = segments(xi, SEGS, 0)
    cens = [col[0] for col in segments(c[None], SEGS, 0)]
    for cf in (coef, coef[:6] + [0.0] + coef[7:]):
        outs, stats = eng.centered_sum_sqdist(segs, cens, cf)
        out, ref = torch.cat(outs).cpu(), restate(xi, c, cf)
        assert torch.equal(out.isnan(), ref.isnan()) and same_bits(out[~out.isnan()], ref[~ref.isnan()])
        assert bool(out[5000].isnan()) if cf[6] == 0.0 else bool(out[5000].isinf())
        s = stats.cpu().numpy()
        assert [i for i in range(k) if not np.isfinite(s[1, i])] == [6]
        assert not np.isfinite(s[0, 6])
    s = eng.centered_sum_sqdist(segs, cens, None)[1].cpu().numpy()
    assert [i for i in range(k) if not np.isfinite(s[0, i])] == [6]
    assert [i for i in range(k) if not np.isfinite(s[1, i])] == [6]


# ----------------------------------------------------------------------------- argument checks
@pytest.mark.parametrize("entry", ["fa_centered_sum_sqdist", "fa_centered_sum_sqdist_tiled"])
def test_entry_rejects_bad_arguments(eng, entry):
    L = N.lib()
    K, NUMEL = 3, 8
    xs = [torch.zeros(1024, device=DEV) for _ in range(K)]
    cen = torch.zeros(NUMEL, device=DEV)
    out = torch.full((NUMEL,), 7.0, device=DEV)
    stats = torch.full((2 * K,), 7.0, dtype=torch.float64, device=DEV)
    need = L.fa_weighted_sum_sqdist_scratch_bytes(1, N.i64_array([NUMEL]), K)
    scratch = torch.zeros(need, dtype=torch.uint8, device=DEV)
    good = [x.data_ptr() for x in xs]

    def call(dtype=N.F32, numel=NUMEL, k=K, ptrs=good, cens=(cen.data_ptr(),), d_center=True, coef=(0.2, 0.3, 0.5),
             outs=(out.data_ptr(),), st=stats.data_ptr(), sptr=scratch.data_ptr(), sbytes=need,
             tile_stride=N.TILE_BYTES):
        return _raw(eng, entry, dtype, [numel], k, ptrs, list(cens), coef, None if outs is None else list(outs), st,
                    sptr, sbytes, tile_stride=tile_stride, d_center=d_center)

    def named(err):
        return err.startswith(entry.encode() + b":")

    for coef in ((0.2, 0.3, 0.5), None):  # the fused and the distance-only mode check alike
        rc, err = call(coef=coef, d_center=False)
        assert rc == N.FA_ERR_INVALID and named(err), err
        rc, err = call(coef=coef, cens=(None,))
        assert rc == N.FA_ERR_INVALID and b"center NULL" in err and named(err), err
        rc, err = call(coef=coef, st=None)
        assert rc == N.FA_ERR_INVALID and b"d_stats" in err and named(err), err
        rc, err = call(coef=coef, sbytes=need - 1)
        assert rc == N.FA_ERR_INVALID and b"scratch" in err and named(err), err
        rc, err = call(coef=coef, sptr=None)
        assert rc == N.FA_ERR_INVALID and b"scratch" in err and named(err), err
        rc, err = call(coef=coef, dtype=N.I64)
        assert rc == N.FA_ERR_DTYPE and named(err), err
        rc, err = call(coef=coef, k=0)
        assert rc == N.FA_ERR_INVALID and named(err), err
        rc, err = call(coef=coef, ptrs=[good[0], None, good[2]])
        assert rc == N.FA_ERR_INVALID and b"input NULL" in err and named(err), err
        rc, err = call(coef=coef, numel=-NUMEL)
        assert rc == N.FA_ERR_INVALID and named(err), err
        if entry.endswith("_tiled"):
            for bad in (1000, 0, -4096):
                rc, err = call(coef=coef, tile_stride=bad)
                assert rc == N.FA_ERR_INVALID and b"tile_stride" in err and named(err), err
    # the documented order: d_center before d_stats before the dtype before a segment's center
    rc, err = call(d_center=False, st=None, dtype=N.I64)
    assert rc == N.FA_ERR_INVALID and b"d_center" in err, err
    rc, err = call(st=None, dtype=N.I64, cens=(None,))
    assert rc == N.FA_ERR_INVALID and b"d_stats" in err, err
    rc, err = call(dtype=N.I64, cens=(None,), sbytes=0)
    assert rc == N.FA_ERR_DTYPE, err
    rc, err = call(cens=(None,), sbytes=0)
    assert rc == N.FA_ERR_INVALID and b"center NULL" in err, err
    rc, err = call(outs=None)  # the fused mode needs d_out
    assert rc == N.FA_ERR_INVALID and named(err), err
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((stats == 7.0).all())  # nothing was launched
    rc, err = call(coef=None, outs=None)
    assert rc == N.FA_OK, err
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((stats == 0.0).all())
    rc, err = call()
    assert rc == N.FA_OK, err
    torch.cuda.synchronize()
    assert bool((out == 0.0).all()) and bool((stats == 0.0).all())


def test_engine_argument_checks(eng):
    xs = [torch.zeros(8, device=DEV) for _ in range(3)]
    c = torch.zeros(8, device=DEV)
    w = [0.2, 0.3, 0.5]
    with pytest.raises(ValueError):
        eng.centered_sum_sqdist([], [], [])
    with pytest.raises(ValueError):
        eng.centered_sum_sqdist([xs], [c], [0.5, 0.5])
    with pytest.raises(TypeError):
        eng.centered_sum_sqdist([[x.long() for x in xs]], [c.long()], w)
    with pytest.raises(ValueError):
        eng.centered_sum_sqdist([xs, xs[:2]], [c, c], w)
    with pytest.raises(ValueError):
        eng.centered_sum_sqdist([xs], [c], w, outs=[torch.zeros(7, device=DEV)])
    for cf in (w, None):
        with pytest.raises(ValueError):
            eng.centered_sum_sqdist([xs], None, cf)
        with pytest.raises(ValueError):
            eng.centered_sum_sqdist([xs], [c, c], cf)
        with pytest.raises(ValueError, match="center"):
            eng.centered_sum_sqdist([xs], [c.double()], cf)
        with pytest.raises(ValueError, match="center"):
            eng.centered_sum_sqdist([xs], [torch.zeros(7, device=DEV)], cf)
        with pytest.raises(ValueError, match="center"):
            eng.centered_sum_sqdist([xs], [torch.zeros(16, device=DEV)[::2]], cf)
        with pytest.raises(ValueError):
            eng.centered_sum_sqdist([xs], [c.cpu()], cf)
    buf = torch.zeros(2, 4, 1024, device=DEV)
    c2 = torch.zeros(2048, device=DEV)
    with pytest.raises(ValueError):
        eng.centered_sum_sqdist_tiled(buf, [0, 1], c2, [1.0])
    with pytest.raises(IndexError):
        eng.centered_sum_sqdist_tiled(buf, [0, 4], c2, [0.5, 0.5])
    with pytest.raises(ValueError):
        eng.centered_sum_sqdist_tiled(buf, [0, 1], None, [0.5, 0.5])
    with pytest.raises(ValueError, match="center"):
        eng.centered_sum_sqdist_tiled(buf, [0, 1], c2[:2047], [0.5, 0.5])
    with pytest.raises(ValueError, match="center"):
        eng.centered_sum_sqdist_tiled(buf, [0, 1], c2.double(), None)
    with pytest.raises(ValueError):
        eng.centered_sum_sqdist_tiled(buf, [0, 1], c2.cpu(), None)
    with pytest.raises(ValueError):
        eng.centered_sum_sqdist_tiled(buf, [0, 1], c2, [0.5, 0.5], out=torch.zeros(7, device=DEV))
    out, stats = eng.centered_sum_sqdist_tiled(buf, [0, 1], c2[:0], [0.5, 0.5], n=0)  # nothing to read: sums are 0
    assert out.numel() == 0 and bool((stats == 0.0).all())


# ----------------------------------------------------------------------------- the defense, replayed
def _center_dict(g, ds):
    """A global model for the clients ``ds``: their keys, values like an honest client's."""
    like = _model_dicts(g, 1, ints=any(v.dtype == torch.int64 for v in ds[0].values()))[0]
    return OrderedDict((key, like[key]) for key in ds[0])


def _float_keys(sd):
    return [key for key, v in sd.items() if v.dtype.is_floating_point]


def _key_dist2(ds, v):
    d2 = np.zeros(len(ds))
    for key, vk in v.items():
        vd = vk.double().cpu().numpy().reshape(-1)
        for i, d in enumerate(ds):
            d2[i] += ((d[key].double().cpu().numpy().reshape(-1) - vd) ** 2).sum()
    return d2


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("k", [10, 33, 128])
def test_defense_replay(eng, k, iters):
    from fedml_amd.core.security.defense.centered_clipping_defense import CenteredClippingDefense
    from fedml_amd.ml.aggregator.agg_operator import FedMLAggOperator
    g = torch.Generator().manual_seed(1700 + k)
    ds = _model_dicts(g, k)
    cen = _center_dict(g, ds)
    counts = [int(v) for v in torch.randint(20, 600, (k,), generator=g)]
    raw = list(zip(counts, ds))
    tau = 120.0  # the honest clients are ~104 from the center, every fifth client ~460
    d = CenteredClippingDefense(_cfg(cclip_tau=tau, cclip_iters=iters))
    out = d.defend_on_aggregation(raw, base_aggregation_func=FedMLAggOperator.agg, extra_auxiliary_info=cen)
    info = d.last_info
    assert info["dropped"] == [] and d.get_malicious_client_idxs() == [] and info["clients"] == list(range(k))
    assert len(info["scale_trace"]) == iters and len(info["d2_trace"]) == iters + 1
    w = [c / sum(float(c) for c in counts) for c in counts]
    fk = _float_keys(ds[0])
    v = OrderedDict((key, cen[key].cpu().reshape(-1)) for key in fk)
    xs = {key: torch.stack([sd[key].cpu().reshape(-1) for sd in ds]) for key in fk}
    for t in range(iters + 1):
        ref = _key_dist2(ds, v)
        got = np.array(info["d2_trace"][t])
        err = np.abs(got - ref) / ref
        print(f"k={k} pass {t}: d2 max rel err {err.max():.3e}")
        assert err.max() <= TOL
        if t < iters:
            scales = cclip_scales(w, info["d2_trace"][t], tau)  # from the DEVICE distances
            assert info["scale_trace"][t] == scales
            v = OrderedDict((key, restate(xs[key], v[key], scales)) for key in fk)
    last = info["scale_trace"][-1]
    assert info["clipped"] == [i for i in range(k) if last[i] < w[i]]
    assert set(i for i in range(k) if i % 5 == 3) <= set(info["clipped"]) and len(info["clipped"]) < k
    assert list(out) == list(ds[0])
    base = FedMLAggOperator.agg(_cfg(), raw)
    for key, o in out.items():
        assert o.shape == ds[0][key].shape and o.device == ds[0][key].device
        if ds[0][key].dtype == torch.int64:
            assert o.dtype == base[key].dtype and torch.equal(o.cpu(), base[key].cpu())
        else:
            assert same_bits(o.reshape(-1).cpu(), v[key]), key
    # no iteration: the start point -- the center, or the FedAvg result
    d0 = CenteredClippingDefense(_cfg(cclip_tau=tau, cclip_iters=0))
    out0 = d0.defend_on_aggregation(raw, base_aggregation_func=FedMLAggOperator.agg, extra_auxiliary_info=cen)
    assert d0.last_info["scale_trace"] == [] and d0.last_info["clipped"] == []
    assert all(same_bits(out0[key], cen[key]) for key in fk)
    out0 = d0.defend_on_aggregation(raw, base_aggregation_func=FedMLAggOperator.agg)
    assert all(same_bits(out0[key], base[key]) for key in out0)
    with pytest.raises(TypeError):  # an int64 key and nothing to aggregate it with
        d.defend_on_aggregation(raw, extra_auxiliary_info=cen)
    # the center must carry every float key with the clients' dtype and shape
    for bad in (OrderedDict((key, t) for key, t in cen.items() if key != "b.emb"),
                OrderedDict((key, t.float() if key == "b.emb" else t) for key, t in cen.items()),
                OrderedDict((key, t.reshape(-1) if key == "a.weight" else t) for key, t in cen.items())):
        with pytest.raises(ValueError, match="center"):
            d.defend_on_aggregation(raw, base_aggregation_func=FedMLAggOperator.agg, extra_auxiliary_info=bad)


# ----------------------------------------------------------------------------- against float64
def _walk64(x, v0, counts, tau, iters):
    xd, v = x.astype(np.float64), v0.astype(np.float64)
    w = np.array(counts, dtype=np.float64) / float(sum(counts))
    for _ in range(iters):
        r = np.sqrt(((xd - v[None, :]) ** 2).sum(axis=1))
        s = np.where(r <= tau, w, w * (tau / np.maximum(r, 1e-300)))
        v = v + (s[:, None] * (xd - v[None, :])).sum(axis=0)
    return v


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("tau", [1.0, 10.0])
@pytest.mark.parametrize("k,n", [(10, 3001), (33, 5003), (128, 2049)])
def test_against_the_float64_algorithm(k, n, tau, iters):
    from fedml_amd.core.security.defense.centered_clipping_defense import CenteredClippingDefense
    g = torch.Generator().manual_seed(1800 + k)
    x = 1.0 + 0.05 * torch.randn(k, n, generator=g)
    for i in range(k // 5):  # one fifth of the clients
        x[i] = 40.0 + 3.0 * torch.randn(n, generator=g)
    x = x[torch.randperm(k, generator=g)]
    v0 = 1.0 + 0.05 * torch.randn(n, generator=g)  # distributed like an honest client
    counts = [float(c) for c in torch.randint(20, 600, (k,), generator=g)]
    ref = _walk64(x.numpy(), v0.numpy(), counts, tau, iters)
    d = CenteredClippingDefense(_cfg(cclip_tau=tau, cclip_iters=iters))
    out = d.defend_on_aggregation([(c, OrderedDict(w=x[i].to(DEV))) for i, c in enumerate(counts)],
                                  extra_auxiliary_info=OrderedDict(w=v0.to(DEV)))
    got = out["w"].double().cpu().numpy()
    err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    print(f"k={k} n={n} tau={tau} iters={iters}: relative L2 error {err:.3e}, |v - v0| "
          f"{np.linalg.norm(got - v0.double().numpy()):.4f}")
    assert err <= 2e-6


# ----------------------------------------------------------------------------- the step bound
@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize("k", [8, 40, 150])
def test_every_step_is_at_most_tau_long(eng, dt, k):
    """|v_{l+1} - v_l| = |sum_i s_i (x_i - v_l)| <= sum_i w_i min(r_i, tau) <= tau by the triangle
    inequality with sum w = 1; the K + 2 roundings per element (2^-24 each at most, K <= 150) stay
    under the 1e-5 allowed.  The second data set is the worst case: every client 1e6 away in one
    direction, so every term is exactly tau long and they all add up."""
    g = torch.Generator().manual_seed(1900 + k)
    n = 3001
    far = torch.randn(n, generator=g, dtype=torch.float64)
    far = far / far.norm()
    v0 = torch.randn(n, generator=g, dtype=torch.float64)
    mixed = v0[None, :] + torch.randn(k, n, generator=g, dtype=torch.float64) * \
        torch.logspace(-3, 3, k, dtype=torch.float64)[torch.randperm(k, generator=g)][:, None]
    worst = v0[None, :] + 1e6 * far[None, :] * (1.0 + 0.01 * torch.rand(k, 1, generator=g, dtype=torch.float64))
    for name, x in (("mixed", mixed), ("worst", worst)):
        for tau in (1.0, 10.0):
            x = x.to(dt)
            segs = segments(x, [n], 0)
            v = v0.to(dt).to(DEV)
            w = coefs(g, k)
            d2 = eng.centered_sum_sqdist(segs, [v], None)[1][0].tolist()
            for it in range(3):
                prev = v.double().cpu()
                _, stats = eng.centered_sum_sqdist(segs, [v], cclip_scales(w, d2, tau), outs=[v])
                d2 = stats[0].tolist()
                step = float((v.double().cpu() - prev).norm())
                print(f"{name} k={k} {dt} tau={tau} step {it}: |v' - v| = {step:.9g} ({step / tau:.9f} tau)")
                assert step <= tau * (1.0 + 1e-5)
                if name == "worst":
                    assert step >= tau * (1.0 - 1e-5)


# ----------------------------------------------------------------------------- every route, same bits
def _bn_model(g):
    m = torch.nn.Sequential(torch.nn.Linear(40, 130), torch.nn.BatchNorm1d(130))
    with torch.no_grad():
        for key, v in m.state_dict().items():
            if v.dtype.is_floating_point:
                v.copy_(torch.randn(v.shape, generator=g))
            else:
                v.fill_(1000)
    return m


def _bn_clients(g, model, k):
    ds = []
    for i in range(k):
        sd = OrderedDict()
        for key, v in model.state_dict().items():
            if v.dtype.is_floating_point:
                sd[key] = (v + (0.02 + (3.0 if i % 4 == 1 else 0.0)) * torch.randn(v.shape, generator=g)).to(DEV)
            else:
                sd[key] = torch.tensor(100 + 7 * i, dtype=torch.int64, device=DEV)
        ds.append(sd)
    return ds


CC = dict(cclip_tau=2.0, cclip_iters=3)  # honest clients ~1.5 from the global model, every fourth ~220


def _through_server_aggregator(model, raw, **kw):
    from fedml_amd.core.security.fedml_defender import FedMLDefender
    from fedml_amd.ml.aggregator.default_aggregator import DefaultServerAggregator
    try:
        agg = DefaultServerAggregator(model, _cfg(enable_defense=True, defense_type="centered_clipping", **CC, **kw))
        kept, _ = agg.on_before_aggregation(raw)
        assert len(kept) == len(raw) and all(a is b for (_, a), (_, b) in zip(kept, raw))
        out = agg.aggregate(kept)
        d = FedMLDefender.get_instance()
        return out, d.get_malicious_client_idxs(), d.defender.last_info
    finally:
        _reset_defender()


def _pack(arena, sd):
    packed = {dt: torch.zeros(n, dtype=dt, device=DEV) for dt, n in arena.layout.group_numel.items()}
    for key in arena.layout.keys:
        dt, off, _, n = arena.layout.where[key]
        packed[dt][off:off + n].copy_(sd[key].reshape(-1))
    return packed


def test_every_route_gives_the_same_bits(eng, monkeypatch):
    from fedml_amd.arena import ClientArena, resident_rows
    from fedml_amd.core.security.defense.centered_clipping_defense import CenteredClippingDefense
    from fedml_amd.ml.aggregator.agg_operator import FedMLAggOperator
    g = torch.Generator().manual_seed(18)
    k = 12
    model = _bn_model(g)
    glob = OrderedDict((key, v.clone()) for key, v in model.state_dict().items())
    ds = _bn_clients(g, model, k)
    fk = _float_keys(ds[0])
    assert len(fk) < len(ds[0])  # float32 keys and the int64 counter
    counts = [int(v) for v in torch.randint(20, 600, (k,), generator=g)]
    raw = list(zip(counts, ds))
    d = CenteredClippingDefense(_cfg(**CC))
    ref = d.defend_on_aggregation(raw, FedMLAggOperator.agg, glob)  # separate tensors, a CPU center
    ref_info = d.last_info
    assert ref_info["dropped"] == [] and 0 < len(ref_info["clipped"]) < k
    assert not any(same_bits(ref[key].cpu(), glob[key]) for key in fk)
    assert all(torch.equal(v, model.state_dict()[key]) for key, v in glob.items())  # the center is only read
    # the full route: get_model_params() is the center
    out, bad, info = _through_server_aggregator(model, raw)
    assert bad == [] and list(out) == list(ref) and all(same_bits(out[key], ref[key]) for key in ref)
    assert info["scale_trace"] == ref_info["scale_trace"]
    # CPU dicts in, CPU tensors out
    cpu = d.defend_on_aggregation([(c, OrderedDict((key, v.cpu()) for key, v in sd.items())) for c, sd in raw],
                                  FedMLAggOperator.agg, glob)
    assert list(cpu) == list(ref) and all(v.device.type == "cpu" for v in cpu.values())
    assert all(same_bits(cpu[key], ref[key]) for key in fk)
    # cclip_center="mean" ignores the global model
    dm = CenteredClippingDefense(_cfg(cclip_center="mean", **CC))
    mean = dm.defend_on_aggregation(raw, FedMLAggOperator.agg, glob)
    none = d.defend_on_aggregation(raw, FedMLAggOperator.agg, None)  # "global" without a dict: the mean too
    assert all(same_bits(mean[key], none[key]) for key in ref)
    assert not any(same_bits(mean[key], ref[key]) for key in fk)
    out, _, _ = _through_server_aggregator(model, raw, cclip_center="mean")
    assert all(same_bits(out[key], mean[key]) for key in ref)
    # the arenas hold the float keys (centered_clip takes float groups only)
    fds = [OrderedDict((key, sd[key]) for key in fk) for sd in ds]
    fglob = OrderedDict((key, glob[key].to(DEV)) for key in fk)
    ta = ClientArena.for_model(fds[0], k + 2, device=DEV, tiled=True)
    rows = [(5 * i + 3) % (k + 2) for i in range(k)]
    for r, sd in zip(rows, fds):
        ta.write(r, sd)
    for center, want in ((_pack(ta, fglob), ref), (None, mean)):
        info = {}
        out = ta.centered_clip(counts, CC["cclip_tau"], CC["cclip_iters"], center=center, clients=rows, info=info)
        assert list(out) == fk and all(same_bits(out[key], want[key]) for key in fk)
        assert len(info["scale_trace"]) == 3 and len(info["d2_trace"]) == 4
    assert info["scale_trace"][0] != ref_info["scale_trace"][0]
    packed = _pack(ta, fglob)
    keep = {dt: t.clone() for dt, t in packed.items()}
    ta.centered_clip(counts, CC["cclip_tau"], CC["cclip_iters"], center=packed, clients=rows)
    assert all(same_bits(packed[dt], keep[dt]) for dt in packed)  # the center is only read
    with pytest.raises(ValueError, match="center"):
        ta.centered_clip(counts, 2.0, 1, center={torch.float32: packed[torch.float32][:-1]}, clients=rows)
    # a client-major arena, driven directly and found by the defense through the adopted rows
    copies = [OrderedDict((key, v.clone()) for key, v in sd.items()) for sd in fds]
    ca = ClientArena.for_model(copies[0], k, device=DEV)
    for i, sd in enumerate(copies):
        ca.adopt(i, sd)
    out = ca.centered_clip(counts, CC["cclip_tau"], CC["cclip_iters"], center=_pack(ca, fglob))
    assert all(same_bits(out[key], ref[key]) for key in fk)
    assert resident_rows(copies) is not None
    calls = []
    real = ClientArena.centered_clip
    monkeypatch.setattr(ClientArena, "centered_clip",
                        lambda self, *a, **kw: calls.append(a) or real(self, *a, **kw))
    for center, want in ((glob, ref), (None, mean)):
        out = d.defend_on_aggregation(list(zip(counts, copies)), extra_auxiliary_info=center)
        assert all(same_bits(out[key], want[key]) for key in fk)
    assert len(calls) == 2
    assert all(torch.equal(v, model.state_dict()[key]) for key, v in glob.items())


def test_a_nan_client_is_dropped(eng):
    from fedml_amd.core.security.defense.centered_clipping_defense import CenteredClippingDefense
    g = torch.Generator().manual_seed(19)
    k = 12
    model = _bn_model(g)
    ds = _bn_clients(g, model, k)
    counts = [int(v) for v in torch.randint(20, 600, (k,), generator=g)]
    clean = [(c, sd) for i, (c, sd) in enumerate(zip(counts, ds)) if i != 4]
    ds[4]["0.weight"][7, 7] = float("nan")
    for kw in (dict(), dict(cclip_center="mean")):
        out, bad, info = _through_server_aggregator(model, list(zip(counts, ds)), **kw)
        assert bad == [4] and info["clients"] == [i for i in range(k) if i != 4]
        ref, none, _ = _through_server_aggregator(model, clean, **kw)
        assert none == []
        for key in _float_keys(ds[0]):
            assert same_bits(out[key], ref[key]), key
    w = torch.ones(100, device=DEV)
    with pytest.raises(ValueError, match="every client"):
        CenteredClippingDefense(_cfg()).defend_on_aggregation([(1, OrderedDict(w=w * float("nan"))),
                                                              (2, OrderedDict(w=w * float("inf")))],
                                                             extra_auxiliary_info=OrderedDict(w=w))
    with pytest.raises(ValueError, match="NaN"):  # a NaN in the center itself
        CenteredClippingDefense(_cfg()).defend_on_aggregation([(1, OrderedDict(w=w)), (2, OrderedDict(w=2 * w))],
                                                             extra_auxiliary_info=OrderedDict(w=w * float("nan")))
