"""The geometric median on the device: the fused pass fa_weighted_sum_sqdist (out bit for bit the MUL_W
weighted sum; the 2K sums within 1e-6 relative of float64 numpy over the returned out), its tiled
entry, special values, determinism, and the defense built on it -- replayed pass by pass, checked
against the all-float64 algorithm, and taken through every route (separate tensors, client-major
and tiled arenas, ServerAggregator + FedMLDefender).

Workgroup chunk of the kernel: 4 tiles of 4 KiB per client = 4096 float32 / 8192 16-bit / 2048 float64
elements; the shapes below cover whole aligned chunks (16-byte loads), ragged last chunks, unaligned
segments (element loads) and segments below one chunk, in the flat and the tiled layout.  float32
with K <= 32 takes the single-read register kernel on whole aligned chunks (one instance per K
rounded up to 8), K >= 33 and every other dtype the generic kernel."""
from __future__ import annotations

import math
import types
from collections import OrderedDict

import numpy as np
import pytest
import torch

from fedml_amd import _native as N
from fedml_amd.weiszfeld import weiszfeld_coef, weiszfeld_driver

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEGS = [1, 2, 3, 257, 4096, 3001]
SINGLE = 20001
TOL = 1e-6
INT_VIEW = {2: torch.int16, 4: torch.int32, 8: torch.int64}
F32_K = [1, 2, 3, 8, 12, 17, 24, 32, 33, 64, 65, 96, 128, 129, 150]  # 12, 24: register-kernel instances 16, 24
OTHER_K = [3, 32, 40, 96]
OTHER_DT = [torch.bfloat16, torch.float16, torch.float64]


@pytest.fixture(scope="module")
def eng():
    from fedml_amd.engine import get_engine
    return get_engine(0)


def bits(t):
    return t.contiguous().view(INT_VIEW[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


def normal_data(g, k, n, dt):
    """N(0, 1) with ties across clients and signed zeros."""
    x = torch.randn(k, n, generator=g, dtype=torch.float64)
    if k > 1:
        tie = torch.rand(n, generator=g) < 0.1
        x[k - 1, tie] = x[0, tie]
    z = torch.rand(k, n, generator=g)
    x[z < 0.03] = 0.0
    x[z > 0.97] = -0.0
    return x.to(dt)


def cluster_data(g, k, n, dt):
    """A cluster 1e-3 wide at offset 50 and (k >= 4) three far clients: d2 of a cluster member is
    ~1e-6 n against ss ~ 2500 n, so a form that cancels (ss - 2 x.z + z.z) would lose the digits."""
    x = 50.0 + 1e-3 * torch.randn(k, n, generator=g, dtype=torch.float64)
    if k >= 4:
        x[1] = -30.0 + torch.randn(n, generator=g, dtype=torch.float64)
        x[k // 2] = 200.0 + 5.0 * torch.randn(n, generator=g, dtype=torch.float64)
        x[k - 1] = 50.0 + 5.0 * torch.randn(n, generator=g, dtype=torch.float64)
    return x.to(dt)


def coefs(g, k):
    w = (torch.rand(k, generator=g, dtype=torch.float64) + 0.05).tolist()
    s = sum(w)
    return [v / s for v in w]


def segments(x, sizes, offset):
    """x [k, n] on the host -> device segments [s][i].  offset 0: each tensor its own (aligned)
    allocation; offset 1: views one element into a larger allocation (unaligned for every dtype)."""
    xd = x.to(DEV)
    segs, pos = [], 0
    for n in sizes:
        col = []
        for i in range(x.shape[0]):
            if offset:
                big = torch.empty(n + offset, dtype=x.dtype, device=DEV)
                big[offset:].copy_(xd[i, pos:pos + n])
                col.append(big[offset:])
            else:
                col.append(xd[i, pos:pos + n].clone())
        segs.append(col)
        pos += n
    return segs


def ref_stats(x, out):
    """float64 numpy over the host copies: x [k, n], out [n] (the RETURNED out)."""
    xd = x.double().numpy()
    od = out.double().cpu().numpy()
    return ((xd - od[None, :]) ** 2).sum(axis=1), (xd ** 2).sum(axis=1)


def check_stats(stats, x, out, what):
    assert stats.dtype == torch.float64 and tuple(stats.shape) == (2, x.shape[0])
    got = stats.cpu().numpy()
    d2, ss = ref_stats(x, out)
    for name, g_, r in (("d2", got[0], d2), ("ss", got[1], ss)):
        assert np.all(np.isfinite(g_)), (what, name)
        err = np.abs(g_ - r) / np.where(r > 0, r, 1.0)
        print(f"{what} {name}: max rel err {err.max():.3e}")
        assert np.all(g_[r == 0] == 0.0), (what, name)
        assert err.max() <= TOL, (what, name, float(err.max()))


def run_flat(eng, x, sizes, offset, coef, what, outs=None):
    from fedml_amd.engine import MUL_W
    segs = segments(x, sizes, offset)
    outs, stats = eng.weighted_sum_sqdist(segs, coef, outs=outs)
    exp = eng.weighted_sum_multi(segs, MUL_W, coef)
    torch.cuda.synchronize()
    for s, (a, b) in enumerate(zip(outs, exp)):
        assert same_bits(a, b), (what, "segment", s)
    out = torch.cat([o.reshape(-1) for o in outs])
    check_stats(stats, x, out, what)
    return out, stats


def _flat_cases(eng, k, dt, seed):
    g = torch.Generator().manual_seed(seed)
    for make in (normal_data, cluster_data):
        for offset in (0, 1):
            x = make(g, k, sum(SEGS), dt)
            run_flat(eng, x, SEGS, offset, coefs(g, k), f"{make.__name__} k={k} {dt} segs offset={offset}")
        x = make(g, k, SINGLE, dt)
        run_flat(eng, x, [SINGLE], 0, coefs(g, k), f"{make.__name__} k={k} {dt} single")


@pytest.mark.parametrize("k", F32_K)
def test_fused_pass_f32(eng, k):
    _flat_cases(eng, k, torch.float32, 100 + k)


@pytest.mark.parametrize("k", OTHER_K)
@pytest.mark.parametrize("dt", OTHER_DT, ids=str)
def test_fused_pass_dtypes(eng, dt, k):
    _flat_cases(eng, k, dt, 200 + k)


MIXED = [0, 5, 0, 4097]


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=str)
def test_empty_segments_among_full_ones(eng, dt, offset):
    """Empty segments before and between non-empty ones: the host path leaves them out of the
    segment table, so the others' pointer-table base and first workgroup must count the kept segments
    only -- here through the entry that appends its coefficients to the same staging slot.  The
    outputs are views of one buffer of sentinels (each at a 16-byte boundary plus ``offset``
    elements): the empty ones, and every element around the others, stay untouched."""
    k = 3
    g = torch.Generator().manual_seed(400 + offset)
    x = normal_data(g, k, sum(MIXED), dt)
    per16 = 16 // x.element_size()
    starts, pos = [], per16
    for n in MIXED:
        starts.append(pos + offset)
        pos += -(-(n + offset) // per16) * per16 + per16
    guard = torch.full((pos,), 7.0, dtype=dt, device=DEV)
    outs = [guard[s:s + n] for s, n in zip(starts, MIXED)]
    out, _ = run_flat(eng, x, MIXED, offset, coefs(g, k), f"mixed k={k} {dt} offset={offset}", outs=outs)
    keep = torch.ones(pos, dtype=torch.bool)
    for s, n in zip(starts, MIXED):
        keep[s:s + n] = False
    got = guard.cpu()
    assert bool((got[keep] == 7.0).all())
    assert same_bits(got[~keep], out)  # the results are in the given outputs


def tiled_buf(g, make, k, cap, n, dt):
    """A tile-interleaved group [tiles, cap, E] with random content in every row and tile, whose rows
    ``rows`` (non-contiguous, not in order) carry the k clients' n elements."""
    E = N.TILE_BYTES // torch.empty((), dtype=dt).element_size()
    nt = -(-n // E)
    x = make(g, k, nt * E, dt)
    buf = torch.randn(nt, cap, E, generator=g).to(dt)
    rows = torch.randperm(cap, generator=g)[:k].tolist()
    for i, r in enumerate(rows):
        buf[:, r, :] = x[i].view(nt, E)
    return buf.to(DEV), rows, x[:, :n], E


@pytest.mark.parametrize("tiles", [3, 9], ids=["3E+17", "9E+17"])
@pytest.mark.parametrize("dt,k", [(torch.float32, 3), (torch.float32, 32), (torch.float32, 129),
                                  (torch.bfloat16, 3), (torch.bfloat16, 40), (torch.float16, 40),
                                  (torch.float64, 3), (torch.float64, 40)], ids=str)
def test_tiled_equals_flat(eng, dt, k, tiles):
    """Arena of capacity K + 3, non-contiguous rows, n = 3 E + 17 (below one chunk: element loads
    over tiles) and 9 E + 17 (two whole chunks of 16-byte loads and a ragged one)."""
    g = torch.Generator().manual_seed(300 + k + tiles)
    for make in (normal_data, cluster_data):
        E = N.TILE_BYTES // torch.empty((), dtype=dt).element_size()
        n = tiles * E + 17
        buf, rows, x, _ = tiled_buf(g, make, k, k + 3, n, dt)
        coef = coefs(g, k)
        out_t, stats_t = eng.weighted_sum_sqdist_tiled(buf, rows, coef, n=n)
        out_f, stats_f = run_flat(eng, x, [n], 0, coef, f"flat {make.__name__} k={k} {dt} n={n}")
        torch.cuda.synchronize()
        assert out_t.shape == (n,) and same_bits(out_t, out_f)
        check_stats(stats_t, x, out_t, f"tiled {make.__name__} k={k} {dt} n={n}")


def test_single_client_distance_is_exactly_zero(eng):
    g = torch.Generator().manual_seed(5)
    for dt in (torch.float32, torch.bfloat16, torch.float16, torch.float64):
        x = normal_data(g, 1, SINGLE, dt)
        segs = segments(x, [SINGLE], 0)
        outs, stats = eng.weighted_sum_sqdist(segs, [1.0])
        assert same_bits(outs[0], segs[0][0])
        s = stats.cpu()
        assert s[0, 0].item() == 0.0 and math.copysign(1.0, s[0, 0].item()) == 1.0
        check_stats(stats, x, outs[0], f"k=1 {dt}")


def test_same_call_gives_the_same_bits(eng):
    g = torch.Generator().manual_seed(6)
    k = 33
    x = normal_data(g, k, sum(SEGS) + SINGLE, torch.float32)
    segs = segments(x, SEGS + [SINGLE], 0)
    coef = coefs(g, k)
    runs = [eng.weighted_sum_sqdist(segs, coef) for _ in range(3)]
    torch.cuda.synchronize()
    for outs, stats in runs[1:]:
        assert torch.equal(stats.view(torch.int64), runs[0][1].view(torch.int64))
        assert all(same_bits(a, b) for a, b in zip(outs, runs[0][0]))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float64], ids=str)
def test_special_values(eng, dt):
    from fedml_amd.engine import MUL_W
    g = torch.Generator().manual_seed(7)
    k = 9
    x = normal_data(g, k, sum(SEGS), dt)
    x[2, 300] = float("nan")
    x[6, 5000] = float("inf")
    segs = segments(x, SEGS, 0)
    coef = coefs(g, k)
    outs, stats = eng.weighted_sum_sqdist(segs, coef)
    exp = eng.weighted_sum_multi(segs, MUL_W, coef)
    torch.cuda.synchronize()
    out, ref = torch.cat(outs).cpu(), torch.cat(exp).cpu()
    assert torch.equal(out.isnan(), ref.isnan()) and bool(out[300].isnan()) and bool(out[5000].isinf())
    assert same_bits(out, ref)
    s = stats.cpu().numpy()
    assert [i for i in range(k) if not np.isfinite(s[1, i])] == [2, 6]
    assert not np.isfinite(s[0, 2]) and not np.isfinite(s[0, 6])
    _, ss = ref_stats(x, out)
    ok = [i for i in range(k) if i not in (2, 6)]
    assert np.max(np.abs(s[1, ok] - ss[ok]) / ss[ok]) <= TOL


# ----------------------------------------------------------------------------- the defense, replayed
def _model_dicts(g, k, n1=3001, n2=517, n3=4099, ints=True, where="cuda"):
    ds = []
    for i in range(k):
        d = OrderedDict()
        d["a.weight"] = (0.5 * torch.randn(n1, generator=g) + (8.0 if i % 5 == 3 else 0.0)).view(-1, 1)
        d["b.emb"] = (torch.randn(n2, generator=g) + (4.0 if i % 5 == 3 else 0.0)).to(torch.bfloat16)
        if ints:
            d["bn.num_batches_tracked"] = torch.tensor(100 + 7 * i, dtype=torch.int64)
        d["c.weight"] = torch.randn(n3, generator=g)
        ds.append(OrderedDict((key, v.to(DEV) if where == "cuda" else v) for key, v in d.items()))
    return ds


def _cfg(**kw):
    return types.SimpleNamespace(federated_optimizer="FedAvg", **kw)


def _groups(ds):
    groups = OrderedDict()
    for key, v in ds[0].items():
        if v.dtype.is_floating_point:
            groups.setdefault(v.dtype, []).append(key)
    return groups


def _wsum(eng, ds, coef):
    """z = the MUL_W weighted sum of every float key, per dtype group as the defense groups them."""
    from fedml_amd.engine import MUL_W
    z = {}
    for dt, keys in _groups(ds).items():
        outs = eng.weighted_sum_multi([[d[key].reshape(-1) for d in ds] for key in keys], MUL_W, coef)
        z.update(zip(keys, outs))
    return z


def _dist2(ds, z):
    """float64 numpy: every client's squared distance to z over all float keys."""
    d2 = np.zeros(len(ds))
    for key, zk in z.items():
        zd = zk.double().cpu().numpy().reshape(-1)
        for i, d in enumerate(ds):
            d2[i] += ((d[key].double().cpu().numpy().reshape(-1) - zd) ** 2).sum()
    return d2


@pytest.mark.parametrize("k", [10, 33, 128])
def test_defense_replay(eng, k):
    from fedml_amd.core.security.defense.geometric_median_defense import GeometricMedianDefense
    from fedml_amd.ml.aggregator.agg_operator import FedMLAggOperator
    g = torch.Generator().manual_seed(400 + k)
    ds = _model_dicts(g, k)
    counts = [int(v) for v in torch.randint(20, 600, (k,), generator=g)]
    raw = list(zip(counts, ds))
    d = GeometricMedianDefense(_cfg(geomed_iters=3))
    out = d.defend_on_aggregation(raw, base_aggregation_func=FedMLAggOperator.agg)
    info = d.last_info
    alpha = [float(c) for c in counts]
    assert info["dropped"] == [] and d.get_malicious_client_idxs() == []
    assert len(info["coef_trace"]) == len(info["d2_trace"]) == len(info["objective_trace"]) == 4
    assert info["coef_trace"][0] == [c / sum(counts) for c in counts]
    z = None
    for t in range(4):
        if t:
            assert info["coef_trace"][t] == weiszfeld_coef(alpha, info["d2_trace"][t - 1], 1e-6)
        z = _wsum(eng, ds, info["coef_trace"][t])
        ref = _dist2(ds, z)
        got = np.array(info["d2_trace"][t])
        err = np.abs(got - ref) / ref
        print(f"k={k} pass {t}: d2 max rel err {err.max():.3e}")
        assert err.max() <= TOL
        assert info["objective_trace"][t] == sum(a * math.sqrt(v) for a, v in zip(alpha, info["d2_trace"][t]))
    assert info["objective_trace"][3] < info["objective_trace"][0]
    assert list(out) == list(ds[0])
    base = FedMLAggOperator.agg(_cfg(), raw)
    for key, v in out.items():
        assert v.shape == ds[0][key].shape and v.device == ds[0][key].device
        if ds[0][key].dtype == torch.int64:
            assert v.dtype == base[key].dtype and torch.equal(v.cpu(), base[key].cpu())
        else:
            assert same_bits(v.reshape(-1), z[key].reshape(-1)), key
    # no iteration: the FedAvg result, bit for bit
    d0 = GeometricMedianDefense(_cfg(geomed_iters=0))
    out0 = d0.defend_on_aggregation(raw, base_aggregation_func=FedMLAggOperator.agg)
    assert len(d0.last_info["coef_trace"]) == 1
    for key in out0:
        assert same_bits(out0[key], base[key]), key
    with pytest.raises(TypeError):  # an int64 key and nothing to aggregate it with
        d.defend_on_aggregation(raw)


# ----------------------------------------------------------------------------- against float64
def _walk(x, alpha, iters, nu, f32):
    """The defense's algorithm on the host.  f32: the contract's arithmetic -- float32 ordered sum
    (coef cast to float32, product and sum each rounded once), exact float64 distances; else float64."""
    xd = x.astype(np.float64)
    z = [None]

    def step(coef, clients):
        if f32:
            acc = x[0] * np.float32(coef[0])
            for i in range(1, len(coef)):
                acc = acc + x[i] * np.float32(coef[i])
        else:
            acc = (np.array(coef)[:, None] * xd).sum(axis=0)
        z[0] = acc
        d = xd - acc.astype(np.float64)[None, :]
        return (d * d).sum(axis=1).tolist(), (xd * xd).sum(axis=1).tolist()

    weiszfeld_driver(alpha, iters, nu, step)
    return z[0].astype(np.float64)


@pytest.mark.parametrize("k,n", [(10, 3001), (33, 5003), (128, 2049)])
def test_against_the_float64_algorithm(k, n):
    from fedml_amd.core.security.defense.geometric_median_defense import GeometricMedianDefense
    g = torch.Generator().manual_seed(500 + k)
    mu = torch.randn(n, generator=g)
    bad = int(0.3 * k)
    x = torch.empty(k, n)
    for i in range(k):
        x[i] = mu + 20.0 + 5.0 * torch.randn(n, generator=g) if i < bad else mu + 0.1 * torch.randn(n, generator=g)
    x = x[torch.randperm(k, generator=g)]
    # random counts within 10 % of each other: the weighted geometric median sees the WEIGHTED share of
    # the bad clients, and the bound below is stated for a 30 % share.  Counts over a wide range move
    # it (20 .. 600 at K = 33 gave 38 %), where three iterations of the float64 reference itself stop
    # at |z - mu| = 2.8 against 10.1 for the mean -- a property of the data, not of the kernel.
    counts = [float(v) for v in torch.randint(90, 111, (k,), generator=g)]
    xn, mun = x.numpy(), mu.double().numpy()
    z32 = _walk(xn, counts, 3, 1e-6, True)
    z64 = _walk(xn, counts, 3, 1e-6, False)
    mean = _walk(xn, counts, 0, 1e-6, False)
    G = np.abs(z32 - z64).max()
    d = GeometricMedianDefense(_cfg(geomed_iters=3))
    out = d.defend_on_aggregation([(c, OrderedDict(w=x[i].to(DEV))) for i, c in enumerate(counts)])
    zg = out["w"].double().cpu().numpy()
    dev, to_mu, mean_mu = np.abs(zg - z64).max(), np.abs(zg - mun).max(), np.abs(mean - mun).max()
    print(f"k={k} n={n}: G {G:.3e}, |z_gpu - z64| {dev:.3e} ({dev / G:.2f} G), |z_gpu - mu| {to_mu:.3f}, "
          f"|mean - mu| {mean_mu:.3f}")
    assert G > 0
    assert np.abs(z64 - mun).max() < mean_mu / 8  # the float64 reference clears the bound below twice over
    # the device differs from z32 only through the <= 1e-6 error of d2
    assert dev <= 4 * G
    assert to_mu < mean_mu / 4


# ----------------------------------------------------------------------------- every route, same bits
def _reset_defender():
    from fedml_amd.core.security.fedml_defender import FedMLDefender
    FedMLDefender.get_instance().init(types.SimpleNamespace())


def _through_server_aggregator(raw):
    from fedml_amd.core.security.fedml_defender import FedMLDefender
    from fedml_amd.ml.aggregator.default_aggregator import DefaultServerAggregator
    try:
        agg = DefaultServerAggregator(torch.nn.Linear(5, 2), _cfg(enable_defense=True, defense_type="geometric_median",
                                                                  geomed_iters=3))
        kept, _ = agg.on_before_aggregation(raw)
        assert len(kept) == len(raw) and all(a is b for (_, a), (_, b) in zip(kept, raw))
        out = agg.aggregate(kept)
        return out, FedMLDefender.get_instance().get_malicious_client_idxs()
    finally:
        _reset_defender()


def test_every_route_gives_the_same_bits(eng, monkeypatch):
    from fedml_amd.arena import ClientArena, resident_rows
    from fedml_amd.core.security.defense.geometric_median_defense import GeometricMedianDefense
    g = torch.Generator().manual_seed(8)
    k = 12
    ds = _model_dicts(g, k, ints=False)
    counts = [int(v) for v in torch.randint(20, 600, (k,), generator=g)]
    raw = list(zip(counts, ds))
    d = GeometricMedianDefense(_cfg(geomed_iters=3))
    ref = d.defend_on_aggregation(raw)  # separate tensors
    ref_info = d.last_info
    # the full route
    out, bad = _through_server_aggregator(raw)
    assert bad == [] and all(same_bits(out[key], ref[key]) for key in ref)
    # CPU dicts in, CPU tensors out
    cpu = d.defend_on_aggregation([(c, OrderedDict((key, v.cpu()) for key, v in sd.items())) for c, sd in raw])
    assert all(v.device.type == "cpu" and same_bits(v, ref[key]) for key, v in cpu.items())
    # a tiled arena, rows out of order, driven directly
    ta = ClientArena.for_model(ds[0], k + 2, device=DEV, tiled=True)
    rows = [(5 * i + 3) % (k + 2) for i in range(k)]
    for r, sd in zip(rows, ds):
        ta.write(r, sd)
    info = {}
    out = ta.geometric_median(counts, 3, 1e-6, clients=rows, info=info)
    assert list(out) == list(ref) and all(same_bits(out[key], ref[key]) for key in ref)
    assert info["coef_trace"][0] == ref_info["coef_trace"][0] and len(info["coef_trace"]) == 4
    # a client-major arena: the defense finds the adopted rows
    copies = [OrderedDict((key, v.clone()) for key, v in sd.items()) for sd in ds]
    ca = ClientArena.for_model(copies[0], k, device=DEV)
    for i, sd in enumerate(copies):
        ca.adopt(i, sd)
    assert resident_rows(copies) is not None
    calls = []
    real = ClientArena.geometric_median
    monkeypatch.setattr(ClientArena, "geometric_median",
                        lambda self, *a, **kw: calls.append(a) or real(self, *a, **kw))
    out = d.defend_on_aggregation(list(zip(counts, copies)))
    assert len(calls) == 1
    assert all(same_bits(out[key], ref[key]) for key in ref)


def test_a_nan_client_is_dropped(eng):
    g = torch.Generator().manual_seed(9)
    k = 12
    ds = _model_dicts(g, k, ints=True)
    counts = [int(v) for v in torch.randint(20, 600, (k,), generator=g)]
    clean = [(c, sd) for i, (c, sd) in enumerate(zip(counts, ds)) if i != 4]
    ds[4]["c.weight"][77] = float("nan")
    out, bad = _through_server_aggregator(list(zip(counts, ds)))
    assert bad == [4]
    ref, none = _through_server_aggregator(clean)
    assert none == []
    for key in ref:
        if ref[key].dtype.is_floating_point and ds[0][key].dtype.is_floating_point:
            assert same_bits(out[key], ref[key]), key
    from fedml_amd.core.security.defense.geometric_median_defense import GeometricMedianDefense
    w = torch.ones(100, device=DEV)
    with pytest.raises(ValueError, match="every client"):
        GeometricMedianDefense(_cfg()).defend_on_aggregation([(1, OrderedDict(w=w * float("nan"))),
                                                              (2, OrderedDict(w=w * float("inf")))])


# ----------------------------------------------------------------------------- argument checks
@pytest.mark.parametrize("entry", ["fa_weighted_sum_sqdist", "fa_weighted_sum_sqdist_tiled"])
def test_entry_rejects_bad_arguments(eng, entry):
    L = N.lib()
    K, NUMEL = 3, 8
    tiled = entry.endswith("_tiled")
    xs = [torch.zeros(1024, device=DEV) for _ in range(K)]
    out = torch.full((NUMEL,), 7.0, device=DEV)
    stats = torch.full((2 * K,), 7.0, dtype=torch.float64, device=DEV)
    need = L.fa_weighted_sum_sqdist_scratch_bytes(1, N.i64_array([NUMEL]), K)
    scratch = torch.zeros(need, dtype=torch.uint8, device=DEV)
    good = [x.data_ptr() for x in xs]
    GOOD_COEF = N.f64_array([0.2, 0.3, 0.5])

    def call(dtype=N.F32, numel=NUMEL, k=K, ptrs=good, tile_stride=N.TILE_BYTES, coef=GOOD_COEF, sbytes=need,
             sptr=scratch.data_ptr(), st=stats.data_ptr()):
        args = [eng._ctx, dtype, 1, N.i64_array([numel]), k, N.ptr_array(ptrs)]
        args += [tile_stride] if tiled else []
        args += [coef, N.ptr_array([out.data_ptr()]), st, sptr, sbytes, None]
        return getattr(L, entry)(*args), L.fa_last_error()

    def named(err):
        return err.startswith(entry.encode() + b":")

    rc, err = call(dtype=N.I64)
    assert rc == N.FA_ERR_DTYPE and named(err), err
    rc, err = call(k=0)
    assert rc == N.FA_ERR_INVALID and named(err), err
    rc, err = call(coef=None)
    assert rc == N.FA_ERR_INVALID and b"coef" in err and named(err), err
    rc, err = call(st=None)
    assert rc == N.FA_ERR_INVALID and b"d_stats" in err and named(err), err
    rc, err = call(sbytes=need - 8)
    assert rc == N.FA_ERR_INVALID and b"scratch" in err and named(err), err
    rc, err = call(sptr=None)
    assert rc == N.FA_ERR_INVALID and b"scratch" in err and named(err), err
    rc, err = call(ptrs=[good[0], None, good[2]])
    assert rc == N.FA_ERR_INVALID and b"input NULL" in err and named(err), err
    rc, err = call(numel=-NUMEL)
    assert rc == N.FA_ERR_INVALID and named(err), err
    if tiled:
        for bad in (1000, 0, -4096):
            rc, err = call(tile_stride=bad)
            assert rc == N.FA_ERR_INVALID and b"tile_stride" in err and named(err), err
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((stats == 7.0).all())  # nothing was launched
    rc, err = call()
    assert rc == N.FA_OK, err
    torch.cuda.synchronize()
    assert bool((out == 0.0).all()) and bool((stats == 0.0).all())


def test_engine_argument_checks(eng):
    xs = [torch.zeros(8, device=DEV) for _ in range(3)]
    with pytest.raises(ValueError):
        eng.weighted_sum_sqdist([], [])
    with pytest.raises(ValueError):
        eng.weighted_sum_sqdist([xs], [0.5, 0.5])
    with pytest.raises(ValueError):
        eng.weighted_sum_sqdist([xs], None)
    with pytest.raises(TypeError):
        eng.weighted_sum_sqdist([[x.long() for x in xs]], [0.2, 0.3, 0.5])
    with pytest.raises(ValueError):
        eng.weighted_sum_sqdist([xs, xs[:2]], [0.2, 0.3, 0.5])
    with pytest.raises(ValueError):
        eng.weighted_sum_sqdist([xs], [0.2, 0.3, 0.5], outs=[torch.zeros(7, device=DEV)])
    buf = torch.zeros(2, 4, 1024, device=DEV)
    with pytest.raises(ValueError):
        eng.weighted_sum_sqdist_tiled(buf, [0, 1], [1.0])
    with pytest.raises(IndexError):
        eng.weighted_sum_sqdist_tiled(buf, [0, 4], [0.5, 0.5])
    out, stats = eng.weighted_sum_sqdist_tiled(buf, [0, 1], [0.5, 0.5], n=0)  # nothing to read: sums are 0
    assert out.numel() == 0 and bool((stats == 0.0).all())
