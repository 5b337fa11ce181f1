"""Differential privacy end to end (fedml_amd/core/dp, ServerAggregator, ClientTrainer, ClientArena):
K = 5 small dicts with two float32 keys, a bfloat16 key and an int64 key, one client 40 away from the
global model so that clipping at C = 1 bites.  Everything is compared bit for bit with kernels and
defenses the tree already tests, composed by hand."""
from __future__ import annotations

import os
import sys
import types
from collections import OrderedDict

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_geometric_median import DEV, same_bits  # noqa: E402

from fedml_amd import dp  # noqa: E402
from fedml_amd.arena import sum_stats  # noqa: E402
from fedml_amd.core.alg_frame.client_trainer import ClientTrainer  # noqa: E402
from fedml_amd.core.alg_frame.server_aggregator import ServerAggregator  # noqa: E402
from fedml_amd.core.dp import FedMLDifferentialPrivacy  # noqa: E402

pytestmark = pytest.mark.gpu

K, C, SEED = 5, 1.0, 0x5EEDC0DE12345678
SHAPES = OrderedDict([("a.weight", ((33, 40), torch.float32)), ("a.steps", ((), torch.int64)),
                      ("b.weight", ((2100,), torch.bfloat16)), ("c.bias", ((7,), torch.float32))])
FKEYS = [k for k, (_, dt) in SHAPES.items() if dt.is_floating_point]
COUNTS = [30, 10, 25, 20, 15]


@pytest.fixture(scope="module")
def eng():
    from fedml_amd.engine import get_engine
    return get_engine(0)


@pytest.fixture(autouse=True)
def _reset():
    yield
    from fedml_amd.core.security.fedml_defender import FedMLDefender
    FedMLDifferentialPrivacy.get_instance().init(types.SimpleNamespace())
    FedMLDefender.get_instance().init(types.SimpleNamespace())


class DictAggregator(ServerAggregator):
    def get_model_params(self):
        return self.model

    def set_model_params(self, p):
        self.model = p

    def test(self, test_data, device, args):
        pass


class DictTrainer(ClientTrainer):
    def get_model_params(self):
        return self.model

    def set_model_params(self, p):
        self.model = p

    def train(self, train_data, device, args):
        pass


def _cfg(**kw):
    base = dict(federated_optimizer="FedAvg", enable_dp=True, dp_solution_type="cdp", mechanism_type="gaussian",
                epsilon=1.0, delta=1e-5, dp_seed=SEED)
    base.update(kw)
    return types.SimpleNamespace(**base)


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(2024)
    glob, ds = OrderedDict(), []
    for key, (shape, dt) in SHAPES.items():
        glob[key] = torch.randn(shape, generator=g).to(dt) if dt.is_floating_point else torch.tensor(1000)
    for i in range(K):
        sd = OrderedDict()
        for key, (shape, dt) in SHAPES.items():
            if dt.is_floating_point:
                step = 0.004 * torch.randn(shape, generator=g)
                if i == 3 and key == "a.weight":  # 40 away from the global model
                    step = step + 40.0 / (33 * 40) ** 0.5
                sd[key] = (glob[key].float() + step).to(dt).to(DEV)
            else:
                sd[key] = torch.tensor(100 + 7 * i, device=DEV)
        ds.append(sd)
    return glob, ds


def run_server(glob, raw, **kw):
    agg = DictAggregator(OrderedDict((k, v.clone()) for k, v in glob.items()), _cfg(**kw))
    kept, _ = agg.on_before_aggregation(raw)
    return agg, agg.on_after_aggregation(agg.aggregate(kept))


def by_hand(eng, glob, ds, scale, mech, seed, rnd):
    """The clipped aggregation from engine calls: per dtype group the norms, then the clipped weights,
    then sign_vote_sum at threshold 0 followed by add_noise."""
    groups = OrderedDict()
    for pos, key in enumerate(FKEYS):
        groups.setdefault(SHAPES[key][1], []).append((pos, key))
    segs = {dt: [[sd[k].reshape(-1) for sd in ds] for _, k in items] for dt, items in groups.items()}
    cens = {dt: [glob[k].to(DEV).reshape(-1) for _, k in items] for dt, items in groups.items()}
    d2, _ = sum_stats([eng.centered_sum_sqdist(segs[dt], cens[dt], None)[1] for dt in groups])
    tot = float(sum(COUNTS))
    w = [c / tot for c in COUNTS]
    scales = dp.clip_scales(w, d2, C)
    out = {}
    for dt, items in groups.items():
        y, _ = eng.sign_vote_sum(segs[dt], cens[dt], scales, 0)
        ids = [p for p, _ in items]
        res = eng.add_noise(y, mech, scale, seed, rnd, ids) if scale else y
        for (_, k), o in zip(items, res):
            out[k] = o.view(SHAPES[k][0])
    return out, d2, scales, w


def test_clipped_aggregation(eng, data):
    from fedml_amd.core.security.defense.centered_clipping_defense import CenteredClippingDefense
    from fedml_amd.ml.aggregator.agg_operator import FedMLAggOperator
    glob, ds = data
    raw = list(zip(COUNTS, ds))
    # sensitivity 0: no noise -- one iteration of centered clipping from the global model
    cc = CenteredClippingDefense(types.SimpleNamespace(federated_optimizer="FedAvg", cclip_tau=C, cclip_iters=1))
    ref = cc.defend_on_aggregation(raw, FedMLAggOperator.agg, glob)
    assert cc.last_info["clipped"] == [3]  # the far client, and only it
    _, out = run_server(glob, raw, clipping_norm=C, sensitivity=0.0)
    assert list(out) == list(SHAPES) and all(same_bits(out[k], ref[k]) for k in SHAPES)
    assert all(out[k].device.type == "cuda" for k in SHAPES)
    # epsilon 1, the default sensitivity C max w: the engine calls composed by hand, same seed and round
    hand0, d2, scales, w = by_hand(eng, glob, ds, 0.0, "gaussian", SEED, 1)
    assert all(same_bits(hand0[k], ref[k]) for k in FKEYS)
    assert 39.0 < d2[3] ** 0.5 < 41.0 and scales[3] < w[3] / 30 and scales[:3] == w[:3]
    for mech in ("gaussian", "laplace"):
        scale = dp.noise_scale(mech, 1.0, 1e-5, C * max(w))
        agg, out1 = run_server(glob, raw, clipping_norm=C, mechanism_type=mech)
        hand1, *_ = by_hand(eng, glob, ds, scale, mech, SEED, 1)
        assert all(same_bits(out1[k], hand1[k]) for k in FKEYS)
        assert not any(same_bits(out1[k], ref[k]) for k in FKEYS)
        assert same_bits(out1["a.steps"], ref["a.steps"])  # the int64 key: the base aggregation's, no noise
        # a second round: the same model, other noise; on_after_aggregation added none of its own
        out2 = agg.on_after_aggregation(agg.aggregate(raw))
        hand2, *_ = by_hand(eng, glob, ds, scale, mech, SEED, 2)
        assert all(same_bits(out2[k], hand2[k]) for k in FKEYS)
        assert not any(same_bits(out2[k], out1[k]) for k in FKEYS)
        # the same seed in a fresh singleton reproduces round 1; another seed does not
        _, again = run_server(glob, raw, clipping_norm=C, mechanism_type=mech)
        assert all(same_bits(again[k], out1[k]) for k in SHAPES)
        _, other = run_server(glob, raw, clipping_norm=C, mechanism_type=mech, dp_seed=SEED + 1)
        assert not any(same_bits(other[k], out1[k]) for k in FKEYS)
    # CPU dicts in, CPU tensors out
    cpu_raw = [(c, OrderedDict((k, v.cpu()) for k, v in sd.items())) for c, sd in raw]
    _, cpu = run_server(glob, cpu_raw, clipping_norm=C, mechanism_type="laplace")
    assert all(v.device.type == "cpu" for v in cpu.values())
    assert all(same_bits(cpu[k], out1[k]) for k in SHAPES)
    with pytest.raises(RuntimeError, match="aggregate"):
        agg.on_after_aggregation(out1)  # a clipped config never adds noise outside aggregate()


def test_resident_and_tiled_arenas(eng, data, monkeypatch):
    from fedml_amd.arena import ClientArena, resident_rows
    glob, ds = data
    fds = [OrderedDict((k, sd[k]) for k in FKEYS) for sd in ds]
    fglob = OrderedDict((k, glob[k]) for k in FKEYS)
    w = [c / float(sum(COUNTS)) for c in COUNTS]
    scale = dp.noise_scale("gaussian", 1.0, 1e-5, C * max(w))
    _, flat = run_server(fglob, list(zip(COUNTS, fds)), clipping_norm=C)
    # rows adopted by a client-major arena are found and take ClientArena.dp_aggregate: the same bits
    copies = [OrderedDict((k, v.clone()) for k, v in sd.items()) for sd in fds]
    ca = ClientArena.for_model(copies[0], K, device=DEV)
    for i, sd in enumerate(copies):
        ca.adopt(i, sd)
    assert resident_rows(copies) is not None
    calls = []
    real = ClientArena.dp_aggregate
    monkeypatch.setattr(ClientArena, "dp_aggregate", lambda self, *a, **kw: calls.append(a) or real(self, *a, **kw))
    _, res = run_server(fglob, list(zip(COUNTS, copies)), clipping_norm=C)
    assert len(calls) == 1 and list(res) == FKEYS and all(same_bits(res[k], flat[k]) for k in FKEYS)
    monkeypatch.undo()
    # a tiled arena takes the tiled entry, one segment per dtype group: the flat entry over the
    # packed rows with the group's id gives the same bits
    ta = ClientArena.for_model(fds[0], K + 2, device=DEV, tiled=True)
    rows = [(3 * i + 1) % (K + 2) for i in range(K)]
    for r, sd in zip(rows, fds):
        ta.write(r, sd)
    packed = {dt: torch.zeros(n, dtype=dt, device=DEV) for dt, n in ta.layout.group_numel.items()}
    for k in FKEYS:
        dt, off, _, n = ta.layout.where[k]
        packed[dt][off:off + n].copy_(glob[k].reshape(-1))
    info = {}
    out = ta.dp_aggregate(COUNTS, C, scale, "gaussian", SEED, 1, center=packed, clients=rows, info=info)
    assert all(same_bits(t, glob[k].to(DEV)) for k, t in ta.layout.carve(packed).items())  # the center is only read
    pa = ClientArena.for_model(fds[0], K, device=DEV)
    for i, sd in enumerate(fds):
        pa.write(i, sd)
    for g, (dt, buf) in enumerate(pa.bufs.items()):
        y, = eng.centered_sum_noise([[buf[i] for i in range(K)]], [packed[dt]], info["scales"], "gaussian", scale, SEED,
                                    1, [ClientArena.TILED_SEG_BASE + g])
        for k in FKEYS:
            kdt, off, shape, n = ta.layout.where[k]
            if kdt == dt:
                assert same_bits(out[k], y[off:off + n].view(shape)), k
    assert info["scales"][3] < w[3] / 30


def test_noise_after_aggregation(eng, data):
    from fedml_amd.ml.aggregator.agg_operator import FedMLAggOperator
    from fedml_amd.ml.aggregator.quantized import quantize_state_dict
    glob, ds = data
    raw = list(zip(COUNTS, ds))
    scale = dp.noise_scale("laplace", 2.0, None, 0.5)

    def noised(plain):
        out = OrderedDict(plain)
        for pos, k in enumerate(FKEYS):
            out[k] = eng.add_noise([plain[k].to(DEV).reshape(-1)], "laplace", scale, SEED, 1, [pos])[0].view(plain[k].shape)
        return out

    kw = dict(mechanism_type="laplace", epsilon=2.0, sensitivity=0.5)
    # plain FedAvg, a defense's result, a q8 sum: add_noise of the undefended / unnoised result
    plain = FedMLAggOperator.agg(_cfg(enable_dp=False), raw)
    _, out = run_server(glob, raw, **kw)
    exp = noised(plain)
    assert list(out) == list(SHAPES) and all(same_bits(out[k], exp[k]) for k in SHAPES)
    assert not any(same_bits(out[k], plain[k]) for k in FKEYS)
    fraw = [(c, OrderedDict((k, sd[k]) for k in FKEYS if SHAPES[k][1] == torch.float32)) for c, sd in raw]
    f32 = [k for k in FKEYS if SHAPES[k][1] == torch.float32]
    agg = DictAggregator(OrderedDict((k, glob[k]) for k in f32), _cfg(enable_defense=True, defense_type="wise_median", **kw))
    med = agg.aggregate(fraw)
    got = agg.on_after_aggregation(OrderedDict(med))
    for pos, k in enumerate(f32):
        e = eng.add_noise([med[k].reshape(-1)], "laplace", scale, SEED, 1, [pos])[0].view(med[k].shape)
        assert same_bits(got[k], e) and not same_bits(got[k], med[k])
    qraw = [(c, quantize_state_dict(OrderedDict((k, sd[k]) for k in f32))) for c, sd in raw]
    qsum = FedMLAggOperator.agg(_cfg(enable_dp=False), qraw)
    _, qout = run_server(OrderedDict((k, glob[k]) for k in f32), qraw, **kw)
    for pos, k in enumerate(f32):
        e = eng.add_noise([qsum[k].reshape(-1)], "laplace", scale, SEED, 1, [pos])[0].view(qsum[k].shape)
        assert same_bits(qout[k], e)


def test_local_noise_through_a_trainer(eng, data):
    glob, ds = data
    scale = dp.noise_scale("gaussian", 1.0, 1e-5, 0.01)
    kw = dict(dp_solution_type="ldp", sensitivity=0.01)
    outs = {}
    for cid in (0, 3):
        tr = DictTrainer(OrderedDict(ds[cid]), _cfg(**kw))
        tr.set_id(cid)
        tr.on_after_local_training(None, DEV, tr.args)
        got = tr.get_model_params()
        assert list(got) == list(SHAPES) and got["a.steps"] is ds[cid]["a.steps"]
        for pos, k in enumerate(FKEYS):
            x = ds[cid][k].reshape(-1)
            e, = eng.add_noise([x], "gaussian", scale, dp.client_seed(SEED, cid), 1, [pos])
            t = torch.empty_like(x)
            eng.add_noise(None, "gaussian", scale, dp.client_seed(SEED, cid), 1, [pos], outs=[t])
            assert same_bits(got[k].reshape(-1), e) and same_bits(e, x + t) and not same_bits(e, x)
        outs[cid] = got
        tr.on_after_local_training(None, DEV, tr.args)  # round 2: other noise on top
        assert not same_bits(tr.get_model_params()["c.bias"] - got["c.bias"], got["c.bias"] - ds[cid]["c.bias"])
    d0 = outs[0]["c.bias"] - ds[0]["c.bias"]
    d3 = outs[3]["c.bias"] - ds[3]["c.bias"]
    assert not torch.equal(d0, d3)  # every client its own stream
    # off: the hook is the identity
    tr = DictTrainer(OrderedDict(ds[0]), types.SimpleNamespace())
    tr.on_after_local_training(None, DEV, tr.args)
    assert all(tr.get_model_params()[k] is ds[0][k] for k in SHAPES)
