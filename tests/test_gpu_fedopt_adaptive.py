"""The adaptive FedOpt server steps on the device (fa_fedavg_adaptive: FedAdam, FedYogi, FedAdagrad,
torch.optim.Adam / Adagrad): p, m and v bit for bit equal to the per-op restatement of the contract in
include/fedagg.h over consecutive rounds in place, hand-built columns, the two identities, the tiled
entry, torch.optim on the CPU as the reference, FedOptAggregator with each of the five names, and
the raw entries' argument checks in their documented order.

A workgroup owns one 4-KiB slot per client, E = 1024 float32 elements, and loads clients in groups of
8.  SEG_LISTS cover one whole aligned slot, two slots and a ragged remainder, a segment below one
slot and empty segments between full ones, each at element offsets 0 and 1 (offset 1: unaligned,
every slot on the element path); LAYOUTS adds the state alone, the parameter alone and the clients
alone unaligned.  KS cover one client, the group-of-8 boundary and the clamped last group."""
from __future__ import annotations

import copy
import os
import sys
import types
from collections import OrderedDict

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from adaptcases import f32, restate, weighted_avg  # noqa: E402,F401
from test_gpu_geometric_median import DEV, coefs, normal_data, same_bits, segments, tiled_buf  # noqa: E402

from fedml_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu

E = N.TILE_BYTES // 4
ADAM, YOGI, ADAGRAD = N.ADAPT_ADAM, N.ADAPT_YOGI, N.ADAPT_ADAGRAD
RULES = {"adam": ADAM, "yogi": YOGI, "adagrad": ADAGRAD}
KS = [1, 7, 8, 9, 17]
SEG_LISTS = [[E], [E, 2 * E + 5], [7], [0, 3, 0]]
# (sizes, element offset of the clients, the parameter, m, v)
LAYOUTS = [(s, o, o, o, o) for s in SEG_LISTS for o in (0, 1)] + \
          [([E, 2 * E + 5],) + offs for offs in ((0, 0, 1, 1), (0, 0, 1, 0), (0, 0, 0, 1), (0, 1, 0, 0), (1, 0, 0, 0))]
GUARD = 7.0


@pytest.fixture(scope="module")
def eng():
    from fedml_amd.engine import get_engine
    return get_engine(0)


def place(flat, sizes, offset):
    """A host vector as guarded device segments: segment s is a view ``offset`` elements into its own
    allocation of GUARD values, with 8 more behind it.  Returns (views, allocations)."""
    views, bigs, pos = [], [], 0
    for n in sizes:
        big = torch.full((offset + n + 8,), GUARD, device=DEV)
        big[offset:offset + n].copy_(flat[pos:pos + n])
        views.append(big[offset:offset + n])
        bigs.append(big)
        pos += n
    return views, bigs


def gather(views):
    return torch.cat([t.reshape(-1) for t in views]).cpu()


def guards_intact(bigs, sizes, offset):
    return all(bool((b[:offset] == GUARD).all()) and bool((b[offset + n:] == GUARD).all()) for b, n in zip(bigs, sizes))


def start_state(g, n, mom):
    """A server state that is not its initial one, so a kernel that did not read it would show."""
    p = torch.randn(n, generator=g)
    m = 0.1 * torch.randn(n, generator=g) if mom else None
    v = 0.05 + 0.1 * torch.rand(n, generator=g)
    return p, m, v


CONFIGS = [(mom, wd, bias) for mom in (True, False) for wd in (0.0, 1e-3) for bias in (True, False)]


# ----------------------------------------------------------------------------- bit-exactness
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("rule", list(RULES), ids=str)
def test_three_rounds_in_place_equal_the_restatement(eng, rule, k):
    g = torch.Generator().manual_seed(3100 + 10 * RULES[rule] + k)
    lr, beta2, eps = 0.05, 0.99, 1e-3
    for sizes, oc, op, om, ov in LAYOUTS:
        n = sum(sizes)
        xs = [normal_data(g, k, n, torch.float32) for _ in range(3)]
        segs = [segments(x, sizes, oc) for x in xs]  # shared by every configuration: the inputs are only read
        coef = coefs(g, k)
        for mom, wd, bias in CONFIGS:
            what = f"{rule} k={k} sizes={sizes} offsets={(oc, op, om, ov)} mom={mom} wd={wd} bias={bias}"
            beta1 = 0.9 if mom else 0.0
            p, m, v = start_state(g, n, mom)
            dp, bp = place(p, sizes, op)
            dv, bv = place(v, sizes, ov)
            dm, bm = place(m, sizes, om) if mom else (None, [])
            for r in range(3):
                eng.fedavg_adaptive(segs[r], coef, dp, dm, dv, RULES[rule], lr, beta1, beta2, eps, weight_decay=wd,
                                    bias_correction=bias, step=r + 1)
                p, m, v = restate(xs[r], coef, p, m, v, RULES[rule], lr, beta1, beta2, eps, wd, bias, r + 1)
                assert same_bits(gather(dp), p), (what, "p", r)
                assert same_bits(gather(dv), v), (what, "v", r)
                assert not mom or same_bits(gather(dm), m), (what, "m", r)
            assert guards_intact(bp, sizes, op) and guards_intact(bv, sizes, ov) and guards_intact(bm, sizes, om), what
        for r in range(3):
            back = torch.stack([torch.cat([col[i] for col in segs[r]]) for i in range(k)]).cpu()
            assert same_bits(back, xs[r])  # the inputs are only read


# ----------------------------------------------------------------------------- hand-built columns
COLUMNS = [  # name, p, x, v: K = 1 with coefficient 1, so g = p - x
    ("yogi v == g2", 1.0, 0.5, 0.25),
    ("yogi v < g2", 1.0, 0.5, 0.125),
    ("yogi v > g2", 1.0, 0.5, 0.5),
    ("v = 0, g = 0", 1.0, 1.0, 0.0),
    ("client NaN", 1.0, float("nan"), 0.25),
    ("client +Inf", 1.0, float("inf"), 0.25),
    ("client -Inf", 1.0, float("-inf"), 0.25),
    ("ordinary", -2.0, 0.75, 0.0625),
]


@pytest.mark.parametrize("eps", [1e-3, 0.0])
@pytest.mark.parametrize("mom", [True, False], ids=["momentum", "no momentum"])
@pytest.mark.parametrize("rule", list(RULES), ids=str)
def test_hand_built_columns(eng, rule, mom, eps):
    names = [c[0] for c in COLUMNS]
    p0 = torch.tensor([c[1] for c in COLUMNS])
    x = torch.tensor([[c[2] for c in COLUMNS]])
    v0 = torch.tensor([c[3] for c in COLUMNS])
    m0 = torch.zeros(len(COLUMNS)) if mom else None
    beta1, beta2, lr = (0.9 if mom else 0.0), 0.99, 0.1
    p, m, v = restate(x, [1.0], p0, m0, v0, RULES[rule], lr, beta1, beta2, eps)
    dp, dv = p0.to(DEV), v0.to(DEV)
    dm = m0.to(DEV) if mom else None
    eng.fedavg_adaptive([[x[0].to(DEV)]], [1.0], [dp], None if dm is None else [dm], [dv], RULES[rule], lr, beta1,
                        beta2, eps)
    for name, got, ref in (("p", dp, p), ("v", dv, v)) + ((("m", dm, m),) if mom else ()):
        got = got.cpu()
        isn = ref.isnan()
        assert torch.equal(got.isnan(), isn), (name, got, ref)  # NaN-ness is compared, not the bits
        bad = [names[i] for i in range(len(names)) if not isn[i] and not same_bits(got[i:i + 1], ref[i:i + 1])]
        assert not bad, (name, bad)
    col = {name: i for i, name in enumerate(names)}
    # the restatement itself on the columns it was built for
    if rule == "yogi":
        assert float(v[col["yogi v == g2"]]) == 0.25  # sign 0: v unchanged
        assert float(v[col["yogi v < g2"]]) > 0.125 and float(v[col["yogi v > g2"]]) < 0.5
        assert float(dv[col["yogi v == g2"]]) == 0.25
    z = col["v = 0, g = 0"]
    if eps == 0.0:
        assert bool(p[z].isnan()) and bool(dp[z].isnan())  # 0 / 0
    else:
        assert float(p[z]) == 1.0 and float(dp[z]) == 1.0 and float(dv[z]) == 0.0  # 0 / eps
    assert bool(p[col["client NaN"]].isnan()) and bool(p[col["client +Inf"]].isnan())  # Inf / Inf
    assert not bool(p[col["ordinary"]].isnan())


# ----------------------------------------------------------------------------- identities
def test_adagrad_without_momentum_takes_no_first_moment(eng):
    """beta1 == 0: d_m is NULL (the engine passes None through) and is never dereferenced."""
    g = torch.Generator().manual_seed(3200)
    k, sizes = 9, [E, 2 * E + 5]
    n = sum(sizes)
    x = normal_data(g, k, n, torch.float32)
    coef = coefs(g, k)
    p, _, v = start_state(g, n, False)
    (dp, _), (dv, _) = place(p, sizes, 0), place(v, sizes, 0)
    L = N.lib()
    segs = segments(x, sizes, 0)
    rc = L.fa_fedavg_adaptive(eng._ctx, len(sizes), N.i64_array(sizes), k,
                              N.ptr_array([t.data_ptr() for col in segs for t in col]),
                              N.f64_array(coef), N.ptr_array([t.data_ptr() for t in dp]), None,
                              N.ptr_array([t.data_ptr() for t in dv]), ADAGRAD, 0.05, 0.0, 0.0, 1e-10, 0.0, 0, 1, None)
    assert rc == N.FA_OK, L.fa_last_error()
    torch.cuda.synchronize()
    p, _, v = restate(x, coef, p, None, v, ADAGRAD, 0.05, 0.0, 0.0, 1e-10)
    assert same_bits(gather(dp), p) and same_bits(gather(dv), v)


@pytest.mark.parametrize("rule", list(RULES), ids=str)
def test_lr_zero_keeps_the_parameter_and_advances_the_state(eng, rule):
    g = torch.Generator().manual_seed(3300 + RULES[rule])
    k, n = 7, 2 * E + 5
    x = normal_data(g, k, n, torch.float32)
    coef = coefs(g, k)
    p0, m0, v0 = start_state(g, n, True)
    dp, dm, dv = p0.to(DEV), m0.to(DEV), v0.to(DEV)
    eng.fedavg_adaptive(segments(x, [n], 0), coef, [dp], [dm], [dv], RULES[rule], 0.0, 0.9, 0.99, 1e-3)
    p, m, v = restate(x, coef, p0, m0, v0, RULES[rule], 0.0, 0.9, 0.99, 1e-3)
    assert same_bits(dp.cpu(), p0)
    assert same_bits(dm.cpu(), m) and same_bits(dv.cpu(), v)
    assert not torch.equal(m, m0) and not torch.equal(v, v0)


# ----------------------------------------------------------------------------- the tiled entry
@pytest.mark.parametrize("k", [7, 9])
@pytest.mark.parametrize("rule,mom", [("adam", True), ("yogi", True), ("adagrad", False)], ids=str)
def test_tiled_equals_flat(eng, rule, mom, k):
    from fedml_amd.arena import ClientArena
    g = torch.Generator().manual_seed(3400 + 10 * RULES[rule] + k)
    n = 3 * E + 17  # not a multiple of the tile
    buf, rows, x, _ = tiled_buf(g, normal_data, k, k + 3, n, torch.float32)  # a subset of the rows, out of order
    keep = buf.clone()
    x = x.contiguous()
    coef = coefs(g, k)
    beta1 = 0.9 if mom else 0.0
    args = (RULES[rule], 0.05, beta1, 0.99, 1e-3)
    p0, m0, v0 = start_state(g, n, mom)

    def fresh():
        return p0.to(DEV), (m0.to(DEV) if mom else None), v0.to(DEV)

    def three_rounds(run):
        """The device state after each of three rounds of ``run(p, m, v, step)``."""
        dp, dm, dv = fresh()
        out = []
        for r in range(3):
            run(dp, dm, dv, r + 1)
            out.append((dp.cpu(), None if dm is None else dm.cpu(), dv.cpu()))
        return out

    def lst(t):
        return None if t is None else [t]

    ref, state = [], (p0, m0, v0)
    for r in range(3):
        state = restate(x, coef, *state, *args, 1e-3, True, r + 1)
        ref.append(state)
    kw = dict(weight_decay=1e-3, bias_correction=True)
    # separate tensors, a client-major arena's rows and the two tiled layouts
    flat_segs = segments(x, [n], 0)
    ca = ClientArena.for_model(OrderedDict(w=torch.zeros(n)), k + 2, device=DEV)
    ta = ClientArena.for_model(OrderedDict(w=torch.zeros(n)), k + 2, device=DEV, tiled=True)
    arows = [(5 * i + 3) % (k + 2) for i in range(k)]
    for i, r in enumerate(arows):
        ca.write(r, {"w": x[i].to(DEV)})
        ta.write(r, {"w": x[i].to(DEV)})
    routes = {
        "flat": lambda p, m, v, s: eng.fedavg_adaptive(flat_segs, coef, [p], lst(m), [v], *args, step=s, **kw),
        "client-major arena": lambda p, m, v, s: eng.fedavg_adaptive([[ca.slot(r)["w"] for r in arows]], coef, [p],
                                                                     lst(m), [v], *args, step=s, **kw),
        "tiled buffer": lambda p, m, v, s: eng.fedavg_adaptive_tiled(buf, rows, coef, p, m, v, *args, step=s, **kw),
        "tiled arena": lambda p, m, v, s: eng.fedavg_adaptive_tiled(ta.bufs[torch.float32], arows, coef, p, m, v,
                                                                    *args, step=s, **kw),
    }
    got = {name: three_rounds(run) for name, run in routes.items()}
    for name, rounds in got.items():
        for r, (gp, gm, gv) in enumerate(rounds):
            for what, a, b, c in (("p", gp, ref[r][0], got["flat"][r][0]), ("v", gv, ref[r][2], got["flat"][r][2])) + \
                    ((("m", gm, ref[r][1], got["flat"][r][1]),) if mom else ()):
                assert same_bits(a, b), (name, what, r, "restatement")
                assert same_bits(a, c), (name, what, r, "flat entry")
    assert same_bits(buf.cpu(), keep.cpu())  # the arena is only read
    # nothing to do: no launch, the state untouched
    dp, dm, dv = fresh()
    eng.fedavg_adaptive_tiled(buf, rows, coef, dp[:0], None if dm is None else dm[:0], dv[:0], *args)
    assert same_bits(dp.cpu(), p0) and same_bits(dv.cpu(), v0)


# ----------------------------------------------------------------------------- against torch.optim
def _torch_rounds(make_opt, xs, coef, p0):
    """A server loop on the CPU: FedAvg, the pseudo-gradient p - avg, one optimizer step per round."""
    p = torch.nn.Parameter(p0.clone())
    opt = make_opt([p])
    out = []
    for x in xs:
        opt.zero_grad()
        p.grad = p.data - weighted_avg(x, coef)
        opt.step()
        out.append(p.data.clone())
    return out


def normwise(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("name,wd", [("adam", 0.0), ("adam", 1e-3), ("adagrad", 0.0)])
def test_against_torch_optim(eng, name, wd):
    """torch.optim.Adam / Adagrad on the CPU are the reference: normwise relative error per round
    <= 1e-6, the bound the RMSprop tests hold the same comparison to (the restatement itself is at
    1e-8 from torch: its lerp and addcdiv round differently).  Elementwise the gap reaches ~2e-3
    relative where p crosses zero, so nothing is asserted elementwise."""
    g = torch.Generator().manual_seed(3500)
    n, k, rounds, lr = 2 * E + 5, 6, 6, 0.01
    xs = [normal_data(g, k, n, torch.float32) for _ in range(rounds)]
    coef = coefs(g, k)
    p0 = torch.randn(n, generator=g)
    if name == "adam":
        exp = _torch_rounds(lambda ps: torch.optim.Adam(ps, lr=lr, weight_decay=wd), xs, coef, p0)
        rule, beta1, beta2, eps, bias = ADAM, 0.9, 0.999, 1e-8, True
    else:
        exp = _torch_rounds(lambda ps: torch.optim.Adagrad(ps, lr=lr, weight_decay=wd), xs, coef, p0)
        rule, beta1, beta2, eps, bias = ADAGRAD, 0.0, 0.0, 1e-10, False
    dp, dv = p0.to(DEV), torch.zeros(n, device=DEV)
    dm = [torch.zeros(n, device=DEV)] if beta1 else None
    for r, x in enumerate(xs):
        eng.fedavg_adaptive(segments(x, [n], 0), coef, [dp], dm, [dv], rule, lr, beta1, beta2, eps, weight_decay=wd,
                            bias_correction=bias, step=r + 1)
        rel = normwise(dp.cpu(), exp[r])
        print(f"{name} wd={wd} round {r}: normwise relative error {rel:.3e}")
        assert rel <= 1e-6, (name, wd, r, rel)


# ----------------------------------------------------------------------------- the driver
class _Agg:
    def __init__(self, m):
        self.model = m

    def get_model_params(self):
        return self.model.state_dict()

    def set_model_params(self, p):
        self.model.load_state_dict(p)


def _model(g):
    m = torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.BatchNorm1d(17), torch.nn.Linear(17, 5))
    with torch.no_grad():
        for key, t in m.state_dict().items():
            if "running_var" in key:
                t.copy_(0.5 + torch.rand(t.shape, generator=g))
            elif t.dtype.is_floating_point:
                t.copy_(0.2 * torch.randn(t.shape, generator=g))
            else:
                t.fill_(40)
    return m


def _client(g, model, i):
    sd = OrderedDict()
    for key, t in model.state_dict().items():
        t = t.detach().cpu()
        if t.dtype.is_floating_point:
            sd[key] = t + 0.05 * torch.randn(t.shape, generator=g)
        else:
            sd[key] = torch.tensor(100 + 7 * i, dtype=torch.int64)
    return sd


def _plain_average(dicts, w, key):
    """The reference's per-key loop (agg_operator.py:37-44) with torch CPU ops."""
    avg = None
    for d, wi in zip(dicts, w):
        t = d[key] * wi
        avg = t if avg is None else avg + t
    return avg


DRIVER = {  # name: (rule, beta1, beta2, eps, bias correction, v at round 1, server_lr)
    "adam": (ADAM, 0.9, 0.999, 1e-8, True, 0.0, 0.01),
    "adagrad": (ADAGRAD, 0.0, 0.0, 1e-10, False, 0.0, 0.01),
    "fedadam": (ADAM, 0.9, 0.99, 1e-3, False, 1e-3 * 1e-3, 0.1),
    "fedyogi": (YOGI, 0.9, 0.99, 1e-3, False, 1e-3 * 1e-3, 0.1),
    "fedadagrad": (ADAGRAD, 0.9, 0.0, 1e-3, False, 1e-3 * 1e-3, 0.1),
}


@pytest.mark.parametrize("where", ["cuda", "cpu"])
@pytest.mark.parametrize("name", list(DRIVER))
def test_fedopt_aggregator(name, where):
    from fedml_amd.simulation.mpi.fedopt_aggregator import FedOptAggregator
    rule, beta1, beta2, eps, bias, v_first, lr = DRIVER[name]
    g = torch.Generator().manual_seed(3600)
    model = _model(g)
    torch_model = copy.deepcopy(model)
    pkeys = [key for key, _ in model.named_parameters()]
    state = {key: (p.detach().clone(), torch.zeros_like(p) if beta1 else None, torch.full_like(p, v_first))
             for key, p in model.named_parameters()}
    model = model.to(DEV if where == "cuda" else "cpu")
    fo = FedOptAggregator(worker_num=4, server_aggregator=_Agg(model),
                          args=types.SimpleNamespace(server_optimizer=name, server_lr=lr))
    assert (fo.beta1, fo.beta2, fo.eps, fo.bias_correction, fo.v0) == (beta1, beta2, eps, bias, v_first)
    opt = {"adam": torch.optim.Adam, "adagrad": torch.optim.Adagrad}.get(name)
    opt = opt(torch_model.parameters(), lr=lr) if opt else None
    for r in range(3):
        dicts = [_client(g, model, i) for i in range(4)]
        counts = [int(c) for c in torch.randint(20, 600, (4,), generator=g)]
        w = [c / sum(counts) for c in counts]
        for i in range(4):
            fo.add_local_trained_result(i, dicts[i], counts[i])
        assert fo.check_whether_all_receive()
        got = OrderedDict((key, t.detach().cpu()) for key, t in fo.aggregate().items())
        assert list(got) == list(dicts[0])
        for key in got:
            if key in pkeys:
                x = torch.stack([d[key].reshape(-1) for d in dicts])
                p, m, v = state[key]
                p, m, v = restate(x, w, p.reshape(-1), None if m is None else m.reshape(-1), v.reshape(-1), rule, lr,
                                  beta1, beta2, eps, 0.0, bias, r + 1)
                state[key] = (p, m, v)
                assert same_bits(got[key].reshape(-1), p), (name, r, key)
                assert same_bits(fo.exp_avg_sq[key].reshape(-1), v), (name, r, key, "v")
                assert (m is None and key not in fo.exp_avg) or same_bits(fo.exp_avg[key].reshape(-1), m), (name, r, key)
            else:  # the BatchNorm buffers: the plain average, cast into the buffer's dtype
                exp = _plain_average(dicts, w, key).to(got[key].dtype)
                assert same_bits(got[key], exp), (name, r, key)
        if opt is not None:
            opt.zero_grad()
            for key, p in torch_model.named_parameters():
                p.grad = p.data - _plain_average(dicts, w, key)
            opt.step()
            for key, p in torch_model.named_parameters():
                rel = normwise(got[key], p.data)
                assert rel <= 1e-6, (name, r, key, rel)
    assert fo.rounds == 3


def test_parameter_first_seen_in_a_later_round():
    """It gets fresh state (m = 0, v = v0) and the aggregator's round counter as its bias-correction
    step; while frozen it keeps its value and has no state."""
    from fedml_amd.simulation.mpi.fedopt_aggregator import FedOptAggregator
    g = torch.Generator().manual_seed(3700)
    model = torch.nn.Linear(5, 3).to(DEV)
    model.bias.requires_grad_(False)
    fo = FedOptAggregator(worker_num=2, server_aggregator=_Agg(model),
                          args=types.SimpleNamespace(server_optimizer="adam", server_lr=0.01))
    counts = [10, 11]
    for r in range(2):
        before = model.bias.detach().cpu().clone()
        dicts = [_client(g, model, i) for i in range(2)]
        for i in range(2):
            fo.add_local_trained_result(i, dicts[i], counts[i])
        assert fo.check_whether_all_receive()
        got = fo.aggregate()["bias"].detach().cpu()
        if r == 0:
            assert same_bits(got, before) and "bias" not in fo.exp_avg_sq and "weight" in fo.exp_avg_sq
            model.bias.requires_grad_(True)
    x = torch.stack([d["bias"] for d in dicts])
    p, m, v = restate(x, [c / sum(counts) for c in counts], before, torch.zeros(3), torch.zeros(3), ADAM, 0.01, 0.9,
                      0.999, 1e-8, 0.0, True, 2)
    assert same_bits(got, p) and same_bits(fo.exp_avg["bias"], m) and same_bits(fo.exp_avg_sq["bias"], v)


def test_fedopt_aggregator_config_and_unknown_names():
    from fedml_amd.simulation.mpi.fedopt_aggregator import FedOptAggregator
    model = torch.nn.Linear(3, 2).to(DEV)

    def make(**kw):
        return FedOptAggregator(worker_num=2, server_aggregator=_Agg(model), args=types.SimpleNamespace(server_lr=0.1, **kw))

    fo = make(server_optimizer="FedYogi", server_beta1=0.5, server_beta2=0.9, server_eps=1e-2, server_weight_decay=1e-4)
    assert (fo.rule, fo.beta1, fo.beta2, fo.eps, fo.weight_decay, fo.v0) == (YOGI, 0.5, 0.9, 1e-2, 1e-4, 1e-2 * 1e-2)
    for bad in ("adamw", "amsgrad", "yogi"):
        with pytest.raises(NotImplementedError, match="fedyogi"):
            make(server_optimizer=bad)


# ----------------------------------------------------------------------------- argument checks
@pytest.mark.parametrize("entry", ["fa_fedavg_adaptive", "fa_fedavg_adaptive_tiled"])
def test_entry_rejects_bad_arguments_in_order(eng, entry):
    K, NUMEL = 3, 8
    tiled = entry.endswith("_tiled")
    xs = [torch.ones(E, device=DEV) for _ in range(K)]
    p, m, v = (torch.full((NUMEL,), GUARD, device=DEV) for _ in range(3))
    L = N.lib()
    good = dict(ctx=eng._ctx, sizes=[NUMEL], k=K, ptrs=[x.data_ptr() for x in xs], tile_stride=N.TILE_BYTES,
                coef=[0.2, 0.3, 0.5], params=[p.data_ptr()], ms=[m.data_ptr()], vs=[v.data_ptr()], rule=ADAM, lr=0.1,
                beta1=0.9, beta2=0.99, eps=1e-3, wd=0.0, bias=0, step=1)

    def call(**kw):
        a = dict(good, **kw)

        def arr(x, make):
            return None if x is None else make(x)
        args = [a["ctx"], len(a["sizes"] or [0]), arr(a["sizes"], N.i64_array), a["k"], arr(a["ptrs"], N.ptr_array)]
        args += [a["tile_stride"]] if tiled else []
        args += [arr(a["coef"], N.f64_array), arr(a["params"], N.ptr_array), arr(a["ms"], N.ptr_array),
                 arr(a["vs"], N.ptr_array), a["rule"], a["lr"], a["beta1"], a["beta2"], a["eps"], a["wd"], a["bias"],
                 a["step"], None]
        return getattr(L, entry)(*args), L.fa_last_error()

    # each list: ways to break one check; the checks in the documented order
    checks = [
        (b"ctx is NULL", [dict(ctx=None)]),
        (b"tile_stride must be > 0", [dict(tile_stride=0), dict(tile_stride=-4096)] if tiled else []),
        (b"invalid arguments", [dict(k=0), dict(sizes=None), dict(ptrs=None), dict(params=None)]),
        (b"coef is NULL", [dict(coef=None)]),
        (b"d_v is NULL", [dict(vs=None)]),
        (b"d_m must be NULL exactly when beta1 == 0", [dict(ms=None), dict(beta1=0.0)]),
        (b"rule", [dict(rule=3), dict(rule=-1)]),
        (b"need 0 <= beta1 < 1", [dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=-0.1),
                                  dict(beta2=float("nan")), dict(eps=-1e-3), dict(step=0)]),
        (b"multiple of", [dict(tile_stride=1000)] if tiled else []),
        (b"NULL", [dict(params=[None]), dict(ptrs=[xs[0].data_ptr(), None, xs[2].data_ptr()]), dict(vs=[None]),
                   dict(ms=[None])]),
    ]
    for i, (msg, ways) in enumerate(checks):
        for way in ways:
            rc, err = call(**way)
            assert rc == N.FA_ERR_INVALID and msg in err, (way, err)
            assert i == 0 or err.startswith(entry.encode() + b":"), err
            # with every later check broken too, this one is still the one reported
            later = {}
            for _, more in checks[i + 1:]:
                if more and not (set(more[0]) & set(way)):
                    later.update(more[0])
            rc, err = call(**dict(later, **way))
            assert rc == N.FA_ERR_INVALID and msg in err, (way, later, err)
    assert b"negative numel" in call(sizes=[-NUMEL])[1]
    torch.cuda.synchronize()
    assert all(bool((t == GUARD).all()) for t in (p, m, v))  # nothing was launched
    # all segments empty: FA_OK, nothing launched, no pointer looked at
    rc, err = call(sizes=[0, 0], ptrs=[None] * (2 * K), params=[None, None], ms=[None, None], vs=[None, None])
    assert rc == N.FA_OK, err
    torch.cuda.synchronize()
    assert all(bool((t == GUARD).all()) for t in (p, m, v))
    rc, err = call()
    assert rc == N.FA_OK, err
    torch.cuda.synchronize()
    full = torch.full((NUMEL,), GUARD)
    rp, rm, rv = restate(torch.ones(K, NUMEL), good["coef"], full, full, full, ADAM, 0.1, 0.9, 0.99, 1e-3)
    assert same_bits(p.cpu(), rp) and same_bits(m.cpu(), rm) and same_bits(v.cpu(), rv)


def test_engine_argument_checks(eng):
    xs = [torch.zeros(8, device=DEV) for _ in range(3)]
    p, m, v = (torch.zeros(8, device=DEV) for _ in range(3))
    w = [0.2, 0.3, 0.5]
    tail = (ADAM, 0.1, 0.9, 0.99, 1e-3)
    with pytest.raises(ValueError):
        eng.fedavg_adaptive([], w, [], [], [], *tail)
    with pytest.raises(ValueError):
        eng.fedavg_adaptive([xs], [0.5, 0.5], [p], [m], [v], *tail)
    with pytest.raises(ValueError, match="beta1"):
        eng.fedavg_adaptive([xs], w, [p], None, [v], *tail)
    with pytest.raises(ValueError, match="beta1"):
        eng.fedavg_adaptive([xs], w, [p], [m], [v], ADAM, 0.1, 0.0, 0.99, 1e-3)
    with pytest.raises(ValueError, match="rule"):
        eng.fedavg_adaptive([xs], w, [p], [m], [v], 3, 0.1, 0.9, 0.99, 1e-3)
    for bad in (dict(step=0), dict(step=1.5), dict(step=True)):
        with pytest.raises(ValueError, match="step"):
            eng.fedavg_adaptive([xs], w, [p], [m], [v], *tail, **bad)
    with pytest.raises(ValueError):
        eng.fedavg_adaptive([xs], w, [p], [m], [v], ADAM, 0.1, 1.0, 0.99, 1e-3)
    with pytest.raises(TypeError):
        eng.fedavg_adaptive([xs], w, [p], [m], [v.double()], *tail)
    with pytest.raises(TypeError):
        eng.fedavg_adaptive([xs], w, [p], [torch.zeros(7, device=DEV)], [v], *tail)
    with pytest.raises(ValueError):
        eng.fedavg_adaptive([xs], w, [p], [m], [v.cpu()], *tail)
    with pytest.raises(ValueError, match="contiguous"):
        eng.fedavg_adaptive([xs], w, [p], [m], [torch.zeros(16, device=DEV)[::2]], *tail)
    with pytest.raises(ValueError, match="contiguous"):
        eng.fedavg_adaptive([xs], w, [torch.zeros(16, device=DEV)[::2]], [m], [v], *tail)
    with pytest.raises(ValueError):
        eng.fedavg_adaptive([[x.double() for x in xs]], w, [p], [m], [v], *tail)
    buf = torch.zeros(2, 4, E, device=DEV)
    p2, m2, v2 = (torch.zeros(2 * E, device=DEV) for _ in range(3))
    with pytest.raises(ValueError):
        eng.fedavg_adaptive_tiled(buf, [0, 1], [1.0], p2, m2, v2, *tail)
    with pytest.raises(IndexError):
        eng.fedavg_adaptive_tiled(buf, [0, 4], [0.5, 0.5], p2, m2, v2, *tail)
    with pytest.raises(TypeError):
        eng.fedavg_adaptive_tiled(buf.double(), [0, 1], [0.5, 0.5], p2, m2, v2, *tail)
    with pytest.raises(TypeError):
        eng.fedavg_adaptive_tiled(buf, [0, 1], [0.5, 0.5], p2, m2, v2[:7], *tail)
    with pytest.raises(ValueError):
        eng.fedavg_adaptive_tiled(buf, [0, 1], [0.5, 0.5], torch.zeros(2 * E + 1, device=DEV), m2, v2, *tail)
    assert all(bool((t == 0).all()) for t in (p, m, v, p2, m2, v2))
