"""Shared helpers: replay a golden case through an aggregation engine and compare bit-for-bit.

An *engine* is an object with
    weighted_sum(xs, mode, coef=None, divisor=1.0) -> tensor       (xs: list of same-shape tensors)
    mix(xs, row_ptr, cols, vals, post_scale=None) -> (outs, outs2)
Both the C oracle (oracle.orc) and the HIP product (fedml_amd) are driven through the same
replay, so a case means the same thing for both.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch

from golden_io import client_dicts, expected_dicts

MUL_W, MUL_N_DIV_N, SUM = 0, 1, 2


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bitwise equality; NaN matches NaN (NaN payloads differ between torch CPU paths)."""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if not a.is_floating_point():
        return torch.equal(a, b)
    ia = {torch.float32: torch.int32, torch.float64: torch.int64,
          torch.bfloat16: torch.int16, torch.float16: torch.int16}[a.dtype]
    nan = torch.isnan(a) & torch.isnan(b)
    return bool(torch.all((a.view(ia) == b.view(ia)) | nan))


def assert_dict_bits(got: OrderedDict, exp: OrderedDict, what: str = ""):
    assert list(got.keys()) == list(exp.keys()), (what, list(got.keys()), list(exp.keys()))
    for k in exp:
        g, e = got[k], exp[k]
        assert g.dtype == e.dtype, (what, k, g.dtype, e.dtype)
        assert tuple(g.shape) == tuple(e.shape), (what, k, g.shape, e.shape)
        if not bits_equal(g.reshape(-1), e.reshape(-1)):
            gd, ed = g.double().reshape(-1), e.double().reshape(-1)
            bad = torch.nonzero(~((gd == ed) | (torch.isnan(gd) & torch.isnan(ed)))).reshape(-1)
            i = int(bad[0]) if bad.numel() else -1
            raise AssertionError(f"{what} key={k}: {bad.numel()} mismatches, first at {i}: "
                                 f"got {gd[i].item()!r} expected {ed[i].item()!r}")


def per_key(engine, dicts, mode, coef=None, divisor=1.0):
    keys = list(dicts[0].keys())
    out = OrderedDict()
    for k in keys:
        xs = [d[k] for d in dicts]
        shape = xs[0].shape
        r = engine.weighted_sum([x.reshape(-1) for x in xs], mode, coef, divisor)
        out[k] = r.reshape(shape)
    return out


def per_key_mix(engine, dicts, row_ptr, cols, vals, post_scale=None):
    keys = list(dicts[0].keys())
    rows = len(row_ptr) - 1
    outs = [OrderedDict() for _ in range(rows)]
    outs2 = [OrderedDict() for _ in range(rows)] if post_scale is not None else None
    for k in keys:
        shape = dicts[0][k].shape
        o, o2 = engine.mix([d[k].reshape(-1) for d in dicts], row_ptr, cols, vals, post_scale)
        for r in range(rows):
            outs[r][k] = o[r].reshape(shape)
            if outs2 is not None:
                outs2[r][k] = o2[r].reshape(shape)
    return outs, outs2


def dense_csr(W):
    n = W.shape[0]
    row_ptr = [i * n for i in range(n + 1)]
    cols = [j for _ in range(n) for j in range(n)]
    vals = [float(W[i, j]) for i in range(n) for j in range(n)]
    return row_ptr, cols, vals


def dsgd_csr(W):
    """Row i = [self, in-neighbours j ascending] with weights [W_ii, W_ji] (client_dsgd.py:92-116)."""
    n = W.shape[0]
    row_ptr, cols, vals = [0], [], []
    for i in range(n):
        cols.append(i)
        vals.append(float(W[i, i]))
        for j in range(n):
            if j != i and W[j, i] != 0:
                cols.append(j)
                vals.append(float(W[j, i]))
        row_ptr.append(len(cols))
    return row_ptr, cols, vals


def replay(engine, meta, arrays):
    """Return the list of output dicts the reference produced for this case, via `engine`."""
    kind = meta["kind"]
    clients = client_dicts(meta, arrays)
    n = meta.get("n")
    if kind in ("agg", "sp_aggregate"):
        opt = meta.get("optimizer", "FedAvg")
        N = sum(n)
        if opt in ("FedAvg", "FedProx"):
            return [per_key(engine, clients, MUL_W, [v / N for v in n])]
        if opt in ("FedAvg_seq", "FedDyn"):
            return [per_key(engine, clients, SUM)]
        cs = []
        for i in range(meta["num_clients"]):
            d = OrderedDict()
            for key in meta["keys"]:
                d[key] = torch.from_numpy(arrays[f"c{i}__{key}"].copy())
            cs.append(d)
        if opt == "SCAFFOLD":
            K = len(clients)
            if K == 1:
                wout = per_key(engine, clients[:1], MUL_W, [n[0] / N])
            else:
                wout = per_key(engine, clients[-1:], SUM)
            cout = per_key(engine, cs[-1:], MUL_W, [1 / meta["client_num_in_total"]])
            return [wout, cout]
        if opt == "Mime":
            w = [v / N for v in n]
            return [per_key(engine, clients, MUL_W, w), per_key(engine, cs, MUL_W, w)]
        raise ValueError(opt)
    if kind == "mpi_fedavg":
        return [per_key(engine, clients, MUL_N_DIV_N, n, sum(n))]
    if kind == "fedavg_seq":
        N = sum(n)
        partials = [per_key(engine, [clients[i] for i in wk], MUL_W, [n[i] / N for i in wk])
                    for wk in meta["schedule"]]
        return [per_key(engine, partials, SUM)]
    if kind == "hier_sp":
        groups = meta["groups"]
        gw, gn = [], []
        for grp in groups:
            Ng = sum(n[i] for i in grp)
            gw.append(per_key(engine, [clients[i] for i in grp], MUL_W, [n[i] / Ng for i in grp]))
            gn.append(Ng)
        Nt = sum(gn)
        return [per_key(engine, gw, MUL_W, [v / Nt for v in gn])]
    if kind == "hier_cloud":
        E, R, ne = meta["edges"], meta["group_comm_round"], meta["edge_counts"]
        avg = None
        for r in range(R):
            ml = [clients[e * R + r] for e in range(E)]
            cnt = [ne[e][r] for e in range(E)]
            avg = per_key(engine, ml, MUL_N_DIV_N, cnt, sum(cnt))
        ml = [avg] + [clients[e * R + R - 1] for e in range(1, E)]
        cnt = [ne[e][R - 1] for e in range(E)]
        return [per_key(engine, ml, MUL_N_DIV_N, cnt, sum(cnt))]
    if kind == "mix_rows":
        W = arrays["W"]
        outs, _ = per_key_mix(engine, clients, *dense_csr(W))
        return outs
    if kind == "hier_mix":
        E, R = meta["edges"], meta["group_comm_round"]
        W = arrays["W"]
        outs = avg = None
        for r in range(R):
            ml = [clients[e * R + r] for e in range(E)]
            outs, _ = per_key_mix(engine, ml, *dense_csr(W))
            avg = per_key(engine, outs, MUL_N_DIV_N, [1] * E, E)
        return [avg] + outs[1:]
    if kind == "dsgd":
        outs, _ = per_key_mix(engine, clients, *dsgd_csr(arrays["W"]))
        return outs
    if kind == "pushsum":
        scale = [1.0 / o for o in meta["omegas_out"]]
        _, z = per_key_mix(engine, clients, *dsgd_csr(arrays["W"]), post_scale=scale)
        return z
    raise ValueError(kind)


def check_case(engine, meta, arrays, what=""):
    got = replay(engine, meta, arrays)
    exp = expected_dicts(meta, arrays)
    assert len(got) == len(exp), (what, len(got), len(exp))
    for j, (g, e) in enumerate(zip(got, exp)):
        assert_dict_bits(g, e, f"{what}{meta['name']}[{j}]")


def fedopt_replay(meta, arrays, weighted_sum, sgd_apply, to_dev=lambda t: t):
    """Replay a FedOpt fixture: per round FedAvg (weighted_sum), then the SGD server step on the
    parameters (sgd_apply, in place) and the averaged buffers cast into their dtype.  Returns the
    list of per-round global state_dicts (CPU)."""
    from golden_io import np_to_tensor
    keys, dtypes, params = meta["keys"], meta["dtypes"], set(meta["params"])
    state = OrderedDict((k, to_dev(np_to_tensor(arrays[f"init__{k}"], dt))) for k, dt in zip(keys, dtypes))
    bufs = {}
    outs = []
    for r, rd in enumerate(meta["rounds"]):
        n = rd["n"]
        N = sum(n)
        W = len(n)
        new = OrderedDict()
        for k, dt in zip(keys, dtypes):
            xs = [to_dev(np_to_tensor(arrays[f"r{r}_x{i}__{k}"], dt)) for i in range(W)]
            avg = weighted_sum([x.reshape(-1) for x in xs], MUL_W, [v / N for v in n]).reshape(xs[0].shape)
            if k in params:
                p = state[k].clone().contiguous()
                first = k not in bufs
                if meta["server_momentum"] != 0 and first:
                    bufs[k] = torch.empty_like(p)
                sgd_apply(avg.contiguous(), p, bufs.get(k) if meta["server_momentum"] != 0 else None,
                          meta["server_lr"], meta["server_momentum"], 0.0, 0.0, False, first)
                new[k] = p
            else:
                new[k] = avg.to(state[k].dtype)  # load_state_dict copy_: float -> int64 truncates
        state = new
        outs.append(OrderedDict((k, v.cpu()) for k, v in state.items()))
    return outs


def fedopt_expected(meta, arrays):
    from golden_io import np_to_tensor
    return [OrderedDict((k, np_to_tensor(arrays[f"r{r}_y__{k}"], dt)) for k, dt in zip(meta["keys"], meta["dtypes"]))
            for r in range(len(meta["rounds"]))]


# ----------------------------------------------------------------------------- finite field (SecAgg)
MOD_FIRST, MOD_EACH, MOD_END, REAL_F64 = 1, 2, 4, 8


def sa_order_and_flags(uploaded):
    """SecAgg reconstruction (sa_fedml_aggregator.py:150-164): clients summed and the mod flags, given
    the per-client upload flags of the first-round active clients [0..N)."""
    order = [0] + [i for i in range(1, len(uploaded)) if uploaded[i]]
    return order, MOD_EACH | MOD_END | (MOD_FIRST if uploaded[0] else 0)


def finite_case_inputs(meta, arrays):
    """(clients as int64/float CPU tensors per key) for a finite-field fixture."""
    return client_dicts(meta, arrays)


# ----------------------------------------------------------------------------- mixing / gossip
def oracle_pushsum(xs, row_ptr, cols, vals, omega_in, outs, outs2, omega_out):
    """The engine's fa_pushsum restated: omega' = the row's ordered float32 chain, z = x' * fp32(1/omega')."""
    from oracle import orc
    om = omega_in.numpy().astype(np.float32)
    new = []
    for r in range(len(row_ptr) - 1):
        acc = np.float32(-0.0)
        for j in range(row_ptr[r], row_ptr[r + 1]):
            acc = np.float32(acc + np.float32(om[cols[j]] * np.float32(vals[j])))
        new.append(acc)
    post = [float(np.float32(1.0) / a) for a in new]
    o, o2 = orc.mix(xs, row_ptr, cols, vals, post_scale=post)
    for a, b in zip(outs, o):
        a.copy_(b)
    for a, b in zip(outs2, o2):
        a.copy_(b)
    omega_out.copy_(torch.tensor([float(a) for a in new], dtype=torch.float32))


MIX_SENTINEL = 7.0
MIX_SPECIALS = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1e-40, -6e-8, 65504.0]
MIX_FINITE = [0.0, -0.0, 2.0, -3.0, 0.5, 1e-40, -6e-8, 65504.0]  # the same slots without inf / NaN
MIX_INPUT0 = [-0.0, -0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]


def mix_tile(dtype) -> int:
    """Elements of one kernel tile (256 lanes x 16 bytes) = of one arena tile."""
    return 256 * (16 // torch.empty(0, dtype=dtype).element_size())


def mix_post_scale(rows: int):
    return [1.0 / (1 + 0.25 * r) for r in range(rows)]


def mix_inputs(dtype, num_in: int, n: int, seed: int, special: bool):
    """num_in CPU vectors of randn * 2^randint(-12, 12); the first eight elements of every input are
    the special values (``special``) or their finite stand-ins, input 0's are MIX_INPUT0.  The two
    copies of one seed differ in those slots only."""
    g = torch.Generator().manual_seed(seed)
    head = MIX_SPECIALS if special else MIX_FINITE
    xs = []
    for i in range(num_in):
        x = torch.randn(n, generator=g, dtype=torch.float64)
        x = x * torch.pow(2.0, torch.randint(-12, 13, (n,), generator=g).double())
        h = torch.tensor(MIX_INPUT0 if i == 0 else head, dtype=torch.float64)
        x[:min(8, n)] = h[:min(8, n)]
        xs.append(x.to(dtype))
    return xs


def torch_mix_reference(xs, row_ptr, cols, vals, post_scale=None):
    """fa_mix per operation in plain torch: every product rounded to the dtype, every sum rounded to
    the dtype, the first term passed through; weights and post-scales as float32."""
    dt = xs[0].dtype
    outs, outs2 = [], ([] if post_scale is not None else None)
    for r in range(len(row_ptr) - 1):
        acc = None
        for j in range(row_ptr[r], row_ptr[r + 1]):
            t = (xs[cols[j]].float() * torch.tensor(vals[j], dtype=torch.float64).float()).to(dt)
            acc = t if acc is None else (acc.float() + t.float()).to(dt)
        outs.append(acc)
        if post_scale is not None:
            outs2.append((acc.float() * torch.tensor(post_scale[r], dtype=torch.float64).float()).to(dt))
    return outs, outs2


def _normalised_rows(a: np.ndarray) -> np.ndarray:
    a = a.astype(np.float32)
    return a / a.sum(1, keepdims=True)


def mix_matrices():
    """name -> (row_ptr, cols, vals, num_in): the irregular gossip matrices of the mixing tests."""
    import os
    from fedml_amd.core.distributed.topology import topology_manager as tm
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "topologies.npz"))
    out = OrderedDict()

    def add(name, csr, num_in):
        out[name] = (list(csr[0]), list(csr[1]), list(csr[2]), num_in)

    def ring(n):
        m = tm.SymmetricTopologyManager(n, 2)
        m.generate_topology()
        return m.topology

    for n in (3, 5, 8, 37):
        add(f"ring{n}", tm.gossip_rows(ring(n)), n)
    chain = np.eye(9) + np.eye(9, k=1) + np.eye(9, k=-1)
    add("chain9", tm.gossip_rows(_normalised_rows(chain)), 9)
    add("isolated9", tm.gossip_rows(tm.overlay_isolated(9)), 9)
    add("star3", tm.gossip_rows(tm.overlay_star(3)), 3)
    perm = np.random.RandomState(5).permutation(11)
    add("ring11_permuted", tm.gossip_rows(ring(11)[np.ix_(perm, perm)]), 11)
    add("balanced_tree7", tm.gossip_rows(tm.overlay_balanced_tree(7, 2)), 7)
    for n in (7, 10):
        a = np.eye(n)
        for i in range(1, n):
            a[i, (i - 1) // 2] = a[(i - 1) // 2, i] = 1
        add(f"undirected_tree{n}", tm.gossip_rows(_normalised_rows(a)), n)
    add("complete4_dense", tm.dense_rows(tm.overlay_complete(4)), 4)
    add("star9", tm.gossip_rows(tm.overlay_star(9)), 9)
    add("star12", tm.gossip_rows(tm.overlay_star(12)), 12)
    add("torus9", tm.gossip_rows(tm.overlay_2d_torus(9)), 9)
    add("random8", tm.gossip_rows(golden["W_random_8_seed3"]), 8)
    add("random12", tm.gossip_rows(golden["W_random_12_seed4"]), 12)
    add("complete11_dense", tm.dense_rows(tm.overlay_complete(11)), 11)
    add("complete9_gossip", tm.gossip_rows(tm.overlay_complete(9)), 9)
    hand = [[2, 0, 2, 1], [1], [0, 3, 3, 3, 3, 3, 3, 3, 3, 0]]
    hvals = [[0.5, 0.0, -0.75, 0.1], [1.25], [0.1, 0.2, 0.0, -0.75, 0.1, 0.3, -0.05, 0.1, 0.25, 0.6]]
    rp = [0]
    for c in hand:
        rp.append(rp[-1] + len(c))
    add("handmade", (rp, sum(hand, []), sum(hvals, [])), 4)
    return out


def guarded_views(dtype, n: int, count: int, shifts=None, device="cuda:0"):
    """``count`` views of n elements into one sentinel-filled buffer, each starting on a 16-byte
    boundary plus shifts[i] elements, at least 16 bytes of sentinel on either side of every view.
    Returns (buffer, views, starts)."""
    vec = 16 // torch.empty(0, dtype=dtype).element_size()
    slot = -(-n // vec) * vec + 2 * vec
    buf = torch.full((count * slot + 2 * vec,), MIX_SENTINEL, dtype=dtype, device=device)
    starts = [vec + i * slot + (shifts[i] if shifts else 0) for i in range(count)]
    return buf, [buf[s:s + n] for s in starts], starts


def guards_intact(buf, starts, n: int) -> bool:
    """Every element of ``buf`` outside the views still holds the sentinel."""
    outside = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    for s in starts:
        outside[s:s + n] = False
    return bool((buf[outside] == MIX_SENTINEL).all())
