"""The device rotation (include/fedagg_rotate.h, fedml_amd/csrc/hadamard.hip) against the numpy restatement
(tests/rhtcases.py), bit for bit (NaN positions equal, every other bit equal): every block size, both
directions, inputs and outputs one word off a 16-byte boundary, segments of one element up to several
slots in one call; the padding, the argument checks, and the state_dict layer end to end."""
from __future__ import annotations

import dataclasses
import os
import sys
import types
from collections import OrderedDict

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rhtcases as R  # noqa: E402

from fedml_amd import _native as N  # noqa: E402
from fedml_amd.ml.aggregator import rotated as RT  # noqa: E402
from fedml_amd.ml.aggregator.agg_operator import FedMLAggOperator  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED, ROUND = 0x0123456789ABCDEF, 7
IDS = [3, 0, 9, 1, 2, 0xFFFFFFFF, 5, 77]
S = N.RHT_SLOT
SENTINEL = -123.0


@pytest.fixture(scope="module")
def eng():
    from fedml_amd.engine import get_engine
    return get_engine(0)


def sizes(b):
    B = 1 << b
    return [1, B - 1, B, B + 1, 3 * B + 17, S, S + 1, 2 * S + B + 37]


def pad(n, b):
    return -(-n >> b) << b


def placed(t, off):
    """t on the device, `off` 4-byte words past a 16-byte boundary."""
    e = off * 4 // t.element_size()
    buf = torch.empty(t.numel() + e + 8, dtype=t.dtype, device=DEV)
    buf[e:e + t.numel()] = t
    return buf[e:e + t.numel()]


def rotate(eng, xs, b, inverse, numels, off_in=0, off_out=0):
    """The device's outputs as numpy, after checking that nothing past an output was written."""
    outs_n = numels if inverse else [pad(n, b) for n in numels]
    bufs = [torch.full((n + off_out + 8,), SENTINEL, dtype=torch.float32, device=DEV) for n in outs_n]
    outs = [buf[off_out:off_out + n] for buf, n in zip(bufs, outs_n)]
    eng.hadamard_rotate([placed(x, off_in) for x in xs], b, SEED, ROUND, IDS[:len(xs)], inverse=inverse,
                        numels=numels if inverse else None, outs=outs)
    torch.cuda.synchronize()
    for buf, n in zip(bufs, outs_n):
        assert (buf[:off_out] == SENTINEL).all() and (buf[off_out + n:] == SENTINEL).all()
    return [o.cpu().numpy() for o in outs]


def expect(xs, b, inverse, numels):
    f32 = [x.to(torch.float32).numpy() for x in xs]
    if inverse:
        return [R.inverse(y, n, b, SEED, ROUND, i) for y, n, i in zip(f32, numels, IDS)]
    return [R.forward(x, b, SEED, ROUND, i) for x, i in zip(f32, IDS)]


def assert_same(got, exp):
    for s, (g, e) in enumerate(zip(got, exp)):
        nan = np.isnan(e)
        assert g.shape == e.shape and (np.isnan(g) == nan).all(), f"segment {s}"
        bad = np.flatnonzero(g.view(np.uint32)[~nan] != e.view(np.uint32)[~nan])
        assert bad.size == 0, f"segment {s}: {bad.size} elements differ, the first at {bad[:4]}"


@pytest.mark.parametrize("off_in,off_out", [(0, 0), (1, 0), (0, 1)])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("b", range(5, 14))
def test_integer_tables(eng, b, inverse, off_in, off_out):
    """Exact in every stage, so any wrong pairing, sign bit or permutation shows."""
    g = torch.Generator().manual_seed(b)
    numels = sizes(b)
    xs = [torch.randint(-1024, 1025, (pad(n, b) if inverse else n,), generator=g).float() for n in numels]
    assert_same(rotate(eng, xs, b, inverse, numels, off_in, off_out), expect(xs, b, inverse, numels))


def wide(g, n, b):
    x = torch.randn(n, generator=g) * torch.exp(3 * torch.randn(n, generator=g))
    B = 1 << b
    if n > 3 * B + 3:  # a -0.0, a subnormal block, a NaN block and an Inf block
        x[1] = -0.0
        x[B:2 * B] *= 1e-42
        x[2 * B + 5] = float("nan")
        x[3 * B + 3] = float("inf")
    return x


@pytest.mark.parametrize("dt,inverse", [(torch.float32, False), (torch.bfloat16, False), (torch.float16, False),
                                        (torch.float32, True)])
@pytest.mark.parametrize("b", range(5, 14))
def test_wide_range_data(eng, b, dt, inverse):
    """Rounding in every stage, so the stage order and any fused or reordered add show."""
    g = torch.Generator().manual_seed(50 + b)
    numels = sizes(b)
    xs = [wide(g, n, b).to(dt) for n in numels]
    if inverse:  # the restatement's forward outputs, NaN and Inf blocks included
        xs = [torch.from_numpy(y) for y in expect(xs, b, False, numels)]
    assert_same(rotate(eng, xs, b, inverse, numels), expect(xs, b, inverse, numels))


def test_argument_errors(eng):
    """Each returns its status at a check that precedes any HIP call."""
    L, ctx = N.lib(), eng._ctx
    one, ids = N.i64_array([64]), N.u32_array([0])
    x = torch.zeros(80, device=DEV)
    p, odd = N.ptr_array([x.data_ptr()]), N.ptr_array([x.data_ptr() + 2])
    for args, code, text in (
            ((N.F32, N.RHT_FORWARD, 4, 0, 0, 1, one, ids, p, p, None), N.FA_ERR_INVALID, "log2_block"),
            ((N.F32, N.RHT_FORWARD, 14, 0, 0, 1, one, ids, p, p, None), N.FA_ERR_INVALID, "log2_block"),
            ((N.F32, 2, 5, 0, 0, 1, one, ids, p, p, None), N.FA_ERR_INVALID, "direction"),
            ((N.F64, N.RHT_FORWARD, 5, 0, 0, 1, one, ids, p, p, None), N.FA_ERR_DTYPE, "dtype"),
            ((N.BF16, N.RHT_INVERSE, 5, 0, 0, 1, one, ids, odd, odd, None), N.FA_ERR_DTYPE, "inverse"),
            ((N.F32, N.RHT_FORWARD, 5, 0, 0, 1, one, ids, odd, p, None), N.FA_ERR_INVALID, "input"),
            ((N.BF16, N.RHT_FORWARD, 5, 0, 0, 1, one, ids, odd, odd, None), N.FA_ERR_INVALID, "output")):
        assert L.fa_hadamard_rotate(ctx, *args) == code, (args, L.fa_last_error())
        assert text.encode() in L.fa_last_error(), L.fa_last_error()
    assert L.fa_hadamard_rotate(ctx, N.F32, N.RHT_FORWARD, 5, 0, 0, 1, N.i64_array([0]), ids, p, p, None) == N.FA_OK


def client_dicts(k):
    g = torch.Generator().manual_seed(11)
    return [OrderedDict([("w", wide(g, 200, 6).view(10, 20).to(DEV)),
                         ("h", torch.randn(65, generator=g).to(torch.bfloat16).to(DEV)),
                         ("steps", torch.tensor(100 + i, device=DEV))]) for i in range(k)]


@pytest.mark.parametrize("compress", [None, "q8", "q1", "fp4"])
def test_operator_end_to_end(eng, compress):
    """FedMLAggOperator.agg on rotated dicts = the inverse restatement of what the existing aggregate*
    returns on the unwrapped inner dicts."""
    rot = RT.Rotation(SEED, ROUND, 6)
    counts = [10, 20, 30]
    ups = [RT.rotate_state_dict(sd, rot, compress) for sd in client_dicts(3)]
    assert [type(v) for v in ups[0].values()] == [RT.RotatedTensor, RT.RotatedTensor, torch.Tensor]
    args = types.SimpleNamespace(federated_optimizer="FedAvg", rotation_seed=SEED)
    got = FedMLAggOperator.agg(args, list(zip(counts, ups)))
    inner = [OrderedDict((k, v.inner if isinstance(v, RT.RotatedTensor) else v) for k, v in d.items()) for d in ups]
    agg = {None: RT.aggregate, "q8": RT.aggregate_q8, "q1": RT.aggregate_q1, "fp4": RT.aggregate_mx}[compress]
    sums = agg(inner, RT.MUL_W, [c / 60 for c in counts])
    torch.cuda.synchronize()
    assert list(got) == ["w", "h", "steps"] and torch.equal(got["steps"], sums["steps"])
    for seg_id, (key, shape, dt) in enumerate([("w", (10, 20), torch.float32), ("h", (65,), torch.bfloat16)]):
        n = got[key].numel()
        exp = torch.from_numpy(R.inverse(sums[key].cpu().numpy(), n, 6, SEED, ROUND, seg_id)).view(shape).to(dt)
        assert got[key].dtype == dt and got[key].shape == shape
        assert_same([got[key].float().cpu().numpy().reshape(-1)], [exp.float().numpy().reshape(-1)])
    back = RT.unrotate_state_dict(ups[0], SEED)
    assert back["w"].shape == (10, 20) and back["h"].dtype == torch.bfloat16


def test_mismatches_and_routing(eng):
    rot = RT.Rotation(SEED, ROUND, 6)
    a, b = (RT.rotate_state_dict(sd, rot) for sd in client_dicts(2))
    plain = OrderedDict(b, w=b["w"].inner)
    with pytest.raises(TypeError):
        RT.aggregate_rotated([a, plain], RT.SUM, None, SEED)
    for change in (dict(shape=(200,)), dict(dtype=torch.float16), dict(seg_id=5), dict(round=8), dict(log2_block=7)):
        other = OrderedDict(b, w=dataclasses.replace(b["w"], **change))
        with pytest.raises(ValueError, match=next(iter(change))):
            RT.aggregate_rotated([a, other], RT.SUM, None, SEED)
    ups = [(1, a), (1, b)]
    ns = types.SimpleNamespace
    with pytest.raises(ValueError, match="rotation_seed"):
        FedMLAggOperator.agg(ns(federated_optimizer="FedAvg"), ups)
    with pytest.raises(NotImplementedError):
        FedMLAggOperator.agg(ns(federated_optimizer="FedOpt", rotation_seed=SEED), ups)
    with pytest.raises(NotImplementedError, match="vote"):
        FedMLAggOperator.agg(ns(federated_optimizer="FedAvg", rotation_seed=SEED, q1_majority_vote=True), ups)
