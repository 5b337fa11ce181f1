"""Block-quantized int8 (q8) updates, the parts that need no device: the symbols, the C ABI's argument
checks (include/fedagg_quant.h: they run before any HIP call, in the stated order), the state_dict
layer's errors, key handling and routing with the engine stubbed -- and the torch-CPU per-op
RESTATEMENT of both contracts (quantize_ref, sum_ref), which tests/test_gpu_quantized.py imports and
compares the kernels with bit for bit.  The restatement is checked here against cases worked by hand.
"""
from __future__ import annotations

import ctypes
import os
import re
import types
from collections import OrderedDict

import pytest
import torch

from conftest import ROOT
from fedml_amd import _native as N

QNAN = 0x7FC00000


# ---------------------------------------------------------------------------------------------------
# the restatement (torch CPU, one rounded float32 op per line; tensors on both sides of every division
# and product, so no op takes a scalar shortcut)

def quantize_ref(x: torch.Tensor, block: int):
    """fa_quantize_q8's contract for one tensor (float32, bfloat16 or float16): (q int8, scale float32)."""
    xf = x.detach().cpu().reshape(-1).to(torch.float32)  # exact widening
    n = xf.numel()
    nb = -(-n // block)
    xb = torch.zeros(nb * block, dtype=torch.float32)
    xb[:n] = xf
    xb = xb.view(nb, block)
    bad = ~torch.isfinite(xb).all(dim=1)
    amax = xb.abs().amax(dim=1)
    scale = amax / torch.full_like(amax, 127.0)
    quot = xb / scale.view(nb, 1).expand(nb, block).contiguous()
    q = torch.round(quot).clamp(-127.0, 127.0)  # torch.round: ties to even
    dead = (bad | (scale == 0)).view(nb, 1).expand(nb, block)
    q = torch.where(dead, torch.zeros_like(q), q).to(torch.int8)
    scale = torch.where(bad, torch.full((nb,), QNAN, dtype=torch.int32).view(torch.float32), scale)
    return q.reshape(-1)[:n].contiguous(), scale.contiguous()


def block_coef(scale: torch.Tensor, mode: int, w) -> torch.Tensor:
    """The per-block factor c of fa_weighted_sum_q8: scale, or rnd(scale * (float)w) for MUL_W."""
    if mode == N.SUM:
        return scale
    wf = torch.full_like(scale, 0.0) + torch.tensor(float(w), dtype=torch.float64).to(torch.float32)
    return scale * wf


def terms_ref(q: torch.Tensor, scale: torch.Tensor, mode: int, w, block: int) -> torch.Tensor:
    """t_i = rnd((float)q * c) of one client, flat float32."""
    n = q.numel()
    c = block_coef(scale.cpu(), mode, w).repeat_interleave(block)[:n]
    return q.cpu().reshape(-1).to(torch.float32) * c


def sum_ref(qs, scales, mode: int, coef, block: int) -> torch.Tensor:
    """fa_weighted_sum_q8's contract for one segment: clients in order, flat float32."""
    out = None
    for i, (q, s) in enumerate(zip(qs, scales)):
        t = terms_ref(q, s, mode, None if coef is None else coef[i], block)
        out = t if out is None else out + t
    return out


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------
# the restatement against cases worked by hand

def test_restatement_all_zero_block_and_negative_zero():
    x = torch.zeros(32)
    x[3] = -0.0
    x[16:] = torch.tensor([-0.0, 127.0] + [0.0] * 14)
    q, s = quantize_ref(x, 16)
    assert bits(s).tolist() == [0, bits(torch.tensor([1.0])).item()]  # amax = |-0| = +0, +0 / 127 = +0
    assert q.tolist() == [0] * 16 + [0, 127] + [0] * 14  # -0 / 1 = -0 -> 0
    d = sum_ref([q], [s], N.SUM, None, 16)
    assert bits(d)[:17].tolist() == [0] * 17 and d[17] == 127.0


def test_restatement_amax_maps_to_127_and_ties_go_to_even():
    x = torch.zeros(16)
    x[:8] = torch.tensor([127.0, -127.0, 0.5, 1.5, 2.5, -2.5, 3.5, -0.5])  # scale = 1 exactly
    q, s = quantize_ref(x, 16)
    assert s.tolist() == [1.0]
    assert q.tolist()[:8] == [127, -127, 0, 2, 2, -2, 4, 0]
    x = torch.tensor([3.0e-3, -3.0e-3] + [1.0e-3] * 14)  # a scale that is not a power of two
    q, s = quantize_ref(x, 16)
    assert q.tolist()[:2] == [127, -127] and int(q.min()) >= -127


def test_restatement_subnormal_scale_clamps():
    u = 2.0 ** -149
    x = torch.zeros(16, dtype=torch.float64)
    x[:4] = torch.tensor([190.0, -190.0, 100.0, -126.0]) * u
    q, s = quantize_ref(x.to(torch.float32), 16)
    assert bits(s).tolist() == [1]  # rnd(190 / 127 * 2^-149) = 2^-149
    assert q.tolist()[:4] == [127, -127, 100, -126]  # quotients 190, -190, 100, -126: the clamp


def test_restatement_nan_and_inf_blocks():
    x = torch.ones(48)
    x[5] = float("nan")
    x[16 + 9] = float("-inf")
    q, s = quantize_ref(x, 16)
    assert bits(s).tolist()[:2] == [QNAN, QNAN] and s[2] == 1.0 / 127.0
    assert q.tolist() == [0] * 32 + [127] * 16
    d = sum_ref([q], [s], N.SUM, None, 16)
    assert torch.isnan(d[:32]).all() and torch.equal(d[32:], torch.full((16,), 127.0) * (torch.ones(16) / 127.0))


def test_restatement_sum_folds_the_weight_into_the_block_scale_and_keeps_client_order():
    q0 = torch.tensor([3, -5] + [0] * 15, dtype=torch.int8)   # 17 elements: a ragged second block
    q1 = torch.tensor([7, 11] + [0] * 14 + [-127], dtype=torch.int8)
    s0, s1 = torch.tensor([0.1, 0.3]), torch.tensor([0.7, 1e-3])
    w = [0.3, 0.7]
    out = sum_ref([q0, q1], [s0, s1], N.MUL_W, w, 16)
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    c0, c1 = f(0.1) * f(0.3), f(0.7) * f(0.7)
    assert out[0] == f(3.0) * c0 + f(7.0) * c1 and out[1] == f(-5.0) * c0 + f(11.0) * c1
    assert out[16] == f(0.0) * (f(0.3) * f(0.3)) + f(-127.0) * (f(1e-3) * f(0.7))
    assert torch.equal(sum_ref([q0, q1], [s0, s1], N.SUM, None, 16)[:2], torch.stack([f(3.0) * f(0.1) + f(7.0) * f(0.7),
                                                                                      f(-5.0) * f(0.1) + f(11.0) * f(0.7)]))


def test_restatement_takes_the_16_bit_types():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(100, generator=g)
    for dt in (torch.bfloat16, torch.float16):
        q, s = quantize_ref(x.to(dt), 32)
        q2, s2 = quantize_ref(x.to(dt).to(torch.float32), 32)
        assert torch.equal(q, q2) and torch.equal(bits(s), bits(s2)) and s.numel() == 4


# ---------------------------------------------------------------------------------------------------
# symbols and the C ABI's argument checks (no device)

def test_symbols_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fedagg_quant.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(fa_[a-z0-9_]+)\s*\(", src)) == set(N.QUANT_SYMBOLS) == {"fa_quantize_q8",
                                                                                        "fa_weighted_sum_q8"}
    L = N.lib()
    for name in N.QUANT_SYMBOLS:
        assert hasattr(L, name) and getattr(L, name).argtypes
    assert L.fa_abi_version() == 3 == N.ABI_VERSION
    mk = open(os.path.join(ROOT, "fedml_amd", "csrc", "Makefile")).read()
    assert "quant.hip" in mk and "fedagg_quant.h" in mk


class _Abi:
    """Fake tables for the checks that run before any HIP call: nothing here is dereferenced on the
    device, the context is an opaque non-NULL address."""

    def __init__(self, nseg=2, k=2):
        self.L = N.lib()
        self.buf = ctypes.create_string_buffer(4096)
        self.ctx = ctypes.cast(self.buf, ctypes.c_void_p)
        self.nseg, self.k = nseg, k
        self.numel = N.i64_array([100, 5000][:nseg])
        self.q = N.ptr_array([0x10000 + 0x2000 * i + 1 for i in range(nseg * k)])  # any alignment
        self.scale = N.ptr_array([0x80000 + 0x100 * i for i in range(nseg * k)])
        self.out = N.ptr_array([0x100000 + 0x10000 * i for i in range(nseg)])
        self.coef = N.f64_array([0.5] * k)

    def sum(self, **kw):
        a = dict(ctx=self.ctx, mode=N.MUL_W, nseg=self.nseg, numel=self.numel, k=self.k, block=128, q=self.q,
                 scale=self.scale, coef=self.coef, out=self.out)
        a.update(kw)
        rc = self.L.fa_weighted_sum_q8(a["ctx"], a["mode"], a["nseg"], a["numel"], a["k"], a["block"], a["q"],
                                       a["scale"], a["coef"], a["out"], None)
        return rc, self.L.fa_last_error().decode()

    def quant(self, **kw):
        a = dict(ctx=self.ctx, dtype=N.F32, nseg=self.nseg, numel=self.numel, block=128,
                 x=N.ptr_array([0x200000 + 0x10000 * i for i in range(self.nseg)]),
                 q=N.ptr_array([0x10000 + 0x2000 * i + 1 for i in range(self.nseg)]),
                 scale=N.ptr_array([0x80000 + 0x100 * i for i in range(self.nseg)]))
        a.update(kw)
        rc = self.L.fa_quantize_q8(a["ctx"], a["dtype"], a["nseg"], a["numel"], a["block"], a["x"], a["q"],
                                   a["scale"], None)
        return rc, self.L.fa_last_error().decode()


@pytest.mark.parametrize("block", [0, 8, 48, 2048, -16, 1 << 20])
def test_abi_rejects_bad_blocks(block):
    a = _Abi()
    for rc, msg in (a.sum(block=block), a.quant(block=block)):
        assert rc == N.FA_ERR_INVALID and "block" in msg


def test_abi_sum_checks_in_order():
    a = _Abi()
    rc, msg = a.sum(ctx=None, block=0, k=0)
    assert rc == N.FA_ERR_INVALID and "ctx" in msg
    rc, msg = a.sum(block=48, k=0, q=None, coef=None, mode=N.MUL_N_DIV_N)
    assert rc == N.FA_ERR_INVALID and "block" in msg
    for kw in (dict(k=0), dict(nseg=0), dict(k=-1)):
        rc, msg = a.sum(q=None, coef=None, mode=N.MUL_N_DIV_N, **kw)
        assert rc == N.FA_ERR_INVALID and "num_segments" in msg
    for name in ("numel", "q", "scale", "out"):
        rc, msg = a.sum(coef=None, mode=N.MUL_N_DIV_N, **{name: None})
        assert rc == N.FA_ERR_INVALID and "table" in msg, name
    for mode in (N.MUL_W, N.MUL_N_DIV_N, 7):
        rc, msg = a.sum(coef=None, mode=mode)
        assert rc == N.FA_ERR_INVALID and "coef" in msg
    for mode in (N.MUL_N_DIV_N, 7, -1):
        rc, msg = a.sum(mode=mode, out=N.ptr_array([0, 0]))
        assert rc == N.FA_ERR_DTYPE and "mode" in msg


def test_abi_sum_checks_each_non_empty_segment():
    a = _Abi()
    assert a.sum(numel=N.i64_array([100, -1]))[0] == N.FA_ERR_INVALID
    for name, bad in (("q", 0), ("scale", 0), ("scale", 0x80002), ("out", 0), ("out", 0x100002)):
        tab = list(getattr(a, name))
        tab[-1] = bad
        rc, msg = a.sum(**{name: N.ptr_array(tab)})
        assert rc == N.FA_ERR_INVALID and "segment 1" in msg, (name, bad, msg)
        # the same entry in an empty segment is never looked at; with every segment empty nothing is launched
        rc, msg = a.sum(numel=N.i64_array([0, 0]), **{name: N.ptr_array(tab)})
        assert rc == N.FA_OK, (name, bad, msg)
    assert a.sum(numel=N.i64_array([0, 0]), mode=N.SUM, coef=None)[0] == N.FA_OK


def test_abi_quantize_checks_in_order():
    a = _Abi()
    rc, msg = a.quant(ctx=None, block=0)
    assert rc == N.FA_ERR_INVALID and "ctx" in msg
    rc, msg = a.quant(block=8, nseg=0)
    assert rc == N.FA_ERR_INVALID and "block" in msg
    rc, msg = a.quant(nseg=0, x=None, dtype=N.F64)
    assert rc == N.FA_ERR_INVALID and "num_segments" in msg
    for name in ("numel", "x", "q", "scale"):
        rc, msg = a.quant(dtype=N.F64, **{name: None})
        assert rc == N.FA_ERR_INVALID and "table" in msg, name
    for dt in (N.F64, N.I64, 9):
        rc, msg = a.quant(dtype=dt, x=N.ptr_array([0, 0]))
        assert rc == N.FA_ERR_DTYPE and "dtype" in msg
    for name, bad, dt in (("x", 0, N.F32), ("x", 0x200002, N.F32), ("x", 0x200001, N.BF16), ("q", 0, N.F16),
                          ("scale", 0, N.F32), ("scale", 0x80001, N.BF16)):
        tab = [0x200000, 0x210000] if name == "x" else [0x10001, 0x12001] if name == "q" else [0x80000, 0x80100]
        tab[1] = bad
        rc, msg = a.quant(dtype=dt, **{name: N.ptr_array(tab)})
        assert rc == N.FA_ERR_INVALID and "segment 1" in msg, (name, bad, msg)
        assert a.quant(dtype=dt, numel=N.i64_array([0, 0]), **{name: N.ptr_array(tab)})[0] == N.FA_OK
    assert a.quant(dtype=N.BF16, x=N.ptr_array([0x200002, 0x210002]), numel=N.i64_array([0, 0]))[0] == N.FA_OK
    assert a.quant(numel=N.i64_array([5, -2]))[0] == N.FA_ERR_INVALID


# ---------------------------------------------------------------------------------------------------
# Q8Tensor, aggregate_q8 and the operator's routing, with the engine stubbed

from fedml_amd.ml.aggregator import agg_operator as AO  # noqa: E402
from fedml_amd.ml.aggregator import quantized as QZ  # noqa: E402
from fedml_amd.ml.aggregator.quantized import Q8Tensor, aggregate_q8  # noqa: E402


def q8_of(x: torch.Tensor, block: int) -> Q8Tensor:
    q, s = quantize_ref(x, block)
    return Q8Tensor(q.view(x.shape), s, block, tuple(x.shape), x.dtype)


class StubEngine:
    """Stands in for AggEngine.weighted_sum_q8 with the restatement, and records the launches."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def weighted_sum_q8(self, qsegs, ssegs, mode, coef=None, block=128, outs=None, stream=None):
        self.calls.append((len(qsegs), len(qsegs[0]), mode, block))
        return [sum_ref(list(qs), list(ss), mode, coef, block).view(qs[0].shape) for qs, ss in zip(qsegs, ssegs)]


def client_dicts(k=3, block=16):
    g = torch.Generator().manual_seed(11)
    plain, quant = [], []
    for i in range(k):
        sd = OrderedDict([("bn.num_batches_tracked", torch.tensor(10 + i)),
                          ("conv.weight", torch.randn(4, 3, 3, generator=g)),
                          ("fc.weight", torch.randn(5, 7, generator=g).to(torch.bfloat16)),
                          ("steps", torch.tensor([i, 2 * i])),
                          ("fc.bias", torch.randn(7, generator=g))])
        plain.append(sd)
        quant.append(OrderedDict((key, q8_of(v, block) if v.dtype in QZ.Q8_DTYPES else v) for key, v in sd.items()))
    return plain, quant


def test_q8tensor_validates_itself():
    q, s = torch.zeros(20, dtype=torch.int8), torch.zeros(2)
    Q8Tensor(q.view(4, 5), s, 16, (4, 5), torch.float16)
    with pytest.raises(TypeError):
        Q8Tensor(q.to(torch.int16), s, 16, (20,), torch.float32)
    with pytest.raises(TypeError):
        Q8Tensor(q, s.double(), 16, (20,), torch.float32)
    with pytest.raises(TypeError):
        Q8Tensor(q, s, 16, (20,), torch.float64)
    with pytest.raises(ValueError):
        Q8Tensor(q, s, 16, (21,), torch.float32)
    with pytest.raises(ValueError):
        Q8Tensor(q, s, 32, (20,), torch.float32)  # one scale expected


def test_aggregate_q8_key_order_split_and_single_launch(monkeypatch):
    plain, quant = client_dicts()
    w = [0.2, 0.3, 0.5]
    seen = []

    def fake_aggregate(dicts, mode, coef=None, divisor=1.0, engine=None):
        seen.append(([list(d.keys()) for d in dicts], mode, coef))
        return OrderedDict((key, sum(d[key] * c for d, c in zip(dicts, coef))) for key in dicts[0])
    monkeypatch.setattr(QZ, "aggregate", fake_aggregate)
    eng = StubEngine()
    out = aggregate_q8(quant, N.MUL_W, w, engine=eng)
    assert list(out.keys()) == list(plain[0].keys())
    assert eng.calls == [(3, 3, N.MUL_W, 16)]  # the three float keys, one launch
    assert seen == [([["bn.num_batches_tracked", "steps"]] * 3, N.MUL_W, w)]
    for key in ("conv.weight", "fc.weight", "fc.bias"):
        exp = sum_ref([d[key].q.reshape(-1) for d in quant], [d[key].scale for d in quant], N.MUL_W, w, 16)
        exp = exp.view(plain[0][key].shape).to(plain[0][key].dtype)  # one cast, for the bfloat16 key
        assert out[key].dtype == plain[0][key].dtype and out[key].shape == plain[0][key].shape
        assert torch.equal(out[key], exp)
    assert torch.equal(out["steps"], sum(d["steps"] * c for d, c in zip(plain, w)))
    # SUM, and a dict with no plain key: `aggregate` is not called at all
    seen.clear()
    only = [OrderedDict((key, d[key]) for key in ("fc.bias", "conv.weight")) for d in quant]
    out = aggregate_q8(only, N.SUM, engine=eng)
    assert list(out.keys()) == ["fc.bias", "conv.weight"] and not seen and eng.calls[-1] == (2, 3, N.SUM, 16)


def test_aggregate_q8_errors():
    _, quant = client_dicts()
    eng = StubEngine()
    with pytest.raises(IndexError):
        aggregate_q8([], N.SUM, engine=eng)
    with pytest.raises(ValueError):
        aggregate_q8(quant, N.MUL_N_DIV_N, [1, 1, 1], engine=eng)
    # clients disagree on which keys are quantized, either way round
    d = [OrderedDict(x) for x in quant]
    d[1]["fc.bias"] = torch.zeros(7)
    with pytest.raises(TypeError, match="fc.bias"):
        aggregate_q8(d, N.SUM, engine=eng)
    d = [OrderedDict(x) for x in quant]
    d[2]["steps"] = q8_of(torch.zeros(2), 16)
    with pytest.raises(TypeError, match="steps"):
        aggregate_q8(d, N.SUM, engine=eng)
    # block, shape
    d = [OrderedDict(x) for x in quant]
    d[1]["fc.bias"] = q8_of(torch.zeros(7), 32)
    with pytest.raises(ValueError, match="block"):
        aggregate_q8(d, N.SUM, engine=eng)
    d = [OrderedDict(x) for x in quant]
    d[2]["conv.weight"] = q8_of(torch.zeros(3, 4, 3), 16)
    with pytest.raises(ValueError, match="shape"):
        aggregate_q8(d, N.SUM, engine=eng)
    d = [OrderedDict(x) for x in quant]
    for x in d:
        x["fc.bias"] = q8_of(torch.zeros(7), 64)  # every client agrees, the keys do not: one block per launch
    with pytest.raises(ValueError, match="block"):
        aggregate_q8(d, N.SUM, engine=eng)
    assert not eng.calls


def test_agg_routes_quantized_dicts_per_optimizer(monkeypatch):
    plain, quant = client_dicts()
    counts = [10, 30, 60]
    calls = []
    monkeypatch.setattr(AO, "aggregate_q8", lambda dicts, mode, coef=None: calls.append(("q8", mode, coef)) or "Q")
    monkeypatch.setattr(AO, "aggregate", lambda dicts, mode, coef=None: calls.append(("plain", mode, coef)) or "P")
    args = lambda opt: types.SimpleNamespace(federated_optimizer=opt, client_num_in_total=3, client_num_per_round=3)
    w = [n / 100 for n in counts]
    for opt, mode, coef in (("FedAvg", N.MUL_W, w), ("FedProx", N.MUL_W, w), ("FedAvg_seq", N.SUM, None),
                            ("FedDyn", N.SUM, None)):
        calls.clear()
        assert AO.FedMLAggOperator.agg(args(opt), list(zip(counts, quant))) == "Q"
        assert calls == [("q8", mode, coef)]
        calls.clear()
        assert AO.FedMLAggOperator.agg(args(opt), list(zip(counts, plain))) == "P"  # today's path, untouched
        assert calls == [("plain", mode, coef)]
    for opt in ("FedOpt", "FedNova", "nonsense"):
        with pytest.raises(NotImplementedError, match=opt):
            AO.FedMLAggOperator.agg(args(opt), list(zip(counts, quant)))
        with pytest.raises(UnboundLocalError):
            AO.FedMLAggOperator.agg(args(opt), list(zip(counts, plain)))
    for opt in ("SCAFFOLD", "Mime"):
        with pytest.raises(NotImplementedError, match=opt):
            AO.FedMLAggOperator.agg(args(opt), [(n, q, q) for n, q in zip(counts, quant)])
        with pytest.raises(NotImplementedError, match=opt):
            AO.FedMLAggOperator.agg(args(opt), [(n, p, q) for n, p, q in zip(counts, plain, quant)])
    calls.clear()
    AO.FedMLAggOperator.agg(args("Mime"), [(n, p, p) for n, p in zip(counts, plain)])
    assert [c[0] for c in calls] == ["plain", "plain"]


def test_engine_rejects_bad_blocks_before_the_device():
    from fedml_amd.engine import AggEngine
    for b in (0, 8, 48, 2048, 128.5):
        with pytest.raises(ValueError, match="block"):
            AggEngine._check_q8_block("quantize_q8", b)
    assert AggEngine._check_q8_block("quantize_q8", 1024) == 1024
