"""OCP Microscaling (mx) updates on the device (include/fedagg_mx.h): fa_weighted_sum_mx and
fa_quantize_mx bit for bit against the plain reference of tests/mx_reference.py, and the state_dict
layer end to end through FedMLAggOperator.agg.  Small sizes take the byte path; S, S + 1 and 2 S + 33
(S = the format's slot) give one, just over one and two-and-a-bit whole slots, odd lengths for the FP4
nibble, ragged blocks and ragged slots; one byte off a 16-byte boundary gives unaligned data and scales,
one float off gives a merely 4-byte aligned output.
"""
from __future__ import annotations

import functools
import os
import sys
import types
from collections import OrderedDict

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mx_reference as R  # noqa: E402

from fedml_amd import _native as N  # noqa: E402
from fedml_amd.ml.aggregator.agg_operator import FedMLAggOperator  # noqa: E402
from fedml_amd.ml.aggregator.microscaled import (MXTensor, mx_dequantize_state_dict,  # noqa: E402
                                                 mx_quantize_state_dict)
from fedml_amd.ml.aggregator.quantized import quantize_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SLOT = {"fp8": N.MX_FP8_SLOT, "fp4": N.MX_FP4_SLOT}
U = N.MX_GROUP
KS = [1, 2, U - 1, U, U + 1, 2 * U + 1]
FMTS = ["fp8", "fp4"]


def seg_lists(fmt):
    s = SLOT[fmt]
    return {"small": [1, 31, 32, 33, 63], "slots": [s, s + 1, 2 * s + 33]}


@pytest.fixture(scope="module")
def eng():
    from fedml_amd.engine import get_engine
    return get_engine(0)


def off_by(t: torch.Tensor, off: int) -> torch.Tensor:
    """A device copy of t whose data starts `off` elements after a 16-byte boundary."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    buf[off:].copy_(t.reshape(-1))
    return buf[off:]


def same_bits(got: torch.Tensor, want: torch.Tensor) -> bool:
    """Bit-equal float32, NaNs by position."""
    gn, wn = torch.isnan(got), torch.isnan(want)
    return bool(torch.equal(gn, wn) and torch.equal(got[~gn].view(torch.int32), want[~wn].view(torch.int32)))


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("fmt", FMTS)
def test_decode_exhaustive(eng, fmt, off):
    """Every scale byte against every element code, on the vector path and on the byte path: this decides
    whether the hardware's scaled conversions may be used as they are.  The codes are rotated by r, so
    that over r every (scale byte, code) pair sits in each of a dword's 4 bytes / 8 nibbles once."""
    for r in range(4 if fmt == "fp8" else 8):
        if fmt == "fp8":  # element e: code (e + r) % 256, X = e // 256 -- 16 whole slots
            n = 256 * 256
            data = np.tile(np.roll(np.arange(256, dtype=np.uint8), -r), 256)
            scale = np.repeat(np.arange(256, dtype=np.uint8), 8)
        else:  # block b: X = b, each of the 16 codes twice, element j holds (j + r) % 16 -- one whole slot
            n = 256 * 32
            codes = np.tile(np.roll(np.arange(16, dtype=np.uint8), -r), 512)
            data = codes[0::2] | (codes[1::2] << 4)
            scale = np.arange(256, dtype=np.uint8)
        got, = eng.weighted_sum_mx([[off_by(torch.from_numpy(data), off)]], [[off_by(torch.from_numpy(scale), off)]],
                                   [n], fmt, N.SUM)
        assert same_bits(got.cpu(), R.decode(data, scale, n, fmt)), r


@functools.lru_cache(maxsize=None)
def sum_inputs(fmt, which):
    """max(KS) clients' (data, scale, decoded row) per segment, from the reference quantizer over
    wide-range data.  Segments of at least 4 blocks get, on blocks that move with the client, a zero
    block, a NaN scale, and scales at each end of the range (E4M3 overflows to Inf at the top)."""
    g = torch.Generator().manual_seed(len(which) + (fmt == "fp4"))
    segs = []
    for n in seg_lists(fmt)[which]:
        rows = []
        for i in range(max(KS)):
            x = torch.randn(n, generator=g) * torch.exp(3 * torch.randn(n, generator=g))
            data, scale = R.quantize(x, fmt)
            nb = scale.size
            if nb >= 4:
                per = 32 if fmt == "fp8" else 16  # data bytes per block
                data[((i + 0) % nb) * per:((i + 0) % nb + 1) * per] = 0
                scale[(i + 1) % nb] = 255
                scale[(i + 2) % nb] = i % 3
                scale[(i + 3) % nb] = 254 - i % 9
            rows.append((data, scale, R.decode(data, scale, n, fmt)))
        segs.append(rows)
    return segs


@pytest.mark.parametrize("out_off", [0, 1], ids=["out16", "out4"])
@pytest.mark.parametrize("off", [0, 1], ids=["data16", "data1"])
@pytest.mark.parametrize("which", ["small", "slots"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("mode", [N.MUL_W, N.SUM], ids=["mul_w", "sum"])
@pytest.mark.parametrize("fmt", FMTS)
def test_sum_bit_exact(eng, fmt, mode, k, which, off, out_off):
    segs = sum_inputs(fmt, which)
    numels = seg_lists(fmt)[which]
    coef = [(i + 1) / 7.3 * (-1) ** i for i in range(k)]  # not dyadic: (float)coef is a rounding
    outs = [off_by(torch.full((n,), 7.0), out_off) for n in numels]
    got = eng.weighted_sum_mx([[off_by(torch.from_numpy(d), off) for d, _, _ in rows[:k]] for rows in segs],
                              [[off_by(torch.from_numpy(s), off) for _, s, _ in rows[:k]] for rows in segs],
                              numels, fmt, mode, coef if mode == N.MUL_W else None, outs=outs)
    for n, rows, o in zip(numels, segs, got):
        assert same_bits(o.cpu(), R.ordered_sum([r[2] for r in rows[:k]], mode == N.MUL_W, coef)), n


def quantizer_data(n, dtype, g):
    """Wide-range data; from 13 blocks on, the first blocks hold the header's edge cases."""
    fi = torch.finfo(dtype)
    x = torch.randn(n, generator=g) * torch.exp((1.0 if dtype == torch.float16 else 3.0) * torch.randn(n, generator=g))
    x[0] = -0.0
    if n >= 13 * 32:
        blk = lambda b: slice(32 * b, 32 * b + 32)  # noqa: E731
        sgn = (-1.0) ** torch.arange(32)
        x[blk(0)] = 0.0 * sgn                                   # zeros and -0
        x[blk(1)][7] = float("nan")
        x[blk(2)][16] = float("-inf")
        x[blk(3)] = torch.randint(-7, 8, (32,), generator=g) * (fi.tiny / 8)  # subnormals
        x[blk(4)][3] = fi.max                                   # the exponent clamp is never reached from above
        x[blk(5)] = torch.rand(32, generator=g) * 2.0 ** -4     # amax exactly a power of two
        x[blk(5)][9] = 2.0 ** -3
        x[blk(6)] = x[blk(5)]                                   # ... and one ulp below it
        x[blk(6)][9] = float(torch.nextafter(torch.tensor(2.0 ** -3, dtype=dtype), torch.tensor(0.0, dtype=dtype)))
        x[blk(7)] = torch.tensor([0.25, 1.25, 2.5, 5, 0.75, 1.75, 3.5, 6] * 4) * 2.0 ** 5 * sgn  # E2M1 ties
        mids = torch.from_numpy((np.abs(R.FP8_VALUES[:0x7E]) + np.abs(R.FP8_VALUES[1:0x7F])) / 2).float()
        x[blk(8)] = torch.cat([mids[0:31], torch.tensor([448.0])]) * 2.0 ** -4 * sgn    # E4M3 ties, subnormal end
        x[blk(9)] = torch.cat([mids[60:91], torch.tensor([448.0])]) * 2.0 ** -4 * sgn   # ... and normal ones
        x[blk(10)] = torch.cat([torch.tensor([7.0, -6.5, 5.0]), torch.rand(29, generator=g)]) * 2.0 ** 3  # 7/6
        x[blk(11)] = torch.cat([torch.tensor([-470.0, 464.0, 432.0]), torch.rand(29, generator=g)]) * 2.0 ** -6
        x[blk(12)] = 0.0                                        # the smallest value alone: E clamps at -127
        x[blk(12)][5] = -fi.smallest_subnormal if hasattr(fi, "smallest_subnormal") else -fi.tiny
    return x.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("fmt", FMTS)
def test_quantizer_byte_exact(eng, fmt, dtype):
    g = torch.Generator().manual_seed(5)
    sizes = [n for ns in seg_lists(fmt).values() for n in ns]
    xs = [quantizer_data(n, dtype, g) for n in sizes]
    epb = 1 if fmt == "fp8" else 2
    # prefilled, so the padding nibble is seen to be written; the outputs of every other segment (the
    # slot + 1 one among them) start one byte off a 16-byte boundary, the last one is aligned throughout
    outs = ([off_by(torch.full((-(-n // epb),), 0xFF, dtype=torch.uint8), 1 - s % 2) for s, n in enumerate(sizes)],
            [off_by(torch.full((-(-n // 32),), 0x55, dtype=torch.uint8), 1 - s % 2) for s, n in enumerate(sizes)])
    got_d, got_s = eng.quantize_mx([x.to(DEV) for x in xs[:5]] + [off_by(x, 8 // x.element_size()) for x in xs[5:6]]
                                   + [x.to(DEV) for x in xs[6:]], fmt, outs=outs)
    for n, x, d, s in zip(sizes, xs, got_d, got_s):
        ed, es = R.quantize(x, fmt)
        assert np.array_equal(s.cpu().numpy(), es), n
        assert np.array_equal(d.cpu().numpy(), ed), n  # an odd n: the last byte's high nibble is 0


def _client_dicts(fmt, k=3):
    g = torch.Generator().manual_seed(11)
    dicts = []
    for i in range(k):
        sd = OrderedDict([("w", torch.randn(37, 250, generator=g) * torch.exp(2 * torch.randn(37, 250, generator=g))),
                          ("steps", torch.tensor(100 + i)),
                          ("b", torch.randn(33, generator=g).to(torch.bfloat16))])
        dicts.append(mx_quantize_state_dict(OrderedDict((key, v.to(DEV)) for key, v in sd.items()), fmt))
    return dicts


@pytest.mark.parametrize("opt", ["FedAvg", "FedAvg_seq"])
@pytest.mark.parametrize("fmt", FMTS)
def test_agg_operator_matches_the_float_route(fmt, opt):
    """The mx round against the existing FLOAT32 route over the decoded dicts.  The decoded bf16 key holds
    its values exactly (a code has at most 4 significant bits), so it is widened to float32 for that route
    and the float32 sum is cast once, as the mx route does; the bf16 route proper rounds every op to bf16."""
    dicts = _client_dicts(fmt)
    assert all(isinstance(d["w"], MXTensor) and isinstance(d["b"], MXTensor) for d in dicts)
    args = types.SimpleNamespace(federated_optimizer=opt)
    counts = [120, 75, 300]
    got = FedMLAggOperator.agg(args, list(zip(counts, dicts)))
    decoded = [mx_dequantize_state_dict(d) for d in dicts]
    assert decoded[0]["b"].dtype == torch.bfloat16 and decoded[0]["w"].shape == (37, 250)
    want = FedMLAggOperator.agg(args, list(zip(counts, [OrderedDict(
        (key, v.float() if v.is_floating_point() else v) for key, v in d.items()) for d in decoded])))
    assert list(got.keys()) == ["w", "steps", "b"]
    for key in got:
        dt = torch.bfloat16 if key == "b" else want[key].dtype
        assert got[key].dtype == dt and got[key].shape == want[key].shape, key
        assert torch.equal(got[key].cpu(), want[key].to(dt).cpu()), key


def test_agg_operator_rejects_mixed_and_disagreeing_rounds():
    args = types.SimpleNamespace(federated_optimizer="FedAvg")
    a, b = _client_dicts("fp8", 2)
    c = _client_dicts("fp4", 1)[0]
    with pytest.raises(TypeError):
        FedMLAggOperator.agg(args, [(1, a), (1, c)])  # FP8 with FP4
    q8 = quantize_state_dict(mx_dequantize_state_dict(b))
    with pytest.raises(TypeError):
        FedMLAggOperator.agg(args, [(1, a), (1, q8)])  # mx with q8
    t = b["w"]
    b["w"] = MXTensor(t.data, t.scale, "fp8", (250, 37), t.dtype)
    with pytest.raises(ValueError):
        FedMLAggOperator.agg(args, [(1, a), (1, b)])
    with pytest.raises(NotImplementedError):
        FedMLAggOperator.agg(types.SimpleNamespace(federated_optimizer="FedOpt"), [(1, a), (1, a)])
