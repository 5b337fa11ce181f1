"""Block-quantized int8 (q8) updates on the device (include/fedagg_quant.h): fa_quantize_q8 and
fa_weighted_sum_q8 bit for bit against the torch-CPU restatement of tests/test_quantized_cpu.py, the
sum also against the existing float32 kernel over the dequantized terms, dequantization, the two
DERIVED error bounds, and the state_dict layer end to end through FedMLAggOperator.agg.

Shapes.  A workgroup owns 4,096 elements of q per client and loads clients in groups of 8.
SEG_LISTS(B) = [1, 15, 16, 17, B-1, B, B+1] (a segment shorter than a block, ragged last blocks, every
slot on the ragged byte path) and [4096, 4097, 2*4096+5] (one, just over one, two-and-a-bit slots: whole
slots take 16-byte loads); B in {16, 128, 1024}; K in {1, 2, 8, 17, 33, 129}; q at byte offsets 0 and 1
(offset 1: every slot on the byte path).  The quantizer's data holds zero blocks, a NaN, an Inf and a
block of subnormals, so the sums also run over NaN scales.

Bounds (derived, not measured; float64 evaluation).  With a normal-range scale s, q = rint(rnd(x / s))
unclamped (|x| <= amax gives |x / s| <= 127 (1 + 2^-23)), the division's rounding error is at most
2^-24 |x / s| <= 128 * 2^-24, rint's is 0.5, and the product rnd(q * s) adds at most 127 * 2^-24 * s:
|x - deq| <= s (0.5 + 255 * 2^-24) < s (0.5 + 2^-16).  The quantized FedAvg against the float64 FedAvg
of the originals adds, per client, the relative errors of (float)w, of c = rnd(s * w) and of
t = rnd(q * c) (3 * 2^-24 each on a value <= w |deq|) and the K - 1 additions (2^-24 each on partial
sums <= sum_i w_i |deq_i|): within sum_i w_i s_i (0.5 + 2^-16) + (K + 2) 2^-23 sum_i w_i |x_i|.
"""
from __future__ import annotations

import functools
import os
import sys
import types
from collections import OrderedDict

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_quantized_cpu import QNAN, bits, quantize_ref, sum_ref, terms_ref  # noqa: E402

from fedml_amd import _native as N  # noqa: E402
from fedml_amd.ml.aggregator.quantized import (Q8Tensor, aggregate_q8, dequantize_state_dict,  # noqa: E402
                                               quantize_state_dict)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SLOT = 4096
BLOCKS = [16, 128, 1024]
KS = [1, 2, 8, 17, 33, 129]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def seg_lists(b):
    return [[1, 15, 16, 17, b - 1, b, b + 1], [SLOT, SLOT + 1, 2 * SLOT + 5]]


@pytest.fixture(scope="module")
def eng():
    from fedml_amd.engine import get_engine
    return get_engine(0)


def coefs(k):
    g = torch.Generator().manual_seed(100 + k)
    n = torch.randint(50, 601, (k,), generator=g).tolist()
    return [v / sum(n) for v in n]


def special_data(sizes, block, dtype, seed):
    """One float tensor per size: wide-range normal data with, somewhere in the list, an all-zero block,
    a block with a NaN, a block with an Inf, a block of subnormals (with the 190-quantum clamp case for
    float32) and a -0.0.  Small segments are specials as a whole, large ones block by block."""
    g = torch.Generator().manual_seed(seed)
    spread = 1.0 if dtype == torch.float16 else 3.0
    quantum = 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -133 if dtype == torch.bfloat16 else 2.0 ** -149
    out = []
    for si, n in enumerate(sizes):
        x = (torch.randn(n, generator=g, dtype=torch.float64) * torch.exp(spread * torch.randn(n, generator=g, dtype=torch.float64)))

        def sub(m):
            v = torch.randint(-189, 190, (m,), generator=g).to(torch.float64)
            v[0] = 190.0
            return v * quantum
        if n >= 4 * block:
            x[:block] = 0.0
            x[1] = -0.0
            x[block + 3] = float("nan")
            x[3 * block - 1] = float("-inf")
            x[3 * block:4 * block] = sub(block)
        elif si % 5 == 1:
            x[:] = 0.0
        elif si % 5 == 2:
            x[0] = float("nan")
        elif si % 5 == 3:
            x[-1] = float("inf")
        elif si % 5 == 4:
            x[:] = sub(n)
        out.append(x.to(torch.float32).to(dtype))
    return out


def wide_data(n, seed):
    """randn * exp(3 randn): no zero, no subnormal-scale block."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * torch.exp(3 * torch.randn(n, generator=g))


def at_offset(t: torch.Tensor, off: int) -> torch.Tensor:
    """t's bytes on the device at byte offset `off` of a fresh (256-byte aligned) allocation."""
    flat = t.reshape(-1)
    buf = torch.empty(flat.numel() * flat.element_size() + 16, dtype=torch.uint8, device=DEV)
    view = buf[off:off + flat.numel() * flat.element_size()].view(flat.dtype)
    view.copy_(flat)
    assert view.data_ptr() % 16 == off
    return view


def same_scales(got: torch.Tensor, exp: torch.Tensor):
    """Bit equality; the NaN scales by position (and they are the contract's quiet NaN)."""
    got = got.cpu()
    nan = torch.isnan(exp)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(bits(got)[~nan], bits(exp)[~nan])
    assert (bits(got)[nan] == QNAN).all()


# ---------------------------------------------------------------------------------------------------
# the quantizer

@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("li", [0, 1])
@pytest.mark.parametrize("block", BLOCKS)
def test_quantizer_bit_equal_to_the_restatement(eng, block, li, dtype):
    sizes = seg_lists(block)[li]
    xs = special_data(sizes, block, dtype, seed=block + li)
    allx = torch.cat([x.float() for x in xs])
    assert torch.isnan(allx).any() and torch.isinf(allx).any() and (allx == 0).any()
    assert ((allx != 0) & (allx.abs() < 2.0 ** -126)).any() or dtype == torch.float16  # float16 subnormals are float32 normals
    for off in (0, 1):  # element offset 1: input and q unaligned, every slot on the element path
        dx = [at_offset(torch.cat([x.new_zeros(off), x]), 0)[off:] for x in xs]
        keep = [d.clone() for d in dx]
        qbuf = [torch.full((n + 16,), 77, dtype=torch.int8, device=DEV) for n in sizes]
        sbuf = [torch.full((-(-n // block) + 2,), 7.0, device=DEV) for n in sizes]
        outs = ([b[off:off + n] for b, n in zip(qbuf, sizes)], [b[1:1 + -(-n // block)] for b, n in zip(sbuf, sizes)])
        qs, scales = eng.quantize_q8(dx, block, outs=outs)
        torch.cuda.synchronize()
        for x, q, s, n in zip(xs, qs, scales, sizes):
            eq, es = quantize_ref(x, block)
            assert torch.equal(q.cpu(), eq)
            same_scales(s, es)
            assert int(q.min()) >= -127
        for b, n in zip(qbuf, sizes):  # nothing written around the outputs
            assert (b[:off] == 77).all() and (b[off + n:] == 77).all()
        for b in sbuf:
            assert b[0] == 7.0 and b[-1] == 7.0
        assert all(torch.equal(bits(a.float()), bits(b.float())) for a, b in zip(dx, keep))  # inputs only read
    # fresh outputs, and twice the same bits
    q1, s1 = eng.quantize_q8([x.to(DEV) for x in xs], block)
    q2, s2 = eng.quantize_q8([x.to(DEV) for x in xs], block)
    for a, b, c, d, x in zip(q1, q2, s1, s2, xs):
        assert a.shape == x.shape and torch.equal(a, b) and torch.equal(bits(c), bits(d))


def test_quantizer_clamp_case_and_hand_blocks(eng):
    u = 2.0 ** -149
    x = torch.zeros(64, dtype=torch.float64)
    x[:4] = torch.tensor([190.0, -190.0, 100.0, -126.0]) * u
    x[16:24] = torch.tensor([127.0, -127.0, 0.5, 1.5, 2.5, -2.5, 3.5, -0.5])
    x[32] = -0.0
    x[48 + 5] = float("nan")
    (q,), (s,) = eng.quantize_q8([x.float().to(DEV)], 16)
    assert q.cpu().tolist()[:4] == [127, -127, 100, -126] and bits(s.cpu()).tolist()[0] == 1
    assert q.cpu().tolist()[16:24] == [127, -127, 0, 2, 2, -2, 4, 0] and s[1] == 1.0
    assert bits(s.cpu()).tolist()[2:] == [0, QNAN] and not q[32:].any()


# ---------------------------------------------------------------------------------------------------
# the sum

@functools.lru_cache(maxsize=2)
def sum_case(block, li, k):
    """K clients' q8 tensors for a segment list, quantized by the restatement from special_data (so NaN,
    zero and subnormal scales take part), and per mode the expected sums and the per-client terms."""
    sizes = seg_lists(block)[li]
    data = [special_data(sizes, block, torch.float32, seed=1000 * k + block + li + 17 * i) for i in range(k)]
    qs = [[None] * k for _ in sizes]
    ss = [[None] * k for _ in sizes]
    for i in range(k):
        for s, x in enumerate(data[i]):
            qs[s][i], ss[s][i] = quantize_ref(x, block)
    w = coefs(k)
    exp, terms = {}, {}
    for mode, coef in ((N.MUL_W, w), (N.SUM, None)):
        terms[mode] = [[terms_ref(qs[s][i], ss[s][i], mode, coef and coef[i], block) for i in range(k)]
                       for s in range(len(sizes))]
        exp[mode] = [sum_ref(qs[s], ss[s], mode, coef, block) for s in range(len(sizes))]
    return sizes, qs, ss, w, exp, terms


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("li", [0, 1])
@pytest.mark.parametrize("block", BLOCKS)
def test_sum_bit_equal_to_the_restatement_and_to_the_float32_kernel(eng, block, li, k):
    sizes, qs, ss, w, exp, terms = sum_case(block, li, k)
    dss = [[s.to(DEV) for s in seg] for seg in ss]
    results = {}
    for off in (0, 1):
        dqs = [[at_offset(q, off) for q in seg] for seg in qs]
        keep_q = [[q.clone() for q in seg] for seg in dqs]
        for mode, coef in ((N.MUL_W, w), (N.SUM, None)):
            got = eng.weighted_sum_q8(dqs, dss, mode, coef, block)
            again = eng.weighted_sum_q8(dqs, dss, mode, coef, block)
            torch.cuda.synchronize()
            for s, n in enumerate(sizes):
                assert got[s].dtype == torch.float32 and got[s].shape == (n,)
                assert torch.equal(bits(got[s].cpu()), bits(exp[mode][s])), (mode, off, s)
                assert torch.equal(bits(got[s]), bits(again[s]))  # deterministic
            results[(off, mode)] = got
        for seg, kseg in zip(dqs, keep_q):  # inputs only read
            assert all(torch.equal(a, b) for a, b in zip(seg, kseg))
    assert all(torch.equal(bits(a), bits(b)) for seg, cseg in zip(dss, ss) for a, b in zip(seg, [c.to(DEV) for c in cseg]))
    # the existing float32 kernel in SUM mode over the terms q.float() * c built on the CPU
    for mode in (N.MUL_W, N.SUM):
        ref = eng.weighted_sum_multi([[t.to(DEV) for t in seg] for seg in terms[mode]], N.SUM)
        for s in range(len(sizes)):
            assert torch.equal(bits(ref[s]), bits(results[(0, mode)][s])), (mode, s)
            assert torch.equal(bits(ref[s]), bits(results[(1, mode)][s])), (mode, s)


@pytest.mark.parametrize("block", BLOCKS)
def test_sum_output_alignment_and_given_outputs(eng, block):
    """A float32 output at element offset 1 (4-byte aligned only) takes element stores: the same bits,
    nothing written around it; an output at 2 bytes is refused."""
    sizes, qs, ss, w, exp, _ = sum_case(block, 1, 8)
    dqs = [[q.to(DEV) for q in seg] for seg in qs]
    dss = [[s.to(DEV) for s in seg] for seg in ss]
    bufs = [torch.full((n + 8,), 5.0, device=DEV) for n in sizes]
    outs = [b[1:1 + n] for b, n in zip(bufs, sizes)]
    got = eng.weighted_sum_q8(dqs, dss, N.MUL_W, w, block, outs=outs)
    for s, (b, n) in enumerate(zip(bufs, sizes)):
        assert got[s].data_ptr() == outs[s].data_ptr()
        assert torch.equal(bits(outs[s].cpu()), bits(exp[N.MUL_W][s]))
        assert b[0] == 5.0 and (b[1 + n:] == 5.0).all()
    L, ctx = N.lib(), eng._ctx
    rc = L.fa_weighted_sum_q8(ctx, N.SUM, 1, N.i64_array([sizes[0]]), 1, block, N.ptr_array([dqs[0][0].data_ptr()]),
                              N.ptr_array([dss[0][0].data_ptr()]), None, N.ptr_array([bufs[0].data_ptr() + 2]), None)
    assert rc == N.FA_ERR_INVALID
    rc = L.fa_weighted_sum_q8(ctx, N.SUM, 1, N.i64_array([sizes[0]]), 1, block, N.ptr_array([dqs[0][0].data_ptr()]),
                              N.ptr_array([dss[0][0].data_ptr() + 2]), None, N.ptr_array([bufs[0].data_ptr()]), None)
    assert rc == N.FA_ERR_INVALID
    with pytest.raises(ValueError):
        eng.weighted_sum_q8(dqs, dss, N.MUL_N_DIV_N, w, block)
    with pytest.raises(ValueError):
        eng.weighted_sum_q8(dqs, dss, N.MUL_W, w, 48)


@pytest.mark.parametrize("li", [0, 1])
@pytest.mark.parametrize("block", BLOCKS)
def test_dequantization_is_the_sum_with_one_client(eng, block, li):
    sizes, qs, ss, _, _, _ = sum_case(block, li, 1)
    got = eng.weighted_sum_q8([[qs[s][0].to(DEV)] for s in range(len(sizes))],
                              [[ss[s][0].to(DEV)] for s in range(len(sizes))], N.SUM, None, block)
    for s, n in enumerate(sizes):
        exp = qs[s][0].float() * ss[s][0].repeat_interleave(block)[:n]
        assert torch.equal(bits(got[s].cpu()), bits(exp))


# ---------------------------------------------------------------------------------------------------
# the derived bounds

@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("block", BLOCKS)
def test_derived_quantization_bounds(eng, block, k):
    sizes = seg_lists(block)[1]
    n = sum(sizes)
    xs = [wide_data(n, seed=7 * k + block + i) for i in range(k)]
    w = coefs(k)
    dx = [[x[o:o + m].to(DEV) for m, o in zip(sizes, (0, sizes[0], sizes[0] + sizes[1]))] for x in xs]
    flat = [t for cl in dx for t in cl]
    qs, scales = eng.quantize_q8(flat, block)
    nseg = len(sizes)
    qseg = [[qs[i * nseg + s] for i in range(k)] for s in range(nseg)]
    sseg = [[scales[i * nseg + s] for i in range(k)] for s in range(nseg)]
    deq = eng.weighted_sum_q8([[q] for q in qs], [[s] for s in scales], N.SUM, None, block)
    avg = eng.weighted_sum_q8(qseg, sseg, N.MUL_W, w, block)
    half = 0.5 + 2.0 ** -16
    worst1 = worst2 = 0.0
    for s, m in enumerate(sizes):
        bound2 = torch.zeros(m, dtype=torch.float64)
        exact = torch.zeros(m, dtype=torch.float64)
        mag = torch.zeros(m, dtype=torch.float64)
        for i in range(k):
            x = dx[i][s].cpu().double()
            sc = scales[i * nseg + s].cpu()
            assert (sc >= 2.0 ** -126).all() and torch.isfinite(sc).all()  # normal-range scales: nothing excluded
            se = sc.double().repeat_interleave(block)[:m]
            err = (x - deq[i * nseg + s].cpu().double()).abs()
            worst1 = max(worst1, float((err / se).max()))
            assert (err <= se * half).all()
            bound2 += w[i] * se * half
            exact += w[i] * x
            mag += w[i] * x.abs()
        bound2 += (k + 2) * 2.0 ** -23 * mag
        err2 = (avg[s].cpu().double() - exact).abs()
        worst2 = max(worst2, float((err2 / bound2).max()))
        assert (err2 <= bound2).all()
    print(f"block {block} k {k}: max |x - deq| / scale = {worst1:.5f}, max FedAvg error / bound = {worst2:.3f}")


# ---------------------------------------------------------------------------------------------------
# the state_dict layer, end to end

def model_dicts(k):
    g = torch.Generator().manual_seed(321)
    out = []
    for i in range(k):
        out.append(OrderedDict([
            ("conv.weight", torch.randn(32, 16, 3, 3, generator=g)),                 # float32, 4608: a slot and a bit
            ("bn.num_batches_tracked", torch.tensor(100 + i)),                        # int64 counter
            ("fc.weight", torch.randn(10, 301, generator=g).to(torch.bfloat16)),      # bfloat16, ragged
            ("fc.bias", torch.randn(10, generator=g))]))
    return out


@pytest.mark.parametrize("opt,mode", [("FedAvg", N.MUL_W), ("FedAvg_seq", N.SUM)])
def test_end_to_end_through_the_operator(eng, opt, mode):
    from fedml_amd.ml.aggregator.agg_operator import FedMLAggOperator
    k, block = 5, 128
    sds = [OrderedDict((key, v.to(DEV)) for key, v in sd.items()) for sd in model_dicts(k)]
    counts = [10, 20, 30, 25, 15]
    w = [c / sum(counts) for c in counts]
    qds = [quantize_state_dict(sd, block) for sd in sds]
    for qd, sd in zip(qds, sds):
        assert list(qd.keys()) == list(sd.keys())
        assert isinstance(qd["conv.weight"], Q8Tensor) and isinstance(qd["fc.weight"], Q8Tensor)
        assert qd["fc.weight"].dtype == torch.bfloat16 and qd["fc.weight"].shape == (10, 301)
        assert qd["bn.num_batches_tracked"] is sd["bn.num_batches_tracked"]
        for key in ("conv.weight", "fc.weight", "fc.bias"):  # the device quantizer == the restatement
            eq, es = quantize_ref(sd[key].cpu(), block)
            assert torch.equal(qd[key].q.cpu().reshape(-1), eq) and torch.equal(bits(qd[key].scale.cpu()), bits(es))
    args = types.SimpleNamespace(federated_optimizer=opt)
    got = FedMLAggOperator.agg(args, list(zip(counts, qds)))
    today = FedMLAggOperator.agg(args, list(zip(counts, sds)))
    direct = aggregate_q8(qds, mode, w if mode == N.MUL_W else None)
    assert list(got.keys()) == list(sds[0].keys())
    coef = w if mode == N.MUL_W else None
    for key in ("conv.weight", "fc.weight", "fc.bias"):
        exp = sum_ref([d[key].q.cpu().reshape(-1) for d in qds], [d[key].scale.cpu() for d in qds], mode, coef, block)
        exp = exp.view(sds[0][key].shape).to(sds[0][key].dtype)
        assert got[key].dtype == sds[0][key].dtype and got[key].shape == sds[0][key].shape
        assert torch.equal(got[key].cpu(), exp) and torch.equal(direct[key].cpu(), exp)
    cnt = "bn.num_batches_tracked"
    assert got[cnt].dtype == today[cnt].dtype and torch.equal(got[cnt].cpu(), today[cnt].cpu())
    # dequantize_state_dict: the k = 1 sum, original shapes and dtypes, the counter untouched
    back = dequantize_state_dict(qds[0])
    for key in ("conv.weight", "fc.weight", "fc.bias"):
        t = qds[0][key]
        exp = (t.q.cpu().reshape(-1).float() * t.scale.cpu().repeat_interleave(block)[:t.numel()]).view(t.shape).to(t.dtype)
        assert back[key].dtype == t.dtype and torch.equal(back[key].cpu(), exp)
    assert back[cnt] is qds[0][cnt]
    with pytest.raises(NotImplementedError, match="FedOpt"):
        FedMLAggOperator.agg(types.SimpleNamespace(federated_optimizer="FedOpt"), list(zip(counts, qds)))
