"""1-bit sign-compressed (q1) updates on the device (include/fedagg_sign.h): fa_quantize_q1,
fa_weighted_sum_q1 and fa_sign_vote_q1 bit for bit against the torch-CPU references of
tests/test_signbits_cpu.py, and the state_dict layer end to end through FedMLAggOperator.agg.
Small sizes take the guarded paths; S (S_v for the vote), S + 1 and 2 S + 37 give one, just over one and
two-and-a-bit whole slots; one word off a 16-byte boundary gives merely 4-byte aligned pointers.
"""
from __future__ import annotations

import os
import sys
import types
from collections import OrderedDict

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_signbits_cpu import bits, count_ref, quantize_ref, sum_ref, unpack_bits, vote_ref  # noqa: E402

from fedml_amd import _native as N  # noqa: E402
from fedml_amd.ml.aggregator.agg_operator import FedMLAggOperator  # noqa: E402
from fedml_amd.ml.aggregator.signcompressed import Q1Tensor, sign_compress_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
S, SV, U = N.Q1_SUM_SLOT, N.Q1_VOTE_SLOT, N.Q1_GROUP
STEP = 0.3  # not dyadic: (float)step is a rounding


@pytest.fixture(scope="module")
def eng():
    from fedml_amd.engine import get_engine
    return get_engine(0)


def off_by(t: torch.Tensor, off: int) -> torch.Tensor:
    """A device copy of t whose data starts `off` words after a 16-byte boundary."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    buf[off:].copy_(t.reshape(-1))
    return buf[off:]


def special_data(sizes, block, dtype, seed):
    """Wide-range data per size; the sizes of at least 5 blocks hold a zero block with a -0.0, a block with
    a NaN, one with an Inf and a subnormal block; every size starts with a -0.0 or a negative value."""
    g = torch.Generator().manual_seed(seed)
    spread = 1.0 if dtype == torch.float16 else 3.0
    out = []
    for n in sizes:
        x = torch.randn(n, generator=g, dtype=torch.float64) * torch.exp(spread * torch.randn(n, generator=g, dtype=torch.float64))
        x[0] = -0.0 if n % 2 else -1.5
        if n >= 5 * block:
            x[:block] = 0.0
            x[3] = -0.0
            x[block + 7] = float("nan")
            x[2 * block + block // 2] = float("-inf")
            x[3 * block:4 * block] = torch.randint(-7, 8, (block,), generator=g).to(torch.float64) * (torch.finfo(dtype).tiny / 8)
        out.append(x.to(dtype))
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("block", [32, 128, 1024])
def test_quantizer_bit_exact(eng, block, dtype):
    sizes = [1, 31, 32, 33, block - 1, block, block + 1, S, S + 1, 2 * S + 37]
    xs = special_data(sizes, block, dtype, seed=block)
    outs = ([torch.full((-(-n // 32),), -1, dtype=torch.int32, device=DEV) for n in sizes],   # padding bits set:
            [torch.full((-(-n // block),), 7.0, device=DEV) for n in sizes])                  # the kernel clears them
    got_b, got_s = eng.quantize_q1([x.to(DEV) for x in xs], block, outs=outs)
    for n, x, b, s in zip(sizes, xs, got_b, got_s):
        eb, es = quantize_ref(x, block)
        assert torch.equal(b.cpu(), eb), n
        assert torch.equal(bits(s.cpu()), bits(es)), n


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("mode", [N.MUL_W, N.SUM], ids=["mul_w", "sum"])
@pytest.mark.parametrize("k,block", [(1, 128), (2, 32), (U, 1024), (U + 1, 128), (2 * U + 1, 32), (129, 128)])
def test_sum_bit_exact(eng, k, block, mode, off):
    sizes = [1, 33, block + 1, S, S + 1, 2 * S + 37]
    g = torch.Generator().manual_seed(k)
    # (a) power-of-two scales and dyadic coefficients: every partial sum is exact, so the float64 sum is the answer
    words = [[torch.randint(-2 ** 31, 2 ** 31, (-(-n // 32),), generator=g).to(torch.int32) for _ in range(k)] for n in sizes]
    scales = [[2.0 ** torch.randint(-3, 4, (-(-n // block),), generator=g).to(torch.float32) for _ in range(k)] for n in sizes]
    coef = None if mode == N.SUM else (torch.randint(1, 9, (k,), generator=g) / 16.0).tolist()
    outs = [off_by(torch.empty(n), off) for n in sizes]
    eng.weighted_sum_q1([[off_by(b, off) for b in seg] for seg in words], [[s.to(DEV) for s in seg] for seg in scales],
                        sizes, mode, coef, block, outs=outs)
    for n, wseg, sseg, o in zip(sizes, words, scales, outs):
        acc = torch.zeros(n, dtype=torch.float64)
        for i in range(k):
            c = sseg[i].double().repeat_interleave(block)[:n] * (1.0 if coef is None else coef[i])
            acc = acc + torch.where(unpack_bits(wseg[i], n), -c, c)
            assert torch.equal(acc.float().double(), acc)  # the reference itself: nothing was rounded
        assert torch.equal(bits(o.cpu()), bits(acc.float())), n
        if k == 1 and mode == N.SUM:  # decompression: +-scale
            assert torch.equal(o.cpu().abs(), sseg[0].repeat_interleave(block)[:n])
            assert torch.equal(torch.signbit(o.cpu()), unpack_bits(wseg[0], n))
    # (b) the quantizer's output on wide-range data, NaN scales included: the op-by-op float32 reference
    xs = [special_data([n] * k, block, torch.float32, seed=n + k) for n in sizes]
    qb, qs = eng.quantize_q1([x.to(DEV) for seg in xs for x in seg], block)
    qb = [qb[j * k:(j + 1) * k] for j in range(len(sizes))]
    qs = [qs[j * k:(j + 1) * k] for j in range(len(sizes))]
    coef = None if mode == N.SUM else [(i % 7 + 1) / (4.1 * k) for i in range(k)]
    outs = [off_by(torch.empty(n), off) for n in sizes]
    eng.weighted_sum_q1([[off_by(b, off) for b in seg] for seg in qb], qs, sizes, mode, coef, block, outs=outs)
    for n, bseg, sseg, o in zip(sizes, qb, qs, outs):
        exp = sum_ref([b.cpu() for b in bseg], [s.cpu() for s in sseg], n, mode, coef, block)
        nan, got = torch.isnan(exp), o.cpu()  # NaN compared as NaN, the rest bit for bit
        assert torch.equal(torch.isnan(got), nan) and torch.equal(bits(got)[~nan], bits(exp)[~nan]), n
        assert n < 5 * block or torch.isnan(exp).any()


thresholds = lambda k: sorted({min(max(t, 1), k) for t in (1, 2, -(-k // 2), k)})  # noqa: E731

@pytest.mark.parametrize("k", [1, 2, 3, 7, 8, 9, 15, 16, 17, 255, 256, 257, 4095])
def test_vote_exact(eng, k):
    sizes = [1, 31, 33, 127, 129, SV, SV + 1, 2 * SV + 37]
    g = torch.Generator(device=DEV).manual_seed(k)
    # the forced columns: all clear, all set, ties, and net = +-t, +-(t - 1) for every threshold of this k
    nets = {k, -k, 0} | {s * v for t in thresholds(k) for v in (t, t - 1) for s in (1, -1)}
    forced = sorted({(k - net) // 2 for net in nets if (k - net) % 2 == 0})
    words, neg = [], []
    for si, n in enumerate(sizes):
        w = torch.randint(-2 ** 31, 2 ** 31, (k, -(-n // 32)), generator=g, device=DEV).to(torch.int32)  # p = 0.5
        for j, c in enumerate(forced):
            e = (j * 4099 + n - 1) % n  # spread over the slots, the segment's last element among them
            m = 1 << (e & 31) if (e & 31) < 31 else -2 ** 31
            w[:c, e >> 5] |= m
            w[c:, e >> 5] &= ~m
        words.append([off_by(w[i], si & 1) for i in range(k)])  # odd segments: one word off a 16-byte boundary
        neg.append(count_ref(list(w.cpu()), n))
        assert n < len(forced) or set(forced) <= set(neg[-1].tolist())  # the forced columns are there
    for t in thresholds(k):
        outs = [off_by(torch.full((n,), 7.0), si & 1) for si, n in enumerate(sizes)]
        eng.sign_vote_q1(words, sizes, t, STEP, outs=outs)
        for n, c, o in zip(sizes, neg, outs):
            assert torch.equal(bits(o.cpu()), bits(vote_ref(c, k, t, STEP))), (n, t)


def test_vote_refuses_more_than_4095_clients(eng):
    b = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.zeros(32, device=DEV)
    rc = N.lib().fa_sign_vote_q1(eng._ctx, 1, N.i64_array([32]), 4096, N.ptr_array([b.data_ptr()] * 4096), 1, 1.0,
                                 N.ptr_array([out.data_ptr()]), None)
    assert rc == N.FA_ERR_INVALID


def test_state_dicts_through_the_operator(eng):
    g = torch.Generator().manual_seed(3)
    k, counts = 5, [10, 30, 60, 25, 75]
    sds = [OrderedDict([("conv.weight", torch.randn(64, 16, 3, 3, generator=g).to(DEV)),          # 9,216: over a slot
                        ("fc.weight", torch.randn(10, 100, generator=g).to(torch.bfloat16).to(DEV)),
                        ("bn.num_batches_tracked", torch.tensor(100 + i, device=DEV)),
                        ("fc.bias", torch.randn(37, generator=g).to(DEV))]) for i in range(k)]  # a ragged block
    comp = [sign_compress_state_dict(sd, 32) for sd in sds]
    fkeys = [key for key, v in comp[0].items() if isinstance(v, Q1Tensor)]
    assert fkeys == ["conv.weight", "fc.weight", "fc.bias"]
    numels = [comp[0][key].numel() for key in fkeys]
    segs = lambda field: [[getattr(d[key], field) for d in comp] for key in fkeys]
    args = lambda opt, **kw: types.SimpleNamespace(federated_optimizer=opt, **kw)
    w = [n / sum(counts) for n in counts]
    for a, exp in ((args("FedAvg"), eng.weighted_sum_q1(segs("bits"), segs("scale"), numels, N.MUL_W, w, 32)),
                   (args("FedAvg_seq"), eng.weighted_sum_q1(segs("bits"), segs("scale"), numels, N.SUM, None, 32)),
                   (args("FedAvg", q1_majority_vote=True, q1_vote_threshold=3, q1_vote_step=STEP),
                    eng.sign_vote_q1(segs("bits"), numels, 3, STEP))):
        out = FedMLAggOperator.agg(a, list(zip(counts, comp)))
        assert list(out.keys()) == list(sds[0].keys())
        for key, e in zip(fkeys, exp):
            ref = sds[0][key]
            assert out[key].dtype == ref.dtype and torch.equal(out[key], e.view(ref.shape).to(ref.dtype)), key
    assert out["bn.num_batches_tracked"].dtype == torch.int64 and out["bn.num_batches_tracked"].item() == sum(100 + i for i in range(k))  # the vote's plain keys: SUM
