"""CPU references and inputs of the column-sort kernels -- the coordinate-wise trimmed mean and the mean
around the median (fedml_amd/csrc/trimmed.hip) and the coordinate-wise median (median.hip) -- shared by
tests/test_gpu_trimmed_mean.py, tests/test_gpu_mean_around_median.py, tests/test_gpu_robust.py and
tests/test_gpu_column_buckets.py.  No tests here: tests/test_trim_cases_cpu.py pins the references on
hand-computed columns and the order-sensitivity of ``cancel_columns``.

The references follow include/fedagg_robust.h: sort the column (NaN last, -0.0 below +0.0), sum the kept
ranks in rank order in float64 FROM the first kept value, divide, round once per format.  They sort with
``numpy.sort`` and repair one thing: ``numpy.sort`` leaves the order of -0.0 and +0.0 unspecified;
``_order_zeros`` rewrites each sorted column's zero block as the column's -0.0s followed by its +0.0s.

Why ``cancel_columns``.  A float64 sum of at most 128 float32 values of similar size is exact, so on
``randn`` data every summation order gives the same bits and the contract's order is never exercised.
Here p = K // 4 clients hold +H and p hold -H (H >= 2^40, rounded to the dtype first so -H is exact),
the others small values.  A symmetric trim keeps the +-H in pairs; in rank order the sum runs down to
-sum(H), takes the small values rounded at ulp64 of that, and climbs back: what is left depends on when
each term was added.  ``order_share`` measures on how many columns the output bits change when the kept
ranks are summed as two halves and then added -- what a two-lane kernel that added its lanes' partial
sums would compute -- instead of straight through.  float16 cannot hold 2^40; its H lives in 2^4 .. 2^16
and its sums are exact in any order (multiples of 2^-24 below 2^16: 128 of them need 47 bits), so it
checks the sorts and sentinels of every bucket but not the order.
"""
from __future__ import annotations

import numpy as np
import torch

INT_VIEW = {8: torch.int64, 4: torch.int32, 2: torch.int16}
NEG_NAN = torch.tensor([-4194304], dtype=torch.int32).view(torch.float32).item()  # 0xFFC00000


# ----------------------------------------------------------------------------- the references
def _order_zeros(s, a):
    """s: the columns of ``a`` sorted ascending along axis 0 (NaN last).  The zeros of a column are one
    block that starts after its negatives; give the block's first rows the column's -0.0s."""
    zero = s == 0
    start = (s < 0).sum(axis=0)
    nneg = ((a == 0) & np.signbit(a)).sum(axis=0)
    r = np.arange(s.shape[0]).reshape((-1,) + (1,) * (s.ndim - 1))
    s[zero & (r < start + nneg)] = -0.0
    s[zero & (r >= start + nneg)] = 0.0
    return s


def _sorted_columns(xs):
    dt = xs[0].dtype
    a = torch.stack([x.to(torch.float64 if dt == torch.float64 else torch.float32) for x in xs]).numpy()
    return _order_zeros(np.sort(a, axis=0), a)


def _round(q, dt):
    """float64 numpy -> ``dt``: as is, or one rounding to float32 and one more to a 16-bit type."""
    q = torch.from_numpy(q)
    return q if dt == torch.float64 else q.to(torch.float32).to(dt)


def _walk(s, b, dt):
    K = s.shape[0]
    acc = s[b].astype(np.float64).copy()
    with np.errstate(all="ignore"):
        for r in range(b + 1, K - b):
            acc += s[r].astype(np.float64)
        q = torch.from_numpy(acc / float(K - 2 * b))
    return q if dt == torch.float64 else q.to(torch.float32).to(dt)


def trimmed_mean_ref(xs, b):
    return _walk(_sorted_columns(xs), b, xs[0].dtype)


def _window(s, keep):
    """Steps 2-4 of the mean around the median on sorted columns s [K, n]: (m, lo) per column."""
    K = s.shape[0]
    h = (K - 1) // 2
    m = s[h]
    s64, m64 = s.astype(np.float64), s[h].astype(np.float64)
    with np.errstate(all="ignore"):
        d = np.abs(s64 - m64[None])
    d[s == m[None]] = 0.0
    d[np.isnan(s)] = np.inf
    lomin, lomax = max(0, h - keep + 1), min(h, K - keep)
    lo = np.full(s.shape[1], lomin, dtype=np.int64)
    for r in range(lomin, lomax):
        lo += d[r] > d[r + keep]
    return m, lo


def _mam(s, keep, dt):
    m, lo = _window(s, keep)
    cols = np.arange(s.shape[1])
    acc = s[lo, cols].astype(np.float64)
    with np.errstate(all="ignore"):
        for i in range(1, keep):
            acc = acc + s[lo + i, cols].astype(np.float64)
        q = acc / float(keep)
    q[np.isnan(m)] = np.nan
    q = torch.from_numpy(q)
    return q if dt == torch.float64 else q.to(torch.float32).to(dt)


def mam_ref(xs, keep):
    return _mam(_sorted_columns(xs), keep, xs[0].dtype)


def assert_same(got, exp, what=""):
    got, exp = got.cpu(), exp.cpu()
    assert got.dtype == exp.dtype and got.shape == exp.shape, what
    gn, en = torch.isnan(got), torch.isnan(exp)
    assert torch.equal(gn, en), f"{what}: NaN positions differ in {int((gn != en).sum())} elements"
    iv = INT_VIEW[got.element_size()]
    bad = (got.view(iv) != exp.view(iv)) & ~en
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements differ, first at {i}: "
                             f"got {got.flatten()[i].item()!r}, expected {exp.flatten()[i].item()!r}")


# ----------------------------------------------------------------------------- the data
def _column_data(g, k, n, dtype, zeros=0.05):
    """"light": 5 % each of -0.0 and +0.0, 2 % half-integer ties, 0.1 % NaN, 1 % +-inf."""
    xs = []
    for i in range(k):
        v = torch.randn(n, generator=g, dtype=torch.float64)
        u = torch.rand(n, generator=g)
        v = torch.where(u < zeros, torch.zeros_like(v), v)
        v = torch.where((u >= zeros) & (u < 2 * zeros), -torch.zeros_like(v), v)
        v = torch.where((u >= 0.5) & (u < 0.52), torch.round(v * 2) / 2, v)  # ties
        v = torch.where((u >= 0.9) & (u < 0.901), torch.full_like(v, float("nan")), v)
        v = torch.where((u >= 0.95) & (u < 0.96), torch.full_like(v, float("inf")) * torch.sign(v - 0.1), v)
        xs.append(v.to(dtype))
    return xs


def _heavy(g, xs):
    """Rewrites the columns e % 16 in 0..4 of the light data ``xs`` (in place is avoided: new tensors)."""
    k, n = len(xs), xs[0].numel()
    m = torch.stack([x.to(torch.float64) for x in xs])  # [k, n]
    e = torch.arange(n)
    # per column: a random subset of c > k/2 clients (all of them when k < 2)
    rank = torch.rand(k, n, generator=g).argsort(dim=0).argsort(dim=0)
    c = k // 2 + 1 + (torch.rand(n, generator=g) * (k - k // 2)).long().clamp(max=k - k // 2 - 1)
    most = rank < c[None]
    m = torch.where(most & (e % 16 == 0)[None], torch.full_like(m, float("inf")), m)
    m = torch.where(most & (e % 16 == 1)[None], torch.full_like(m, float("-inf")), m)
    m = torch.where(most & (e % 16 == 2)[None], torch.full_like(m, float("nan")), m)
    m = torch.where((e % 16 == 3)[None], m[:1].nan_to_num(1.25, 2.5, -2.5).expand(k, n), m)
    two = torch.where(torch.rand(k, n, generator=g) < 0.5, torch.full_like(m, -0.75), torch.full_like(m, 3.5))
    m = torch.where((e % 16 == 4)[None], two, m)
    out = [row.to(xs[0].dtype).contiguous() for row in m]
    if xs[0].dtype == torch.float32:  # some of the NaNs with the sign bit set
        neg = (rank % 2 == 1) & (e % 16 == 2)[None] & most
        for i in range(k):
            out[i] = torch.where(neg[i], torch.full_like(out[i], NEG_NAN), out[i])
    return out


def _keeps(k):
    return sorted({c for c in (1, 2, 3, k // 2, k - 1, k, k - 2 * (k // 5)) if 1 <= c <= k})


def _special_columns(g, k, n, dtype):
    """Columns mixing normal values with the bit patterns a float-key network could mishandle:
    subnormals of both signs (denormal flushing would change the selected bits), signalling and
    negative / payload NaNs, +-0, +-inf and the largest finite values."""
    fb = dtype
    if dtype == torch.float32:
        pats = [0x00000001, 0x007FFFFF, 0x80000001, 0x807FFFFF, 0x00400000, 0x80400000, 0x7F800001, 0xFFC00000,
                0x7FC12345, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF]
    elif dtype == torch.bfloat16:
        pats = [0x0001, 0x007F, 0x8001, 0x807F, 0x0040, 0x7F81, 0xFFC0, 0x0000, 0x8000, 0x7F80, 0xFF80, 0x7F7F, 0xFF7F]
    else:
        pats = [0x0001, 0x03FF, 0x8001, 0x83FF, 0x0200, 0x7C01, 0xFE00, 0x0000, 0x8000, 0x7C00, 0xFC00, 0x7BFF, 0xFBFF]
    w = (np.uint32, np.int32) if dtype == torch.float32 else (np.uint16, np.int16)
    pats = torch.from_numpy(np.array(pats, dtype=w[0]).view(w[1]))
    xs = []
    for i in range(k):
        v = (torch.randn(n, generator=g) * 1e-3).to(fb)
        u = torch.rand(n, generator=g)
        # most columns: subnormals / extremes only (no NaN) so the network, not the rescan, selects
        sel = torch.randint(0, len(pats), (n,), generator=g)
        special = pats[sel].view(fb)
        nan = (special != special)
        pick = (u < 0.6) & ~nan | (u < 0.002)
        xs.append(torch.where(pick, special, v))
    return xs


# ----------------------------------------------------------------------------- every bucket, order-sensitive sums
def bucket_ks():
    """Both ends of every bucket B = K rounded up to 8: K = 8Q - 7 (seven +inf sentinels) and K = 8Q
    (none; the median's FULL variant), Q = 1..16."""
    return [k for q in range(1, 17) for k in (8 * q - 7, 8 * q)]


def cancel_columns(k, n, dtype, seed):
    """k client tensors of n columns whose kept sums depend on their order (the module docstring):
    p = k // 4 clients hold +H, p hold -H, H = |randn| 2^e + 2^40 with e uniform in 40..60, rounded to
    ``dtype`` before it is negated; the others randn 2^e', e' in 0..10; the clients shuffled
    independently per column.  float16: H = |randn| 2^e + 2^4, e in 4..12, clamped to the largest
    finite value, and e' in -10..0, so the small values stay below every H.  No NaN, no infinity."""
    g = torch.Generator().manual_seed(seed)
    p = k // 4
    f16 = dtype == torch.float16
    e_lo, e_hi = (4, 12) if f16 else (40, 60)
    e = torch.randint(e_lo, e_hi + 1, (p, n), generator=g)
    h = torch.randn(p, n, generator=g, dtype=torch.float64).abs() * torch.exp2(e.double()) + 2.0 ** e_lo
    if f16:
        h = h.clamp(max=torch.finfo(torch.float16).max)
    h = h.to(dtype)
    es = torch.randint(-10 if f16 else 0, 1 if f16 else 11, (k - 2 * p, n), generator=g)
    small = (torch.randn(k - 2 * p, n, generator=g, dtype=torch.float64) * torch.exp2(es.double())).to(dtype)
    m = torch.cat([h, -h, small])
    m = torch.gather(m, 0, torch.rand(k, n, generator=g).argsort(dim=0))
    return [row.contiguous() for row in m]


def _rank_sum(s, lo, cnt):
    """Per column the float64 sum of ranks lo .. lo + cnt - 1 in rank order, from the first."""
    cols = np.arange(s.shape[1])
    acc = s[lo, cols].astype(np.float64)
    with np.errstate(all="ignore"):
        for i in range(1, cnt):
            acc = acc + s[lo + i, cols].astype(np.float64)
    return acc


def order_share(sorted_cols, lo, hi, dtype):
    """The share of columns whose reference output bits (sum / (hi - lo), rounded to ``dtype``) change
    when ranks lo .. hi-1 are summed as two halves, each in rank order, and the halves then added, instead
    of straight through.  ``lo`` and ``hi`` are ints or per-column arrays with one common hi - lo."""
    n = sorted_cols.shape[1]
    lo = np.broadcast_to(np.asarray(lo, dtype=np.int64), (n,))
    cnts = np.unique(np.broadcast_to(np.asarray(hi, dtype=np.int64), (n,)) - lo)
    assert cnts.size == 1 and cnts[0] >= 1
    cnt = int(cnts[0])
    if cnt < 2:
        return 0.0
    half = cnt // 2
    with np.errstate(all="ignore"):
        straight = _rank_sum(sorted_cols, lo, cnt) / float(cnt)
        halves = (_rank_sum(sorted_cols, lo, half) + _rank_sum(sorted_cols, lo + half, cnt - half)) / float(cnt)
    a, b = _round(straight, dtype), _round(halves, dtype)
    iv = INT_VIEW[a.element_size()]
    differ = (a.view(iv) != b.view(iv)) & ~(torch.isnan(a) & torch.isnan(b))
    return float(differ.sum()) / n
