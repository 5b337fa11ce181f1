"""FoolsGold's device pass fa_pairwise_dot / fa_pairwise_dot_tiled (include/fedagg_robust.h): the history
update bit for bit against a per-op restatement with torch CPU ops in the storage dtype, and the Gram
matrix G against the float64 Gram (numpy, CPU) of the DEVICE'S OWN stored y within the header's derived
bound, so that the bound tests the sums alone:

    |G[i][j] - exact| <= 4e-6 * sqrt(exact_ii * exact_jj)      (1e-12 for float64)

(65 roundings of 2^-24 per run of <= 64 products, then Cauchy-Schwarz: 3.9e-6.)  The shapes are the
smallest at which the kernel can go wrong: client counts at the boundaries of a 4-client block and of
32, one call over segments of [0, 1, 63, 64, 65, 1000, 4099] elements (empty, below / at / above one
float32 run, ragged chunks, more than one workgroup), aligned pointers and pointers one element past a
16-byte boundary.  Every check prints its largest |G - exact| / sqrt(exact_ii exact_jj) as
``pairdot-err``."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_geometric_median import DEV, same_bits, segments, tiled_buf  # noqa: E402

from fedml_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 1000, 4099]
K_ALL = [1, 2, 3, 4, 5, 8, 9, 31, 32, 33, 64, 65, 97, 128]
K_OFFSET = [5, 32, 33, 97]  # every pointer one element past a 16-byte boundary
ALL_DT = [torch.float32, torch.bfloat16, torch.float16, torch.float64]
MODES = [(False, False), (True, False), (False, True), (True, True)]  # (center, history)


def bound(dt):
    return 1e-12 if dt == torch.float64 else 4e-6


@pytest.fixture(scope="module")
def eng():
    from fedml_amd.engine import get_engine
    return get_engine(0)


def scaled_data(g, k, n, dt, positive=False):
    """Normal data, client i scaled by a magnitude drawn log-uniformly from [1e-6, 1e3] (the float16
    top stays below the type's range after two rounds of sums), with zeros and signed zeros."""
    x = torch.randn(k, n, generator=g, dtype=torch.float64)
    if positive:
        x = x.abs() + 0.5  # every product positive: the runs grow, the bound's worst case
    z = torch.rand(k, n, generator=g)
    x[z < 0.02] = 0.0
    x[z > 0.98] = -0.0
    scale = 10.0 ** (torch.rand(k, 1, generator=g, dtype=torch.float64) * 9.0 - 6.0)
    return (x * scale).to(dt)


def restate(x, c, h):
    """The contract's bit-exact part with torch CPU ops in the storage dtype (one rounding per op):
    returns (the new history or None, y)."""
    u = x - c[None, :] if c is not None else x
    if h is None:
        return None, u
    hn = h + u
    return hn, hn


def check_gram(G, y, dt, what):
    """G (device) against the float64 Gram of y (host tensor [k, n]) within the bound; returns the
    largest error on the bound's scale."""
    G = G.cpu()
    k = y.shape[0]
    assert G.dtype == torch.float64 and tuple(G.shape) == (k, k), what
    assert same_bits(G, G.T.contiguous()), what  # both triangles, one bit pattern
    yd = y.double().numpy()
    ref = yd @ yd.T
    scale = np.sqrt(np.outer(np.diag(ref), np.diag(ref)))
    err = np.abs(G.numpy() - ref)
    zero = scale == 0
    assert (G.numpy()[zero] == 0).all(), what  # an all-zero client: exactly zero
    rel = float((err[~zero] / scale[~zero]).max()) if (~zero).any() else 0.0
    print(f"pairdot-err {rel:.3e} {what}")
    assert rel <= bound(dt), (what, rel)
    return rel


def history_bits(got, want, what):
    """The stored history against the restatement, bit for bit; a mismatch names its first elements.
    A NaN of a 16-bit type is compared by position, not by payload: the restatement's own payload there
    is an artefact of the host's conversion (torch's vectorised CPU rounding of a float32 NaN to
    bfloat16 gives 0xffff, its scalar one 0x7fc0), while the device stores the quiet NaN 0x7fc0.
    float32 and float64 NaNs are compared by their bits like every other value."""
    if got.element_size() == 2:
        assert torch.equal(got.isnan(), want.isnan()), what
        got, want = got.clone(), want.clone()
        got[got.isnan()] = 0
        want[want.isnan()] = 0
    if not same_bits(got, want):
        iv = {2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
        gb, wb = got.contiguous().view(iv), want.contiguous().view(iv)
        at = (gb != wb).nonzero()[:5].tolist()
        raise AssertionError(f"{what}: history differs at {at}: got "
                             f"{[hex(int(gb[i, j]) & (2 ** (8 * got.element_size()) - 1)) for i, j in at]}, want "
                             f"{[hex(int(wb[i, j]) & (2 ** (8 * got.element_size()) - 1)) for i, j in at]}")


def cat(segs, i):
    return torch.cat([col[i].reshape(-1) for col in segs]).cpu()


def run_flat(eng, x, c, h, sizes, offset, what):
    """One flat call; checks the inputs and the center are only read, the history bit for bit and G
    within the bound.  Returns (G, the stored history on the host or None)."""
    k = x.shape[0]
    segs = segments(x, sizes, offset)
    cens = None if c is None else [col[0] for col in segments(c[None], sizes, offset)]
    hs = None if h is None else segments(h, sizes, offset)
    G = eng.pairwise_dot(segs, cens, hs)
    torch.cuda.synchronize()
    assert same_bits(torch.stack([cat(segs, i) for i in range(k)]), x), what
    if c is not None:
        assert same_bits(torch.cat([t.reshape(-1) for t in cens]).cpu(), c), what
    href, yref = restate(x, c, h)
    hdev = None
    if h is not None:
        hdev = torch.stack([cat(hs, i) for i in range(k)])
        history_bits(hdev, href, what)
    check_gram(G, hdev if hdev is not None else yref, x.dtype, what)
    return G, hdev


@pytest.mark.parametrize("k", K_ALL)
def test_client_counts_every_mode(eng, k):
    g = torch.Generator().manual_seed(1000 + k)
    n = sum(SIZES)
    for offset in ([0, 1] if k in K_OFFSET else [0]):
        for cen, hist in MODES:
            x = scaled_data(g, k, n, torch.float32)
            c = (0.1 * x[0] + 0.01 * torch.randn(n, generator=g)).float() if cen else None
            h = scaled_data(g, k, n, torch.float32) if hist else None
            run_flat(eng, x, c, h, SIZES, offset, f"k={k} offset={offset} center={cen} history={hist}")


@pytest.mark.parametrize("k", [3, 33])
@pytest.mark.parametrize("dt", ALL_DT, ids=str)
def test_dtypes_every_mode(eng, dt, k):
    g = torch.Generator().manual_seed(2000 + k)
    n = sum(SIZES)
    for offset in (0, 1):
        for cen, hist in MODES:
            x = scaled_data(g, k, n, dt)
            c = (0.1 * x[0].double() + 0.01 * torch.randn(n, generator=g, dtype=torch.float64)).to(dt) if cen else None
            h = scaled_data(g, k, n, dt) if hist else None
            run_flat(eng, x, c, h, SIZES, offset, f"{dt} k={k} offset={offset} center={cen} history={hist}")


@pytest.mark.parametrize("k", [4, 33, 128])
def test_all_positive_input(eng, k):
    """Every product positive: each float32 run grows to its full length's sum, the bound's worst case."""
    g = torch.Generator().manual_seed(3000 + k)
    n = sum(SIZES)
    for dt in (torch.float32, torch.bfloat16):
        x = scaled_data(g, k, n, dt, positive=True)
        run_flat(eng, x, None, None, SIZES, 0, f"positive {dt} k={k}")
        run_flat(eng, x, None, scaled_data(g, k, n, dt, positive=True), SIZES, 0, f"positive {dt} k={k} history")


@pytest.mark.parametrize("dt,k", [(torch.float32, 9), (torch.float16, 33), (torch.float64, 5)], ids=str)
def test_two_rounds_on_one_history(eng, dt, k):
    g = torch.Generator().manual_seed(4000 + k)
    n = sum(SIZES)
    x1, x2 = scaled_data(g, k, n, dt), scaled_data(g, k, n, dt)
    c = (0.05 * torch.randn(n, generator=g, dtype=torch.float64)).to(dt)
    segs1, segs2 = segments(x1, SIZES, 0), segments(x2, SIZES, 1)
    cens = [col[0] for col in segments(c[None], SIZES, 0)]
    hs = segments(torch.zeros(k, n, dtype=dt), SIZES, 0)  # the defense's memory starts at zero
    eng.pairwise_dot(segs1, cens, hs)
    G2 = eng.pairwise_dot(segs2, None, hs)
    torch.cuda.synchronize()
    h1, _ = restate(x1, c, torch.zeros(k, n, dtype=dt))
    h2, _ = restate(x2, None, h1)
    hdev = torch.stack([cat(hs, i) for i in range(k)])
    history_bits(hdev, h2, f"two rounds {dt} k={k}")
    check_gram(G2, hdev, dt, f"two rounds {dt} k={k}")


@pytest.mark.parametrize("tiles", [3, 9], ids=["3E+17", "9E+17"])
@pytest.mark.parametrize("dt,k", [(torch.float32, 3), (torch.float32, 33), (torch.bfloat16, 3), (torch.float16, 33),
                                  (torch.float64, 3), (torch.float64, 33)], ids=str)
def test_tiled_equals_flat(eng, dt, k, tiles):
    """Arena of capacity K + 3, non-consecutive rows, n = tiles E + 17: the history bit for bit the flat
    entry's, G within the bound, in every mode."""
    g = torch.Generator().manual_seed(5000 + k + tiles)
    E = N.TILE_BYTES // torch.empty((), dtype=dt).element_size()
    n = tiles * E + 17
    buf, rows, x, _ = tiled_buf(g, lambda g_, k_, n_, dt_: scaled_data(g_, k_, n_, dt_), k, k + 3, n, dt)
    before = buf.clone()
    for cen, hist in MODES:
        what = f"tiled {dt} k={k} tiles={tiles} center={cen} history={hist}"
        c = (0.1 * x[0].double()).to(dt) if cen else None
        h = scaled_data(g, k, n, dt) if hist else None
        Gf, hflat = run_flat(eng, x, c, h, [n], 0, what + " (flat)")
        cd = None if c is None else c.to(DEV)
        hd = None if h is None else [t.clone() for t in h.to(DEV)]
        Gt = eng.pairwise_dot_tiled(buf, rows, cd, hd, n=n)
        torch.cuda.synchronize()
        assert same_bits(buf, before), what  # the arena is only read
        if hist:
            ht = torch.stack([t.cpu() for t in hd])
            history_bits(ht, hflat, what)
            check_gram(Gt, ht, dt, what)
        else:
            check_gram(Gt, restate(x, c, None)[1], dt, what)


@pytest.mark.parametrize("k", [8, 65])
def test_same_call_same_bits(eng, k):
    g = torch.Generator().manual_seed(6000 + k)
    n = sum(SIZES)
    x, h = scaled_data(g, k, n, torch.float32), scaled_data(g, k, n, torch.float32)
    segs = segments(x, SIZES, 0)
    got = []
    for _ in range(2):
        hs = segments(h, SIZES, 0)  # the same histories again
        got.append((eng.pairwise_dot(segs, None, hs).cpu(), torch.stack([cat(hs, i) for i in range(k)])))
        got.append((eng.pairwise_dot(segs).cpu(), None))
    assert same_bits(got[0][0], got[2][0]) and same_bits(got[0][1], got[2][1])
    assert same_bits(got[1][0], got[3][0])
    for G, _ in got:
        assert same_bits(G, G.T.contiguous())


@pytest.mark.parametrize("k", [5, 40])
def test_zero_client_gives_a_zero_row_and_column(eng, k):
    g = torch.Generator().manual_seed(7000 + k)
    n = sum(SIZES)
    x = scaled_data(g, k, n, torch.float32)
    c = (0.01 * torch.randn(n, generator=g)).float()
    z = k // 2
    x[z] = c  # the update x - c is exactly zero ...
    h = scaled_data(g, k, n, torch.float32)
    h[z] = 0.0  # ... and so is its history
    for cen, hist in MODES:
        xx = x if cen else x.clone()
        if not cen:
            xx[z] = 0.0
        G, _ = run_flat(eng, xx, c if cen else None, h if hist else None, SIZES, 0, f"zero client k={k} {cen} {hist}")
        G = G.cpu()
        assert (G[z] == 0).all() and (G[:, z] == 0).all()
        assert (torch.diagonal(G)[torch.arange(k) != z] > 0).all()


@pytest.mark.parametrize("dt,k", [(torch.float32, 6), (torch.float32, 37), (torch.bfloat16, 6)], ids=str)
def test_non_finite_clients_taint_their_own_row_and_column_only(eng, dt, k):
    g = torch.Generator().manual_seed(8000 + k)
    n = sum(SIZES)
    x, h = scaled_data(g, k, n, dt), scaled_data(g, k, n, dt)
    a, b = 1, k - 2
    x[a, 70] = float("nan")
    x[b, 4000] = float("inf")
    x[b, 4100] = float("-inf")
    segs, hs = segments(x, SIZES, 0), segments(h, SIZES, 0)
    G = eng.pairwise_dot(segs, None, hs).cpu()
    hdev = torch.stack([cat(hs, i) for i in range(k)])
    history_bits(hdev, h + x, f"non-finite {dt} k={k}")  # NaNs included
    assert torch.isnan(hdev[a, 70]) and torch.isinf(hdev[b, 4000])
    bad = torch.zeros(k, dtype=torch.bool)
    bad[[a, b]] = True
    assert not torch.isfinite(G[a]).any() and not torch.isfinite(G[:, a]).any()
    assert not torch.isfinite(G[b, b]) and not torch.isfinite(G[b, ~bad]).any() and not torch.isfinite(G[~bad, b]).any()
    assert torch.isfinite(G[~bad][:, ~bad]).all()
    good = [i for i in range(k) if i not in (a, b)]
    check_gram(G[good][:, good].to(DEV), hdev[good], dt, f"non-finite {dt} k={k}: the finite clients")
    # without a history the non-finite values reach G the same way and nothing else is written
    G0 = eng.pairwise_dot(segs).cpu()
    assert torch.isfinite(G0[~bad][:, ~bad]).all() and not torch.isfinite(torch.diagonal(G0)[bad]).any()


@pytest.mark.parametrize("dt", ALL_DT, ids=str)
def test_all_segments_empty_zeroes_gram(eng, dt):
    k = 5
    segs = [[torch.empty(0, dtype=dt, device=DEV) for _ in range(k)] for _ in range(2)]
    G = eng.pairwise_dot(segs)
    assert same_bits(G.cpu(), torch.zeros(k, k, dtype=torch.float64))
    G = eng.pairwise_dot(segs, [torch.empty(0, dtype=dt, device=DEV)] * 2,
                         [[torch.empty(0, dtype=dt, device=DEV) for _ in range(k)] for _ in range(2)])
    assert same_bits(G.cpu(), torch.zeros(k, k, dtype=torch.float64))
    E = N.TILE_BYTES // torch.empty((), dtype=dt).element_size()
    buf = torch.ones(2, k + 1, E, dtype=dt, device=DEV)
    assert same_bits(eng.pairwise_dot_tiled(buf, list(range(k)), n=0).cpu(), torch.zeros(k, k, dtype=torch.float64))


def test_raw_entry_checks_in_the_documented_order(eng):
    """One bad argument at a time, then pairs of them: the earlier check answers.  Every one of these
    returns before any device work."""
    L, ctx = eng._lib, eng._ctx
    k, n = 3, 100
    x = [torch.ones(n, device=DEV) for _ in range(k)]
    h = [torch.zeros(n, device=DEV) for _ in range(k)]
    c = torch.zeros(n, device=DEV)
    G = torch.empty(k, k, dtype=torch.float64, device=DEV)
    nm = N.i64_array([n])
    need = L.fa_pairwise_dot_scratch_bytes(1, nm, k)
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    good = dict(dtype=N.F32, nseg=1, nm=nm, k=k, d_in=[t.data_ptr() for t in x], stride=4096, cen=[c.data_ptr()],
                hist=[t.data_ptr() for t in h], gram=G.data_ptr(), scratch=scratch.data_ptr(), sbytes=need)

    def call(tiled, **bad):
        a = dict(good, **bad)
        ptrs = lambda v: None if v is None else N.ptr_array(v)  # noqa: E731
        head = (ctx, a["dtype"], a["nseg"], a["nm"], a["k"], ptrs(a["d_in"]))
        tail = (ptrs(a["cen"]), ptrs(a["hist"]), a["gram"], a["scratch"], a["sbytes"], None)
        rc = L.fa_pairwise_dot_tiled(*head, a["stride"], *tail) if tiled else L.fa_pairwise_dot(*head, *tail)
        return rc, L.fa_last_error().decode()

    null_in, null_h = [x[0].data_ptr(), 0, x[2].data_ptr()], [0] + [t.data_ptr() for t in h[1:]]
    for tiled in (False, True):
        name = "fa_pairwise_dot_tiled" if tiled else "fa_pairwise_dot"
        for bad, code, msg in [
                (dict(k=129), N.FA_ERR_INVALID, "invalid arguments (1 <= k <= 128)"),
                (dict(k=0), N.FA_ERR_INVALID, "invalid arguments"),
                (dict(nseg=0), N.FA_ERR_INVALID, "invalid arguments"),
                (dict(nm=None), N.FA_ERR_INVALID, "invalid arguments"),
                (dict(d_in=None), N.FA_ERR_INVALID, "invalid arguments"),
                (dict(gram=None), N.FA_ERR_INVALID, "d_gram is NULL"),
                (dict(dtype=N.I64), N.FA_ERR_DTYPE, "dtype"),
                (dict(nm=N.i64_array([-1])), N.FA_ERR_INVALID, "negative numel"),
                (dict(cen=[0]), N.FA_ERR_INVALID, "segment 0: center NULL"),
                (dict(hist=null_h), N.FA_ERR_INVALID, "segment 0 client 0: history NULL"),
                (dict(d_in=null_in), N.FA_ERR_INVALID, "segment 0 client 1: input NULL"),
                (dict(sbytes=need - 1), N.FA_ERR_INVALID, "scratch must hold"),
                (dict(scratch=None), N.FA_ERR_INVALID, "scratch must hold"),
                # two at a time: the earlier check answers
                (dict(k=129, gram=None), N.FA_ERR_INVALID, "invalid arguments"),
                (dict(gram=None, dtype=N.I64), N.FA_ERR_INVALID, "d_gram is NULL"),
                (dict(dtype=N.I64, cen=[0]), N.FA_ERR_DTYPE, "dtype"),
                (dict(cen=[0], hist=null_h, d_in=null_in), N.FA_ERR_INVALID, "center NULL"),
                (dict(hist=null_h, d_in=null_in), N.FA_ERR_INVALID, "history NULL"),
                (dict(d_in=null_in, sbytes=0), N.FA_ERR_INVALID, "input NULL")]:
            rc, err = call(tiled, **bad)
            assert rc == code and err.startswith(name + ":") and msg in err, (tiled, bad, rc, err)
    for bad, code, msg in [(dict(stride=0), N.FA_ERR_INVALID, "tile_stride must be > 0"),
                           (dict(stride=-4096, k=0), N.FA_ERR_INVALID, "tile_stride must be > 0"),
                           (dict(stride=100), N.FA_ERR_INVALID, "multiple of 4096"),
                           (dict(stride=100, dtype=N.I64), N.FA_ERR_DTYPE, "dtype"),
                           (dict(stride=100, d_in=null_in), N.FA_ERR_INVALID, "multiple of 4096")]:
        rc, err = call(True, **bad)
        assert rc == code and msg in err, (bad, rc, err)
    torch.cuda.synchronize()
    assert (torch.stack(h) == 0).all()  # nothing ran


def test_engine_argument_checks(eng):
    k, n = 3, 50
    x = [[torch.ones(n, device=DEV) for _ in range(k)]]
    h = [[torch.zeros(n, device=DEV) for _ in range(k)]]
    c = [torch.zeros(n, device=DEV)]
    with pytest.raises(ValueError, match="at most 128"):
        eng.pairwise_dot([[x[0][0]] * 129])
    with pytest.raises(ValueError, match="no client"):
        eng.pairwise_dot([[]])
    with pytest.raises(TypeError, match="unsupported dtype"):
        eng.pairwise_dot([[t.long() for t in x[0]]])
    with pytest.raises(ValueError, match="mismatch"):
        eng.pairwise_dot([[x[0][0], x[0][1], x[0][2].double()]])
    with pytest.raises(ValueError, match="clients, expected"):
        eng.pairwise_dot([x[0], x[0][:2]])
    with pytest.raises(ValueError):
        eng.pairwise_dot([[t.cpu() for t in x[0]]])
    with pytest.raises(ValueError, match="one center per segment"):
        eng.pairwise_dot(x, c + c)
    with pytest.raises(ValueError, match="center must be"):
        eng.pairwise_dot(x, [c[0][:10]])
    with pytest.raises(ValueError, match="one list of histories per segment"):
        eng.pairwise_dot(x, None, h + h)
    with pytest.raises(ValueError, match="2 histories, expected 3"):
        eng.pairwise_dot(x, None, [h[0][:2]])
    with pytest.raises(ValueError, match="history must be a contiguous"):
        eng.pairwise_dot(x, None, [[h[0][0], h[0][1], h[0][2].half()]])
    with pytest.raises(ValueError, match="history must be a contiguous"):
        eng.pairwise_dot(x, None, [[h[0][0], h[0][1], torch.zeros(2 * n, device=DEV)[::2]]])
    with pytest.raises(ValueError, match="aliases"):
        eng.pairwise_dot(x, None, [[h[0][0], h[0][1], x[0][2]]])  # an input
    with pytest.raises(ValueError, match="aliases"):
        eng.pairwise_dot(x, c, [[h[0][0], h[0][1], c[0]]])  # the center
    with pytest.raises(ValueError, match="aliases"):
        eng.pairwise_dot(x, None, [[h[0][0], h[0][1], h[0][0]]])  # another history
    big = torch.zeros(2 * n, device=DEV)
    with pytest.raises(ValueError, match="aliases"):
        eng.pairwise_dot(x, None, [[h[0][0], big[:n], big[n - 1:2 * n - 1]]])  # overlapping by one element
    E = N.TILE_BYTES // 4
    buf = torch.ones(2, 140, E, device=DEV)
    with pytest.raises(ValueError, match="at most 128"):
        eng.pairwise_dot_tiled(buf, list(range(129)))
    with pytest.raises(IndexError):
        eng.pairwise_dot_tiled(buf, [0, 140])
    with pytest.raises(TypeError):
        eng.pairwise_dot_tiled(buf.long(), [0, 1])
    with pytest.raises(ValueError, match="center must be"):
        eng.pairwise_dot_tiled(buf, [0, 1], torch.zeros(5, device=DEV))
    with pytest.raises(ValueError, match="2 histories|1 histories"):
        eng.pairwise_dot_tiled(buf, [0, 1], None, [torch.zeros(2 * E, device=DEV)])
    with pytest.raises(ValueError, match="aliases"):
        eng.pairwise_dot_tiled(buf, [0, 1], None, [torch.zeros(2 * E, device=DEV), buf.view(-1)[:2 * E]])
    torch.cuda.synchronize()
    assert all((t == 0).all() for t in h[0])  # no rejected call touched a history
