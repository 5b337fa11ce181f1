"""Exact inputs for the two kernel families that add per-workgroup float64 partial sums in a second
kernel -- FoolsGold's pairwise dot (fedml_amd/csrc/pairdot.hip) and the fused sum-and-distance pass of
the geometric median and centered clipping (fedml_amd/csrc/wsum_dist.hip) -- with the layouts that take
them past one chunk per workgroup and the plain integer references they are held against.  No tests
here: tests/test_chunk_cases_cpu.py checks the tables, the layouts and the restated layout facts,
tests/test_gpu_pairwise_dot_exact.py and tests/test_gpu_sum_sqdist_exact.py run the HIP kernels over
them.  The generic layout helpers are tests/krumcases.py's.  Everything is built in code.

Pairwise dot, why the results are exact.  x, the centre c and the history h hold integers in
[-15, 15]: u = x - c has |u| <= 30 and y = h + u has |y| <= 45, exact in float32, float16, bfloat16
(integers up to 256) and float64; a product is at most 2,025, a float32 run of at most 64 of them
(kPE) sums to at most 129,600 < 2^24, and the sums across runs, slices, workgroups and lanes are
float64 integers below 2^53.  So the stored history is the integer h + u and G is the integer Gram of
y, bit for bit, whatever the order; a lost, doubled or misrouted coordinate changes it.  The same
tables times 2^s stay exact while nothing leaves the type's range (G is the integer Gram times
2^(2s)): a flushed subnormal, a stray rescale or an early overflow changes the bits.  The one-hot
table (client i holds a_i = 1 + i % 13 at one coordinate p_i dealt from the layout's boundaries)
makes G = diag(a_i^2): a wrong diagonal entry names the lost position, a non-zero one off the
diagonal a misrouted LDS column.

The run-length table tests the documented rule "float32 runs of <= 64 coordinates, then float64"
itself: even clients hold 545 everywhere, odd clients 481, both exact in float16, and
545 * 481 = 262,145 = 2^18 + 1.  m * 262,145 is a float32 value for every m <= 64 (m = 64 gives
2^24 + 64) and is not one for m = 65, and a sequential float32 sum of L copies is exact if and only
if L <= 64 (simulated for L = 1..1024 in the CPU test).  So G[even][odd] = n * 262,145 exactly under
the rule, and a run that grows past 64 coordinates misses it.  bfloat16 is left out: 545 is not a
bfloat16 value, and no two integers with 8 significant bits have a product 2^18 + 1.

Sum-and-distance, why the results are exact.  float32 and float64 storage: x and the centre are
integers in [-15, 15], the coefficients are m_i / 256 with positive integers m_i that sum to 256.
Every term x_i c_i (or (x_i - centre) c_i, |x_i - centre| <= 30), every partial sum of out and out
itself is a multiple of 2^-8 of magnitude <= 30: at most 13 significant bits, so every rounding of
the ordered sum is exact.  Every difference x_i - out is a multiple of 2^-8 below 2^6 (exact in
float32), every square a multiple of 2^-16 below 2^12 (exact in float64), and a float64 sum of them
over fewer than 2^23 coordinates stays below 2^53 units of 2^-16.  bfloat16 and float16 storage: x and
the centre in [-3, 3], coefficients m_i / 16 summing to 1: every value is a multiple of 1/16 of
magnitude <= 6, at most 7 significant bits.  So out is the exact rational weighted sum and the 2K
sums are exact integers over 2^16 (2^8), in whatever order rows and lanes are added; a lost or
doubled row of the per-chunk partials changes them.  The one-hot rows (client i non-zero in one chunk
r_i only) give each split and both loops of k_wsd_reduce a named row."""
from __future__ import annotations

import functools

import numpy as np
import torch

from krumcases import (TAIL, boundary_positions, chunk_map, model_sizes, onehot_amplitudes,  # noqa: F401
                       onehot_table, place, segment_of, three_sizes, total)

MAG = 15             # largest magnitude of an entry of x, the centre and the history
KPE = 64             # the header's float32 run length (pairdot.hip: kPE)
DOT_BLOCKS = 1024    # workgroup cap of k_pairdot (kDotBlocks)
ELEM = {torch.float32: 4, torch.bfloat16: 2, torch.float16: 2, torch.float64: 8}
MODES = [(False, False), (True, False), (False, True), (True, True)]  # (centre, history)

# power-of-two scalings by storage dtype.  float32 and bfloat16: products stay within [2^-110,
# 2^111]; float16: 45 * 2^10 = 46,080 is finite and multiples of 2^-24 are float16 subnormals, which
# widen to float32 exactly; float64: far below float32's range
SCALES = {torch.float32: (50, -55), torch.bfloat16: (50, -55), torch.float16: (10, -24), torch.float64: (-300,)}

RUN_EVEN, RUN_ODD = 545, 481      # the run-length table's two values
RUN_PRODUCT = RUN_EVEN * RUN_ODD  # 262,145 = 2^18 + 1

WSD_CHUNK = {torch.float32: 4096, torch.bfloat16: 8192, torch.float16: 8192, torch.float64: 2048}
WSD_SPLITS = 64      # k_wsd_reduce splits the rows 64 ways (kRS), 8 rows of a split per unrolled pass
WSD_NAMED_ROWS = (0, 63, 64, 447, 448, 449, 511, 512, 513)  # and the last row
WSD_MAG = {torch.float32: 15, torch.float64: 15, torch.bfloat16: 3, torch.float16: 3}
WSD_DENOM = {torch.float32: 256, torch.float64: 256, torch.bfloat16: 16, torch.float16: 16}


# ------------------------------------------------------------------ pairwise dot: layout facts
def dot_plan(k: int, dtype) -> dict:
    """pairdot.hip's dot_plan restated: pe (coordinates per chunk), esplit (coordinate slices of a
    chunk), cemax (longest slice), nthreads, ntiles.  The library exposes only the block count of the
    dtype with the smallest chunk (float64's), which tests/test_chunk_cases_cpu.py pins for every K.
    This restatement only steers where boundary positions are placed and how long a layout is: every
    expected value is computed from the data, so a restatement that drifted from the source weakens a
    test (the intended path may no longer be reached) and never makes one fail falsely."""
    sz = ELEM[dtype]
    v, asz = 16 // sz, 8 if sz == 8 else 4
    kp = (k + 3) & ~3
    nb = kp // 4
    ntiles = nb * (nb + 1) // 2
    cap = 256 if ntiles <= 64 else 512
    esplit = max(1, min(KPE, cap // ntiles))
    nthreads = max(256, (ntiles * esplit + 63) // 64 * 64)
    row = asz * (kp + 4)
    lim = min(256, 2 * nthreads * v // k, 64 * 1024 // (2 * row), KPE * esplit)
    pe = v
    while pe * 2 <= lim:
        pe *= 2
    return {"pe": pe, "esplit": esplit, "cemax": -(-pe // esplit), "nthreads": nthreads, "ntiles": ntiles}


def flush_every(k: int, dtype) -> int:
    """Chunks between two in-loop flushes of k_pairdot's float32 sums (run += cemax; flush once
    run + cemax > 64)."""
    cemax = dot_plan(k, dtype)["cemax"]
    chunks, run = 0, 0
    while True:
        chunks, run = chunks + 1, run + cemax
        if run + cemax > KPE:
            return chunks


def dot_blocks(k: int, n: int) -> int:
    """Workgroups of one segment of n coordinates for the dtype with the smallest chunk, read from the
    size of the per-workgroup partials (a host-only call)."""
    from fedml_amd import _native as N
    ntri = k * (k + 1) // 2
    nbytes = int(N.lib().fa_pairwise_dot_scratch_bytes(1, N.i64_array([n]), k))
    assert nbytes > 0 and nbytes % (8 * ntri) == 0, (k, n, nbytes)
    return nbytes // (8 * ntri)


def probe_min_pe(k: int) -> int:
    """The smallest chunk of any dtype at k clients: the smallest n that makes two chunks is pe + 1."""
    lo, hi = 1, 4096
    assert dot_blocks(k, lo) == 1 and dot_blocks(k, hi) >= 2, k
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if dot_blocks(k, mid) >= 2 else (mid, hi)
    return hi - 1


def dot_layouts(k: int, dtype, per_group: int = 4) -> dict:
    """name -> (sizes, aligned flags) of the flat layouts a (k, dtype) case runs: n = total(pe, 1024,
    per_group) coordinates cut like a model (a dozen segments; three for K > 33, where the engine's
    alias check of K histories per segment would dominate the test's time), every segment aligned,
    every segment one element past alignment, and one unaligned segment between aligned ones (the
    model's second large piece, or the three-piece layout's short middle one)."""
    pe = dot_plan(k, dtype)["pe"]
    n = total(pe, DOT_BLOCKS, per_group)
    sizes = model_sizes(n, pe) if k <= 33 else three_sizes(n, pe)
    odd = 5 if k <= 33 else 1
    return {"aligned": (sizes, [True] * len(sizes)), "offset": (sizes, [False] * len(sizes)),
            "mixed": (sizes, [s != odd for s in range(len(sizes))])}


def layout_facts(sizes, pe: int) -> dict:
    """What chunk_map says of a layout: the chunk count, the chunks per workgroup (min, max), the
    workgroups whose run crosses a segment boundary, and those whose run steps from a ragged chunk
    (shorter than pe: the element path) into a whole one."""
    chunks, ranges = chunk_map(sizes, pe, DOT_BLOCKS)
    starts = np.cumsum([0] + list(sizes))
    seg = np.searchsorted(starts, [c[0] for c in chunks], side="right") - 1
    per = [b - a for a, b in ranges]
    cross = sum(any(seg[c] != seg[c - 1] for c in range(a + 1, b)) for a, b in ranges)
    ragged = sum(any(chunks[c - 1][1] < pe and chunks[c][1] == pe for c in range(a + 1, b)) for a, b in ranges)
    return {"pe": pe, "nchunks": len(chunks), "min": min(per), "max": max(per), "cross": cross,
            "ragged_to_whole": ragged}


# ------------------------------------------------------------------ pairwise dot: tables
@functools.lru_cache(maxsize=2)
def dot_tables(k: int, n: int) -> tuple:
    """(x [k, n], c [n], h [k, n]) int8, uniform integers in [-15, 15] from a seeded generator (zeros,
    and with them signed zeros of the differences, included); read only."""
    g = torch.Generator().manual_seed(9000 + k)
    draw = lambda *shape: torch.randint(-MAG, MAG + 1, shape, dtype=torch.int8, generator=g)  # noqa: E731
    return draw(k, n), draw(n), draw(k, n)


def dot_y(x: torch.Tensor, c, h) -> torch.Tensor:
    """The integer y = h + (x - c) of the contract (c, h: given or None), int16."""
    y = x.to(torch.int16)
    if c is not None:
        y = y - c.to(torch.int16)[None, :]
    if h is not None:
        y = y + h.to(torch.int16)
    assert int(y.abs().max()) ** 2 * KPE < 2 ** 24
    return y


def int_gram(y: torch.Tensor, block: int = 1 << 16) -> torch.Tensor:
    """The Gram matrix of an integer table in float64 on the CPU (BLAS), in column blocks: exact,
    whatever the order, while every partial sum is an integer below 2^53."""
    k, n = y.shape
    assert int(y.abs().max()) ** 2 * n < 2 ** 53
    G = torch.zeros((k, k), dtype=torch.float64)
    for lo in range(0, n, block):
        Y = y[:, lo:lo + block].to(torch.float64)
        G += Y @ Y.T
    return G


@functools.lru_cache(maxsize=8)
def dot_reference(k: int, n: int, cen: bool, hist: bool) -> tuple:
    """(y, G) of dot_tables(k, n) in one (centre, history) mode; computed once, shared, never written."""
    x, c, h = dot_tables(k, n)
    y = dot_y(x, c if cen else None, h if hist else None)
    return y, int_gram(y)


def onehot_gram(k: int) -> torch.Tensor:
    """G = diag(a_i^2) of the one-hot table (distinct positions), exact zeros off the diagonal."""
    return torch.diag(onehot_amplitudes(k).double() ** 2)


def run_table(k: int, n: int, dtype, device="cpu") -> torch.Tensor:
    """The run-length table: even clients 545 everywhere, odd clients 481 (float32 / float16)."""
    assert dtype in (torch.float32, torch.float16)
    v = torch.where(torch.arange(k, device=device) % 2 == 0, float(RUN_EVEN), float(RUN_ODD)).to(dtype)
    assert v.double().tolist() == [float(RUN_EVEN if i % 2 == 0 else RUN_ODD) for i in range(k)]
    return v[:, None].expand(k, n).contiguous()


def f32_run_sums(longest: int = 1024) -> np.ndarray:
    """s[L] = the sequential float32 sum of L copies of 262,145, L = 0..longest."""
    s = np.zeros(longest + 1, dtype=np.float32)
    p = np.float32(RUN_PRODUCT)
    for L in range(1, longest + 1):
        s[L] = np.float32(s[L - 1] + p)
    return s


def run_rule_sum(n: int, run: int) -> float:
    """n products of 262,145 added in float32 runs of ``run`` coordinates, the runs in float64."""
    s = f32_run_sums(max(run, 1))
    return float(n // run) * float(s[run]) + float(s[n % run])


def assert_gram_exact(got: torch.Tensor, exp: torch.Tensor, what: str, positions=None) -> None:
    """Bit equality of two K x K float64 matrices and of G's two triangles; a failure names the first
    entries, both values and -- for a one-hot table -- the two clients' coordinates."""
    got = got.detach().cpu()
    assert got.dtype == torch.float64 and exp.dtype == torch.float64 and got.shape == exp.shape, what
    bad = torch.nonzero(got.view(torch.int64) != exp.view(torch.int64))
    if bad.numel():
        lines = []
        for i, j in bad[:8].tolist():
            where = f" (coordinates {positions[i]} and {positions[j]})" if positions is not None else ""
            lines.append(f"G[{i}][{j}]{where}: got {got[i, j].item()!r} expected {exp[i, j].item()!r} "
                         f"(difference {got[i, j].item() - exp[i, j].item()!r})")
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} entries differ\n  " + "\n  ".join(lines))
    assert torch.equal(got.view(torch.int64), got.T.contiguous().view(torch.int64)), f"{what}: not symmetric"


# ------------------------------------------------------------------ sum and distance: layout facts
def wsd_rows_probe(sizes, k: int) -> int:
    """Rows of per-chunk partials for float64 storage (the smallest chunk), from the scratch size."""
    from fedml_amd import _native as N
    nbytes = int(N.lib().fa_weighted_sum_sqdist_scratch_bytes(len(sizes), N.i64_array(list(sizes)), k))
    assert nbytes % (16 * k) == 0, (sizes, k, nbytes)
    return nbytes // (16 * k)


def wsd_chunks(sizes, k: int, dtype) -> int:
    """Rows the sum-and-distance pass writes (one per chunk; a chunk never spans two segments): read
    from the library for float64, sum(ceil(n_s / C)) with C = 4096 / 8192 elements otherwise."""
    if dtype == torch.float64:
        return wsd_rows_probe(sizes, k)
    return sum(-(-s // WSD_CHUNK[dtype]) for s in sizes)


def wsd_single(rows: int, dtype) -> int:
    """Coordinates of one segment of ``rows`` chunks with a ragged last one."""
    return (rows - 1) * WSD_CHUNK[dtype] + TAIL


def wsd_named_rows(rows: int) -> list:
    """The named rows a layout of ``rows`` rows has: each split's first step, the first rows of the
    unrolled loop's last addend (447, 448), the rows around one whole unrolled pass (511 - 513), the
    last row."""
    return sorted({r for r in WSD_NAMED_ROWS if r < rows} | {rows - 1})


def wsd_reduce_steps(rows: int) -> tuple:
    """(unrolled passes, tail steps) of k_wsd_reduce's split 0 and of its last split."""
    out = []
    for rs in (0, WSD_SPLITS - 1):
        b, main, tail = rs, 0, 0
        while b + 7 * WSD_SPLITS < rows:
            b, main = b + 8 * WSD_SPLITS, main + 1
        while b < rows:
            b, tail = b + WSD_SPLITS, tail + 1
        out.append((main, tail))
    return tuple(out)


# ------------------------------------------------------------------ sum and distance: tables
def wsd_coef(k: int, dtype) -> tuple:
    """(m, coef): positive integers m_i summing to 256 (16 for the 16-bit types) and coef_i = m_i / sum."""
    den = WSD_DENOM[dtype]
    assert 1 <= k <= (150 if den == 256 else 16)
    g = torch.Generator().manual_seed(9100 + k)
    m = torch.ones(k, dtype=torch.int64)
    m += torch.bincount(torch.randint(0, k, (den - k,), generator=g), minlength=k)
    assert int(m.sum()) == den and int(m.min()) >= 1
    return m, [int(v) / den for v in m]


@functools.lru_cache(maxsize=2)
def wsd_tables(k: int, n: int, mag: int) -> tuple:
    """(x [k, n], centre [n]) int8, uniform integers in [-mag, mag]; read only."""
    g = torch.Generator().manual_seed(9200 + k)
    return (torch.randint(-mag, mag + 1, (k, n), dtype=torch.int8, generator=g),
            torch.randint(-mag, mag + 1, (n,), dtype=torch.int8, generator=g))


def wsd_onehot_rows(x: torch.Tensor, sizes, dtype, rows) -> torch.Tensor:
    """x with client i zeroed outside the chunk rows[i] (a row of the layout's per-chunk partials)."""
    chunks, _ = chunk_map(sizes, WSD_CHUNK[dtype], 1 << 40)
    assert len(rows) == x.shape[0]
    out = torch.zeros_like(x)
    for i, r in enumerate(rows):
        lo, ln = chunks[r]
        out[i, lo:lo + ln] = x[i, lo:lo + ln]
        out[i, lo] = 1 + i % 3  # never all zero
    return out


def wsd_reference(x: torch.Tensor, cen, m, den: int, mode: str, block: int = 1 << 18) -> tuple:
    """The pass on integers.  x [k, n] int8, cen [n] int8 or None, m [k] int64, coefficients m / den.
    mode "plain": out = sum_i x_i m_i / den; "center": out = cen + sum_i (x_i - cen) m_i / den;
    "dist": out is the centre and nothing is stored.  Returns (O, D2, SS): O = den * out [n] int64 (None
    for "dist"), D2_i = den^2 * sum_e (x_i - out)^2 and SS_i = sum_e x_i^2, both [k] int64, as
    include/fedagg_robust.h defines the 2K sums.  Plain integer tensor arithmetic on x's device (the CPU
    test holds it against the per-op restatement; the GPU tests run it where the table already is)."""
    k, n = x.shape
    O = torch.empty(n, dtype=torch.int64, device=x.device)
    D2 = torch.zeros(k, dtype=torch.int64, device=x.device)
    SS = torch.zeros(k, dtype=torch.int64, device=x.device)
    m32 = m.to(device=x.device, dtype=torch.int32)[:, None]
    for lo in range(0, n, block):
        xb = x[:, lo:lo + block].to(torch.int32)
        if mode == "plain":
            ob = (xb * m32).sum(0, dtype=torch.int32)
        else:
            cb = cen[lo:lo + block].to(torch.int32)
            ob = den * cb if mode == "dist" else den * cb + ((xb - cb[None, :]) * m32).sum(0, dtype=torch.int32)
        d = den * xb - ob[None, :]   # |d| <= 2 * 15 * 256: squares fit int32
        D2 += (d * d).sum(1, dtype=torch.int64)
        SS += (xb * xb).sum(1, dtype=torch.int64)
        O[lo:lo + block] = ob
    return (None if mode == "dist" else O), D2, SS


def wsd_expected_stats(D2: torch.Tensor, SS: torch.Tensor, den: int) -> torch.Tensor:
    """The [2, K] float64 stats of the integer sums: exact while D2 < 2^53."""
    assert int(D2.max()) < 2 ** 53 and int(SS.max()) < 2 ** 53
    return torch.stack([D2.double() / float(den * den), SS.double()]).cpu()


def wsd_restate(x: torch.Tensor, cen, coef, mode: str) -> tuple:
    """The contract per op with torch CPU ops in the storage dtype (one rounding per op; the product
    in the op type -- float32 for the 16-bit types -- with the coefficient cast to it, rounded once).
    x [k, n] and cen [n] in the storage dtype.  Returns (out or None, stats [2, k] float64, sums in
    float64 over differences formed in the op type)."""
    dt = x.dtype
    a = torch.float64 if dt == torch.float64 else torch.float32
    out = None
    if mode != "dist":
        cf = torch.tensor(list(coef), dtype=torch.float64).to(a)
        for i in range(x.shape[0]):
            u = x[i] - cen if mode == "center" else x[i]
            t = (u.to(a) * cf[i]).to(dt)
            out = t if out is None else out + t
        if mode == "center":
            out = cen + out
    ref = cen if mode == "dist" else out
    d = (x.to(a) - ref.to(a)[None, :]).double()
    return out, torch.stack([(d * d).sum(1), (x.double() ** 2).sum(1)])


# ------------------------------------------------------------------ the cases the GPU tests run
F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
DOT_EXACT_CASES = [(F32, k) for k in (3, 9, 33, 65, 88, 97, 128)] + \
                  [(dt, k) for dt in (BF16, F16, F64) for k in (3, 33, 97)]
DOT_OFFSET_KS = (3, 33, 97)  # also every pointer one element past alignment, and the mixed layout
DOT_ONEHOT_CASES = [(dt, k) for dt in (F32, BF16) for k in (5, 33, 128)]
DOT_RUN_CASES = [(F32, 4), (F32, 33), (F32, 128), (F16, 33)]
DOT_TILED_CASES = [(F32, 3), (F32, 33), (BF16, 3)]
DOT_TWO_CALLS = (F32, 9)

WSD_ROWS = (449, 512, 513, 1061)
WSD_CASES = [(F32, 3, p) for p in WSD_ROWS] + [(F32, 32, p) for p in WSD_ROWS] + \
            [(F32, 33, p) for p in WSD_ROWS[:3]] + [(F64, 3, p) for p in WSD_ROWS] + \
            [(F64, 33, p) for p in WSD_ROWS[:3]] + [(dt, k, 513) for dt in (BF16, F16) for k in (3, 16)]
WSD_OFFSET_K = 3             # also every pointer one element past alignment
WSD_MODES = ("plain", "center", "dist")


def dot_case_layouts(dt, k, kind: str) -> list:
    """[(name, sizes, flags)] of the flat layouts one GPU case runs (kind: exact, onehot, run, two)."""
    if kind == "run":
        lay = dot_layouts(k, dt, flush_every(k, dt) + 2)
        return [("aligned",) + lay["aligned"]]
    lay = dot_layouts(k, dt)
    if kind == "exact":
        names = ["aligned"] + (["offset", "mixed"] if k in DOT_OFFSET_KS else [])
    elif kind == "onehot":
        names = ["aligned", "offset"]
    else:
        names = ["aligned", "offset"]
    return [(name,) + lay[name] for name in names]


def wsd_model_sizes(dtype) -> list:
    """A model-like dozen of segments whose rows total more than 1,024, with an empty segment and
    segments shorter than a chunk."""
    ch = WSD_CHUNK[dtype]
    return model_sizes(total(ch, 1024, 1), ch)
