"""Exact inputs for Krum's pairwise squared distances (fedml_amd/csrc/robust.hip) and the plain
float64 reference they are held against.  No tests here: tests/test_krum_cases_cpu.py pins the
reference to the C oracle on small sizes and checks the tables and layouts themselves,
tests/test_gpu_krum_exact.py runs every form of the kernels over them at the sizes where a workgroup
processes four or five chunks.  Everything is built in code (no fixture files).

Why the results are exact.  The clients hold integers in [-15, 15], so on every path
  differences are integers of magnitude <= 30 (representable in float32, bfloat16 and float16),
  squares are <= 900, and a float32 run of <= 64 coordinates (kPE) sums to <= 57,600 < 2^24;
  Gram form: y = x - c is an integer of magnitude <= 30 (the centre is a median of clients' elements),
  the bf16x3 split holds y in its first part, products are <= 900 and a float32 run of <= 256 of them
  sums to <= 230,400 < 2^24; A_i + A_j - 2 G_ij and every sum across runs are float64 (< 2^53).
So every form must return the exact integer distance, bit for bit, and a dropped or doubled coordinate
changes it.  The same table times 2^s stays exact while nothing leaves the normal range (the
expectation is the integer result times 2^(2s)): a flushed subnormal, a stray rescale or a premature
overflow changes the bits.

The one-hot tables (client i holds a_i = 1 + i % 13 at one coordinate p_i, zero elsewhere; the p_i
distinct, dealt from the boundary positions of the layout) make D_ij = a_i^2 + a_j^2, so a wrong
entry names the pair and with it the lost position."""
from __future__ import annotations

import functools

import numpy as np
import torch

MAG = 15             # largest magnitude of a table entry
RUN = 256            # longest float32 run of any form (Gram, float32 inputs: 256 products)
PAIR_BLOCKS = 1024   # workgroup cap of the direct kernels (pair_split's nblocks)
GRAM_CHUNK = 128     # coordinates per chunk of the Gram kernels (kGE)
GRAM_BLOCKS = 1024   # the largest workgroup cap of the Gram kernels (gram_nblocks; 512 / 256 for K > 32)
F64_CHUNK = 32       # coordinates per chunk of k_pairdist_f64 (kC64)
TAIL = 37            # ragged tail of every total
KPE = 64             # the header's float32 run length of the direct kernels

# power-of-two scalings by difference dtype: squares stay within [2^-110, 2^118] (float32 and
# bfloat16 differences); float16 differences stay representable (30 * 2^11 = 61,440 is finite, the
# smallest are multiples of the smallest float16 subnormal 2^-24); float64 far below float32's range
SCALES = {torch.float32: (50, -55), torch.bfloat16: (50, -55), torch.float16: (11, -24), torch.float64: (-300,)}


# ------------------------------------------------------------------ the library's chunk size
def direct_chunks(K: int, n: int) -> int:
    """Workgroups of the direct kernels for one segment of n coordinates, min(ceil(n / pe), 1024), read
    from the size of their per-workgroup partial sums (a host-only call)."""
    from fedml_amd import _native as N
    pairs = K * (K - 1) // 2
    nbytes = int(N.lib().fa_pairwise_sqdist_scratch_bytes(1, N.i64_array([n]), K))
    assert nbytes > 0 and nbytes % (8 * pairs) == 0, (K, n, nbytes)
    return nbytes // (8 * pairs)


@functools.lru_cache(maxsize=None)
def probe_pe(K: int) -> int:
    """Coordinates per chunk of the direct float32 kernels at K clients: the smallest n that makes two
    chunks is pe + 1."""
    lo, hi = 1, 4096  # one chunk at lo, at least two at hi
    assert direct_chunks(K, lo) == 1 and direct_chunks(K, hi) >= 2, K
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if direct_chunks(K, mid) >= 2 else (mid, hi)
    return hi - 1


def total(chunk: int, cap: int = PAIR_BLOCKS, per_group: int = 4) -> int:
    """Coordinates that give every one of ``cap`` workgroups ``per_group`` or one more chunks."""
    return per_group * cap * chunk + TAIL


# ------------------------------------------------------------------ layouts
def model_sizes(n: int, chunk: int) -> list:
    """n coordinates cut like a model: two large pieces, pieces of 1 and 5, an exact multiple of the
    chunk, an empty segment, a piece shorter than a chunk between two large ones, a ragged last one."""
    a, b, c = (n * 3 // 8) | 1, (n * 2 // 7) | 1, n // 5 + 2
    sizes = [a, 1, 3 * chunk, 5, 0, b, chunk // 2 + 3, c, 2 * chunk + 1, 13, chunk - 1]
    rest = n - sum(sizes)
    assert rest > chunk and rest % chunk != 0, (n, chunk, rest)
    return sizes + [rest]


def three_sizes(n: int, chunk: int) -> list:
    """Three segments: a large odd piece, one shorter than a chunk, the rest."""
    a = (n * 5 // 9) | 1
    return [a, chunk // 2 + 3, n - a - chunk // 2 - 3]


def chunk_map(sizes, chunk: int, cap: int) -> tuple:
    """(chunks, ranges): the (first coordinate, length) of every chunk -- a chunk never spans two
    segments -- and the chunk range [c0, c1) of every workgroup, as the kernels deal them
    (nchunks * b / grid, grid = min(nchunks, cap))."""
    chunks, pos = [], 0
    for s in sizes:
        chunks += [(pos + o, min(chunk, s - o)) for o in range(0, s, chunk)]
        pos += s
    grid = max(1, min(len(chunks), cap))
    return chunks, [(len(chunks) * b // grid, len(chunks) * (b + 1) // grid) for b in range(grid)]


def segment_of(sizes, p: int) -> int:
    """Index of the segment that holds global coordinate p."""
    for s, size in enumerate(sizes):
        if p < size:
            return s
        p -= size
    raise IndexError(p)


def boundary_positions(sizes, chunk: int, cap: int, count: int) -> list:
    """``count`` distinct coordinates dealt from the layout's boundaries: the first coordinate of a
    workgroup's second and third chunk, coordinate 0, the last coordinate of the ragged tail, the first
    and last coordinate of every segment and of a chunk inside a run; then the same chunk positions of
    further workgroups.  Fewer clients than boundaries: a window of the list that moves with count."""
    chunks, ranges = chunk_map(sizes, chunk, cap)
    n = sum(sizes)
    deep = [r for r in ranges if r[1] - r[0] >= 3]
    assert deep, "no workgroup with three chunks"
    first = lambda c: chunks[c][0]
    last = lambda c: chunks[c][0] + chunks[c][1] - 1
    w = deep[len(deep) // 3]
    head = [first(w[0] + 1), first(w[0] + 2), 0, n - 1, last(w[0] + 1), last(w[0])]
    pos = 0
    for s in sizes:
        if s:
            head += [pos, pos + s - 1]
        pos += s
    head = list(dict.fromkeys(head))
    more = []
    for r in deep[::max(1, len(deep) // 64)]:
        more += [first(r[0] + 1), first(r[0] + 2), last(r[1] - 1), last(r[0])]
    if count < len(head):
        r = 3 * count % len(head)
        return [head[(r + j) % len(head)] for j in range(count)]
    out = list(dict.fromkeys(head + more))
    if len(out) < count:  # a small layout: every chunk's first and last coordinate
        out = list(dict.fromkeys(out + [f(c) for c in range(len(chunks)) for f in (first, last)]))
    assert len(out) >= count, (len(out), count)
    return out[:count]


def place(table: torch.Tensor, sizes, aligned, dtype=torch.float32) -> tuple:
    """(buffer, segments): the [K, n] table widened to ``dtype`` on the table's device and cut into
    ``sizes``; segments[s][i] is client i's piece s, a view that starts on a 16-byte boundary
    (aligned) or one element past one -- ``aligned`` is one flag for every piece or one per piece.
    The gaps between the pieces hold NaN: a read outside a piece poisons the result."""
    K, n = table.shape
    assert sum(sizes) == n
    per16 = 16 // torch.empty(0, dtype=dtype).element_size()
    flags = [aligned] * len(sizes) if isinstance(aligned, bool) else list(aligned)
    assert len(flags) == len(sizes)
    offs, cur = [], 0
    for s, al in zip(sizes, flags):
        cur = -(-cur // per16) * per16 + (0 if al else 1)
        offs.append(cur)
        cur += s
    width = -(-(cur + 1) // per16) * per16
    buf = torch.full((K, width), float("nan"), dtype=dtype, device=table.device)
    segs, a = [], 0
    for s, o in zip(sizes, offs):
        buf[:, o:o + s] = table[:, a:a + s]
        segs.append([buf[i, o:o + s] for i in range(K)])
        a += s
    return buf, segs


# ------------------------------------------------------------------ tables
def check_exact(table: torch.Tensor) -> None:
    """The precondition of exactness: (2 max|x|)^2 times the longest float32 run is below 2^24."""
    m = int(table.abs().max()) if table.numel() else 0
    assert (2 * m) ** 2 * RUN < 2 ** 24, m


@functools.lru_cache(maxsize=2)
def dense_table(K: int, n: int) -> torch.Tensor:
    """[K, n] int8, integers in [-15, 15] from a seeded generator (widened on the device); read only."""
    g = torch.Generator().manual_seed(7000 + K)
    t = torch.randint(-MAG, MAG + 1, (K, n), dtype=torch.int8, generator=g)
    check_exact(t)
    return t


def onehot_amplitudes(K: int) -> torch.Tensor:
    return 1 + torch.arange(K) % 13


def onehot_table(K: int, n: int, positions, device="cpu") -> torch.Tensor:
    """[K, n] int8 of zeros but a_i = 1 + i % 13 at client i's coordinate positions[i]."""
    assert len(positions) == K and len(set(positions)) == K and 0 <= min(positions) and max(positions) < n
    t = torch.zeros((K, n), dtype=torch.int8, device=device)
    t[torch.arange(K, device=device), torch.tensor(positions, device=device)] = \
        onehot_amplitudes(K).to(device=device, dtype=torch.int8)
    check_exact(t)
    return t


def onehot_expected(K: int) -> torch.Tensor:
    """D_ij = a_i^2 + a_j^2 off the diagonal (the positions are distinct), float64."""
    a2 = onehot_amplitudes(K).double() ** 2
    d = a2[:, None] + a2[None, :]
    d.fill_diagonal_(0.0)
    return d


# ------------------------------------------------------------------ the reference
def reference(table: torch.Tensor, block: int = 1 << 16) -> torch.Tensor:
    """D = a_i + a_j - 2 X X^T with X the table in float64 on the CPU (BLAS), in column blocks.  Exact
    on integer tables whatever the order: every partial sum is an integer below 2^53."""
    K, n = table.shape
    G = torch.zeros((K, K), dtype=torch.float64)
    for lo in range(0, n, block):
        X = table[:, lo:lo + block].to(torch.float64)
        G += X @ X.T
    a = G.diagonal()
    return a[:, None] + a[None, :] - 2.0 * G


@functools.lru_cache(maxsize=None)
def dense_reference(K: int, n: int) -> torch.Tensor:
    """The reference of dense_table(K, n); computed once, shared by the tests, never written."""
    return reference(dense_table(K, n))


def scaled(expected: torch.Tensor, s: int) -> torch.Tensor:
    """The expectation of the table times 2^s: the integer result times 2^(2s), exactly."""
    return expected * 2.0 ** (2 * s)


# ------------------------------------------------------------------ non-finite inputs
def poisons(K: int) -> dict:
    """name -> [(client, value)]: a NaN in the last real client (next to the padding clients), a +Inf
    in client 0, and +Inf in two clients at the same coordinate."""
    inf, nan = float("inf"), float("nan")
    return {"nan_last": [(K - 1, nan)], "inf_first": [(0, inf)], "inf_pair": [(0, inf), (K // 2, inf)]}


def poison_classes(K: int, poison) -> tuple:
    """(nan, posinf) K x K masks of the distances' classes: float64 arithmetic on the poisoned
    coordinate alone (every other coordinate adds a finite term).  Inf against a finite value gives
    +Inf; Inf against Inf, and anything against NaN, gives NaN."""
    col = np.zeros(K)
    for i, v in poison:
        col[i] = v
    with np.errstate(invalid="ignore"):
        d = col[:, None] - col[None, :]
        sq = d * d
    np.fill_diagonal(sq, 0.0)  # the diagonal is written as zero, not computed
    return torch.from_numpy(np.isnan(sq)), torch.from_numpy(np.isposinf(sq))


# ------------------------------------------------------------------ reporting
def assert_exact(got: torch.Tensor, exp: torch.Tensor, what: str, positions=None) -> None:
    """Bit equality of two K x K float64 matrices, symmetry and a zero diagonal; a failure names the
    first pairs, both values and -- for a one-hot table -- the two clients' coordinates."""
    got = got.detach().cpu()
    assert got.dtype == torch.float64 and exp.dtype == torch.float64 and got.shape == exp.shape, what
    bad = torch.nonzero(got.view(torch.int64) != exp.view(torch.int64))
    if bad.numel():
        lines = []
        for i, j in bad[:8].tolist():
            where = f" (coordinates {positions[i]} and {positions[j]})" if positions is not None else ""
            lines.append(f"D[{i}][{j}]{where}: got {got[i, j].item()!r} expected {exp[i, j].item()!r} "
                         f"(difference {got[i, j].item() - exp[i, j].item()!r})")
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} entries differ\n  " + "\n  ".join(lines))
    assert torch.equal(got.view(torch.int64), got.T.contiguous().view(torch.int64)), f"{what}: not symmetric"
    assert bool((got.diagonal().view(torch.int64) == 0).all()), f"{what}: diagonal not +0.0"
