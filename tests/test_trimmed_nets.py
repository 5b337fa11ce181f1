"""CPU check of the committed full sorts and bitonic mergers of the trimmed-mean, mean-around-the-median
and two-lane median kernels: SortNet<8 / 16 / 24> and BitonicLo / BitonicHi<36 .. 64> in
fedml_amd/csrc/trimmed_nets.h (tools/gen_trimmed_nets.py), SortNet<32, 36, .., 64> in median_nets.h
(tools/gen_median_nets.py).  The generators check their own op lists as they run; this file evaluates
the TEXT that was committed.

Every network is a formula of min and max, so it commutes with every threshold x -> [x > t] (0-1
principle, which needs no more than monotone gates): it sorts all inputs if it sorts all 0-1 inputs, and
it sorts all inputs of a shape (up-then-down, two sorted halves) if it sorts that shape's 0-1 inputs.

  SortNet<8 / 16 / 24>   every 0-1 input (2^24 of them bit-sliced into uint64 words: min = AND, max = OR).
  BitonicLo / Hi<N>      every 0-1 input of the shape, 0^a 1^b 0^c / 1^a 0^b 1^c, and random bitonic
                         columns with ties.
  SortNet<N>, N >= 32    2^N inputs cannot be enumerated.  The generator's comparator list
                         oddeven_merge_sort(P2), P2 = 32 and 64, is proved by composition: it IS
                         sort(lower half) + sort(upper half) + merge (compared as lists), the 16-key base
                         sorts all 2^16 inputs, and each merge sorts every 0-1 input made of two sorted
                         halves (17 * 17 and 33 * 33 of them).  Folding the P2 - N high sentinels away is
                         running the list with +inf in those slots.  The committed text is then tied to
                         that list: equal outputs on 3 * 2^16 random 0-1 columns (densities 1/8, 1/2,
                         7/8), on every input with at most two ones or at most two zeros, and on random
                         real columns with ties.
"""
from __future__ import annotations

import itertools
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

TRIMMED_HDR = os.path.join(ROOT, "fedml_amd", "csrc", "trimmed_nets.h")
MEDIAN_HDR = os.path.join(ROOT, "fedml_amd", "csrc", "median_nets.h")
MERGES = list(range(36, 65, 4))
BIG_SORTS = [32] + MERGES

sys.path.insert(0, os.path.join(ROOT, "tools"))


# ----------------------------------------------------------------------------- the committed text
def _parse(path):
    """{(struct name, N): statements of run()} for every in-place network ``void run(K (&x)[N])``."""
    src = open(path).read()
    out = {}
    for m in re.finditer(r"template <> struct (\w+)<(\d+)> \{\n[^\n]*static void run\(K \(&x\)\[(\d+)\]\) \{\n(.*?)\n  \}\n\};",
                         src, re.S):
        assert m.group(2) == m.group(3), m.group(0)[:80]
        out[m.group(1), int(m.group(2))] = [l.strip() for l in m.group(4).split("\n")]
    return out


_CACHE = {}


def _nets(path):
    if path not in _CACHE:
        _CACHE[path] = _parse(path)
    return _CACHE[path]


_PAIR = re.compile(r"const K (i\d+) = kmin\(([^,]+), ([^)]+)\), (a\d+) = kmax\(([^,]+), ([^)]+)\);$")
_COPY = re.compile(r"const K (o\d+) = ([^;]+);$")
_BACK = re.compile(r"x\[(\d+)\] = (o\d+);$")


def _run(stmts, x, mn, mx):
    """Evaluates the statements as written on x (a list of N arrays) -- each kmin and each kmax with its
    own operands -- and returns the N outputs.  An unknown statement or operand fails."""
    x = list(x)
    env = {}
    val = lambda t: x[int(t[2:-1])] if t.startswith("x[") else env[t]  # noqa: E731
    stores = False
    for s in stmts:
        m = _PAIR.match(s)
        if m:
            assert not stores, s
            lo, hi = mn(val(m.group(2)), val(m.group(3))), mx(val(m.group(5)), val(m.group(6)))
            assert m.group(1) not in env and m.group(4) not in env, s  # single assignment
            env[m.group(1)], env[m.group(4)] = lo, hi
            continue
        m = _COPY.match(s)
        if m:
            assert not stores and m.group(1) not in env, s
            env[m.group(1)] = val(m.group(2))
            continue
        m = _BACK.match(s)
        assert m, s
        stores = True  # every output was read before the first x[] is overwritten
        x[int(m.group(1))] = env[m.group(2)]
    return x


def _run_real(stmts, cols):
    """cols [N, n] -> the outputs [N, n]."""
    return np.stack(_run(stmts, list(cols), np.minimum, np.maximum))


def _run_list(comps, cols, pad):
    """A comparator list [(i, j)], i takes the min, on cols [N, n] padded to P2 rows with ``pad`` (the
    folded high sentinels); the first N outputs."""
    n_in = cols.shape[0]
    p2 = 1 + max(j for _, j in comps)
    x = list(cols) + [np.full(cols.shape[1], pad, dtype=cols.dtype)] * (p2 - n_in)
    for i, j in comps:
        x[i], x[j] = np.minimum(x[i], x[j]), np.maximum(x[i], x[j])
    return np.stack(x[:n_in])


# ----------------------------------------------------------------------------- 0-1 inputs, bit-sliced
_LOW6 = [0xAAAAAAAAAAAAAAAA, 0xCCCCCCCCCCCCCCCC, 0xF0F0F0F0F0F0F0F0, 0xFF00FF00FF00FF00, 0xFFFF0000FFFF0000,
         0xFFFFFFFF00000000]


def _all_inputs(n):
    """Wire i of all 2^n 0-1 inputs as uint64 words: input v is bit v % 64 of word v // 64."""
    words = max(1, (1 << n) >> 6)
    w = np.arange(words, dtype=np.uint64)
    wires = []
    for i in range(n):
        if i < 6:
            wires.append(np.full(words, _LOW6[i], dtype=np.uint64))
        else:
            wires.append(np.where((w >> np.uint64(i - 6)) & np.uint64(1), np.uint64(2 ** 64 - 1), np.uint64(0)))
    return wires


def _assert_sorts_words(wires, outs, what):
    """outs == the inputs sorted ascending, for 0-1 inputs: rank r is 1 iff more than N - 1 - r inputs
    are.  The count is kept bit-sliced (a ripple-carry add of each wire), then compared per rank."""
    n = len(wires)
    nbits = n.bit_length()
    cnt = [np.zeros_like(wires[0]) for _ in range(nbits)]
    for wv in wires:
        carry = wv
        for b in range(nbits):
            cnt[b], carry = cnt[b] ^ carry, cnt[b] & carry
    full = np.uint64(2 ** 64 - 1)
    for r in range(n):
        t = n - r  # out[r] = [count >= t]: compare the bit-sliced count with the constant, MSB first
        ge, eq = np.zeros_like(wires[0]), np.full_like(wires[0], full)
        for b in reversed(range(nbits)):
            if (t >> b) & 1:
                eq = eq & cnt[b]
            else:
                ge, eq = ge | (eq & cnt[b]), eq & ~cnt[b]
        ge = ge | eq
        assert np.array_equal(outs[r], ge), f"{what}: rank {r} is wrong on some 0-1 input"


# ----------------------------------------------------------------------------- presence
def test_all_networks_present():
    t, m = _nets(TRIMMED_HDR), _nets(MEDIAN_HDR)
    assert sorted(n for s, n in t if s == "SortNet") == [8, 16, 24]
    assert sorted(n for s, n in t if s == "BitonicLo") == MERGES
    assert sorted(n for s, n in t if s == "BitonicHi") == MERGES
    assert sorted(n for s, n in m if s == "SortNet") == BIG_SORTS
    assert {s for s, _ in t} == {"SortNet", "BitonicLo", "BitonicHi"} and {s for s, _ in m} == {"SortNet"}


# ----------------------------------------------------------------------------- SortNet<8 / 16 / 24>
@pytest.mark.parametrize("N", [8, 16, 24])
def test_small_sort_on_every_01_input(N):
    stmts = _nets(TRIMMED_HDR)["SortNet", N]
    wires = _all_inputs(N)
    outs = _run(stmts, wires, np.bitwise_and, np.bitwise_or)
    _assert_sorts_words(wires, outs, f"SortNet<{N}>")


def test_bit_sliced_check_catches_a_wrong_network():
    """The checker itself: a sorted-but-wrong output (all minima) and an unsorted one must both fail."""
    wires = _all_inputs(8)
    good = _run(_nets(TRIMMED_HDR)["SortNet", 8], wires, np.bitwise_and, np.bitwise_or)
    _assert_sorts_words(wires, good, "SortNet<8>")
    with pytest.raises(AssertionError):
        _assert_sorts_words(wires, [good[0]] * 8, "all minima")
    with pytest.raises(AssertionError):
        _assert_sorts_words(wires, good[:3] + [good[4], good[3]] + good[5:], "two ranks swapped")
    ref = np.sort(np.array([[(v >> i) & 1 for v in range(256)] for i in range(8)], dtype=np.uint8), axis=0)
    bits = np.array([[(int(good[r][v // 64]) >> (v % 64)) & 1 for v in range(256)] for r in range(8)], dtype=np.uint8)
    assert np.array_equal(bits, ref)


# ----------------------------------------------------------------------------- the mergers
def _bitonic_01(N, hi):
    cols = [[hi] * a + [not hi] * b + [hi] * (N - a - b) for a in range(N + 1) for b in range(N + 1 - a)]
    return np.array(cols, dtype=np.float64).T


def _bitonic_random(N, hi, cols=2048):
    rng = np.random.default_rng(4000 + 2 * N + hi)
    x = rng.integers(0, 9, size=(N, cols)).astype(np.float64)  # heavy ties
    x[:, : cols // 2] = rng.standard_normal((N, cols // 2)).astype(np.float32)
    cut = rng.integers(0, N + 1, size=cols)
    for c in range(cols):
        up, down = np.sort(x[:cut[c], c]), np.sort(x[cut[c]:, c])[::-1]
        x[:, c] = np.concatenate([down, up]) if hi else np.concatenate([up, down])
    return x


@pytest.mark.parametrize("hi", [False, True], ids=["Lo", "Hi"])
@pytest.mark.parametrize("N", MERGES)
def test_merger_on_every_01_input_of_its_shape(N, hi):
    stmts = _nets(TRIMMED_HDR)["BitonicHi" if hi else "BitonicLo", N]
    x = _bitonic_01(N, hi)
    assert x.shape == (N, (N + 1) * (N + 2) // 2)
    assert np.array_equal(_run_real(stmts, x), np.sort(x, axis=0))
    x = _bitonic_random(N, hi)
    assert np.array_equal(_run_real(stmts, x), np.sort(x, axis=0))


# ----------------------------------------------------------------------------- SortNet<N>, N >= 32
def _shift(comps, d):
    return [(i + d, j + d) for i, j in comps]


def test_merge_sort_list_is_two_sorts_and_a_merge():
    """Steps 1-3 of the composition argument, for P2 = 32 and 64."""
    from gen_median_nets import G16, oddeven_merge_sort
    base = oddeven_merge_sort(16)
    assert base == list(G16)
    wires = _all_inputs(16)
    x = list(wires)
    for i, j in base:
        x[i], x[j] = x[i] & x[j], x[i] | x[j]
    _assert_sorts_words(wires, x, "the 16-key base")
    for p2 in (32, 64):
        full, half = oddeven_merge_sort(p2), oddeven_merge_sort(p2 // 2)
        h = len(half)
        assert full[:h] == half and full[h:2 * h] == _shift(half, p2 // 2)
        merge = full[2 * h:]
        assert merge and all(0 <= i < j < p2 for i, j in merge)
        n = p2 // 2
        cols = [[0] * (n - a) + [1] * a + [0] * (n - b) + [1] * b for a in range(n + 1) for b in range(n + 1)]
        x = np.array(cols, dtype=np.uint8).T
        assert x.shape == (p2, (n + 1) ** 2)
        assert np.array_equal(_run_list(merge, x, 1), np.sort(x, axis=0)), p2


def _few(N, ones):
    """Every 0-1 column with at most two entries equal to ``ones``."""
    cols = [np.full(N, 1 - ones, dtype=np.uint8)]
    for c in itertools.chain(itertools.combinations(range(N), 1), itertools.combinations(range(N), 2)):
        v = np.full(N, 1 - ones, dtype=np.uint8)
        v[list(c)] = ones
        cols.append(v)
    return np.stack(cols, axis=1)


@pytest.mark.parametrize("N", BIG_SORTS)
def test_big_sort_text_equals_the_proved_list(N):
    from gen_median_nets import oddeven_merge_sort
    stmts = _nets(MEDIAN_HDR)["SortNet", N]
    p2 = 1 << (N - 1).bit_length()
    comps = oddeven_merge_sort(p2)
    rng = np.random.default_rng(5000 + N)
    # 3 * 2^16 random 0-1 columns, bit-sliced: 1024 words per density
    r = lambda: rng.integers(0, 2 ** 64, size=(N, 1024), dtype=np.uint64)  # noqa: E731
    words = np.concatenate([r() & r() & r(), r(), r() | r() | r()], axis=1)
    got = _run(stmts, list(words), np.bitwise_and, np.bitwise_or)
    x = list(words) + [np.full(words.shape[1], 2 ** 64 - 1, dtype=np.uint64)] * (p2 - N)
    for i, j in comps:
        x[i], x[j] = x[i] & x[j], x[i] | x[j]
    assert all(np.array_equal(g, e) for g, e in zip(got, x[:N]))
    _assert_sorts_words(list(words), got, f"SortNet<{N}>")
    # at most two ones, at most two zeros
    for ones in (1, 0):
        x = _few(N, ones)
        assert x.shape == (N, 1 + N + N * (N - 1) // 2)
        got = _run_real(stmts, x)
        assert np.array_equal(got, _run_list(comps, x, 1)) and np.array_equal(got, np.sort(x, axis=0))
    # real columns: distinct float32 values, and small integers with many ties
    x = rng.integers(0, 5, size=(N, 4096)).astype(np.float64)
    x[:, :2048] = rng.standard_normal((N, 2048)).astype(np.float32)
    got = _run_real(stmts, x)
    assert np.array_equal(got, _run_list(comps, x, np.inf)) and np.array_equal(got, np.sort(x, axis=0))


@pytest.mark.parametrize("N", [8, 16, 24])
def test_small_sort_text_equals_the_folded_list(N):
    """The small sorts are the same list with P2 - N sentinels folded: tie them to it as well."""
    from gen_median_nets import oddeven_merge_sort
    stmts = _nets(TRIMMED_HDR)["SortNet", N]
    comps = oddeven_merge_sort(1 << (N - 1).bit_length())
    rng = np.random.default_rng(6000 + N)
    x = rng.integers(0, 5, size=(N, 4096)).astype(np.float64)
    x[:, :2048] = rng.standard_normal((N, 2048)).astype(np.float32)
    got = _run_real(stmts, x)
    assert np.array_equal(got, _run_list(comps, x, np.inf)) and np.array_equal(got, np.sort(x, axis=0))


# ----------------------------------------------------------------------------- the generator
def test_header_matches_generator(tmp_path):
    import gen_trimmed_nets
    out = tmp_path / "nets.h"
    gen_trimmed_nets.main(str(out))
    assert out.read_text() == open(TRIMMED_HDR).read()
