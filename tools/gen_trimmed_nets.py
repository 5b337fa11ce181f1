#!/usr/bin/env python
"""Generates fedml_amd/csrc/trimmed_nets.h: the extra straight-line networks of the coordinate-wise
trimmed-mean kernels (trimmed.hip).  median_nets.h is not touched (tools/gen_median_nets.py owns it);
this header includes it and adds

  SortNet<N>, N = 8, 16, 24   full sorts for small K (median_nets.h has N = 32, 36, ..., 64), the same
                              odd-even merge sort with the extra inputs folded away as high sentinels;
  BitonicLo<N> / BitonicHi<N>, N = 36, 40, ..., 64
                              the two-lanes-per-column kernel's final merge of N keys in registers:
                              Lo sorts an up-then-down sequence (the N smallest keys of a column,
                              min(A[j], C[N-1-j])), Hi a down-then-up one (the N largest).  Both are the
                              bitonic merger of 64 keys with the 64 - N extra inputs as compile-time
                              sentinels appended where they keep the sequence bitonic (low ones after an
                              up-down sequence, high ones after a down-up one); a comparator with a
                              constant input is a renaming.

Every network is checked on generation: the sorts on random columns with ties, the mergers on every
0-1 input of their shape (0-1 principle) and on random bitonic columns.

Run: python tools/gen_trimmed_nets.py   (prints the min/max count per network)
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_median_nets import check_sortnet, oddeven_merge_sort, verify_g16  # noqa: E402

SMALL_SORTS = [8, 16, 24]
MERGES = list(range(36, 65, 4))


def fold(comps, pos):
    """Runs comparators (i, j) (i takes the min) over positions holding ('x', i) inputs or ('L',) /
    ('H',) constants; returns the ops [(a, b, t)] with a real instruction and the final positions."""
    ops, tmp = [], 0
    for i, j in comps:
        a, b = pos[i], pos[j]
        ca, cb = a[0] in "LH", b[0] in "LH"
        if ca and cb:
            if a[0] == "H" and b[0] == "L":
                pos[i], pos[j] = b, a
        elif ca:
            pos[i], pos[j] = (a, b) if a[0] == "L" else (b, a)
        elif cb:
            pos[i], pos[j] = (b, a) if b[0] == "L" else (a, b)
        else:
            ops.append((a, b, tmp))
            pos[i], pos[j] = ("t", tmp, "min"), ("t", tmp, "max")
            tmp += 1
    return ops, pos


def emit(name, N, ops, outs):
    """outs[i]: the operand that becomes x[i]."""
    ref = lambda o: f"x[{o[1]}]" if o[0] == "x" else ("i" if o[2] == "min" else "a") + str(o[1])
    L = [f"template <> struct {name}<{N}> {{",
         f"  template <typename K> __device__ __forceinline__ static void run(K (&x)[{N}]) {{"]
    for a, b, t in ops:
        L.append(f"    const K i{t} = kmin({ref(a)}, {ref(b)}), a{t} = kmax({ref(a)}, {ref(b)});")
    moved = [i for i in range(N) if outs[i] != ("x", i)]
    for i in moved:  # read every output before any x[] is overwritten
        L.append(f"    const K o{i} = {ref(outs[i])};")
    for i in moved:
        L.append(f"    x[{i}] = o{i};")
    L += ["  }", "};"]
    return "\n".join(L)


def small_sort(N):
    P2 = 1 << (N - 1).bit_length()
    ops, pos = fold(oddeven_merge_sort(P2), [("x", i) for i in range(N)] + [("H",)] * (P2 - N))
    assert all(pos[i][0] != "H" for i in range(N))
    check_sortnet(N, ops, pos)
    return emit("SortNet", N, ops, pos[:N]), 2 * len(ops)


def bitonic_merge(P2):
    comps, s = [], P2 // 2
    while s:
        comps += [(i, i + s) for i in range(P2) if not i & s]
        s //= 2
    return comps


def run_ops(ops, outs, x):
    import numpy as np
    val = {}
    get = lambda o: x[o[1]] if o[0] == "x" else val[o[1]][0 if o[2] == "min" else 1]
    for a, b, t in ops:
        val[t] = (np.minimum(get(a), get(b)), np.maximum(get(a), get(b)))
    return np.stack([get(o) for o in outs])


def merger(N, hi):
    """Lo: inputs up-then-down + low constants, the reals come out at ranks 64-N..63.
    Hi: inputs down-then-up + high constants, the reals come out at ranks 0..N-1."""
    import numpy as np
    P2 = 64
    ops, pos = fold(bitonic_merge(P2), [("x", i) for i in range(N)] + [("H",) if hi else ("L",)] * (P2 - N))
    outs = pos[:N] if hi else pos[P2 - N:]
    assert all(o[0] not in "LH" for o in outs)
    # every 0-1 input of the shape: 0^a 1^b 0^c (Lo) / 1^a 0^b 1^c (Hi)
    cols = [[hi] * a + [not hi] * b + [hi] * (N - a - b) for a in range(N + 1) for b in range(N + 1 - a)]
    x = np.array(cols, dtype=np.float64).T
    assert (run_ops(ops, outs, x) == np.sort(x, axis=0)).all(), N
    # random columns with ties: a sorted run then a reversed sorted run (Lo), mirrored for Hi
    rng = np.random.default_rng(2000 + N + hi)
    x = rng.integers(0, 9, size=(N, 4096)).astype(np.float64)
    x[:, :2048] = rng.standard_normal((N, 2048))
    cut = rng.integers(0, N + 1, size=4096)
    for c in range(4096):
        up, down = np.sort(x[:cut[c], c]), np.sort(x[cut[c]:, c])[::-1]
        x[:, c] = np.concatenate([down, up]) if hi else np.concatenate([up, down])
    assert (run_ops(ops, outs, x) == np.sort(x, axis=0)).all(), N
    return emit("BitonicHi" if hi else "BitonicLo", N, ops, outs), 2 * len(ops)


def main(path):
    verify_g16()
    body, counts = [], {}
    for N in SMALL_SORTS:
        code, counts[f"SortNet<{N}>"] = small_sort(N)
        body.append(code)
    body.append("// BitonicLo<N>::run(x): x up-then-down -> ascending; BitonicHi<N>::run(x): x down-then-up -> ascending\n"
                "template <int N> struct BitonicLo;\ntemplate <int N> struct BitonicHi;")
    for N in MERGES:
        for hi in (False, True):
            code, counts[f"Bitonic{'Hi' if hi else 'Lo'}<{N}>"] = merger(N, hi)
            body.append(code)
    hdr = ("// trimmed_nets.h -- GENERATED by tools/gen_trimmed_nets.py; do not edit.\n"
           "// Networks of the coordinate-wise trimmed-mean kernels (trimmed.hip) that median_nets.h does not\n"
           "// have: full sorts of 8 / 16 / 24 keys and the two-lanes-per-column kernel's bitonic mergers.\n"
           "// min/max per network: " + str(counts) + "\n"
           "#pragma once\n\n#include \"median_nets.h\"\n\n")
    with open(path, "w") as f:
        f.write(hdr + "\n\n".join(body) + "\n")
    print(counts)


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "fedml_amd", "csrc", "trimmed_nets.h"))
