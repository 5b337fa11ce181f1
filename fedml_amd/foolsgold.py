"""FoolsGold's client weights (Fung, Yoon, Beschastnikh, "Mitigating Sybils in Federated Learning
Poisoning", 2018; RAID 2020) from the Gram matrix of the clients' update histories.

The K x K inner products are the device's work (include/fedagg_robust.h, fa_pairwise_dot); what is
left is arithmetic over K^2 numbers, done here in Python floats (float64) on the host.  Shared by
``FoolsGoldDefense`` and its tests.
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple


def _rows(G) -> List[List[float]]:
    if hasattr(G, "tolist"):  # a torch tensor (any device) or a numpy array
        G = G.tolist()
    rows = [[float(v) for v in r] for r in G]
    if any(len(r) != len(rows) for r in rows) or not rows:
        raise ValueError("foolsgold_weights: G must be a non-empty square matrix")
    return rows


def _clamp(x: float, lo: float, hi: float) -> float:
    return lo if x < lo else hi if x > hi else x


def foolsgold_weights(G, confidence: float = 1.0) -> Tuple[List[float], List[List[float]]]:
    """(weights, cs) for the K clients whose histories have the Gram matrix ``G`` (G[i][j] = <h_i, h_j>,
    d_i = G[i][i]).

    1. Client i is *void* if d_i is not finite, or if some finite-d client j has a non-finite G[i][j];
       it is *silent* if d_i == 0.
    2. cs[i][j] = clamp(G[i][j] / (sqrt(d_i) sqrt(d_j)), -1, 1) for i != j when both are neither void
       nor silent; otherwise 0.
    3. v_i = max_{j != i} cs[i][j] (0 for K = 1).
    4. Pardoning: where v_j > v_i and v_j > 0, cs[i][j] *= v_i / v_j -- an honest client that resembles
       a sybil is not punished for the sybil's larger similarity to its own kind.
    5. a_i = clamp(1 - max_{j != i} cs[i][j], 0, 1), m = max_i a_i over the non-void clients.
    6. w_i = 0 if client i is void or m <= 0; otherwise with x = a_i / m: w_i = 1 if x >= 1, 0 if
       x <= 0, else clamp(confidence * (ln(x / (1 - x)) + 0.5), 0, 1).

    ``cs`` is returned after the pardoning.  A void client leaves the others' weights as if it were
    absent; a silent client (no update yet) resembles nobody and gets weight 1."""
    g = _rows(G)
    k = len(g)
    d = [g[i][i] for i in range(k)]
    fin = [math.isfinite(x) for x in d]
    void = [not fin[i] or any(fin[j] and not math.isfinite(g[i][j]) for j in range(k) if j != i) for i in range(k)]
    live = [not void[i] and d[i] > 0 for i in range(k)]
    root = [math.sqrt(d[i]) if live[i] else 0.0 for i in range(k)]
    cs = [[0.0] * k for _ in range(k)]
    for i in range(k):
        for j in range(k):
            if i != j and live[i] and live[j]:
                cs[i][j] = _clamp(g[i][j] / (root[i] * root[j]), -1.0, 1.0)

    def row_max(i: int) -> float:
        return max((cs[i][j] for j in range(k) if j != i), default=0.0)

    v = [row_max(i) for i in range(k)]
    for i in range(k):
        for j in range(k):
            if i != j and v[j] > v[i] and v[j] > 0:
                cs[i][j] *= v[i] / v[j]
    a = [_clamp(1.0 - row_max(i), 0.0, 1.0) for i in range(k)]
    m = max((a[i] for i in range(k) if not void[i]), default=0.0)
    w = []
    for i in range(k):
        if void[i] or m <= 0:
            w.append(0.0)
            continue
        x = a[i] / m
        if x >= 1:
            w.append(1.0)
        elif x <= 0:
            w.append(0.0)
        else:
            w.append(_clamp(confidence * (math.log(x / (1.0 - x)) + 0.5), 0.0, 1.0))
    return w, cs


def largest_similarity(cs: Sequence[Sequence[float]]) -> List[float]:
    """Each client's largest cs towards another client (0 for K = 1)."""
    k = len(cs)
    return [max((cs[i][j] for j in range(k) if j != i), default=0.0) for i in range(k)]
