"""Host side of Bulyan's first stage (El Mhamdi, Guerraoui, Rouault 2018, "The Hidden Vulnerability of
Distributed Learning in Byzantium"), next to cclip.py and weiszfeld.py.  Pure Python over the K x K
squared distances that ONE fa_pairwise_sqdist launch produces (KrumDefense.pairwise_sq_distances):
Krum repeated K - 2f times on the clients not yet chosen.  The second stage, per coordinate the mean
of the K - 4f values nearest to the median over the chosen clients, is the device's
(fa_coord_mean_around_median, include/fedagg_robust.h).
"""
from __future__ import annotations

import math
from typing import List, Sequence


def bulyan_select(D: Sequence[Sequence[float]], f: int) -> List[int]:
    """The theta = K - 2f clients of Bulyan's first stage, in selection order.

    ``D``: K x K squared distances, taken as returned (no rounding to a norm's dtype); a non-finite
    entry counts as +inf.  With R = all clients, K - 2f times: nn = min(|R| - 1, max(1, |R| - f - 2));
    score_i = the sum of the nn smallest D[i][j] over j in R without i, added ascending; the client of
    the smallest score -- the lowest index on a tie -- moves from R to the selection.  The clamp on nn
    serves the last iterations, which have fewer than 2f + 3 clients left (exact ties are normal
    there: with nn = 1 two mutual nearest neighbours score the same)."""
    K = len(D)
    f = int(f)
    if f < 0 or K < 4 * f + 3:
        raise ValueError(f"bulyan_select: needs f >= 0 and K >= 4 f + 3 (K {K}, f {f})")
    inf = math.inf
    d = [[float(v) if math.isfinite(v) else inf for v in row] for row in D]
    rest = list(range(K))
    sel: List[int] = []
    for _ in range(K - 2 * f):
        nn = min(len(rest) - 1, max(1, len(rest) - f - 2))
        best, best_score = rest[0], None
        for i in rest:
            near = sorted(d[i][j] for j in rest if j != i)[:nn]
            score = 0.0
            for v in near:
                score += v
            if best_score is None or score < best_score:
                best, best_score = i, score
        rest.remove(best)
        sel.append(best)
    return sel
