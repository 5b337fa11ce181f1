"""Host driver of the geometric median by the smoothed Weiszfeld iteration (Pillutla, Kakade,
Harchaoui, "Robust Aggregation for Federated Learning"), shared by ``ClientArena.geometric_median``
and ``GeometricMedianDefense``.  Pure Python: the per-element work of a pass -- the weighted sum
z = sum_i coef_i x_i and every client's d2_i = |x_i - z|^2, ss_i = |x_i|^2 -- is the caller's ``step``
(one fa_weighted_sum_sqdist launch per dtype group, include/fedagg_robust.h); the driver only turns the
2K sums of one pass into the K weights of the next.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Sequence, Tuple


def weiszfeld_coef(alpha: Sequence[float], d2: Sequence[float], nu: float) -> List[float]:
    """The smoothed Weiszfeld weights: b_i = alpha_i / max(nu, sqrt(d2_i)), coef_i = b_i / sum(b) with
    the builtin left-to-right sum.  A client at infinite distance gets weight 0; sum(b) == 0 (every
    client at infinite distance) raises ValueError."""
    b = [a / max(nu, math.sqrt(d)) for a, d in zip(alpha, d2)]
    s = sum(b)
    if s == 0:
        raise ValueError("geometric_median: every client is at infinite distance (the weights sum to 0)")
    return [x / s for x in b]


def weiszfeld_driver(alpha: Sequence[float], iters: int, nu: float,
                     step: Callable[[List[float], List[int]], Tuple[Sequence[float], Sequence[float]]]) -> Dict:
    """Run ``iters`` Weiszfeld iterations after the weighted-mean pass (``iters`` + 1 passes).

    ``step(coef, clients)`` runs one pass over the clients ``clients`` (indices into ``alpha``) with
    the weights ``coef`` (aligned with ``clients``), leaves z in the caller's output, and returns
    (d2, ss) as host floats, one per listed client (2K doubles copied to the host per pass).

    Pass 0 uses coef_i = alpha_i / sum(alpha).  Clients whose ss is not finite (a NaN or +-Inf in
    their update) are dropped, alpha renormalised over the rest and pass 0 redone once; none left, or
    a NaN distance after that, raises ValueError.  Returns the info dict: ``clients`` (the indices
    kept, which the traces are aligned with), ``dropped``, and per pass ``coef_trace``, ``d2_trace``
    and ``objective_trace`` (sum_i alpha_i sqrt(d2_i)); the last pass's z is the result."""
    alpha = [float(a) for a in alpha]
    if len(alpha) == 0:
        raise ValueError("geometric_median: no clients")
    if not all(a > 0 and math.isfinite(a) for a in alpha):
        raise ValueError("geometric_median: every client weight must be positive and finite")
    if int(iters) != iters or iters < 0:
        raise ValueError(f"geometric_median: iters must be an integer >= 0 (got {iters})")
    if not (nu > 0 and math.isfinite(nu)):
        raise ValueError(f"geometric_median: nu must be positive and finite (got {nu})")

    def first(clients):
        a = [alpha[i] for i in clients]
        tot = sum(a)
        coef = [x / tot for x in a]
        d2, ss = step(coef, clients)
        return a, coef, [float(x) for x in d2], [float(x) for x in ss]

    clients = list(range(len(alpha)))
    a, coef, d2, ss = first(clients)
    dropped = [clients[j] for j, s in enumerate(ss) if not math.isfinite(s)]
    if dropped:
        clients = [i for i in clients if i not in set(dropped)]
        if not clients:
            raise ValueError("geometric_median: every client holds a NaN or Inf")
        a, coef, d2, ss = first(clients)
    info = {"clients": clients, "dropped": dropped, "coef_trace": [], "d2_trace": [], "objective_trace": []}

    def record(coef, d2):
        if any(math.isnan(d) for d in d2):
            raise ValueError("geometric_median: a client's distance to the aggregate is NaN")
        info["coef_trace"].append(list(coef))
        info["d2_trace"].append(list(d2))
        info["objective_trace"].append(sum(x * math.sqrt(d) for x, d in zip(a, d2)))

    record(coef, d2)
    for _ in range(int(iters)):
        coef = weiszfeld_coef(a, d2, nu)
        d2, ss = step(coef, clients)
        d2 = [float(x) for x in d2]
        record(coef, d2)
    return info
