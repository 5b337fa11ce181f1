"""Host driver of centered clipping (Karimireddy, He, Jaggi, "Learning from History for Byzantine Robust
Optimization"), shared by ``ClientArena.centered_clip`` and ``CenteredClippingDefense``; the
counterpart of weiszfeld.py.  Pure Python: the per-element work of a pass -- v' = v + sum_i s_i (x_i - v)
and every client's d2_i = |x_i - v'|^2, ss_i = |x_i|^2 -- is the caller's ``step`` (one
fa_centered_sum_sqdist launch per dtype group, include/fedagg_robust.h), the distances to the start
point the caller's ``first``; the driver only turns the K distances of one pass into the K scales of
the next.  One iteration from the global model is norm-difference clipping followed by FedAvg.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Sequence, Tuple


def cclip_scales(w: Sequence[float], d2: Sequence[float], tau: float) -> List[float]:
    """The clipped weights: r_i = sqrt(d2_i), s_i = w_i if r_i <= tau else w_i * (tau / r_i).  A client
    at infinite distance gets 0.0."""
    out = []
    for wi, d in zip(w, d2):
        r = math.sqrt(d)
        out.append(wi if r <= tau else wi * (tau / r))
    return out


def cclip_driver(alpha: Sequence[float], iters: int, tau: float,
                 first: Callable[[List[int]], Tuple[Sequence[float], Sequence[float]]],
                 step: Callable[[List[float], List[int]], Tuple[Sequence[float], Sequence[float]]]) -> Dict:
    """Run ``iters`` clipping iterations from the caller's start point v_0.

    ``first(clients)`` leaves v_0 in the caller's output and returns (d2, ss) of the clients
    ``clients`` (indices into ``alpha``) to it; ``step(scales, clients)`` replaces v by
    v + sum_i scales_i (x_i - v) and returns (d2, ss) to the new v.  Both return host floats, one per
    listed client (2K doubles copied to the host per pass).

    The weights are w_i = alpha_i / sum(alpha) over the clients kept.  Clients whose ss is not finite
    (a NaN or +-Inf in their update) are dropped and ``first`` redone once over the rest; none left,
    or a NaN distance after that, raises ValueError.  Returns the info dict: ``clients`` (the indices
    kept, which the traces are aligned with), ``dropped``, ``scale_trace`` (one list per iteration),
    ``d2_trace`` (``iters`` + 1 lists: the distances to v_0, then to every iterate) and ``clipped``
    (the clients whose last scale was below their weight); the last pass's v is the result."""
    alpha = [float(a) for a in alpha]
    if len(alpha) == 0:
        raise ValueError("centered_clipping: no clients")
    if not all(a > 0 and math.isfinite(a) for a in alpha):
        raise ValueError("centered_clipping: every client weight must be positive and finite")
    if isinstance(iters, bool) or int(iters) != iters or iters < 0:
        raise ValueError(f"centered_clipping: iters must be an integer >= 0 (got {iters})")
    if not (tau > 0 and math.isfinite(tau)):
        raise ValueError(f"centered_clipping: tau must be positive and finite (got {tau})")

    def start(clients):
        d2, ss = first(clients)
        return [float(x) for x in d2], [float(x) for x in ss]

    clients = list(range(len(alpha)))
    d2, ss = start(clients)
    dropped = [clients[j] for j, s in enumerate(ss) if not math.isfinite(s)]
    if dropped:
        clients = [i for i in clients if i not in set(dropped)]
        if not clients:
            raise ValueError("centered_clipping: every client holds a NaN or Inf")
        d2, ss = start(clients)
    tot = sum(alpha[i] for i in clients)
    w = [alpha[i] / tot for i in clients]
    info = {"clients": clients, "dropped": dropped, "scale_trace": [], "d2_trace": [], "clipped": []}

    def record(d2):
        if any(math.isnan(d) for d in d2):
            raise ValueError("centered_clipping: a client's distance to the center is NaN")
        info["d2_trace"].append(list(d2))

    record(d2)
    for _ in range(int(iters)):
        scales = cclip_scales(w, d2, tau)
        info["scale_trace"].append(list(scales))
        d2, _ss = step(scales, clients)
        d2 = [float(x) for x in d2]
        record(d2)
    if info["scale_trace"]:
        info["clipped"] = [i for i, s, wi in zip(clients, info["scale_trace"][-1], w) if s < wi]
    return info
