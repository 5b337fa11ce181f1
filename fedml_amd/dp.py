"""Host side of differential privacy (include/fedagg_dp.h), the counterpart of cclip.py.  Pure Python:
the noise scale of a mechanism, the clipped client weights, the validation of the arguments.  The
per-element work -- the norms (fa_centered_sum_sqdist without coefficients), the clipped sum and the
noise (fa_centered_sum_noise), the noise alone (fa_add_noise) -- is the engine's.

Limits: float32 noise with truncated tails (5.77 sigma for Gaussian, ln 2^23 = 15.9 b for Laplace); no
privacy accountant; no protection against floating-point attacks on the noise's low bits (Mironov
2012); in 16-bit storage, noise below half an ulp of the value it is added to vanishes.
"""
from __future__ import annotations

import math
from typing import List, Sequence

from . import _native as N
from .cclip import cclip_scales

GAUSSIAN, LAPLACE = "gaussian", "laplace"
MECHANISMS = (GAUSSIAN, LAPLACE)
SEED_MASK = (1 << 64) - 1
CLIENT_SEED_MUL = 0x9E3779B97F4A7C15


def mech_code(mechanism) -> int:
    """FA_NOISE_GAUSSIAN / FA_NOISE_LAPLACE of "gaussian" / "laplace" (or of the code itself)."""
    if isinstance(mechanism, str) and mechanism in MECHANISMS:
        return N.NOISE_GAUSSIAN if mechanism == GAUSSIAN else N.NOISE_LAPLACE
    if isinstance(mechanism, int) and not isinstance(mechanism, bool) \
            and mechanism in (N.NOISE_GAUSSIAN, N.NOISE_LAPLACE):
        return mechanism
    raise ValueError(f"dp: mechanism must be 'gaussian' or 'laplace' (got {mechanism!r})")


def _positive(name: str, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not (v > 0 and math.isfinite(v)):
        raise ValueError(f"dp: {name} must be a positive finite number (got {v!r})")
    return float(v)


def noise_scale(mechanism, epsilon, delta, sensitivity) -> float:
    """The noise's scale: Gaussian sigma = sensitivity sqrt(2 ln(1.25 / delta)) / epsilon (Dwork and
    Roth 2014, Theorem A.1; 0 < delta < 1), Laplace b = sensitivity / epsilon (``delta`` is ignored).
    ``sensitivity`` >= 0; 0 gives scale 0: no noise."""
    m = mech_code(mechanism)
    eps = _positive("epsilon", epsilon)
    if isinstance(sensitivity, bool) or not isinstance(sensitivity, (int, float)) \
            or not (sensitivity >= 0 and math.isfinite(sensitivity)):
        raise ValueError(f"dp: sensitivity must be a finite number >= 0 (got {sensitivity!r})")
    if m == N.NOISE_LAPLACE:
        return float(sensitivity) / eps
    d = _positive("delta", delta)
    if not d < 1:
        raise ValueError(f"dp: delta must lie in (0, 1) (got {delta!r})")
    return float(sensitivity) * math.sqrt(2.0 * math.log(1.25 / d)) / eps


def clip_scales(w: Sequence[float], d2: Sequence[float], clip: float) -> List[float]:
    """The clipped weights w_i min(1, clip / |x_i - g|) from the squared distances d2: ``cclip_scales``."""
    clip = _positive("clipping_norm", clip)
    if any(math.isnan(d) for d in d2):
        raise ValueError("dp: a client's distance to the center is NaN")
    return cclip_scales(w, d2, clip)


def client_seed(dp_seed: int, client_id: int) -> int:
    """A local client's seed: dp_seed ^ (client_id * 0x9E3779B97F4A7C15 mod 2^64)."""
    return (int(dp_seed) ^ ((int(client_id) * CLIENT_SEED_MUL) & SEED_MASK)) & SEED_MASK


def check_seed_round(seed, round) -> None:
    for name, v, bits in (("seed", seed, 64), ("round", round, 32)):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < (1 << bits):
            raise ValueError(f"dp: {name} must be an integer in [0, 2^{bits}) (got {v!r})")
