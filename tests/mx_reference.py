"""Plain reference of the Microscaling ("mx") format of include/fedagg_mx.h, for test_gpu_mx.py: the
two decode tables in float64, 2.0 ** (X - 127), the float32 ordered sum in torch on the CPU, and the
quantizer restated from the header in float64 (every step below is exact in float64)."""
from __future__ import annotations

import numpy as np
import torch

FP8_VALUES = np.array([np.nan if c & 0x7F == 0x7F else
                       (-1.0 if c & 0x80 else 1.0) *
                       ((c & 7) * 2.0 ** -9 if (c >> 3) & 15 == 0 else (8 + (c & 7)) * 2.0 ** (((c >> 3) & 15) - 10))
                       for c in range(256)])
FP4_VALUES = np.array([(-1.0 if c & 8 else 1.0) * (0, 0.5, 1, 1.5, 2, 3, 4, 6)[c & 7] for c in range(16)])
EMAX = {"fp8": 8, "fp4": 2}


def codes_of(data: np.ndarray, n: int, fmt: str) -> np.ndarray:
    """The n element codes held by the data bytes (FP4: the even element in the low nibble)."""
    if fmt == "fp8":
        return data[:n]
    return np.stack([data & 15, data >> 4], axis=1).reshape(-1)[:n]


def decode(data: np.ndarray, scale: np.ndarray, n: int, fmt: str) -> torch.Tensor:
    """float32 tensor of n elements: rnd(element * 2^(X - 127)), NaN where X = 255."""
    vals = (FP8_VALUES if fmt == "fp8" else FP4_VALUES)[codes_of(data, n, fmt)]
    x = np.repeat(scale.astype(np.int64), 32)[:n]
    with np.errstate(over="ignore", invalid="ignore"):
        d = (vals * 2.0 ** (x - 127.0)).astype(np.float32)
    d[x == 255] = np.nan
    return torch.from_numpy(d)


def ordered_sum(rows, mode_mul_w: bool, coef) -> torch.Tensor:
    """out = t_0; out = rnd(out + t_i) in float32, t_i = rnd(d_i * (float)coef[i]) or d_i."""
    out = None
    for i, d in enumerate(rows):
        t = d * torch.tensor(coef[i], dtype=torch.float64).to(torch.float32) if mode_mul_w else d
        out = t.clone() if out is None else out + t
    return out


def quantize(x: torch.Tensor, fmt: str):
    """(data bytes, scale bytes) of a flat float tensor, as the header states the quantizer."""
    v = x.detach().cpu().to(torch.float64).numpy().reshape(-1)
    n = v.size
    nb = -(-n // 32)
    blocks = np.zeros(nb * 32)
    blocks[:n] = v
    blocks = blocks.reshape(nb, 32)
    bad = ~np.isfinite(blocks).all(axis=1)
    blocks[bad] = 0.0
    amax = np.abs(blocks).max(axis=1)
    e = np.frexp(amax)[1] - 1 - EMAX[fmt]  # floor(log2 amax) - emax
    e = np.where(amax == 0, -127, np.clip(e, -127, 127))
    mags = np.abs(FP8_VALUES[:0x7F] if fmt == "fp8" else FP4_VALUES[:8])
    mids = (mags[:-1] + mags[1:]) / 2
    q = np.ldexp(np.abs(blocks), -e[:, None])  # |x| / 2^E, exact
    lo, hi = np.searchsorted(mids, q, "left"), np.searchsorted(mids, q, "right")
    code = np.where(lo == hi, lo, hi - (hi & 1))  # a tie: the even mantissa
    code = code | (np.signbit(blocks) << (7 if fmt == "fp8" else 3))
    code[bad] = 0
    code = code.reshape(-1)[:n].astype(np.uint8)
    scale = np.where(bad, 255, e + 127).astype(np.uint8)
    if fmt == "fp4":
        code = np.concatenate([code, np.zeros(n & 1, np.uint8)])
        code = code[0::2] | (code[1::2] << 4)
    return code, scale
