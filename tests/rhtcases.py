"""A numpy restatement of the rotation contract (include/fedagg_rotate.h): the signs from the noise
generator's words (tests/dpcases.py), the staged float32 butterflies and the scale
(tests/test_rht_cases_cpu.py pins it; tests/test_gpu_rht.py compares the device against it)."""
from __future__ import annotations

import numpy as np

from dpcases import words


def signs(seed: int, rnd: int, seg_id: int, n_pad: int) -> np.ndarray:
    """uint32 [n_pad]: 0x80000000 where element e' flips: bit e' & 31 of word (e' >> 5) & 3 of block e' >> 7."""
    w = words(seed, rnd, seg_id, 0, (n_pad + 127) // 128).reshape(-1)  # word e' >> 5 of the stream
    e = np.arange(n_pad, dtype=np.int64)
    return ((w[e >> 5] >> (e & 31).astype(np.uint32)) & np.uint32(1)) << np.uint32(31)


def stages(x: np.ndarray, b: int) -> np.ndarray:
    """The stages h = 1, 2, ..., 2^(b-1) on every block of 2^b float32 values; every add rounded once."""
    x = x.astype(np.float32).reshape(-1, 1 << b)
    for p in range(b):
        v = x.reshape(x.shape[0], -1, 2, 1 << p)  # [..., 0, :] = i with (i & h) == 0, [..., 1, :] = i + h
        x = np.stack([v[:, :, 0] + v[:, :, 1], v[:, :, 0] - v[:, :, 1]], axis=2).reshape(x.shape[0], -1)
        assert x.dtype == np.float32
    return x.reshape(-1)


def scale(b: int) -> np.float32:
    c = np.uint32(0x3fb504f3).view(np.float32) if b & 1 else np.float32(1.0)
    return np.float32(c * np.float32(2.0 ** -((b + 1) // 2)))  # a power of two: exact


def flip(x: np.ndarray, s: np.ndarray) -> np.ndarray:
    return (x.view(np.uint32) ^ s).view(np.float32)


def forward(x: np.ndarray, b: int, seed: int, rnd: int, seg_id: int) -> np.ndarray:
    """x (float32, float16, or bfloat16 already widened): n elements -> n_pad float32."""
    n_pad = -(-x.size >> b) << b
    xp = np.zeros(n_pad, np.float32)
    xp[:x.size] = x.astype(np.float32)
    with np.errstate(all="ignore"):
        return stages(flip(xp, signs(seed, rnd, seg_id, n_pad)), b) * scale(b)


def inverse(y: np.ndarray, n: int, b: int, seed: int, rnd: int, seg_id: int) -> np.ndarray:
    """y: n_pad float32 -> the first n float32."""
    with np.errstate(all="ignore"):
        return flip(stages(y, b) * scale(b), signs(seed, rnd, seg_id, y.size))[:n]
