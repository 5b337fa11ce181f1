"""A numpy restatement of the noise contract (include/fedagg_dp.h): the Philox4x32-10 words, the
uniform, and the float64 deviates of both mechanisms, for the tests of the device generator
(tests/test_dp_cases_cpu.py pins it; tests/test_gpu_dp_*.py compare the device against it)."""
from __future__ import annotations

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)

ANCHOR_SEED, ANCHOR_ROUND, ANCHOR_SEG = 0x0123456789ABCDEF, 1, 0

# Random123's known answers for philox4x32-10: (counter, key, output)
KAT = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def kat_args(counter, key):
    """(seed, round, seg_id, first_block) that form the counter and the key."""
    return key[0] | (key[1] << 32), counter[3], counter[2], counter[0] | (counter[1] << 32)


def philox(c, k):
    """Philox4x32-10 of counters c ([n, 4] uint32 values held in uint64) under key k (2 ints)."""
    c0, c1, c2, c3 = (np.asarray(c[:, j], dtype=np.uint64) for j in range(4))
    k0, k1 = int(k[0]), int(k[1])
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK,
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK)
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def words(seed: int, round: int, seg_id: int, first_block: int, nblocks: int) -> np.ndarray:
    """[nblocks, 4] uint32: the words of blocks first_block .. first_block + nblocks - 1."""
    b = np.uint64(first_block) + np.arange(nblocks, dtype=np.uint64)
    c = np.stack([b & MASK, b >> np.uint64(32), np.full(nblocks, seg_id, np.uint64),
                  np.full(nblocks, round, np.uint64)], axis=1)
    return philox(c, (seed & 0xFFFFFFFF, seed >> 32))


def uniform(w: np.ndarray) -> np.ndarray:
    """u = ((w >> 9) + 0.5) 2^-23 as float32 (exact) ."""
    u = ((w >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    assert u.dtype == np.float32
    return u


def z64(mech: str, seed: int, round: int, seg_id: int, n: int) -> np.ndarray:
    """The first n deviates of the stream in float64, from the exact words and uniforms."""
    nb = (n + 3) // 4
    u = uniform(words(seed, round, seg_id, 0, nb)).astype(np.float64)  # [nb, 4]
    if mech == "gaussian":
        ua, ub = u[:, 0::2], u[:, 1::2]  # [nb, 2]: the pairs (u0, u1), (u2, u3)
        r = np.sqrt(-2.0 * np.log(ua))
        z = np.stack([r * np.cos(2.0 * np.pi * ub), r * np.sin(2.0 * np.pi * ub)], axis=2)  # [nb, 2, 2]
    elif mech == "laplace":
        v = u - 0.5
        z = -np.sign(v) * np.log(1.0 - 2.0 * np.abs(v))
    else:
        raise ValueError(mech)
    return z.reshape(-1)[:n]


# five standard errors of the moments of n deviates: (statistic, target, bound factor)
def moment_checks(mech: str, z: np.ndarray):
    """[(name, |statistic - target|, bound)] over the deviates z (float64)."""
    n = z.size
    m, v = z.mean(), z.var()
    if mech == "gaussian":
        return [("mean", abs(m), 5 / np.sqrt(n)), ("var", abs(v - 1), 5 * np.sqrt(2 / n)),
                ("kurt", abs((z ** 4).mean() - 3), 5 * np.sqrt(96 / n))]
    return [("mean", abs(m), 5 * np.sqrt(2 / n)), ("var", abs(v - 2), 5 * np.sqrt(20 / n))]
