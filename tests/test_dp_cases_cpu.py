"""The numpy restatement of the noise contract (tests/dpcases.py) pinned by Random123's known answers
for philox4x32-10, by an anchor of the stream, and by the moments of its first 2^20 deviates."""
import numpy as np
import pytest

from tests import dpcases as D

ANCHOR_WORDS = ((0xd0e1fe69, 0xfee38b5f, 0xe81334ee, 0x6ad4edf0), (0x702f1bd3, 0x7201ad2f, 0x60aeaf84, 0xcc9aa80a))
ANCHOR_Z = {"gaussian": (0.63757805, -0.01739233, -0.3845283, 0.21993511),
            "laplace": (0.99939209, 4.7466255, 1.67710747, -0.18077518)}


@pytest.mark.parametrize("counter,key,out", D.KAT)
def test_philox_known_answers(counter, key, out):
    got = D.philox(np.array([counter], dtype=np.uint64), key)
    assert tuple(int(x) for x in got[0]) == out
    seed, rnd, seg, first = D.kat_args(counter, key)
    assert tuple(int(x) for x in D.words(seed, rnd, seg, first, 1)[0]) == out


def test_block_carry():
    w = D.words(D.ANCHOR_SEED, 3, 7, 2 ** 32 - 2, 4)
    for j, b in enumerate(range(2 ** 32 - 2, 2 ** 32 + 2)):
        c = np.array([[b & 0xFFFFFFFF, b >> 32, 7, 3]], dtype=np.uint64)
        assert (w[j] == D.philox(c, (D.ANCHOR_SEED & 0xFFFFFFFF, D.ANCHOR_SEED >> 32))[0]).all()
    assert len({tuple(r) for r in w.tolist()}) == 4


def test_anchor_words_and_deviates():
    w = D.words(D.ANCHOR_SEED, D.ANCHOR_ROUND, D.ANCHOR_SEG, 0, 2)
    assert tuple(tuple(int(x) for x in r) for r in w) == ANCHOR_WORDS
    for mech, exp in ANCHOR_Z.items():
        z = D.z64(mech, D.ANCHOR_SEED, D.ANCHOR_ROUND, D.ANCHOR_SEG, 4)
        np.testing.assert_allclose(z, exp, rtol=0, atol=5e-8)  # the digits the anchor is given to


def test_uniform_is_exact_and_open():
    w = np.array([0, 0x1FF, 0x200, 0xFFFFFFFF, 0x80000000], dtype=np.uint32)
    u = D.uniform(w)
    assert u.dtype == np.float32
    m = (w >> np.uint32(9)).astype(np.int64)
    assert (u.astype(np.float64) == (2 * m + 1) / 2.0 ** 24).all()
    assert u.min() > 0 and u.max() < 1
    assert (u - np.float32(0.5) != 0).all()


@pytest.mark.parametrize("mech", ["gaussian", "laplace"])
def test_moments(mech):
    z = D.z64(mech, D.ANCHOR_SEED, D.ANCHOR_ROUND, D.ANCHOR_SEG, 1 << 20)
    assert np.abs(z).max() <= (5.77 if mech == "gaussian" else 15.95)
    for name, err, bound in D.moment_checks(mech, z):
        assert err <= bound, (mech, name, err, bound)
