"""Philox4x32-10 known answers for the numpy restatement (tests/_entry_ref.py) that
test_gpu_philox holds rae_neg_sample_philox to, bit for bit.  No GPU needed.

The three vectors are the Random123 known-answer tests of philox4x32 with 10 rounds
(Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)."""
import numpy as np

import _entry_ref as E

KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox4x32_10_known_answers():
    for ctr, key, want in KAT:
        got = E.philox4x32_10([np.array([c], np.uint32) for c in ctr], key)
        assert tuple(int(w[0]) for w in got) == want, (ctr, key, [hex(int(w[0])) for w in got])
    # vectorised: the three at once under one key each
    for ctr, key, want in KAT:
        got = E.philox4x32_10([np.array([c, c], np.uint32) for c in ctr], key)
        assert all(int(w[1]) == x for w, x in zip(got, want))


def test_philox_uniforms_counter_and_key_words():
    """idx = offset + i fills counter words 0 and 1 (the carry included), seed fills the two key
    words, u = ((c0 >> 5) 2^26 + (c1 >> 6)) / 2^53."""
    seed, off = (1 << 63) + 12345, (1 << 32) - 2
    u = E.philox_uniforms(seed, off, 4)
    for i in range(4):
        idx = off + i
        c = E.philox4x32_10([np.array([w], np.uint32)
                             for w in (idx & 0xFFFFFFFF, idx >> 32, 0, 0)],
                            (seed & 0xFFFFFFFF, seed >> 32))
        want = ((int(c[0][0]) >> 5) * (1 << 26) + (int(c[1][0]) >> 6)) / float(1 << 53)
        assert u[i] == want and 0.0 <= u[i] < 1.0
    assert u[1] != u[2]                      # idx = 2^32 - 1 and 2^32 differ in both words
    # wraps modulo 2^64 like the device's uint64 sum
    assert np.array_equal(E.philox_uniforms(3, (1 << 64) - 1, 3)[1:], E.philox_uniforms(3, 0, 2))
