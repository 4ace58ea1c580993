"""Memory self-test patterns, NumPy restatement (TEST ORACLE) of ``ginsim_pattern_fill`` and ``ginsim_digest``
(``gnss-ins-sim_amd/csrc/selftest.hip``, ABI 9).

    word i of a pattern   = (tag << 40) | i                      i = 64-bit word index from the region's start, tag < 2^24
    digest of words w_i   = sum_i splitmix64(w_i ^ (i * 0x9E3779B97F4A7C15)) mod 2^64
    splitmix64(z)         = z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
                            z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31        (all mod 2^64)

Everything is uint64 arithmetic, which NumPy wraps modulo 2^64 as the device does.
"""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def pattern(tag, nwords, first=0):
    """Words first .. first + nwords - 1 of the pattern of `tag` (uint64)."""
    i = np.arange(int(first), int(first) + int(nwords), dtype=np.uint64)
    return (np.uint64((int(tag) << 40) & 0xFFFFFFFFFFFFFFFF)) | i


def splitmix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over='ignore'):
        z = z + GOLDEN
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


def digest(words, chunk=1 << 22):
    """The digest of a uint64 array (any shape; word i is its i-th element in C order) as a Python int."""
    w = np.ascontiguousarray(words).view(np.uint64).reshape(-1)
    total = 0
    for s in range(0, w.size, chunk):
        i = np.arange(s, min(s + chunk, w.size), dtype=np.uint64)
        with np.errstate(over='ignore'):
            h = splitmix64(w[s:s + i.size] ^ (i * GOLDEN))
        total = (total + int(h.sum(dtype=np.uint64))) & 0xFFFFFFFFFFFFFFFF
    return total


def decode(word):
    """(tag, word index) a pattern word names."""
    word = int(word)
    return word >> 40, word & ((1 << 40) - 1)
