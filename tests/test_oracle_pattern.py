"""The NumPy statement of the memory self-test patterns (oracle/pattern.py) that tests/test_gpu_placed_integrity.py holds the
device's ginsim_pattern_fill / ginsim_digest to: against the published splitmix64 outputs and a word-by-word Python loop."""
import numpy as np

from oracle import pattern as pat

M64 = (1 << 64) - 1


def _splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def test_splitmix64_known_answers():
    # the first outputs of the splitmix64 generator seeded with 0: its state steps by the golden gamma
    assert int(pat.splitmix64(np.uint64(0))) == 0xE220A8397B1DCDAF
    assert int(pat.splitmix64(np.uint64(0x9E3779B97F4A7C15))) == 0x6E789E6AA1B965F4
    z = np.random.default_rng(5).integers(0, 2 ** 64, size=1000, dtype=np.uint64)
    assert [int(x) for x in pat.splitmix64(z)] == [_splitmix64(int(x)) for x in z]


def test_pattern_words_and_digest_against_a_python_loop():
    w = pat.pattern(0xABCDEF, 3000, first=5)
    assert [int(x) for x in w] == [(0xABCDEF << 40) | i for i in range(5, 3005)]
    assert pat.decode(w[7]) == (0xABCDEF, 12)
    words = np.random.default_rng(9).integers(0, 2 ** 64, size=5000, dtype=np.uint64)
    want = 0
    for i, x in enumerate(int(v) for v in words):
        want = (want + _splitmix64(x ^ ((i * 0x9E3779B97F4A7C15) & M64))) & M64
    assert pat.digest(words) == want
    assert pat.digest(words, chunk=7) == want            # the split into chunks does not matter
    assert pat.digest(np.zeros(0, dtype=np.uint64)) == 0
    swapped = words.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    assert pat.digest(swapped) != want                   # position enters the digest
