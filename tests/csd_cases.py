"""The shapes of the Welch cross-spectral tests, shared by test_csd_oracle.py (the plan and the float64 restatement of every shape,
without a device) and test_gpu_csd.py (parity with csd_exact under its tolerance).

A case: id, L, D, K, tail, kinds, pad, window, detrend, where -- psd_cases' tuple:
  n = (K - 1) D + L + tail samples per series (tail < D: samples the call must not read), series_stride = n + pad,
  one series per entry of `kinds`, `where` = (a, b) when the case sits at K = a * segs_per_part + b.
`kinds` are psd_exact.series' and three scaled ones: 'small' and 'large', white noise times 1e-6 and 1e3, and 'smalltone', the
tone times 1e-6.  The pairs of a case are ``pairs_of(case)``: every series with its successor, cyclically, or the case's own table.

The chosen shapes: every segment length at K = 3 (odd) and D = L/2 + 1 (unaligned) under both windows with and without detrend --
L = 8, 16, 32 leave most of a wavefront without a butterfly, 128 is exactly one wavefront of them, 512 the first with several;
the part boundary at K = segs_per_part - 1, segs_per_part, + 1 and 2 segs_per_part + 1 for a half-overlapped and a disjoint
partition; the largest segment with two parts and one segment more; and TABLE, 65 pairs over 9 series."""
import numpy as np

SCALED = {'small': (1e-6, 'white'), 'large': (1e3, 'white'), 'smalltone': (1e-6, 'tone')}
TRIO = ('white', 'tone', 'offset')


def _every_length():
    out = []
    for lg in range(3, 13):
        L = 1 << lg
        for win in ('hann', 'boxcar'):
            for det in (True, False):
                name = 'L%d_K3_unaligned_%s_%s' % (L, win, 'detrend' if det else 'raw')
                # a tail and a stride larger than n on the Hann / detrend quarter of them
                out.append((name, L, L // 2 + 1, 3, 2 if win == 'hann' else 0, TRIO, 3 if det else 0, win, det, None))
    return out


CASES = _every_length() + [
    # id                                  L     D     K    tail kinds                          pad window    detrend where
    ('L1024_half_overlap_part_minus_1',   1024, 512,  31,  0,   ('white', 'tone'),             0,  'hann',   True,  (0, 31)),
    ('L1024_half_overlap_one_part',       1024, 512,  32,  100, ('white', 'small'),            0,  'hann',   True,  (1, 0)),
    ('L1024_half_overlap_part_plus_1',    1024, 512,  33,  0,   ('walk', 'offset'),            5,  'hann',   True,  (1, 1)),
    ('L1024_half_overlap_2_parts_plus_1', 1024, 512,  65,  511, ('tone', 'smalltone'),         0,  'boxcar', True,  (2, 1)),
    ('L256_no_overlap_part_minus_1',      256,  256,  63,  0,   ('white', 'large'),            0,  'boxcar', False, (0, 63)),
    ('L256_no_overlap_one_part',          256,  256,  64,  0,   ('constant', 'white'),         0,  'hann',   True,  (1, 0)),
    ('L256_no_overlap_part_plus_1',       256,  256,  65,  255, ('small', 'offset'),           9,  'hann',   True,  (1, 1)),
    ('L256_no_overlap_2_parts_plus_1',    256,  256,  129, 0,   ('white', 'walk'),             0,  'hann',   False, (2, 1)),
    ('L4096_no_overlap_2_parts_plus_1',   4096, 4096, 9,   0,   ('white', 'tone', 'small'),    0,  'hann',   True,  (2, 1)),
]

# the table: 65 pairs over 9 series at K = segs_per_part + 1, a tail of unread samples and a stride larger than n
TABLE_KINDS = ('white', 'white', 'small', 'offset', 'walk', 'tone', 'smalltone', 'constant', 'large')
TABLE = ('L256_table_of_65_pairs_over_9_series', 256, 128, 129, 100, TABLE_KINDS, 7, 'hann', True, (1, 1))


def _table_pairs():
    t = [(i, i) for i in range(9)]                                                       # a series with itself
    t += [(0, 1), (1, 0), (2, 3), (3, 2), (5, 6), (6, 5), (2, 8), (8, 2)]                # (i, j) together with (j, i)
    t += [(0, j) for j in range(2, 9)]                                                   # series 0 in more than eight pairs
    t += [(8, 7), (7, 6), (6, 4), (5, 4), (4, 3), (3, 1), (2, 1)]                        # descending
    t += [(3, 4), (5, 0), (7, 1)]                        # with the above: every scale pair of csd_exact.PAIR_KINDS
    rest = [(i, j) for i in range(9) for j in range(9) if i != j and (i, j) not in t]
    t += rest[:65 - len(t)]
    assert len(t) == 65 and sum(0 in p for p in t) >= 8
    return t


TABLE_PAIRS = _table_pairs()
CASES.append(TABLE)
IDS = [c[0] for c in CASES]


def shape(case):
    """(n, S, stride) of a case."""
    _, L, D, K, tail, kinds, pad, _, _, _ = case
    assert 0 <= tail < D
    n = (K - 1) * D + L + tail
    return n, len(kinds), n + pad


def pairs_of(case):
    if case is TABLE or case[0] == TABLE[0]:
        return list(TABLE_PAIRS)
    S = len(case[5])
    return [(i, (i + 1) % S) for i in range(S)]


def rows(case, seed=23):
    """The case's series as an (S, stride) array; the pad between the series holds NaN, which nothing may read."""
    import psd_exact as px
    n, S, stride = shape(case)
    a = np.full((S, stride), np.nan)
    for s, kind in enumerate(case[5]):
        f, base = SCALED.get(kind, (1.0, kind))
        a[s, :n] = f * px.series(base, n, seed + 17 * s)
    return a


def device_csd(ctx, a, n, pairs, L, D, win, det, fs=100.0):
    """ginsim.welch_csd on the rows of `a` (S, stride), of which n samples each are the series: a CsdResult."""
    import ginsim
    buf = ctx.upload(np.ascontiguousarray(a))
    try:
        return ginsim.welch_csd(ctx, buf, n, a.shape[0], a.shape[1], fs, pairs, L, D, win, det)
    finally:
        buf.free()
