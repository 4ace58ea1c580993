"""The edge shapes of the Welch cross-spectral tests, shared by test_csd_edges_oracle.py (the float64 restatement of every shape
and constructed input, without a device) and test_gpu_csd_edges.py (the device).  The tuple, `shape`, `rows`, `pairs_of` and
`device_csd` are csd_cases'; every case here states where it sits, `where` = (a, b) with K = a * segs_per_part + b.

The shapes: one segment with n = L exactly and two segments at D = L and D = 1 (L = 8, 128, 512, 4096, both windows; csd_cases
has K >= 3 throughout); D = 1 over three part boundaries at L = 8 and one at L = 64, parts of 16384 segments that start on every
residue; half overlap over three part boundaries at L = 512, which has none in csd_cases; D = L - 1 at L = 2048.

The constructed inputs: `single_bins(L)`, noise-free cosines and sines on single bins, which leave the exact spectrum of the
OTHER series of a pair at zero, so that csd_exact.tol is its term e alone there; `placements(L, K, spp)`, one non-finite mark per
odd row; `scaled_rows(name)`, the two rows of a csd_cases shape that the power-of-two scalings use."""
import numpy as np

import csd_cases as cc
import psd_cases as pc

shape, rows, pairs_of, device_csd = cc.shape, cc.rows, cc.pairs_of, cc.device_csd

KIND_PAIRS = (('white', 'tone'), ('constant', 'white'), ('offset', 'small'))
FEW_L = (8, 128, 512, 4096)


def _few_segments():
    out, i = [], 0
    for L in FEW_L:
        for win in ('hann', 'boxcar'):
            for kp in KIND_PAIRS:                        # one segment: n = L exactly, no tail, no pad
                i += 1
                out.append(('L%d_K1_n_equals_L_%s_%s_%s' % ((L, win) + kp), L, L, 1, 0, kp, 0, win, i % 2 == 0, (0, 1)))
            for D in (L, 1):                             # two segments, disjoint and at the largest overlap
                i += 1
                out.append(('L%d_K2_D%d_%s' % (L, D, win), L, D, 2, 0, KIND_PAIRS[i % 3], 0, win, i % 2 == 0, (0, 2)))
    return out


def _spp_case(name, L, D, a, b, kinds, win, det):
    return (name, L, D, a * pc.segs_per_part(L, D) + b, 0, kinds, 0, win, det, (a, b))


CASES = _few_segments() + [
    _spp_case('L8_D1_3_parts_plus_1', 8, 1, 3, 1, ('white', 'walk', 'tone'), 'hann', True),
    _spp_case('L64_D1_part_plus_1', 64, 1, 1, 1, ('white', 'walk', 'tone'), 'boxcar', False),
    _spp_case('L512_half_overlap_3_parts_plus_1', 512, 256, 3, 1, ('white', 'tone'), 'hann', True),
    _spp_case('L2048_step_L_minus_1', 2048, 2047, 2, 1, ('walk', 'small'), 'hann', False),
]
IDS = [c[0] for c in CASES]
assert len(set(IDS)) == len(IDS)


def case_of(name):
    return CASES[IDS.index(name)]


# ---- single bins
BIN_L = (8, 128, 1024, 4096)
BIN_OPTIONS = (('boxcar', False), ('hann', True))
BIN_AMPS = (1.0, 1e-6)
BIN_K, BIN_PHASE = 3, 0.3


def bins_of(L):
    """0, 1, 2, 3, L/4 - 1 .. L/4 + 1, L/2 - 2 .. L/2 and every 2^k, 2^k +- 1 below L/2, ascending; up to L = 128, where it is
    cheap, EVERY bin, so that every butterfly of a one-wavefront transform owns a bin of the list.  (A butterfly that read its own
    odd output for the mirror would mix bin k with L/2 - k: the list sees that where it has k or L/2 - k, the broadband shapes
    see it everywhere.)"""
    if L <= 128:
        return list(range(L // 2 + 1))
    b = {0, 1, 2, 3, L // 4 - 1, L // 4, L // 4 + 1, L // 2 - 2, L // 2 - 1, L // 2}
    p = 1
    while p < L // 2:
        b |= {p - 1, p, p + 1}
        p *= 2
    return sorted(k for k in b if 0 <= k <= L // 2)


def single_bins(L):
    """(a, n, pairs, what): K = 3 segments at D = L.  Row 3 i is cos at bin k_i, rows 3 i + 1 and 3 i + 2 are sin at bin k_i times
    1 and 1e-6, all with a phase of 0.3.  Per bin and amplitude two pairs: ('next', k_i, k_i+1, amp), x = cos at k_i against
    y = sin at the NEXT bin of the list (cyclically) -- pxx lives at k_i, pyy at k_i+1 and pxy nowhere -- and ('same', k_i, k_i,
    amp), the quadrature pair on one bin."""
    ks = bins_of(L)
    n = BIN_K * L
    t = np.arange(n)
    a = np.empty((3 * len(ks), n))
    for i, k in enumerate(ks):
        th = 2 * np.pi * ((k * t) % L) / L + BIN_PHASE
        a[3 * i] = np.cos(th)
        for m, amp in enumerate(BIN_AMPS):
            a[3 * i + 1 + m] = amp * np.sin(th)
    pairs, what = [], []
    for i, k in enumerate(ks):
        nx = (i + 1) % len(ks)
        for m, amp in enumerate(BIN_AMPS):
            pairs.append((3 * i, 3 * nx + 1 + m))
            what.append(('next', k, ks[nx], amp))
            pairs.append((3 * i, 3 * i + 1 + m))
            what.append(('same', k, k, amp))
    return a, n, pairs, what


# ---- where a non-finite sample sits
PLACE_SHAPES = ((128, 2, 1), (2048, 1, 1))               # (L, a, b): K = a segs_per_part + b at D = L
PLACE_OPTIONS = (('hann', True), ('hann', False), ('boxcar', False))


def placement_segments(K, spp):
    """The first two segments, one in the middle of part 0, its last, the first and the last of part 1 and the first of part 2,
    where the series has them."""
    return sorted(s for s in {0, 1, spp // 2, spp - 1, spp, 2 * spp - 1, 2 * spp} if s < K)


def placement_pairs(K, spp):
    """The length of `placements`' table: four pairs per marked row (9 per segment and 4 more) and the +-Inf pair."""
    return 4 * (9 * len(placement_segments(K, spp)) + 4) + 1


def placements(L, K, spp):
    """D = L, so every sample belongs to exactly one segment.  Clean series on the even rows; every odd row holds ONE mark of its
    own.  Returns (clean, marked, table, hit, what, inf_pair): `table` has, for every marked row m with clean neighbours c0 = m - 1
    and c1 = m + 1, the pairs (c0, m), (m, c0), (m, m), (c0, c1), and last the pair of the two rows with +Inf and -Inf at the same
    sample; `hit` is the set of table rows that hold a marked series."""
    import psd_exact as px
    n = K * L
    segs = placement_segments(K, spp)
    places = [(s, k, v) for s in segs for k in (0, L // 2, L - 1) for v in (np.nan, np.inf, -np.inf)]
    M = len(places) + 4
    S = 2 * M + 1
    kinds = ('white', 'tone', 'walk')
    clean = np.stack([px.series(kinds[r % 3], n, 100 + r) for r in range(S)])
    marked = clean.copy()
    what = {}
    for i, (s, k, v) in enumerate(places):
        marked[2 * i + 1, s * L + k] = v
        what[2 * i + 1] = 'segment %d sample %d value %r' % (s, k, v)
    r = 2 * len(places) + 1
    mid = segs[len(segs) // 2]
    marked[r, mid * L + 3] = np.inf
    marked[r, mid * L + L - 5] = -np.inf
    what[r] = '+Inf and -Inf in segment %d' % mid
    marked[r + 2, mid * L + 7] = np.inf
    what[r + 2] = '+Inf in segment %d sample 7' % mid
    marked[r + 4, mid * L + 7] = -np.inf
    what[r + 4] = '-Inf in segment %d sample 7' % mid
    marked[r + 6, :] = 1.7e308
    what[r + 6] = '1.7e308 throughout: finite samples, the segment sum overflows'
    assert np.isfinite(marked[r + 6]).all() and sorted(what) == list(range(1, S, 2)) and r + 6 == S - 2
    assert np.isfinite(marked[0::2]).all() and np.array_equal(marked[0::2], clean[0::2])
    table, hit = [], []
    for m in sorted(what):
        table += [(m - 1, m), (m, m - 1), (m, m), (m - 1, m + 1)]
        hit += [len(table) - 4, len(table) - 3, len(table) - 2]
    table.append((r + 2, r + 4))
    hit.append(len(table) - 1)
    assert len(table) == placement_pairs(K, spp)
    return clean, marked, table, hit, what, (r + 2, r + 4)


# ---- magnitude alone
SCALED_SHAPES = ('L128_K3_unaligned_hann_detrend', 'L4096_no_overlap_2_parts_plus_1')
UP, DOWN = 460, -300


def scaled_rows(name):
    """(case, a, n): the 'white' and the 'tone' row of a csd_cases shape, nothing else -- not the offset of 1e6 and not 1e-6."""
    case = cc.CASES[cc.IDS.index(name)]
    n = cc.shape(case)[0]
    kinds = case[5]
    a = cc.rows(case)[[kinds.index('white'), kinds.index('tone')]][:, :n]
    return case, np.ascontiguousarray(a), n


SCALED_PAIRS = [(0, 1), (1, 0), (0, 0)]

# ---- the sampling rate
RATES = (1e-3, 1.0, 12345.678, 1e6)
RATE_SHAPE = 'L256_K3_unaligned_hann_detrend'

# ---- as many pairs as the grid takes: L = 8, D = 3, n = 17, a table that cycles over 64 base pairs of 16 series
GRID_L, GRID_D, GRID_N = 8, 3, 17


def grid_inputs():
    import psd_exact as px
    a = np.stack([(1e-6 if r % 7 == 3 else 1.0) * px.series(px.KINDS[r % 5], GRID_N, 300 + r) for r in range(16)])
    base = [(i, i) for i in range(16)] + [(i, (i + 3) % 16) for i in range(16)] + [((i + 3) % 16, i) for i in range(16)]
    base += [(i, (5 * i + 2) % 16) for i in range(16)]
    assert len(base) == 64 and len(set(base)) == 64
    return a, base
