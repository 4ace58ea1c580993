"""The shapes of the multi-resolution PSD tests, shared by test_lpsd_oracle.py (the plan and the float64 restatement of every shape,
without a device) and test_gpu_lpsd.py (the device against the long-double restatement).

A case: id, L, D, J, K_last, short, extra, kinds, pad, window, detrend, min_segments, levels.
  n = lpsd_ref.shortest(J, L, D, K_last) - short + extra samples per series: with short = extra = 0 the last level J has exactly
  K_last segments; one sample fewer (short = 1) drops it.  series_stride = n + pad (the pad holds NaN, which nothing may read), one
  series per entry of `kinds` (psd_exact.series), `levels` = the levels the cascade then has (J + 1, or J with short = 1).
The cross product is not run: every edge appears at least once and the id says which.

DEV[id][j]: the float64 restatement (lpsd_ref.lpsd) against the long-double one at level j, the largest |difference| / tolerance
over the case's series and the bins that level reports, with the tolerance of lpsd_ref.level_tol -- psd_exact.tol of the level's
Welch estimate.  Measured on the CPU (long double of 64 mantissa bits) and rounded up to two digits;
test_lpsd_oracle.py::test_recorded_deviation_of_the_float64_restatement recomputes every figure and holds it under its record.
The device is allowed tol * (1 + MARGIN * DEV[id][j]) per bin: the tolerance of the level's Welch estimate plus 16 times what the
restatement's own float64 arithmetic, decimations included, is off by -- the project's margin over an error measured on the
reference side.  psd_exact.tol alone does not cover a level past 0: it bounds the transform's error by the size of the level's own
series, and a decimation rounds at the size of its INPUT.  L1024_J5_raw shows it (4.2 at level 5): the tone of 100 is filtered
away after two levels, its rounding residue of 1e-14 is not, and what is left of the series is noise of 1e-3."""
import numpy as np

KINDS3 = ('white', 'walk', 'tone')
FS = 100.0
MARGIN = 16.0

CASES = [
    # id                            L     D     J  K_last short extra kinds                      pad window    detrend minseg levels
    ('L8_J1_one_segment',           8,    4,    1, 1,     0,    0,    ('white', 'offset', 'tone'), 0,  'hann',   True,  1,     2),
    ('L8_J1_one_short_dropped',     8,    4,    1, 1,     1,    0,    ('white', 'offset', 'tone'), 0,  'hann',   True,  1,     1),
    ('L8_J5_one_bin_levels_raw',    8,    3,    5, 4,     0,    0,    KINDS3,                      3,  'boxcar', False, 1,     6),
    ('L64_J2_minseg3',              64,   32,   2, 3,     0,    0,    KINDS3,                      0,  'hann',   True,  3,     3),
    ('L64_J2_minseg3_one_short',    64,   32,   2, 3,     1,    0,    KINDS3,                      0,  'hann',   True,  3,     2),
    ('L64_J5_D1_boxcar',            64,   1,    5, 2,     0,    0,    ('white', 'walk'),           0,  'boxcar', True,  1,     6),
    ('L1024_J1_stride',             1024, 512,  1, 2,     0,    1,    KINDS3,                      5,  'hann',   True,  1,     2),
    ('L1024_J2_boxcar',             1024, 1024, 2, 2,     0,    0,    ('white', 'offset', 'walk'), 0,  'boxcar', True,  1,     3),
    ('L1024_J5_raw',                1024, 512,  5, 1,     0,    0,    KINDS3,                      0,  'hann',   False, 1,     6),
    ('L8192_J1_one_segment',        8192, 4096, 1, 1,     0,    0,    KINDS3,                      0,  'hann',   True,  1,     2),
    ('L8192_J2_one_short_dropped',  8192, 4096, 2, 1,     1,    0,    ('white', 'tone'),           0,  'hann',   True,  1,     2),
    ('L8192_J5_boxcar',             8192, 4096, 5, 2,     0,    0,    ('white', 'walk'),           0,  'boxcar', True,  1,     6),
]
IDS = [c[0] for c in CASES]

DEV = {
    'L8_J1_one_segment':             (0.026, 0.061),
    'L8_J1_one_short_dropped':       (0.041,),
    'L8_J5_one_bin_levels_raw':      (4.8e-05, 1.4e-05, 1.7e-05, 0.083, 0.002, 0.14),
    'L64_J2_minseg3':                (0.012, 0.00073, 0.02),
    'L64_J2_minseg3_one_short':      (0.012, 0.0031),
    'L64_J5_D1_boxcar':              (3.5e-05, 2.3e-05, 1.4e-05, 1.2e-05, 8.9e-06, 0.00095),
    'L1024_J1_stride':               (0.079, 0.092),
    'L1024_J2_boxcar':               (4.6e-05, 0.069, 0.13),
    'L1024_J5_raw':                  (0.028, 0.029, 0.034, 0.22, 0.49, 4.2),
    'L8192_J1_one_segment':          (0.12, 0.21),
    'L8192_J2_one_short_dropped':    (0.13, 0.13),
    'L8192_J5_boxcar':               (0.00019, 0.00022, 0.00033, 0.00034, 0.00056, 0.0066),
}


def shape(case):
    """(n, S, stride) of a case."""
    import lpsd_ref as ref
    _, L, D, J, K_last, short, extra, kinds, pad = case[:9]
    n = ref.shortest(J, L, D, K_last) - short + extra
    return n, len(kinds), n + pad


def rows(case, seed=23):
    """The case's series as an (S, stride) array; the pad between the series holds NaN."""
    import psd_exact as px
    n, S, stride = shape(case)
    a = np.full((S, stride), np.nan)
    for s, kind in enumerate(case[7]):
        a[s, :n] = px.series(kind, n, seed + 17 * s)
    return a


_reference = {}


def reference(case):
    """(exact, tol, freq, level) of a case, the first two as (S, nbins) arrays: the long-double restatement rounded to float64
    and its tolerance.  Computed once per process and shared; callers leave it unchanged."""
    import lpsd_ref as ref
    if case[0] not in _reference:
        _, L, D, _, _, _, _, _, _, win, det, ms, _ = case
        n, S, _ = shape(case)
        a = rows(case)
        e, t = [], []
        for s in range(S):
            p, f, lev = ref.lpsd(a[s, :n], FS, L, D, win, det, ms, np.longdouble)
            e.append(p.astype(np.float64))
            t.append(ref.level_tol(a[s, :n], FS, L, D, win, det, ms, e[-1]))
        _reference[case[0]] = (np.array(e), np.array(t), f, lev)
    return _reference[case[0]]


def allowed(case):
    """The device's bound per bin as a multiple of the tolerance: 1 + MARGIN * DEV[id][level of the bin]."""
    lev = reference(case)[3]
    return 1.0 + MARGIN * np.asarray(DEV[case[0]])[lev]
