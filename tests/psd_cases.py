"""The shapes of the Welch PSD tests, shared by test_psd_oracle.py (the plan and the float64 restatement of every shape, without a
device), test_gpu_psd.py (parity with psd_exact under its tolerance) and test_gpu_psd_edges.py (which also takes the helper that
runs a batch on the device from here), and the margin of the test that takes a requested vibration spectrum back out.

A case: id, L, D, K, tail, kinds, pad, window, detrend, where.
  n = (K - 1) D + L + tail samples per series (tail < D: samples the call must not read), series_stride = n + pad,
  one series per entry of `kinds` (psd_exact.series), `where` = (a, b) when the case sits at K = a * segs_per_part + b.
The cross product is not run: every edge appears at least once and the id says which.

Requested spectrum (test_gpu_psd.py::test_the_requested_vibration_spectrum_comes_back): measured on the CPU, the float64 NumPy
chain -- ginsim.psd_amplitudes, a random phase per bin, np.fft.irfft, the constant of gravity added, psd_exact.restated -- against
the requested PSD on the series' grid reaches REQUESTED_NUMPY = 0.022 of psd_exact.tol (with the requested PSD as P) at worst over
8 draws of the phases (tests/test_psd_oracle.py::test_requested_spectrum_chain_in_numpy prints and bounds it); the device is
allowed REQUESTED_MARGIN = 16 times that, the project's convention for a device against its restatement."""
import numpy as np

KINDS5 = ('white', 'offset', 'walk', 'tone', 'constant')


def segs_per_part(L, D):
    """The partition of csrc/psd.hpp restated: segments per part, a function of (L, D) alone."""
    return 2 * max(8192 // D, 2 * L // D, 1)


CASES = [
    # id                                      L     D     K   tail kinds                       pad window    detrend where
    ('L8_K3_odd_count_tail',                  8,    4,    3,  3,   ('white', 'offset', 'tone'), 0,  'hann',   True,  None),
    ('L8_D1_boxcar_raw_S1',                   8,    1,    50, 0,   ('white',),                  0,  'boxcar', False, None),
    ('L64_D3_fewer_bins_than_lanes',          64,   3,    41, 2,   KINDS5,                      5,  'hann',   True,  None),
    ('L64_D1_raw',                            64,   1,    300, 0,  ('walk',),                   0,  'hann',   False, None),
    ('L128_one_bin_more_than_lanes',          128,  32,   7,  0,   ('white', 'tone', 'offset'), 0,  'boxcar', True,  None),
    ('L256_step_half_plus_one',               256,  129,  6,  100, KINDS5,                      0,  'hann',   True,  None),
    ('L512_half_overlap_stride',              512,  256,  5,  0,   ('white', 'walk', 'tone'),   3,  'hann',   True,  None),
    ('L1024_S65_K_part_plus_1_stride_tail',   1024, 512,  33, 100, KINDS5 * 13,                 24, 'hann',   True,  (1, 1)),
    ('L1024_K_2_parts_plus_1_no_overlap',     1024, 1024, 33, 0,   ('white', 'offset', 'walk'), 0,  'boxcar', True,  (2, 1)),
    ('L1024_K2_quarter_step_raw',             1024, 256,  2,  17,  ('tone',),                   0,  'hann',   False, None),
    ('L4096_K_one_part_no_tail',              4096, 4096, 4,  0,   KINDS5,                      0,  'hann',   True,  (1, 0)),
    ('L4096_quarter_step_boxcar_raw',         4096, 1024, 9,  500, ('white', 'offset', 'tone'), 0,  'boxcar', False, None),
    ('L8192_K1_n_equals_L',                   8192, 4096, 1,  0,   ('white', 'offset', 'walk'), 0,  'hann',   True,  None),
    ('L8192_half_overlap_K_part_plus_1_tail', 8192, 4096, 9,  1000, KINDS5,                     0,  'hann',   True,  (1, 1)),
    # appended (the ids and positions above stay): the three segment lengths no case above launches -- 16 and 32, smaller than a
    # wavefront and a single row of the planes, 2048, the first with 512 threads -- and part boundaries crossed at small and odd
    # steps, with last parts of 1, 2 and 3 segments and a series of three full parts
    ('L16_K5_odd_tail',                       16,   5,    5,  4,   ('white', 'offset', 'tone'), 0,  'hann',   True,  None),
    ('L32_D7_boxcar_raw_stride',              32,   7,    12, 0,   KINDS5,                      3,  'boxcar', False, None),
    ('L2048_half_overlap_part_plus_3',        2048, 1024, 19, 700, KINDS5,                      0,  'hann',   True,  (1, 3)),
    ('L2048_no_overlap_boxcar_raw',           2048, 2048, 9,  0,   ('white', 'offset', 'walk'), 8,  'boxcar', False, (1, 1)),
    ('L8_D1_two_parts_plus_1',                8,    1,    32769, 0, ('white', 'walk', 'offset'), 0, 'hann',   True,  (2, 1)),
    ('L64_D3_part_plus_2',                    64,   3,    5462, 2, ('white', 'walk', 'tone'),   1,  'hann',   True,  (1, 2)),
    ('L128_no_overlap_part_plus_1',           128,  128,  129, 0,  ('white', 'offset', 'constant'), 0, 'boxcar', True, (1, 1)),
    ('L256_D129_three_full_parts',            256,  129,  378, 100, KINDS5,                     0,  'hann',   True,  (3, 0)),
    ('L512_D511_part_plus_3',                 512,  511,  35, 0,   ('white', 'walk', 'tone'),   5,  'boxcar', True,  (1, 3)),
    ('L4096_D64_dense_overlap_part_plus_1',   4096, 64,   257, 63, ('white', 'offset', 'walk'), 0,  'hann',   True,  (1, 1)),
    ('L8192_no_overlap_two_parts_plus_1',     8192, 8192, 9,  0,   ('white', 'tone', 'walk'),   0,  'hann',   False, (2, 1)),
]
IDS = [c[0] for c in CASES]


def shape(case):
    """(n, S, stride) of a case."""
    _, L, D, K, tail, kinds, pad, _, _, _ = case
    assert 0 <= tail < D or tail == 0
    n = (K - 1) * D + L + tail
    return n, len(kinds), n + pad


def rows(case, seed=11):
    """The case's series as an (S, stride) array; the pad between the series holds NaN, which nothing may read."""
    import psd_exact as px
    n, S, stride = shape(case)
    a = np.full((S, stride), np.nan)
    for s, kind in enumerate(case[5]):
        a[s, :n] = px.series(kind, n, seed + 17 * s)
    return a


def device_psd(ctx, a, n, L, D, win, det, fs=100.0):
    """ginsim.welch_psd on the rows of `a` (S, stride), of which n samples each are the series: (psd, freq)."""
    import ginsim
    buf = ctx.upload(np.ascontiguousarray(a))
    try:
        return ginsim.welch_psd(ctx, buf, n, a.shape[0], a.shape[1], fs, L, D, win, det)
    finally:
        buf.free()


# the requested vibration spectrum: four points up to fs / 2 = 50 Hz, NOT the series' own grid, zero at fs / 2 (the generator
# takes the real part of that bin only, so its line would scatter with the phase)
REQUESTED_FS = 100.0
REQUESTED_N = 8192
REQUESTED_FREQ = np.array([0.0, 5.0, 20.0, 50.0])
REQUESTED_PSD = {'x': np.array([1e-4, 4e-4, 1e-4, 0.0]), 'y': np.array([2e-4, 2e-4, 2e-4, 0.0]), 'z': np.array([0.0, 9e-4, 1e-5, 0.0])}
REQUESTED_NUMPY = 0.022
REQUESTED_MARGIN = 16.0


def requested_on_grid(axis):
    """The requested PSD interpolated to the 4097 bins of the 8192-sample series."""
    L = REQUESTED_N // 2 + 1
    return np.interp(np.linspace(0, REQUESTED_FS / 2.0, L), REQUESTED_FREQ, REQUESTED_PSD[axis])
