"""The readers of kept trajectories across the runs (csrc/traj_error.hpp: WorkUnit, run_origin, quantity_error, run_slices) on
CONSTRUCTED planes and origin tables (tests/traj_planes.py): curve_partial / curve_final (error_curve.hip), cov_partial / cov_final
(error_cov.hip), radial_keys (error_quantile.hip), process_stats and the end statistics from trajectories (stats.hip), each through
its raw entry point, fp64 and fp32, against the NumPy restatements tests/error_curve_ref.py, error_covariance_ref.py and
error_quantiles_ref.py.  Six samples per plane; nothing here runs a Monte-Carlo launch.

The fp32 planes hold displacements from an origin table with MORE THAN ONE ROW, whose rows differ by kilometres (ref_frame 1) or by
1e-3 rad and 50 m (ref_frame 0).  The expectations are formed from float64(origin[row(r)]) + float64(float32 displacement), row(r)
= ini_first + r < n_ini ? ini_first + r : 0.  A reader that took another row for a run -- the lane, the run of the slice, the first
run of a pair, ini_first forgotten -- moves that run's position error by kilometres or by 1e-3 rad: no tolerance below can absorb
that (the largest is 2e-8 m plus rounding).

What each run count reaches (n = 6; slice counts are csrc's run_slices, restated in traj_planes.py and asserted by
test_every_shape_reaches_the_path_it_is_here_for, so that a change of kTargetWaves or of a cap cannot turn these into one-slice
cases unnoticed).  "all" = every sample (m = 6), "one" = [5] (m = 1), "list" = 128 shuffled entries with repeats (m = 128):

    runs    curve (error_curve.hip)                                cov / keys (one run per lane)
    1, 2    one run per lane, 1 slice                              1 slice; most lanes empty
    64      one run per lane, 1 slice, every lane one run          1 slice
    65      one run per lane, 2 slices (lane 0 of slice 1)         2 slices
    127     one run per lane (odd), 2 slices                       2 slices
    128     TWO runs per lane, 1 slice, every lane a pair          2 slices
    129     one run per lane (odd), 3 slices                       3 slices
    130     two runs per lane, 2 slices, 63 lanes of slice 1 empty 3 slices
    8322    two per lane: all / one 66 slices, one pass, the       all / one 131 slices (cov_final: three rounds);
            final kernel folds in two rounds of 64; list: 64       list: 64 slices, three passes of 4096 runs: kCovBatch's
            slices, TWO passes of the run loop.  Unaligned planes  second load of the second trip is past the end
            (offset): one per lane, 131 slices
    16449   odd, one per lane: all / one 258 slices wanted, 256    cov 256 (the cap), keys 258; slice 0 and lane 0 of slice 1
            taken: slice 0 and lane 0 of slice 1 make a second     take run 16384 and on in a second pass (cov: the second
            pass; list: 64 slices, five passes                     load of the one trip)

Sample traj_planes.EDGE_SAMPLE carries attitude errors of exactly +-pi, +-2 pi, +-nextafter(pi), +-7 in its first runs; sample
traj_planes.BAD_SAMPLE is not finite in run 0 (NaN in c3, +inf in c7) and in the last run (-inf in c7), so the shift about the
first run's error falls back to 0 there; c5 and c8 carry a common offset 1e6 and 1e12 times their spread.

Tolerances.  Curve: test_gpu_error_curve._assert_curve (rtol 1e-12 mean / max, 1e-9 std, atol 1e-9, 2e-8 for NED metres, or the
restatement's own bound where larger), and for c5, c6 and c8 ALSO the long-double statistic of the same float64 errors with mean
rtol 1e-12, std rtol 1e-9 and no absolute floor (c6: std at most the restated bound, which is 0): NumPy's float64 np.std is the
inaccurate side at c8, its floor would hide an accumulator that forgot the shift.  c5 is left out of that second comparison where
the position error is formed in NED metres: there it is no longer "the same float64 error" -- the device's geodetic conversion and
NumPy's differ by the rounding of ECEF coordinates (1e-9 m, 1e-6 of c5's spread), which the project bounds by 2e-8 m absolute.
Covariance: error_covariance_ref.bounded / assert_record, with input_slack(2e-8 m) for NED positions only.  Keys:
error_quantiles_ref.key_tolerance.  Process statistics: rtol 1e-12 max and mean, 1e-9 std, atol 1e-10 (2e-8 for NED metres), the
absolute terms of tests/test_process_stats.py.  Every comparison prints its largest |d| / tol; the module prints the largest per
family when it is done.  Measured on the MI355X: curve 0.064, curve against long double 5.8e-5, covariance 0.12, keys 0.11,
process statistics 0.62 (c8's std over six samples, 1e-11 against the 1e-10 floor), end statistics against the curve 1.8e-6.
"""
import functools
import os

import numpy as np
import pytest

from conftest import PKG
import error_covariance_ref as cov_ref
import error_curve_ref
import error_quantiles_ref as key_ref
import traj_planes as tp
from test_gpu_error_curve import _assert_curve, _atol, RTOL

pytestmark = pytest.mark.gpu

N = 6
RUNS = (1, 2, 64, 65, 127, 128, 129, 130, 8322, 16449)
FRAMES = ('rf1', 'rf0', 'rf0_ned')
LIST128 = np.random.RandomState(128).randint(0, N, size=128)         # shuffled, every sample many times
SAMPLE_SETS = (('all', None), ('one', np.array([N - 1])), ('list', LIST128))
K = tp.kernel_constants(os.path.join(PKG, 'csrc'))
WORST = {}


def _tables(runs):
    """The fp32 origin tables (n_ini, ini_first) by name.  The last two are the two sides of the fall-back to row 0: only run 0 has
    a row of its own / no run has."""
    return {'t1_0': (1, 0), 't3_0': (3, 0), 't3_2': (3, 2), 'tR5_2': (runs + 5, 2), 'tR_Rm1': (runs, runs - 1), 't4_4': (4, 4)}


def _variants(runs):
    """fp64 and the six fp32 tables of a run count."""
    return ['f64'] + list(_tables(runs))


CASES = [pytest.param(r, v, id='%d-%s' % (r, v)) for r in RUNS for v in _variants(r)]
SMALL_CASES = [pytest.param(r, v, id='%d-%s' % (r, v)) for r in (1, 65, 130) for v in _variants(r)]


@pytest.fixture(scope='module')
def ctx():
    import ginsim
    c = ginsim.Context(0)
    yield c
    c.close()
    for family in sorted(WORST):
        print('largest |d| / tol, %s: %.3g' % (family, WORST[family]))


def _note(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), float(ratio))


def _frame(frame):
    return (1 if frame == 'rf1' else 0), frame == 'rf0_ned'


class _Case(object):
    """The planes of one (runs, ref_frame, variant) and, computed once and left unchanged, the restatements on what a reader sees."""

    def __init__(self, runs, rf, variant):
        self.runs, self.rf, self.f32 = runs, rf, variant != 'f64'
        series, self.ref_nav = tp.planes(runs, N, rf, seed=1000 * rf + runs)
        if self.f32:
            self.n_ini, self.first = _tables(runs)[variant]
            self.host, self.origin, self.seen = tp.split(series, rf, self.n_ini, self.first)
        else:
            self.host, self.origin, self.seen, self.first = series, None, series, 0
        self._memo = {}

    def upload(self, ctx, offset=False):
        return tp.Planes(ctx, self.host, self.ref_nav, f32=self.f32, origin=self.origin, first=self.first, offset=offset)

    def _once(self, key, make):
        if key not in self._memo:
            with np.errstate(invalid='ignore', over='ignore'):
                self._memo[key] = make()
        return self._memo[key]

    def errors(self, ned):
        return self._once(('e', ned), lambda: error_curve_ref.errors(self.seen, self.ref_nav, None, ned))

    def curve(self, ned):
        return self._once(('curve', ned), lambda: error_curve_ref.curve(self.seen, self.ref_nav, None, ned))

    def exact(self, ned):
        """(mean, std) (n, 9) of the float64 errors, evaluated in long double: about the first run's error (the differences of
        neighbouring float64 numbers are exact in long double) and with the runs on the last, contiguous axis, which NumPy sums
        pairwise.  Summed row by row along axis 0 the long-double mean of 8322 equal numbers of 1e6 came out 1e-10 off, 1e-4 of
        c8's spread."""
        def make():
            e = np.ascontiguousarray(np.moveaxis(self.errors(ned), 0, 2)).astype(np.longdouble)      # (n, 9, runs)
            d = e - e[:, :, 0:1]
            return e[:, :, 0] + d.mean(axis=2), d.std(axis=2)
        return self._once(('exact', ned), make)

    def cov(self, which, ned):
        def make():
            e = cov_ref.errors3(self.seen, self.ref_nav, None, which, ned)
            b = cov_ref.bounded(e)
            slack = cov_ref.input_slack(b['rec'], cov_ref.component_tolerance(e, which, ned)) if (ned and which == 0) else None
            return b, slack
        return self._once(('cov', which, ned), make)

    def keys(self, which, ned):
        return self._once(('keys', which, ned), lambda: key_ref.keys(self.seen, self.ref_nav, None, which, ned))


@functools.lru_cache(maxsize=None)
def _case(runs, rf, variant):
    return _Case(runs, rf, variant)


def _rows(rows):
    return np.arange(N) if rows is None else np.asarray(rows)


# ------------------------------------------------------------------------------------------ the shapes
def test_every_shape_reaches_the_path_it_is_here_for():
    """The slice counts and passes the module docstring names, from the restatement of run_slices with kTargetWaves and the caps
    read from the sources."""
    assert K == {'target': 8192, 'curve': 256, 'cov': 256, 'cov_batch': 2, 'keys': 1024}
    m_of = {'all': N, 'one': 1, 'list': 128}
    curve = {(r, s): tp.curve_slices(r, m_of[s], K) for r in RUNS for s in m_of}
    cov = {(r, s): tp.cov_slices(r, m_of[s], K) for r in RUNS for s in m_of}
    keys = {(r, s): tp.key_slices(r, m_of[s], K) for r in RUNS for s in m_of}
    assert [tp.curve_vec(r) for r in RUNS] == [1, 1, 1, 1, 1, 2, 1, 2, 2, 1]
    assert [curve[r, 'all'] for r in RUNS] == [1, 1, 1, 2, 2, 1, 3, 2, 66, 256]
    assert [curve[r, 'one'] for r in RUNS] == [1, 1, 1, 2, 2, 1, 3, 2, 66, 256]
    assert [curve[r, 'list'] for r in RUNS] == [1, 1, 1, 2, 2, 1, 3, 2, 64, 64]
    assert [cov[r, 'all'] for r in RUNS] == [1, 1, 1, 2, 2, 2, 3, 3, 131, 256] == [cov[r, 'one'] for r in RUNS]
    assert [keys[r, 'all'] for r in RUNS] == [1, 1, 1, 2, 2, 2, 3, 3, 131, 258] == [keys[r, 'one'] for r in RUNS]
    assert [cov[r, 'list'] for r in RUNS] == [1, 1, 1, 2, 2, 2, 3, 3, 64, 64] == [keys[r, 'list'] for r in RUNS]
    # more than 64 slices: the final kernels fold in more than one round
    assert curve[8322, 'all'] > 64 and cov[8322, 'all'] > 128
    # passes of the run loop
    assert tp.passes(8322, curve[8322, 'all'], 128) == 1 and tp.passes(8322, curve[8322, 'list'], 128) == 2
    assert tp.passes(8322, keys[8322, 'list'], 64) == 3
    trips = tp.passes(8322, cov[8322, 'list'], 64 * K['cov_batch'])
    assert trips == 2 and (trips * K['cov_batch'] - 1) * cov[8322, 'list'] * 64 >= 8322      # the last load of slice 0 is past the end
    assert tp.passes(16449, curve[16449, 'all'], 64) == 2 and tp.passes(16449, keys[16449, 'all'], 64) == 1
    assert tp.passes(16449, cov[16449, 'all'], 64) == 2 and tp.passes(16449, curve[16449, 'list'], 64) == 5
    # planes that are not 16-byte aligned: one run per lane
    assert [tp.curve_slices(r, N, K, aligned=False) for r in (128, 130, 8322)] == [2, 3, 131]
    # the rows the origin tables give: every rule of row(r) occurs
    for runs in RUNS:
        t = _tables(runs)
        assert np.all(tp.origin_row(np.arange(runs), *t['t1_0']) == 0) and np.all(tp.origin_row(np.arange(runs), *t['t4_4']) == 0)
        assert tp.origin_row(np.arange(runs), *t['tR5_2']).tolist() == list(range(2, runs + 2))
        assert tp.origin_row(np.arange(runs), *t['tR_Rm1']).tolist() == [runs - 1] + [0] * (runs - 1)
        assert tp.origin_row(np.arange(runs), *t['t3_2']).tolist() == [2] + [0] * (runs - 1)
        assert tp.origin_row(np.arange(runs), *t['t3_0']).tolist() == ([0, 1, 2] + [0] * runs)[:runs]


def test_the_constructed_planes_are_what_they_claim():
    """Wraps, edge rows, non-finite sample, conditioning and the split into origin + float displacement, on the host."""
    for rf in (0, 1):
        series, ref = tp.planes(130, N, rf, seed=3)
        with np.errstate(invalid='ignore'):
            e = series - ref[None]
        assert np.array_equal(e[:8, tp.EDGE_SAMPLE, 0], tp.EDGE_ERRORS) and np.array_equal(e[:8, tp.EDGE_SAMPLE, 1], -tp.EDGE_ERRORS)
        wraps = np.mean(np.abs(e[:, 0, 0]) > np.pi)
        assert 0.2 < wraps < 0.6, wraps
        bad = ~np.isfinite(series)
        assert bad.sum() == 3 and bad[0, tp.BAD_SAMPLE, 3] and bad[0, tp.BAD_SAMPLE, 7] and bad[129, tp.BAD_SAMPLE, 7]
        assert np.all(e[:, :, 6] == e[0:1, :, 6]) and np.all(e[:, :, 6] != 0.0)
        clean = np.delete(e, tp.BAD_SAMPLE, axis=1)
        assert np.all(np.abs(clean[..., 5].mean(0)) > 1e5 * clean[..., 5].std(0))
        assert np.all(np.abs(clean[..., 8].mean(0)) > 1e11 * clean[..., 8].std(0))
        disp, origin, seen = tp.split(series, rf, 135, 2)
        assert disp.dtype == np.float32 and origin.shape == (135, 3)
        step = np.abs(np.diff(origin, axis=0)).mean(axis=0)
        assert np.all(step > (np.array([1e-4, 1e-4, 5.0]) if rf == 0 else 300.0))
        fin = np.isfinite(series[..., 3:6])
        close = np.array([1e-9, 1e-9, 1e-2]) if rf == 0 else np.full(3, 1e-3)       # half a float ulp of the displacement
        assert np.all(np.abs(np.where(fin, seen[..., 3:6] - series[..., 3:6], 0.0)) <= close)
        assert np.array_equal(seen[1, :, 3:6], origin[3][None] + disp[1, :, 3:6].astype(np.float64))


# ------------------------------------------------------------------------------------------ the curve
def _curve_ratio(got, want, rows, ned):
    rows, worst = _rows(rows), 0.0
    with np.errstate(invalid='ignore'):
        for key, dev in (('max', got.maxabs), ('avg', got.mean), ('std', got.std)):
            ref = want[key][rows]
            tol = np.maximum(_atol(ned) + RTOL[key] * np.abs(ref), want['tol_' + key][rows])
            fin = np.isfinite(ref)
            worst = max(worst, np.max(np.where(fin, np.abs(dev - ref) / tol, 0.0)))
    return worst


def _assert_exact(got, case, want, rows, ned, what):
    """c5 (not in NED metres), c6 and c8 against the long-double statistic of the same float64 errors: mean rtol 1e-12, std rtol
    1e-9 (c6: at most the restated bound), no absolute term."""
    rows = _rows(rows)
    mean, std = case.exact(ned)
    for c in ((6, 8) if ned else (5, 6, 8)):
        dm = np.abs(got.mean[:, c].astype(np.longdouble) - mean[rows, c])
        rm = float(np.max(dm / (1e-12 * np.abs(mean[rows, c]))))
        _note('curve, c5 c6 c8 against long double', rm)
        assert rm <= 1.0, '%s c%d: mean is %.3g x (1e-12 |mean|) from the long-double mean' % (what, c, rm)
        if c == 6:
            assert np.all(got.std[:, c] <= want['tol_std'][rows, c]), '%s c6: std %s' % (what, got.std[:, c])
            continue
        ds = np.abs(got.std[:, c].astype(np.longdouble) - std[rows, c])
        bound = 1e-9 * std[rows, c]
        assert np.all(ds <= bound), '%s c%d: std %s, long double %s' % (what, c, got.std[:, c], std[rows, c].astype(np.float64))
        rs = float(np.max(np.where(bound > 0, ds / np.where(bound > 0, bound, 1), 0.0)))
        _note('curve, c5 c6 c8 against long double', rs)
        print('%s c%d: mean %.3g, std %.3g of the rtol-only bound' % (what, c, rm, rs))


@pytest.mark.parametrize('frame', FRAMES)
@pytest.mark.parametrize('runs,variant', CASES)
def test_curve(ctx, runs, variant, frame):
    """ginsim_error_curve[_f32]: every record of every sample set; two launches give the same bytes; planes that start 8 (fp64) or
    4 (fp32) bytes into their region, which are read one run per lane, meet the same tolerances."""
    rf, ned = _frame(frame)
    case = _case(runs, rf, variant)
    want = case.curve(ned)
    if runs >= 3:
        bad = ~np.isfinite(want['avg'])
        assert bad[tp.BAD_SAMPLE, 3] and bad[tp.BAD_SAMPLE, 7] and not np.delete(bad, tp.BAD_SAMPLE, axis=0).any()
        assert np.isnan(want['avg'][tp.BAD_SAMPLE, 7]) and np.isinf(want['max'][tp.BAD_SAMPLE, 7])    # +inf and -inf: no mean
    aligned, shifted = case.upload(ctx), case.upload(ctx, offset=True)
    for name, rows in SAMPLE_SETS:
        what = 'curve %s %d %s %s' % (frame, runs, variant, name)
        got = aligned.curve(rows, ned)
        assert np.all(got.count == runs)
        _assert_curve(got, want, rows, ned, what=what)
        _note('curve', _curve_ratio(got, want, rows, ned))
        _assert_exact(got, case, want, rows, ned, what)
        assert aligned.curve(rows, ned).pack().tobytes() == got.pack().tobytes(), what + ': two launches of the same shape differ'
        off = shifted.curve(rows, ned)
        assert np.all(off.count == runs)
        _assert_curve(off, want, rows, ned, what=what + ' offset')
        _note('curve', _curve_ratio(off, want, rows, ned))
        _assert_exact(off, case, want, rows, ned, what + ' offset')
    aligned.free()
    shifted.free()


# ------------------------------------------------------------------------------------------ the covariance
def _cov_ratio(got, b, slack):
    tm, tc = b['tol_mean'].copy(), b['tol_c'].copy()
    if slack is not None:
        tm, tc = tm + slack[0], tc + slack[1]
    want = b['rec']
    fin = np.isfinite(want[:, 1:])
    d = np.where(fin, np.abs(np.where(fin, got[:, 1:], 0.0) - np.where(fin, want[:, 1:], 0.0)), 0.0)
    tol = np.where(fin, np.concatenate([tm, tc], axis=1), 0.0)
    with np.errstate(invalid='ignore', divide='ignore'):
        return float(np.max(np.where(d > 0.0, d / tol, 0.0)))


@pytest.mark.parametrize('frame', FRAMES)
@pytest.mark.parametrize('runs,variant', CASES)
def test_covariance(ctx, runs, variant, frame):
    """ginsim_error_cov[_f32], position and velocity.  At the sample that is not finite run 0 is counted out of the position record
    and runs 0 and runs - 1 out of the velocity record, and only there."""
    rf, ned = _frame(frame)
    case = _case(runs, rf, variant)
    planes = case.upload(ctx)
    for which in (0, 1):
        b, slack = case.cov(which, ned)
        count = np.full(N, float(runs))
        if runs >= 3:
            count[tp.BAD_SAMPLE] -= 2.0 if which else 1.0
        assert np.array_equal(b['rec'][:, 0], count)
        for name, rows in SAMPLE_SETS:
            what = 'cov %s %d %s which %d %s' % (frame, runs, variant, which, name)
            pick = _rows(rows)
            got = planes.cov(rows, which, ned)
            assert np.array_equal(got.count, count[pick]), what
            bb = {k: v[pick] for k, v in b.items()}
            ss = None if slack is None else (slack[0][pick], slack[1][pick])
            cov_ref.assert_record(got.pack(), bb, what, ss)
            _note('covariance', _cov_ratio(got.pack(), bb, ss))
            assert planes.cov(rows, which, ned).pack().tobytes() == got.pack().tobytes(), what + ': two launches differ'
    planes.free()


# ------------------------------------------------------------------------------------------ the keys
@pytest.mark.parametrize('frame', FRAMES)
@pytest.mark.parametrize('runs,variant', CASES)
def test_keys(ctx, runs, variant, frame):
    """ginsim_radial_keys[_f32], position and velocity, into rows of runs + 3 keys from column 2: the three gap columns keep their
    -7.0.  At 8322 runs ginsim_quantile_rows (0.5, 0.95) over those strided rows is the restatement's nearest rank on the downloaded
    keys, bit for bit."""
    import ginsim
    rf, ned = _frame(frame)
    case = _case(runs, rf, variant)
    planes = case.upload(ctx)
    for which in (0, 1):
        full = case.keys(which, ned)                                            # (3, N, runs)
        for name, rows in SAMPLE_SETS:
            what = 'keys %s %d %s which %d %s' % (frame, runs, variant, which, name)
            want = full[:, _rows(rows)]
            host, buf = planes.keys(rows, which, ned)
            assert host.shape == (3, want.shape[1], runs + 3)
            assert np.all(host[:, :, :2] == -7.0) and np.all(host[:, :, -1] == -7.0), what + ': a gap column was written'
            got = host[:, :, 2:2 + runs]
            np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what + ': NaN mask')
            np.testing.assert_array_equal(np.isinf(got), np.isinf(want), err_msg=what + ': inf mask')
            fin = np.isfinite(want)
            assert np.all(got[fin] >= 0.0)
            tol = np.where(fin, key_ref.key_tolerance(want, which, ned), 0.0)    # the keys that are not finite: by their masks, above
            d = np.where(fin, np.abs(np.where(fin, got, 0.0) - np.where(fin, want, 0.0)), 0.0)
            ratio = np.max(d / np.where(fin, tol, 1.0))
            print('%s: largest |d| / tol = %.3g (|d| %.3g)' % (what, ratio, d.max()))
            _note('keys', ratio)
            worst = np.unravel_index(np.argmax(d - tol), d.shape)
            assert d[worst] <= tol[worst], '%s: key %s is %.3e from the restatement, tolerance %.3e' % (what, worst, d[worst], tol[worst])
            if runs == 8322:
                m = want.shape[1]
                q = ginsim.quantile_rows(ctx, buf.ptr + 2 * 8, 3 * m, runs, runs + 3, (0.5, 0.95))
                qv, qn = key_ref.quantile_rows(got.reshape(3 * m, runs), (0.5, 0.95))
                np.testing.assert_array_equal(q.count, qn, err_msg=what)
                assert np.array_equal(q.values.view(np.uint64), qv.view(np.uint64)), what + ': quantiles'
                np.testing.assert_array_equal(qn, fin.sum(axis=2).reshape(-1), err_msg=what + ': keys that are not finite are left out')
            buf.free()
    planes.free()


# ------------------------------------------------------------------------------------------ the per-run statistics
@pytest.mark.parametrize('frame', FRAMES)
@pytest.mark.parametrize('runs,variant', SMALL_CASES)
def test_process_stats(ctx, runs, variant, frame):
    """ginsim_process_stats[_f32] with 6, 2 and 1 samples in the window: process_stats_kernel cuts it into four segments, so two
    and three of them are empty; against __array_stats over the time axis of the restated errors."""
    rf, ned = _frame(frame)
    case = _case(runs, rf, variant)
    planes = case.upload(ctx)
    e = case.errors(ned)
    atol = np.full(9, 1e-10)
    if ned:
        atol[3:6] = 2e-8
    for first in (0, 4, 5):
        what = 'process %s %d %s first %d' % (frame, runs, variant, first)
        with np.errstate(invalid='ignore', over='ignore'):
            want = error_curve_ref.array_stats(np.moveaxis(e[:, first:], 1, 0))
        got = planes.process_stats(first, ned)
        assert got.shape == (runs, 3, 9)
        worst = 0.0
        for k, (key, rtol) in enumerate((('max', 1e-12), ('avg', 1e-12), ('std', 1e-9))):
            dev, ref = got[:, k], want[key]
            np.testing.assert_array_equal(np.isnan(dev), np.isnan(ref), err_msg='%s %s: NaN mask' % (what, key))
            np.testing.assert_array_equal(np.isposinf(dev), np.isposinf(ref), err_msg='%s %s: +inf mask' % (what, key))
            np.testing.assert_array_equal(np.isneginf(dev), np.isneginf(ref), err_msg='%s %s: -inf mask' % (what, key))
            fin = np.isfinite(ref)
            tol = atol[None] + rtol * np.abs(np.where(fin, ref, 0.0))
            d = np.where(fin, np.abs(np.where(fin, dev, 0.0) - np.where(fin, ref, 0.0)), 0.0)
            worst = max(worst, float(np.max(d / tol)))
            at = np.unravel_index(np.argmax(d - tol), d.shape)
            assert d[at] <= tol[at], '%s %s: run, component %s is %.3e from the restatement, tolerance %.3e' % (what, key, at, d[at], tol[at])
        if runs >= 3 and first <= tp.BAD_SAMPLE:
            assert np.isnan(got[0, :, 3]).all() and got[0, 0, 7] == np.inf and got[0, 1, 7] == np.inf and np.isnan(got[0, 2, 7])
            assert got[runs - 1, 1, 7] == -np.inf and np.isfinite(got[1:runs - 1]).all()
        else:
            assert np.isfinite(got).all()
        print('%s: largest |d| / tol = %.3g' % (what, worst))
        _note('process statistics', worst)
    planes.free()


@pytest.mark.parametrize('frame', FRAMES)
@pytest.mark.parametrize('runs,variant', CASES)
def test_end_statistics_are_the_last_row_of_the_curve(ctx, runs, variant, frame):
    """ginsim_end_stats_from_traj[_f32] against the curve at the last sample, under the rule of tests/test_gpu_error_curve.py's
    test_last_row_is_the_end_point_record: the same maxima, mean and std to rounding, and at 64 runs -- one wavefront, one run per
    lane, the same butterfly about the same shift -- the same bits.  The curve itself is held to the restatement by test_curve."""
    rf, ned = _frame(frame)
    case = _case(runs, rf, variant)
    planes = case.upload(ctx)
    end = planes.end_stats(ned)
    got = planes.curve([N - 1], ned)
    assert got.count[0] == end.count == runs
    if runs == 64:
        assert got.mean[0].tobytes() == end.mean.tobytes()
        assert got.m2[0].tobytes() == end.m2.tobytes()
        assert got.maxabs[0].tobytes() == end.maxabs.tobytes()
    a = _atol(ned)
    np.testing.assert_array_equal(got.maxabs[0], end.maxabs)
    tol_mean, tol_std = a + 1e-12 * np.abs(end.mean), a + 1e-9 * np.abs(end.std)
    assert np.all(np.abs(got.mean[0] - end.mean) <= tol_mean) and np.all(np.abs(got.std[0] - end.std) <= tol_std)
    ratio = max(np.max(np.abs(got.mean[0] - end.mean) / tol_mean), np.max(np.abs(got.std[0] - end.std) / tol_std))
    print('end %s %d %s: largest |d| / tol = %.3g' % (frame, runs, variant, ratio))
    _note('end statistics', ratio)
    # and against the restatement itself, at the curve's tolerance
    want = case.curve(ned)
    import ginsim
    rec = np.empty((1, 9, 4))
    rec[0, :, 0], rec[0, :, 1], rec[0, :, 2], rec[0, :, 3] = end.count, end.mean, end.m2, end.maxabs
    _assert_curve(ginsim.CurveResult(rec), want, [N - 1], ned, what='end %s %d %s' % (frame, runs, variant))
    planes.free()
