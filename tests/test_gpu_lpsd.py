"""The multi-resolution PSD on the device: ginsim_decimate2 against the long-double restatement of tests/lpsd_ref.py at every tile
edge, its reproducibility and its non-finite rule; ginsim_lpsd against its own parts (bit for bit) and against the restatement
(tests/lpsd_cases.py); the NaN rule per level, the refusals that need a context, the job, job-set and plugin surface, and once the
spectrum of the sensor model's drift.

Measured on one MI355X (every test prints its figure; DESIGN 4.3d has them): decimate2 reaches 0.133 of its a-priori bound; lpsd
reaches 0.097 of its bound at worst (L8_J1_one_segment) and 2.5 of psd_exact.tol alone at level 5 of L1024_J5_raw, where the
float64 restatement is at 4.2; the drift corner's octave medians are within 0.30 of their five standard errors."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import lpsd_cases as lc
import lpsd_ref as ref
import psd_exact as px

pytestmark = pytest.mark.gpu

FS = 100.0
B = ref.TILE


@pytest.fixture(scope='module')
def ctx():
    import ginsim
    c = ginsim.Context(0)
    yield c
    c.close()


def dev_decimate(ctx, a, n, y_pad=2, fill=-7.0):
    """ginsim.decimate2 on the rows of `a` (S, stride), of which n samples each are the series: (S, n_out).  The outputs are
    y_pad apart more than they need, and what lies between them must stay as it was."""
    import ginsim
    S, stride = a.shape
    no = ref.n_out(n)
    xb, yb = ctx.upload(np.ascontiguousarray(a)), ctx.upload(np.full((S, no + y_pad), fill))
    try:
        assert ginsim.decimate2(ctx, xb, n, S, stride, yb, no + y_pad) == no
        y = ctx.download(yb, (S, no + y_pad))
    finally:
        xb.free()
        yb.free()
    assert np.all(y[:, no:] == fill)
    return y[:, :no].copy()


def rows(S, n, pad, seed=3):
    a = np.full((S, n + pad), np.nan)               # the pad holds NaN, which nothing may read
    for s in range(S):
        a[s, :n] = px.series(('white', 'offset', 'walk', 'tone')[s % 4], n, seed + s)
    return a


# ---- one decimation
@pytest.mark.parametrize('n', [27, 28, 29, 2 * B + 25, 2 * B + 26, 2 * B + 27, 4 * B + 26])
def test_decimate2_parity_at_every_tile_edge(ctx, n):
    """Every output within 32 * 2^-53 * sum_t |h[t]| |x[2i+t]| of the long-double restatement: the a-priori bound of the dot
    product for at most 30 operations, whether or not they are fused."""
    worst = 0.0
    for S in (1, 3, 65):
        a = rows(S, n, 3)
        y = dev_decimate(ctx, a, n)
        assert y.shape == (S, ref.n_out(n))
        e = ref.decimate(a[:, :n], np.longdouble)
        bound = ref.decimate_bound(a[:, :n])
        assert np.all(np.isfinite(y)) and np.all(bound > 0)
        r = float(np.max(np.abs(y - e).astype(np.float64) / bound))
        worst = max(worst, r)
        assert r <= 1.0, (n, S, r)
    print('decimate2 n %d (%d outputs, %d tiles): error / bound %.3g' % (n, ref.n_out(n), -(-ref.n_out(n) // B), worst))


def test_decimate2_gives_the_same_bits_whatever_runs_next_to_it(ctx):
    n = 4 * B + 26
    a = rows(3, n, 3)
    y = dev_decimate(ctx, a, n)
    np.testing.assert_array_equal(dev_decimate(ctx, a, n), y)                       # two launches
    b = a.copy()
    b[0, :n] = px.series('walk', n, 99)
    b[2, :n] = 1e300
    np.testing.assert_array_equal(dev_decimate(ctx, b, n)[1], y[1])                 # other neighbours
    np.testing.assert_array_equal(dev_decimate(ctx, a[1:2], n)[0], y[1])            # alone
    big = rows(65, n, 0, seed=40)
    big[37, :n] = a[1, :n]
    np.testing.assert_array_equal(dev_decimate(ctx, big, n)[37], y[1])              # another nseries, stride and place
    # and an output depends on its 27 inputs alone: the same samples 2 * 700 further on come out 700 outputs further on
    c = rows(1, n, 0, seed=8)
    c[0, 1400:n] = a[1, :n - 1400]
    np.testing.assert_array_equal(dev_decimate(ctx, c, n)[0, 700:], y[1, :ref.n_out(n) - 700])
    print('decimate2 reproducibility: error / bound 0 (bitwise)')


def test_decimate2_non_finite_samples_reach_the_outputs_whose_taps_touch_them(ctx):
    n = 4 * B + 26                                  # 2B outputs in two tiles; the last sample, n - 1, is not read at all
    places = [0, n - 1, n - 2, 2 * B - 1, 2 * B, 2 * B + 24]        # first, last, last read, and around the edge of tile 0
    x = px.series('white', n, 21)
    bad = []
    for p in places:
        q = p + 2 if p + 2 < n else p - 2
        bad += [([p], [np.nan]), ([p], [np.inf]), ([p, q], [np.inf, -np.inf])]
    a = np.tile(x, (len(bad) + 1, 1))
    for s, (where, what) in enumerate(bad):
        a[s + 1, where] = what
    y = dev_decimate(ctx, a, n, y_pad=0)
    clean = y[0]
    assert np.all(np.isfinite(clean))
    np.testing.assert_array_equal(clean, dev_decimate(ctx, x[None, :], n)[0])
    for s, (where, what) in enumerate(bad):
        hit = ref.touched(n, where)
        np.testing.assert_array_equal(~np.isfinite(ref.decimate(a[s + 1])), hit)   # the restatement's set
        np.testing.assert_array_equal(~np.isfinite(y[s + 1]), hit)
        np.testing.assert_array_equal(y[s + 1][~hit], clean[~hit])
        if len(where) == 1 and np.isnan(what[0]):
            assert np.all(np.isnan(y[s + 1][hit]))
    assert ref.touched(n, [n - 1]).sum() == 0 and ref.touched(n, [2 * B]).sum() == 14 and ref.touched(n, [2 * B - 1]).sum() == 1
    print('decimate2 non-finite samples: %d placements, the touched sets are the restatement\'s' % len(bad))


# ---- the cascade against its own parts: no tolerance
def dev_lpsd(ctx, a, n, L, D, win, det, ms=1, fs=FS):
    import ginsim
    buf = ctx.upload(np.ascontiguousarray(a))
    try:
        return ginsim.lpsd(ctx, buf, n, a.shape[0], a.shape[1], fs, L, D, win, det, ms)
    finally:
        buf.free()


def test_lpsd_is_welch_psd_of_the_chained_decimations_bit_for_bit(ctx):
    for case in lc.CASES:
        name, L, D, _, _, _, _, _, _, win, det, ms, levels = case
        n, S, stride = lc.shape(case)
        a = lc.rows(case)
        p, f, lev = dev_lpsd(ctx, a, n, L, D, win, det, ms)
        assert p.shape == (S, f.size) and lev.max() == levels - 1, name
        bands = ref.bands(levels, L)
        xj, nj = a, n
        for j in range(levels):
            want, fw = lc_welch(ctx, xj, nj, L, D, win, det, FS / 2 ** j)
            lo, hi = bands[j]
            np.testing.assert_array_equal(p[:, lev == j], want[:, lo:hi + 1], err_msg='%s level %d' % (name, j))
            np.testing.assert_array_equal(f[lev == j], fw[lo:hi + 1])
            if j + 1 < levels:
                xj = dev_decimate(ctx, xj, nj, y_pad=0)
                nj = xj.shape[1]
        assert np.all(np.diff(f) > 0) and f[0] == 0.0 and f[-1] == FS / 2
    print('lpsd vs welch_psd of decimate2 chains over %d shapes: error / bound 0 (bitwise)' % len(lc.CASES))


def lc_welch(ctx, a, n, L, D, win, det, fs):
    import psd_cases as pc
    return pc.device_psd(ctx, a, n, L, D, win, det, fs)


def test_a_series_too_short_for_level_1_gives_welch_psd(ctx):
    """n_1 = (n - 27) // 2 + 1 reaches L at n = 2L + 25: up to 2L + 24 the whole result is welch_psd's."""
    for L, D in ((8, 4), (64, 32), (1024, 512)):
        for n in (L, 2 * L + 24):
            a = rows(3, n, 2)
            p, f, lev = dev_lpsd(ctx, a, n, L, D, 'hann', True)
            want, fw = lc_welch(ctx, a, n, L, D, 'hann', True, FS)
            np.testing.assert_array_equal(p, want)
            np.testing.assert_array_equal(f, fw)
            assert np.all(lev == 0) and f.size == L // 2 + 1
        a = rows(3, 2 * L + 25, 0)
        assert dev_lpsd(ctx, a, 2 * L + 25, L, D, 'hann', True)[2].max() == 1
        assert dev_lpsd(ctx, a, 2 * L + 25, L, D, 'hann', True, ms=2)[2].max() == 0         # level 1 would have one segment
    print('lpsd with a single level: error / bound 0 (bitwise)')


# ---- the cascade against the restatement
@pytest.mark.parametrize('case', lc.CASES, ids=lc.IDS)
def test_lpsd_parity_with_the_long_double_restatement(ctx, case):
    """Per bin within psd_exact.tol of the level's Welch estimate plus 16 times the float64 restatement's recorded deviation at
    that level (lpsd_cases.DEV)."""
    name, L, D, _, _, _, _, _, _, win, det, ms, levels = case
    n, S, stride = lc.shape(case)
    e, t, f, lev = lc.reference(case)
    p, fd, levd = dev_lpsd(ctx, lc.rows(case), n, L, D, win, det, ms)
    np.testing.assert_array_equal(fd, f)
    np.testing.assert_array_equal(levd, lev)
    assert p.shape == e.shape
    bound = t * lc.allowed(case)[None, :]
    r = px.ratio(p, e, bound)
    r_tol = px.ratio(p, e, t)
    print('lpsd %s (%d levels, n %d): error / bound %.3g (error / tol alone %.3g)' % (name, levels, n, r, r_tol))
    assert r <= 1.0


def test_a_non_finite_sample_marks_the_levels_that_read_it(ctx):
    """L = 64, D = 48, n = 351: level 0 reads 304 samples, level 1 (163 samples, 3 segments) the outputs 0 .. 159, that is the
    samples up to 344.  Sample 330 reaches the outputs 152 .. 165 of level 1, of which level 2 (69 samples, one segment of the
    outputs 0 .. 63 made from level 1's 0 .. 152) reads the first."""
    L, D, n = 64, 48, 351
    assert ref.level_lengths(n, L, D) == [351, 163, 69] and (px.segments(n, L, D) - 1) * D + L == 304
    a = rows(3, n, 1)
    clean, f, lev = dev_lpsd(ctx, a, n, L, D, 'hann', True)
    assert np.all(np.isfinite(clean))
    for val in (np.nan, np.inf):
        b = a.copy()
        b[1, 330] = val
        p, _, _ = dev_lpsd(ctx, b, n, L, D, 'hann', True)
        np.testing.assert_array_equal(p[[0, 2]], clean[[0, 2]])
        np.testing.assert_array_equal(p[1, lev == 0], clean[1, lev == 0])
        assert np.all(np.isnan(p[1, lev == 1])) and np.all(np.isnan(p[1, lev == 2]))
    b = a.copy()
    b[1, 346] = np.nan              # outputs 160 .. 166 of level 1: read by no level
    np.testing.assert_array_equal(dev_lpsd(ctx, b, n, L, D, 'hann', True)[0], clean)
    print('lpsd NaN rule per level: error / bound 0 (bitwise)')


def _err():
    from ginsim import _lib
    return _lib.lib.ginsim_last_error().decode()


def test_device_refusals_and_their_order(ctx):
    from ginsim import _lib
    n, L = 400, 64
    buf = ctx.upload(rows(2, n, 0))
    ybuf = ctx.malloc(8 * 2 * n)
    freq, p, lev, nb, no = np.full(200, -3.0), np.full((2, 200), -3.0), np.full(200, -3, dtype=np.int32), C.c_int32(-7), C.c_int64(-7)
    try:
        def call(n=n, S=2, stride=n, fs=FS, L=L, D=32, w=1, d=1, ms=1, cap=200):
            return _lib.lib.ginsim_lpsd(ctx.handle, buf.ptr, n, S, stride, fs, L, D, w, d, ms, _lib.dptr(freq), _lib.dptr(p),
                                        lev.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nb), cap)
        assert call(S=0, L=7, D=0, w=5, ms=0, cap=0) == _lib.ERR_ARG and _err() == 'lpsd: bad sizes'
        assert call(L=7, D=0, w=5, ms=0, cap=0) == _lib.ERR_ARG and _err() == 'lpsd: nperseg 7 is not a power of two in [8, 8192]'
        assert call(D=0, w=5, ms=0, cap=0) == _lib.ERR_ARG and _err() == 'lpsd: step 0 outside [1, 64]'
        assert call(w=5, n=10, ms=0, cap=0) == _lib.ERR_ARG and _err() == 'lpsd: window 5 (0 boxcar, 1 hann) or detrend 1 (0, 1) out of range'
        assert call(n=10, stride=10, ms=0, cap=0) == _lib.ERR_RANGE and _err() == 'lpsd: a series of n = 10 samples is shorter than one segment of nperseg = 64'
        assert call(ms=0, cap=0) == _lib.ERR_ARG and _err() == 'lpsd: min_segments 0 must be at least 1'
        assert call(ms=12, cap=0) == _lib.ERR_RANGE and _err() == 'lpsd: 11 segments at level 0 are fewer than min_segments = 12'
        assert nb.value == 0
        want = ref.plan(n, 2, L, 32)['nbins']
        assert call(cap=want - 1) == _lib.ERR_RANGE and _err() == 'lpsd: %d bins but capacity %d' % (want, want - 1) and nb.value == want
        assert np.all(freq == -3.0) and np.all(p == -3.0) and np.all(lev == -3)             # nothing written by a refused call
        assert call() == _lib.OK and nb.value == want and np.all(p[:, :want] > 0) and np.all(p[:, want:] == -3.0)         # rows cap apart
        assert np.all(np.diff(freq[:want]) > 0) and np.all(freq[want:] == -3.0) and set(lev[:want]) == {0, 1, 2} and np.all(lev[want:] == -3)

        def dec(n=n, S=2, stride=n, y=ybuf.ptr, ys=n):
            return _lib.lib.ginsim_decimate2(ctx.handle, buf.ptr, n, S, stride, y, ys, C.byref(no))
        for kw in (dict(n=26), dict(S=0), dict(stride=n - 1)):
            assert dec(**kw) == _lib.ERR_ARG and _err().startswith('decimate2: bad sizes') and no.value == 0, kw
        assert dec(ys=ref.n_out(n) - 1) == _lib.ERR_RANGE and 'y_stride' in _err() and no.value == ref.n_out(n)
        for y in (buf.ptr, buf.ptr + 8 * (2 * n - 1), buf.ptr - 8 * (n + ref.n_out(n) - 1)):
            assert dec(y=y) == _lib.ERR_RANGE and _err() == 'decimate2: the ranges of x and y overlap', y
        assert dec() == _lib.OK and no.value == ref.n_out(n)
    finally:
        buf.free()
        ybuf.free()
    print('lpsd and decimate2 refusals on the device: in order')


# ---- the surface
def _static_truth(n, fs=FS):
    import ginsim
    from ginsim import workloads
    text = open(workloads.profile_path('static_1800s')).read().split('\n')
    ini, _ = workloads.parse_motion('\n'.join(text[:4]))
    raw = ginsim.pathgen(ini, np.array([[1.0, 0, 0, 0, 0, 0, 0, n / fs, 0.0]]), fs, 0.0, workloads.HIGH_MOBILITY, 1)
    truth = {'ref_accel': np.ascontiguousarray(raw['imu'][:, 1:4]), 'ref_gyro': np.ascontiguousarray(raw['imu'][:, 4:7]),
             'ref_pos': raw['nav'][:, 1:4], 'ref_vel': raw['nav'][:, 4:7], 'ref_att': raw['nav'][:, 7:10]}
    assert truth['ref_accel'].shape[0] == n
    return ini, truth


def _series_of(job, runs):
    host = {nm: job.sensors(nm, list(range(runs))) for nm in ('accel', 'gyro')}             # (runs, n, 3)
    return np.concatenate([host[nm].transpose(0, 2, 1).reshape(3 * runs, -1) for nm in ('accel', 'gyro')])     # [sensor][run][axis][n]


def test_job_and_jobset_lpsd_are_lpsd_host_of_their_series(ctx):
    import ginsim
    from ginsim import multi, workloads
    n, runs = 3000, 5
    _, truth = _static_truth(n)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    kw = dict(algos=(), seed=77, keep_sensors=True)
    job = ginsim.MonteCarloJob(ctx, FS, 1, truth, acc, gyr, None, runs=runs, **kw).run()
    series = _series_of(job, runs)
    freq, p, lev = job.lpsd(nperseg=256, min_segments=2)
    want, f2, l2 = ginsim.lpsd_host(ctx, series, FS, 256, min_segments=2)
    np.testing.assert_array_equal(freq, f2)
    np.testing.assert_array_equal(lev, l2)
    assert lev.max() >= 2
    for i, nm in enumerate(('accel', 'gyro')):
        assert p[nm].shape == (runs, freq.size, 3)
        np.testing.assert_array_equal(p[nm], want.reshape(2, runs, 3, -1)[i].transpose(0, 2, 1))
    f3, p3, _ = job.lpsd(FS, names=('gyro',), nperseg=64, step=64, window='boxcar', detrend=False)
    w3, _, _ = ginsim.lpsd_host(ctx, series[3 * runs:], FS, 64, 64, 'boxcar', False)
    np.testing.assert_array_equal(p3['gyro'], w3.reshape(runs, 3, -1).transpose(0, 2, 1))
    fp, pp = job.psd(nperseg=256)                       # psd() next to it is what it was
    wp, _ = ginsim.welch_psd_host(ctx, series, FS, 256)
    np.testing.assert_array_equal(pp['gyro'], wp.reshape(2, runs, 3, -1)[1].transpose(0, 2, 1))
    ds = multi.DeviceSet([0, 0])
    js = multi.JobSet(ds, FS, 1, truth, acc, gyr, None, runs, **kw).run()
    fj, pj, lj = js.lpsd(nperseg=256, min_segments=2)
    np.testing.assert_array_equal(fj, freq)
    np.testing.assert_array_equal(lj, lev)
    for nm in ('accel', 'gyro'):
        np.testing.assert_array_equal(pj[nm], p[nm])
    js.release()
    ds.close()
    job.release()
    print('lpsd job and JobSet vs host series: error / bound 0 (bitwise)')


def test_sim_with_the_multires_plugin(ctx):
    import ginsim
    from gnss_ins_sim.sim import imu_model, ins_sim
    from demo_algorithms import psd_analysis
    from conftest import PKG
    with open(os.path.join(PKG, 'motion_profiles', 'static_1800s.csv')) as f:
        lines = f.read().splitlines()
    short = os.path.join(os.environ.get('TMPDIR', '/tmp'), 'static_lpsd_%d.csv' % os.getpid())
    cmd = lines[3].split(',')
    cmd[7] = '20'
    with open(short, 'w') as f:
        f.write('\n'.join(lines[:3] + [','.join(cmd)]) + '\n')
    try:
        runs = 2
        imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=False)
        got = {}
        for multires in (True, False):
            algo = psd_analysis.Psd(nperseg=256, multires=True, min_segments=2) if multires else psd_analysis.Psd(nperseg=256)
            sim = ins_sim.Sim([FS, 0.0, 0.0], short, ref_frame=1, imu=imu, mode=None, env=None, algorithm=algo, seed=5)
            sim.run(runs)
            d = sim.dmgr
            for r in range(runs):
                key = 'algo0_%d' % r
                for nm, out in (('accel', d.psd_accel.data[key]), ('gyro', d.psd_gyro.data[key])):
                    x = getattr(d, nm).data[r]                                      # (n, 3): the run's series on the host
                    if multires:
                        want, fw, lev = ginsim.lpsd_host(ctx, x.T, FS, 256, min_segments=2)
                        assert lev.max() >= 1 and out.shape == (fw.size, 3) and fw.size > 129
                    else:
                        want, fw = ginsim.welch_psd_host(ctx, x.T, FS, 256)
                        assert out.shape == (129, 3)
                    np.testing.assert_array_equal(out, want.T)
                    np.testing.assert_array_equal(d.psd_freq.data[key], fw)
            got[multires] = (d.accel.data[0].copy(), d.gyro.data[0].copy(), d.psd_gyro.data['algo0_0'].copy())
        # the plugin on host arrays
        q = psd_analysis.Psd(nperseg=256, multires=True, min_segments=2)
        q.run([FS, got[True][0], got[True][1]])
        np.testing.assert_array_equal(q.get_results()[2], got[True][2])
    finally:
        os.remove(short)
    print('lpsd Sim plugin vs host series, multires on and off: error / bound 0 (bitwise)')


# ---- physics, once
def test_the_drift_corner_of_the_gyro_model(ctx):
    """2 runs x 3 axes x 2^18 samples at 100 Hz, a gyroscope with white noise and a first-order drift of Tc = 2 s (corner
    1 / (2 pi Tc) = 0.08 Hz; the plateau, 4 drift^2 Tc, is 64 times the white level).  L = 1024 at half overlap, at least 16
    segments per level: five levels, the lowest bin at 6 mHz.  Per octave, the median over its bins and the six series of
    lpsd / ginsim.model_psd.  A bin averaged over K Hann segments at half overlap is a scaled chi-square of nu = 2 K_eff degrees,
    K_eff = K / (1 + 2/36 (K - 1) / K); its median is (1 - 2 / (9 nu))^3 of its mean (Wilson-Hilferty), which the median is
    divided by, and its relative deviation 1 / sqrt(K_eff).  A median of N independent values has the standard error
    sqrt(pi / 2) sigma / sqrt(N); neighbouring Hann bins correlate, N = M / (1 + 8/9 + 2/36) for M bins as in test_gpu_psd.py's
    white level, times six series.  The two lowest bins of the last level (detrend, window) are left out.  The band is stated from
    K_j, not tuned."""
    import ginsim
    runs, n, L, Tc = 2, 1 << 18, 1024, 2.0
    _, truth = _static_truth(n)
    quiet = {'b': np.zeros(3), 'b_drift': np.zeros(3), 'b_corr': np.full(3, np.inf)}
    acc = dict(quiet, vrw=np.full(3, 1e-3))
    gyr = {'b': np.zeros(3), 'b_drift': np.full(3, 1e-3), 'b_corr': np.full(3, Tc), 'arw': np.full(3, 2.5e-4)}
    job = ginsim.MonteCarloJob(ctx, FS, 1, truth, acc, gyr, None, runs=runs, algos=(), seed=31, keep_sensors=True).run()
    freq, p, lev = job.lpsd(names=('gyro',), nperseg=L, min_segments=16)
    fw, pw = job.psd(names=('gyro',), nperseg=L)
    job.release()
    levels = int(lev.max()) + 1
    ns = ref.level_lengths(n, L, L // 2, 16)
    assert levels == len(ns) == 5
    model = ginsim.model_psd(gyr, 'arw', FS, freq)                      # (nbins, 3)
    ratio = p['gyro'] / model[None, :, :]                                # (runs, nbins, 3)
    corner = 1.0 / (2 * math.pi * Tc)
    assert freq[2] < corner / 4 and fw[1] > corner                       # inside the cascade's curve, below psd()'s first bin
    worst = 0.0
    for j in range(levels):
        K = px.segments(ns[j], L, L // 2)
        keff = K / (1 + 2 / 36 * (K - 1) / K)
        sel = (lev == j) & (np.arange(freq.size) >= 2)
        M = int(sel.sum())
        med = float(np.median(ratio[:, sel, :])) / (1 - 2 / (9 * 2 * keff)) ** 3
        se = math.sqrt(math.pi / 2) / math.sqrt(keff) / math.sqrt(M / (1 + 8 / 9 + 2 / 36) * 3 * runs)
        worst = max(worst, abs(med - 1) / (5 * se))
        print('lpsd drift corner, level %d: K %d, %d bins, median / model %.4f, 5 standard errors %.4f' % (j, K, M, med, 5 * se))
        assert abs(med - 1.0) <= 5 * se, (j, med, se)
    print('lpsd drift corner: error / bound %.3g over %d octaves' % (worst, levels))
