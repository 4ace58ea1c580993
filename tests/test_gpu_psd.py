"""Welch's power spectral density on the device (csrc/psd.hip through ginsim_psd_welch): every result is held to the exact values
of tests/psd_exact.py within the tolerance derived there, on the shapes of tests/psd_cases.py (each asserts from ginsim.welch_plan
WHERE it sits in the partition), then the guarantees of include/ginsim_psd.h, the layers above the C ABI, the white level of the
sensor model and the spectrum of a 'psd' vibration taken back out of the series.  Every test prints its error over its bound."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import psd_cases as pc
import psd_exact as px

pytestmark = pytest.mark.gpu

FS = 100.0


@pytest.fixture(scope='module')
def ctx():
    import ginsim
    c = ginsim.Context(0)
    yield c
    c.close()


device_psd = pc.device_psd          # shared with test_gpu_psd_edges.py; fs defaults to FS


# ---- parity with the exact values
@pytest.mark.parametrize('case', pc.CASES, ids=pc.IDS)
def test_parity_with_exact(ctx, case):
    import ginsim
    name, L, D, K, tail, kinds, pad, win, det, where = case
    n, S, stride = pc.shape(case)
    g = ginsim.welch_plan(n, S, stride, FS, L, D)
    assert g['segments'] == K and g['nparts'] == -(-K // g['segs_per_part'])
    if where is not None:
        assert K == where[0] * g['segs_per_part'] + where[1]
    a = pc.rows(case)
    p, f = device_psd(ctx, a, n, L, D, win, det)
    assert p.shape == (S, L // 2 + 1)
    np.testing.assert_array_equal(f, px.freqs(FS, L))
    worst = 0.0
    for s in range(S):
        e, _ = px.exact(a[s, :n], FS, L, D, win, det)
        worst = max(worst, px.ratio(p[s], e, px.tol(a[s, :n], FS, L, D, win, det, e)))
    print('psd %s (n %d x %d, %d parts): error / tol %.3g' % (name, n, S, g['nparts'], worst))
    assert worst <= 1.0


# ---- guarantees
GUARANTEE = pc.CASES[pc.IDS.index('L1024_S65_K_part_plus_1_stride_tail')]


@pytest.fixture(scope='module')
def batch(ctx):
    """The 65-series case and its device result, computed once."""
    _, L, D, K, tail, kinds, pad, win, det, _ = GUARANTEE
    n, S, stride = pc.shape(GUARANTEE)
    a = pc.rows(GUARANTEE)
    p, _ = device_psd(ctx, a, n, L, D, win, det)
    a.setflags(write=False)
    p.setflags(write=False)
    return a, n, L, D, win, det, p


def test_two_launches_give_the_same_bits(ctx, batch):
    a, n, L, D, win, det, p = batch
    again, _ = device_psd(ctx, a, n, L, D, win, det)
    np.testing.assert_array_equal(again, p)
    assert np.isfinite(p).all()
    print('psd two launches: error / bound 0 (bitwise)')


def test_a_series_alone_has_the_bits_it_has_in_the_batch(ctx, batch):
    a, n, L, D, win, det, p = batch
    for s in (0, 31, 64):
        alone, _ = device_psd(ctx, a[s:s + 1, :n], n, L, D, win, det)
        np.testing.assert_array_equal(alone[0], p[s])
    print('psd alone vs batch of 65: error / bound 0 (bitwise)')


def test_non_finite_samples_give_nan_in_their_series_only(ctx, batch):
    a, n, L, D, win, det, p = batch
    K = px.segments(n, L, D)
    last_read = (K - 1) * D + L - 1
    assert last_read < n - 1                            # the case has a tail of unread samples
    for det2, win2 in ((det, win), (False, 'boxcar')):   # without detrending an Inf would otherwise stay an Inf
        ref, _ = device_psd(ctx, a, n, L, D, win2, det2)
        b = a.copy()
        b[3, 0] = np.nan                                # the first sample read
        b[17, last_read] = np.inf                       # the last one
        b[40, n // 2] = -np.inf
        b[41, n // 3] = np.inf
        b[41, n // 3 + 1] = -np.inf
        got, _ = device_psd(ctx, b, n, L, D, win2, det2)
        hit = [3, 17, 40, 41]
        assert np.isnan(got[hit]).all()
        rest = [s for s in range(a.shape[0]) if s not in hit]
        np.testing.assert_array_equal(got[rest], ref[rest])
    c = a.copy()
    c[:, last_read + 1:n] = np.nan                      # the unread tail of every series
    c[5, n - 1] = np.inf
    got, _ = device_psd(ctx, c, n, L, D, win, det)
    np.testing.assert_array_equal(got, p)
    print('psd non-finite: error / bound 0 (bitwise)')


def test_device_refusals_and_their_order(ctx):
    """The refusals behind the NULL context (tests/test_psd_oracle.py has that one), in the order of include/ginsim_psd.h."""
    from ginsim import _lib
    err = lambda: _lib.lib.ginsim_last_error().decode()     # noqa: E731
    freq, p, nf = np.empty(64), np.empty(64), C.c_int32(-7)
    buf = ctx.upload(np.zeros(256))

    def call(n=256, S=1, stride=None, fs=1.0, L=64, D=32, w=1, d=1, cap=33):
        return _lib.lib.ginsim_psd_welch(ctx.handle, buf.ptr, n, S, n if stride is None else stride, fs, L, D, w, d, _lib.dptr(freq),
                                         _lib.dptr(p), C.byref(nf), cap)
    try:
        assert call(n=0, L=7, D=0, w=5, cap=0) == _lib.ERR_ARG and err() == 'psd: bad sizes'
        assert call(stride=255, L=7) == _lib.ERR_ARG and err() == 'psd: bad sizes'
        assert call(L=48, D=0, w=5, cap=0) == _lib.ERR_ARG and err() == 'psd: nperseg 48 is not a power of two in [8, 8192]'
        assert call(D=65, w=5, cap=0) == _lib.ERR_ARG and err() == 'psd: step 65 outside [1, 64]'
        for kw in (dict(w=2), dict(w=-1), dict(d=2), dict(d=-1)):
            assert call(n=10, cap=0, **kw) == _lib.ERR_ARG and err().startswith('psd: window'), kw       # before the series' length
        assert call(n=63, cap=0) == _lib.ERR_RANGE
        assert err() == 'psd: a series of n = 63 samples is shorter than one segment of nperseg = 64'
        assert call(n=64, S=2 ** 31 - 1, cap=0) == _lib.ERR_RANGE                                        # the grid limit before the capacity
        found = re.search(r'the device takes (\d+)', err())
        assert found, err()
        limit = int(found.group(1))
        assert 65535 <= limit < 2 ** 31 - 1
        assert call(n=64, S=limit + 1, cap=0) == _lib.ERR_RANGE
        msg = err()
        assert msg.startswith('psd:') and '%d series' % (limit + 1) in msg and 'takes %d' % limit in msg and 'split the batch' in msg
        nf.value = -7
        assert call(cap=32) == _lib.ERR_RANGE and err() == 'psd: 33 frequencies but capacity 32' and nf.value == 33
        assert call() == _lib.OK and nf.value == 33 and np.all(p[:33] == 0.0)
    finally:
        buf.free()


def test_device_refuses_what_the_plan_cannot_state(ctx):
    """The call's half of tests/test_psd_oracle.py::test_plan_refuses_what_it_cannot_state: more than 2^31 - 1 parts, or records
    past 2^63 bytes, are refused under 'psd:' after "n < nperseg" and before the grid's y limit; nothing is launched, so the
    256 samples behind the pointer are never read at those lengths."""
    from ginsim import _lib
    err = lambda: _lib.lib.ginsim_last_error().decode()     # noqa: E731
    freq, p, nf = np.full(8, -3.0), np.full(8, -3.0), C.c_int32(-7)
    buf = ctx.upload(np.zeros(256))
    n_last = (2 ** 31 - 1) * 16384 + 7                  # L = 8, D = 1: 2^31 - 1 full parts of 16384 segments

    def call(n, S=1, L=8, D=1, cap=5):
        return _lib.lib.ginsim_psd_welch(ctx.handle, buf.ptr, n, S, n, 1.0, L, D, 1, 1, _lib.dptr(freq), _lib.dptr(p), C.byref(nf), cap)
    try:
        for n in (n_last + 1, 2 ** 62):
            for S in (1, 2 ** 31 - 1):                   # the parts before the grid's y limit
                assert call(n, S) == _lib.ERR_RANGE
                msg = err()
                assert msg.startswith('psd: ') and '%d parts' % (-(-(n - 7) // 16384)) in msg, msg
                assert nf.value == 0
        assert call(n_last, 2 ** 31 - 1) == _lib.ERR_RANGE                                              # the bytes before it too
        msg = err()
        assert msg.startswith('psd: ') and '%d parts' % (2 ** 31 - 1) in msg and '2^63 bytes' in msg, msg
        assert call(7, 2 ** 31 - 1) == _lib.ERR_RANGE and 'shorter than one segment' in err()           # n < nperseg before both
        assert call(n_last + 1, cap=0) == _lib.ERR_RANGE and 'parts' in err()                           # and the capacity after
        assert np.all(freq == -3.0) and np.all(p == -3.0)
        assert call(256) == _lib.OK and nf.value == 5 and np.all(p[:5] == 0.0)                          # the context still works
    finally:
        buf.free()
    print('psd unstatable shapes on the device: refused in order')
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


def test_job_psd_is_welch_psd_of_its_series(ctx):
    import ginsim
    from ginsim import workloads
    n = 3000
    ini, truth = _static_truth(n)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    layouts = set()
    for runs in (1, 5):
        for algos in ((), ('free',)):
            job = ginsim.MonteCarloJob(ctx, FS, 1, truth, acc, gyr, ini if algos else None, runs=runs, algos=algos, seed=77,
                                       keep_sensors=True).run()
            layouts.add(job.sensor_layout)
            series = _series_of(job, runs)
            freq, p = job.psd(nperseg=256)
            want, f2 = ginsim.welch_psd_host(ctx, series, FS, 256)
            np.testing.assert_array_equal(freq, f2)
            for i, nm in enumerate(('accel', 'gyro')):
                assert p[nm].shape == (runs, 129, 3)
                np.testing.assert_array_equal(p[nm], want.reshape(2, runs, 3, -1)[i].transpose(0, 2, 1))
            f3, p3 = job.psd(FS, names=('gyro',), nperseg=64, step=64, window='boxcar', detrend=False)
            w3, _ = ginsim.welch_psd_host(ctx, series[3 * runs:], FS, 64, 64, 'boxcar', False)
            np.testing.assert_array_equal(p3['gyro'], w3.reshape(runs, 3, -1).transpose(0, 2, 1))
            e, _ = px.exact(series[1], FS, 256, 128, 'hann', True)
            assert px.ratio(want[1], e, px.tol(series[1], FS, 256, 128, 'hann', True, e)) <= 1.0
            tau, ad = job.allan(FS)                  # the helper the two share leaves allan() what it was
            av, t0 = ginsim.allan_var_host(ctx, series, FS)
            np.testing.assert_array_equal(ad['gyro'], np.sqrt(av).reshape(2, runs, 3, -1)[1].transpose(0, 2, 1))
            job.release()
    assert layouts == {'series', 'runs'}
    print('psd job vs host series: error / bound 0 (bitwise)')


def test_jobset_on_two_contexts_equals_the_single_job(ctx):
    import ginsim
    from ginsim import multi, workloads
    n, runs = 2000, 5
    _, truth = _static_truth(n)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    kw = dict(algos=(), seed=9, keep_sensors=True)
    one = ginsim.MonteCarloJob(ctx, FS, 1, truth, acc, gyr, None, runs=runs, **kw).run()
    ds = multi.DeviceSet([0, 0])
    js = multi.JobSet(ds, FS, 1, truth, acc, gyr, None, runs, **kw).run()
    f1, p1 = one.psd(nperseg=512, step=100)
    f2, p2 = js.psd(nperseg=512, step=100)
    np.testing.assert_array_equal(f1, f2)
    for nm in ('accel', 'gyro'):
        assert p2[nm].shape == (runs, 257, 3)
        np.testing.assert_array_equal(p1[nm], p2[nm])
    js.release()
    one.release()
    ds.close()
    print('psd JobSet vs job: error / bound 0 (bitwise)')


def test_sim_with_the_plugin(ctx):
    import ginsim
    from gnss_ins_sim.sim import imu_model, ins_sim
    from demo_algorithms import psd_analysis
    from conftest import PKG
    with open(os.path.join(PKG, 'motion_profiles', 'static_1800s.csv')) as f:
        lines = f.read().splitlines()
    short = os.path.join(os.environ.get('TMPDIR', '/tmp'), 'static_psd_%d.csv' % os.getpid())
    cmd = lines[3].split(',')
    cmd[7] = '20'
    with open(short, 'w') as f:
        f.write('\n'.join(lines[:3] + [','.join(cmd)]) + '\n')
    try:
        runs = 2
        imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=False)
        sim = ins_sim.Sim([FS, 0.0, 0.0], short, ref_frame=1, imu=imu, mode=None, env=None, algorithm=psd_analysis.Psd(nperseg=256), seed=5)
        sim.run(runs)
        d = sim.dmgr
        for r in range(runs):
            key = 'algo0_%d' % r
            np.testing.assert_array_equal(d.psd_freq.data[key], px.freqs(FS, 256))
            for nm, got in (('accel', d.psd_accel.data[key]), ('gyro', d.psd_gyro.data[key])):
                assert got.shape == (129, 3)
                x = getattr(d, nm).data[r]                                      # (n, 3): the run's series on the host
                want, _ = ginsim.welch_psd_host(ctx, x.T, FS, 256)
                np.testing.assert_array_equal(got, want.T)
        # and the plugin on host arrays
        p = psd_analysis.Psd(nperseg=256)
        p.run([FS, d.accel.data[0], d.gyro.data[0]])
        f, pa, pg = p.get_results()
        np.testing.assert_array_equal(pa, d.psd_accel.data['algo0_0'])
        np.testing.assert_array_equal(pg, d.psd_gyro.data['algo0_0'])
    finally:
        os.remove(short)
    print('psd Sim plugin vs host series: error / bound 0 (bitwise)')


# ---- the white level of the sensor model
def test_white_level_of_the_gyro_model(ctx):
    """64 runs x 65 536 samples, a gyroscope with white noise only: the mean of the PSD over runs, axes and interior bins is
    2 sigma^2 / fs with sigma^2 the per-sample variance of the model, arw^2 fs.  Margin: five standard errors of that mean.
    A bin of one periodogram of white Gaussian noise is exponential (relative standard deviation 1).  Over K Hann segments at half
    overlap neighbours correlate by 1/6 in amplitude, 1/36 in power: the variance of the average is (1 + 2/36 (K-1)/K) / K, about
    1 / (0.95 K).  Across bins the Hann window (taps 1/2, -1/4, -1/4) correlates neighbours by -2/3 and next neighbours by 1/6 in
    amplitude, 4/9 and 1/36 in power: the mean over M bins has variance (1 + 8/9 + 2/36) / M.  Runs and axes are independent."""
    import ginsim
    runs, n, L = 64, 65536, 1024
    _, truth = _static_truth(n)
    arw = 2.5e-4
    quiet = {'b': np.zeros(3), 'b_drift': np.zeros(3), 'b_corr': np.full(3, np.inf)}
    acc = dict(quiet, vrw=np.full(3, 1e-3))
    gyr = dict(quiet, arw=np.full(3, arw))
    job = ginsim.MonteCarloJob(ctx, FS, 1, truth, acc, gyr, None, runs=runs, algos=(), seed=31, keep_sensors=True).run()
    freq, p = job.psd(names=('gyro',), nperseg=L)
    job.release()
    K = (n - L) // (L // 2) + 1
    interior = p['gyro'][:, 2:L // 2 - 1, :]                # without the bins the detrending and the window's leak touch
    M = interior.shape[1]
    level = interior.mean()
    want = 2.0 * (arw * arw * FS) / FS
    se = math.sqrt((1.0 + 2.0 / 36.0 * (K - 1) / K) / K * (1.0 + 8.0 / 9.0 + 2.0 / 36.0) / M / (3 * runs))
    print('psd white level: %.6e against %.6e, error / bound %.3g (5 standard errors = %.3g relative, K %d, %d bins)'
          % (level, want, abs(level / want - 1.0) / (5 * se), 5 * se, K, M))
    assert abs(level / want - 1.0) <= 5 * se


# ---- the spectrum that was asked for comes back
def test_the_requested_vibration_spectrum_comes_back(ctx):
    """A 'psd' vibration on the accelerometer, no sensor errors, one period of 8192 samples analysed as one boxcar segment: at bins
    1 .. L/2 the result is the requested PSD interpolated to the series' grid -- the amplitudes are fixed, only the phases are
    drawn, so there is no scatter; two runs show that the phases differ and the spectrum does not."""
    import ginsim
    n, fs = pc.REQUESTED_N, pc.REQUESTED_FS
    _, truth = _static_truth(n, fs)
    quiet = {'b': np.zeros(3), 'b_drift': np.zeros(3), 'b_corr': np.full(3, np.inf)}
    acc, gyr = dict(quiet, vrw=np.zeros(3)), dict(quiet, arw=np.zeros(3))
    vib = dict(type='psd', freq=pc.REQUESTED_FREQ.copy(), **{k: v.copy() for k, v in pc.REQUESTED_PSD.items()})
    job = ginsim.MonteCarloJob(ctx, fs, 1, truth, acc, gyr, None, runs=2, algos=(), seed=12, keep_sensors=True, vib_accel=vib).run()
    x = job.sensors('accel', [0, 1])                          # (2, n, 3)
    freq, p = job.psd(names=('accel',), nperseg=n, step=n, window='boxcar', detrend=True)
    job.release()
    assert freq[-1] == fs / 2 and p['accel'].shape == (2, n // 2 + 1, 3)
    assert np.max(np.abs(x[0] - x[1])) > 1e-3                 # other phases
    worst = 0.0
    for r in range(2):
        for c, axis in enumerate('xyz'):
            want = pc.requested_on_grid(axis)
            t = px.tol(x[r, :, c], fs, n, n, 'boxcar', True, want)
            worst = max(worst, px.ratio(p['accel'][r, 1:, c], want[1:], t[1:]))
    bound = pc.REQUESTED_MARGIN * pc.REQUESTED_NUMPY
    print('psd requested spectrum: error / tol %.3g, allowed %.3g: error / bound %.3g' % (worst, bound, worst / bound))
    assert worst <= bound
