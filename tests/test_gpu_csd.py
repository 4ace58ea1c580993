"""Welch's cross-spectral density on the device (csrc/csd.hip through ginsim_csd_welch): all four outputs are held to the exact
values of tests/csd_exact.py within the tolerance derived there, on the shapes of tests/csd_cases.py (each asserts from
ginsim.csd_plan WHERE it sits in the partition), then the guarantees of include/ginsim_csd.h and the layers above the C ABI.
Every test prints its error over its bound.

Measured on one MI355X: at most 0.122 (pxx, pyy) and 0.152 (pxy) of the tolerance over the 50 shapes, all at
L4096_K3_unaligned_boxcar_raw; the float64 restatement is at 0.25 on the same shapes (tests/test_csd_oracle.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import csd_cases as cc
import csd_exact as cx
import psd_cases as pc

pytestmark = pytest.mark.gpu

FS = 100.0


@pytest.fixture(scope='module')
def ctx():
    import ginsim
    c = ginsim.Context(0)
    yield c
    c.close()


def _held_to_exact(r, a, n, pairs, L, D, win, det):
    """Largest error / tol of (pxx, pyy, pxy) over the pairs; asserts the properties every finite result has."""
    worst = np.zeros(3)
    for p, (i, j) in enumerate(pairs):
        x, y = a[i, :n], a[j, :n]
        exx, eyy, exy, _ = cx.exact(x, y, FS, L, D, win, det)
        t = cx.tol(x, y, FS, L, D, win, det, exx, eyy)
        worst = np.maximum(worst, cx.ratios((r.pxx[p], r.pyy[p], r.pxy[p]), (exx, eyy, exy), t))
    edge = r.pxy.imag[:, [0, -1]]
    assert np.all(edge == 0.0) and not np.signbit(edge).any()           # +0.0, sign bit included
    coh = r.coherence
    assert np.all(coh[np.isfinite(coh)] <= 1 + 1e-12)
    return worst


# ---- parity with the exact values
@pytest.mark.parametrize('case', cc.CASES, ids=cc.IDS)
def test_parity_with_exact(ctx, case):
    import ginsim
    name, L, D, K, tail, kinds, pad, win, det, where = case
    n, S, stride = cc.shape(case)
    pairs = cc.pairs_of(case)
    g = ginsim.csd_plan(n, S, stride, FS, len(pairs), L, D)
    assert g['segments'] == K and g['nparts'] == -(-K // g['segs_per_part'])
    if where is not None:
        assert K == where[0] * g['segs_per_part'] + where[1]
    a = cc.rows(case)
    r = cc.device_csd(ctx, a, n, pairs, L, D, win, det)
    assert r.pxx.shape == r.pyy.shape == r.pxy.shape == (len(pairs), L // 2 + 1) and r.pxy.dtype == np.complex128
    np.testing.assert_array_equal(r.freq, cx.freqs(FS, L))
    np.testing.assert_array_equal(r.pairs, pairs)
    worst = _held_to_exact(r, a, n, pairs, L, D, win, det)
    print('csd %s (n %d, %d pairs, %d parts): error / tol pxx %.3g pyy %.3g pxy %.3g' % ((name, n, len(pairs), g['nparts']) + tuple(worst)))
    assert worst.max() <= 1.0


# ---- guarantees
@pytest.fixture(scope='module')
def table(ctx):
    """The 65-pair case and its device result, computed once."""
    _, L, D, K, tail, kinds, pad, win, det, _ = cc.TABLE
    n, S, stride = cc.shape(cc.TABLE)
    a = cc.rows(cc.TABLE)
    r = cc.device_csd(ctx, a, n, cc.TABLE_PAIRS, L, D, win, det)
    a.setflags(write=False)
    for v in (r.pxx, r.pyy, r.pxy):
        v.setflags(write=False)
    return a, n, L, D, win, det, r


def _same_bits(r, q, rows_r=slice(None), rows_q=slice(None)):
    for k in ('pxx', 'pyy', 'pxy'):
        np.testing.assert_array_equal(getattr(r, k)[rows_r], getattr(q, k)[rows_q])


def test_two_launches_give_the_same_bits(ctx, table):
    a, n, L, D, win, det, r = table
    again = cc.device_csd(ctx, a, n, cc.TABLE_PAIRS, L, D, win, det)
    _same_bits(again, r)
    assert np.isfinite(r.pxx).all() and np.isfinite(r.pyy).all() and np.isfinite(r.pxy).all()
    print('csd two launches: error / bound 0 (bitwise)')


def test_a_pair_alone_has_the_bits_it_has_in_the_table(ctx, table):
    a, n, L, D, win, det, r = table
    for p in (0, 10, 33, 64):
        alone = cc.device_csd(ctx, a, n, [cc.TABLE_PAIRS[p]], L, D, win, det)
        _same_bits(alone, r, [0], [p])
    i, j = cc.TABLE_PAIRS[12]                     # and with nothing but its two series in the buffer
    two = cc.device_csd(ctx, a[[i, j]], n, [(0, 1)], L, D, win, det)
    _same_bits(two, r, [0], [12])
    print('csd alone vs table of 65: error / bound 0 (bitwise)')


def test_permuting_the_table_permutes_the_result(ctx, table):
    a, n, L, D, win, det, r = table
    perm = np.random.default_rng(4).permutation(65)
    q = cc.device_csd(ctx, a, n, [cc.TABLE_PAIRS[p] for p in perm], L, D, win, det)
    _same_bits(q, r, slice(None), perm)
    print('csd permuted table: error / bound 0 (bitwise)')


def test_non_finite_samples_give_nan_in_their_pairs_only(ctx, table):
    a, n, L, D, win, det, r = table
    K = cx.segments(n, L, D)
    last_read = (K - 1) * D + L - 1
    assert last_read < n - 1                            # the case has a tail of unread samples
    for bad in (np.inf, -np.inf):
        for det2, win2 in ((det, win), (False, 'boxcar')):   # without detrending an Inf would otherwise stay an Inf
            ref = r if (det2, win2) == (det, win) else cc.device_csd(ctx, a, n, cc.TABLE_PAIRS, L, D, win2, det2)
            b = a.copy()
            b[4, 0] = np.nan                            # the first sample read
            b[6, last_read] = bad                       # the last one
            got = cc.device_csd(ctx, b, n, cc.TABLE_PAIRS, L, D, win2, det2)
            hit = [p for p, ij in enumerate(cc.TABLE_PAIRS) if 4 in ij or 6 in ij]
            rest = [p for p in range(65) if p not in hit]
            assert len(hit) > 10 and len(rest) > 10
            for v in (got.pxx, got.pyy, got.pxy.real, got.pxy.imag):
                assert np.isnan(v[hit]).all()
            _same_bits(got, ref, rest, rest)
    c = a.copy()
    c[:, last_read + 1:n] = np.nan                      # the unread tail of every series
    c[5, n - 1] = np.inf
    _same_bits(cc.device_csd(ctx, c, n, cc.TABLE_PAIRS, L, D, win, det), r)
    print('csd non-finite: error / bound 0 (bitwise)')


def test_pxx_of_a_pair_is_the_psd_of_its_series(ctx, table):
    a, n, L, D, win, det, r = table
    p, _ = pc.device_psd(ctx, a, n, L, D, win, det)
    worst = 0.0
    for q, (i, j) in enumerate(cc.TABLE_PAIRS):
        exx, eyy, _, _ = cx.exact(a[i, :n], a[j, :n], FS, L, D, win, det)
        txx, tyy, txy = cx.tol(a[i, :n], a[j, :n], FS, L, D, win, det, exx, eyy)
        worst = max(worst, cx.ratio(r.pxx[q], p[i], txx), cx.ratio(r.pyy[q], p[j], tyy))
        if i == j:                                      # a series with itself: one spectrum three times, each within its tolerance
            same = max(cx.ratio(r.pxy[q].real, exx, txy), cx.ratio(r.pxy[q].imag, np.zeros(exx.shape), txy))
            print('csd pair (%d, %d): pxy against pxx + 0i, error / tol %.3g' % (i, j, same))
            assert same <= 1.0
    print('csd pxx / pyy against welch_psd of the series: error / tol %.3g' % worst)
    assert worst <= 1.0


def test_device_refusals_and_their_order(ctx):
    """The refusals behind the NULL context (tests/test_csd_oracle.py has that one), in the order of include/ginsim_csd.h."""
    from ginsim import _lib
    err = lambda: _lib.lib.ginsim_last_error().decode()     # noqa: E731
    freq, nf = np.empty(64), C.c_int32(-7)
    out = [np.full(64, -3.0) for _ in range(4)]
    buf = ctx.upload(np.zeros(512))
    n_last = (2 ** 31 - 1) * 16384 + 7                  # L = 8, D = 1: 2^31 - 1 full parts of 16384 segments

    def call(n=256, S=2, stride=None, fs=1.0, pairs=((0, 1),), P=None, L=64, D=32, w=1, d=1, cap=33):
        tab = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32))
        return _lib.lib.ginsim_csd_welch(ctx.handle, buf.ptr, n, S, n if stride is None else stride, fs,
                                         tab.ctypes.data_as(C.POINTER(C.c_int32)), len(pairs) if P is None else P, L, D, w, d,
                                         _lib.dptr(freq), *[_lib.dptr(o) for o in out], C.byref(nf), cap)
    try:
        assert call(n=0, P=0, L=7, D=0, w=5, cap=0) == _lib.ERR_ARG and err() == 'csd: bad sizes'
        assert call(stride=255, P=0, L=7) == _lib.ERR_ARG and err() == 'csd: bad sizes'
        assert call(P=0, L=48, D=0, w=5, cap=0) == _lib.ERR_ARG and err().startswith('csd: npairs 0')
        assert call(L=48, D=0, w=5, cap=0) == _lib.ERR_ARG and err() == 'csd: nperseg 48 is not a power of two in [8, 4096]'
        assert call(L=8192, D=0, w=5, cap=0) == _lib.ERR_ARG and err().startswith('csd: nperseg 8192 is not taken')
        assert call(D=65, w=5, cap=0) == _lib.ERR_ARG and err() == 'csd: step 65 outside [1, 64]'
        for kw in (dict(w=2), dict(w=-1), dict(d=2), dict(d=-1)):
            assert call(n=10, pairs=((0, 2),), cap=0, **kw) == _lib.ERR_ARG and err().startswith('csd: window'), kw    # before the table
        for bad in ((0, 2), (2, 0), (-1, 0), (0, -1)):
            assert call(n=10, pairs=((0, 1), bad), cap=0) == _lib.ERR_ARG                                # before the series' length
            assert err() == 'csd: pair 1 is (%d, %d) but the series are 0 .. 1' % bad
        assert call(n=63, cap=0) == _lib.ERR_RANGE
        assert err() == 'csd: a series of n = 63 samples is shorter than one segment of nperseg = 64'
        assert call(n=n_last + 1, S=1, pairs=((0, 0),), L=8, D=1, cap=0) == _lib.ERR_RANGE and '%d parts' % 2 ** 31 in err()
        assert call(n=7, S=1, pairs=((0, 0),), L=8, D=1, cap=0) == _lib.ERR_RANGE and 'shorter than one segment' in err()
        assert nf.value == 0
        # the parts before the grid's limit, the limit before the capacity.  The limit is the one ginsim_psd_welch names; a table
        # past it has to be a real one, every entry legal, since the entries are checked first
        p1 = np.empty(1)
        assert _lib.lib.ginsim_psd_welch(ctx.handle, buf.ptr, 64, 2 ** 31 - 1, 64, 1.0, 64, 32, 1, 1, _lib.dptr(freq), _lib.dptr(p1),
                                         C.byref(nf), 0) == _lib.ERR_RANGE
        limit = int(re.search(r'the device takes (\d+)', err()).group(1))
        assert 65535 <= limit < 2 ** 20
        big = np.zeros((limit + 1, 2), dtype=np.int32)
        assert call(n=n_last + 1, S=1, pairs=big, L=8, D=1, cap=0) == _lib.ERR_RANGE and '%d parts' % 2 ** 31 in err()
        assert call(n=64, S=1, pairs=big, cap=0) == _lib.ERR_RANGE
        msg = err()
        assert msg.startswith('csd:') and '%d pairs' % (limit + 1) in msg and 'takes %d' % limit in msg and 'split the table' in msg
        assert call(n=64, S=1, pairs=big[:limit], cap=0) == _lib.ERR_RANGE and err() == 'csd: 33 frequencies but capacity 0'
        nf.value = -7
        assert call(cap=32) == _lib.ERR_RANGE and err() == 'csd: 33 frequencies but capacity 32' and nf.value == 33
        assert all(np.all(o == -3.0) for o in out)
        assert call() == _lib.OK and nf.value == 33 and all(np.all(o[:33] == 0.0) for o in out)
        assert not np.signbit(out[3][:33]).any()
    finally:
        buf.free()
    print('csd refusals on the device: in order')


# ---- the layers above the C ABI
def test_result_properties_are_their_formulas(ctx, table):
    a, n, L, D, win, det, r = table
    with np.errstate(divide='ignore', invalid='ignore'):
        den = r.pxx * r.pyy
        np.testing.assert_array_equal(r.coherence, np.where(den == 0, np.nan, np.abs(r.pxy) ** 2 / den))
        np.testing.assert_array_equal(r.phase, np.angle(r.pxy))
        np.testing.assert_array_equal(r.transfer, r.pxy / r.pxx)
        np.testing.assert_array_equal(r.gain, np.abs(r.pxy / r.pxx))


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


def _job_table(pairs, runs):
    names = ('accel', 'gyro')
    return [((names.index(a[0]) * runs + r) * 3 + a[1], (names.index(b[0]) * runs + r) * 3 + b[1]) for r in range(runs) for a, b in pairs]


def test_job_csd_is_welch_csd_of_its_series(ctx):
    import ginsim
    from ginsim import workloads
    from demo_algorithms import csd_analysis
    n, runs = 2048, 3
    ini, truth = _static_truth(n)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    job = ginsim.MonteCarloJob(ctx, FS, 1, truth, acc, gyr, None, runs=runs, algos=(), seed=77, keep_sensors=True).run()
    series = _series_of(job, runs)
    freq, c = job.csd(nperseg=256)
    assert len(c['pairs']) == 15 and c['pairs'] == csd_analysis.default_pairs()
    want = ginsim.welch_csd_host(ctx, series, FS, _job_table(c['pairs'], runs), 256)
    np.testing.assert_array_equal(freq, want.freq)
    for k in ('pxx', 'pyy', 'pxy', 'coherence', 'phase'):
        assert c[k].shape == (runs, 15, 129)
        np.testing.assert_array_equal(c[k], getattr(want, k).reshape(runs, 15, 129))
    mine = [(('gyro', 2), ('accel', 0)), (('accel', 1), ('accel', 1))]
    f2, c2 = job.csd(FS, mine, nperseg=64, step=64, window='boxcar', detrend=False)
    w2 = ginsim.welch_csd_host(ctx, series, FS, _job_table(mine, runs), 64, 64, 'boxcar', False)
    np.testing.assert_array_equal(c2['pxy'], w2.pxy.reshape(runs, 2, 33))
    x, y = series[0], series[1]                          # run 0: accel x against accel y, held to the exact values
    exx, eyy, exy, _ = cx.exact(x, y, FS, 256, 128, 'hann', True)
    r = cx.ratios((c['pxx'][0, 0], c['pyy'][0, 0], c['pxy'][0, 0]), (exx, eyy, exy), cx.tol(x, y, FS, 256, 128, 'hann', True, exx, eyy))
    assert max(r) <= 1.0
    with pytest.raises(ValueError, match='pairs'):
        job.csd(pairs=[(('accel', 3), ('gyro', 0))])
    job.release()
    bare = ginsim.MonteCarloJob(ctx, FS, 1, truth, acc, gyr, ini, runs=runs, algos=('free',), seed=77, keep_sensors=False).run()
    with pytest.raises(ValueError, match='keep_sensors=True'):
        bare.csd()
    bare.release()
    print('csd job vs host series: error / bound 0 (bitwise); against exact %.3g' % max(r))


def test_jobset_on_two_contexts_equals_the_single_job(ctx):
    import ginsim
    from ginsim import multi, workloads
    n, runs = 2048, 3
    _, truth = _static_truth(n)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    kw = dict(algos=(), seed=9, keep_sensors=True)
    one = ginsim.MonteCarloJob(ctx, FS, 1, truth, acc, gyr, None, runs=runs, **kw).run()
    ds = multi.DeviceSet([0, 0])
    js = multi.JobSet(ds, FS, 1, truth, acc, gyr, None, runs, **kw).run()
    f1, c1 = one.csd(nperseg=512, step=100)
    f2, c2 = js.csd(nperseg=512, step=100)
    np.testing.assert_array_equal(f1, f2)
    assert c1['pairs'] == c2['pairs']
    for k in ('pxx', 'pyy', 'pxy', 'coherence', 'phase'):
        assert c2[k].shape == (runs, 15, 257)
        np.testing.assert_array_equal(c1[k], c2[k])
    js.release()
    one.release()
    ds.close()
    print('csd JobSet vs job: error / bound 0 (bitwise)')


def test_sim_with_the_plugin(ctx):
    from gnss_ins_sim.sim import imu_model, ins_sim
    from demo_algorithms import csd_analysis
    from conftest import PKG
    with open(os.path.join(PKG, 'motion_profiles', 'static_1800s.csv')) as f:
        lines = f.read().splitlines()
    short = os.path.join(os.environ.get('TMPDIR', '/tmp'), 'static_csd_%d.csv' % os.getpid())
    cmd = lines[3].split(',')
    cmd[7] = '20'
    with open(short, 'w') as f:
        f.write('\n'.join(lines[:3] + [','.join(cmd)]) + '\n')
    try:
        runs = 2
        imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=False)
        sim = ins_sim.Sim([FS, 0.0, 0.0], short, ref_frame=1, imu=imu, mode=None, env=None,
                          algorithm=csd_analysis.Coherence(nperseg=256), seed=5)
        sim.run(runs)
        d = sim.dmgr
        for r in range(runs):
            key = 'algo0_%d' % r
            np.testing.assert_array_equal(d.csd_freq.data[key], cx.freqs(FS, 256))
            p = csd_analysis.Coherence(nperseg=256)          # the plugin on the run's host arrays
            p.run([FS, d.accel.data[r], d.gyro.data[r]])
            f, coh, ph = p.get_results()
            assert coh.shape == ph.shape == (129, 15)
            np.testing.assert_array_equal(d.coherence.data[key], coh)
            np.testing.assert_array_equal(d.csd_phase.data[key], ph)
            assert np.all(coh <= 1 + 1e-12)
    finally:
        os.remove(short)
    print('csd Sim plugin, run_device vs run: error / bound 0 (bitwise)')
