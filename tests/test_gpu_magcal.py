"""GPU: the soft / hard-iron magnetometer calibration (csrc/magcal.hip, ginsim.MagCalJob, MagCal of
demo_algorithms.mag_calibrate_device) -- against the NumPy restatement (tests/magcal_ref.py) on the magnetometer series AuxSensorJob
materialises, the given form against the generated one, the reference's own library through the drop-in Sim
(tests/golden/magcal/), 65 536 runs statistics-only, degenerate ranges, refusals.  Nothing here reads a reference checkout.

Tolerance of a device result against the restatement, per quantity (soft_iron, hard_iron, mag_cal): 16 x the golden's
`reorder_spread` -- what the restatement itself moves by when the rows inside a range are summed in another order, measured by the
golden's maker on the reference side only.  The device sums in another order and from moments, which is what that spread prices;
16 covers the fused multiply-adds and the 3x3 / 4x4 eliminations.  Capped at the 1e-9 the inclinometers are allowed."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, REPO
import magcal_ref

pytestmark = pytest.mark.gpu
SEED = 4242
CSV = os.path.join(GOLDEN, 'magcal', 'motion_def_mag_cal.csv')


def _golden(name):
    return dict(np.load(os.path.join(GOLDEN, 'magcal', name + '.npz'), allow_pickle=False))


def _ndev():
    try:
        import ginsim
        return ginsim.device_count()
    except Exception:
        return 0


NDEV = _ndev()
need2 = pytest.mark.skipif(NDEV < 2, reason='needs >= 2 visible HIP devices, this box has %d' % NDEV)


def _ctx():
    import ginsim
    return ginsim.default_context()


def _truth():
    t = _golden('truth')
    return t, {'si': t['si'], 'hi': t['hi'], 'std': t['std']}


def _segments(name):
    return tuple((int(a), int(b)) for a, b in _golden(name)['segments'])


def _tol(name, extra=False):
    g = _golden(name)
    t = 16.0 * g['reorder_spread'] + (g['lib_vs_restatement'] if extra else 0.0)
    assert np.all(t > 0.0)
    return np.minimum(t, 1e-9)


def _aux(runs, seed=SEED, run_offset=0):
    import ginsim
    t, err = _truth()
    return ginsim.AuxSensorJob(_ctx(), runs, seed=seed, run_offset=run_offset, ref_mag=t['ref_mag'], mag_err=err).run()


def _job(runs, seg, seed=SEED, run_offset=0, **kw):
    import ginsim
    t, err = _truth()
    return ginsim.MagCalJob(_ctx(), t['ref_mag'], err, runs, seg, seed=seed, run_offset=run_offset, **kw)


def _check(got, want, tol, what):
    d = [float(np.max(np.abs(a - b))) for a, b in zip(got, want)]
    print('%s: max |device - checker|  soft_iron %.3g  hard_iron %.3g  mag_cal %.3g   (tolerance %.3g %.3g %.3g)' % ((what,) + tuple(d) + tuple(tol)))
    for a, b in zip(got, want):
        assert a.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all()
    assert d[0] <= tol[0] and d[1] <= tol[1] and d[2] <= tol[2], (d, tol)


# ------------------------------------------------------------------------------- 1. generated form against the restatement
def test_generated_form_equals_the_restatement_on_the_materialised_series():
    R, seg = 64, _segments('full')
    aux = _aux(R)
    mag = aux.series('mag', np.arange(R))
    job = _job(R, seg, keep=True).run()
    try:
        want = magcal_ref.calibrate_series(mag, seg)
        _check((job.soft_iron(), job.hard_iron(), job.mag_cal(np.arange(R))), want, _tol('full'), 'generated, 64 runs')
        st = job.stats()
        assert np.allclose(st['soft_iron']['mean'], job.soft_iron().mean(axis=0), rtol=1e-13, atol=0) and st['hard_iron']['std'].shape == (4,)
        assert np.all(st['soft_iron']['min'] <= st['soft_iron']['max'])
    finally:
        job.release()
        aux.release()


@pytest.mark.parametrize('name', ['arc', 'unequal'])
def test_generated_form_on_other_ranges(name):
    R, seg = 64, _segments(name)
    aux = _aux(R, run_offset=5)
    job = _job(R, seg, run_offset=5, keep=True).run()
    try:
        want = magcal_ref.calibrate_series(aux.series('mag', np.arange(R)), seg)
        _check((job.soft_iron(), job.hard_iron(), job.mag_cal(np.arange(R))), want, _tol(name), name)
    finally:
        job.release()
        aux.release()


# ------------------------------------------------------------------------------- 2. given form == generated form
def test_given_form_on_the_materialised_series_is_the_generated_form_bit_for_bit():
    R, seg = 64, _segments('unequal')
    aux = _aux(R)
    gen = _job(R, seg, keep=True).run()
    import ginsim
    giv = ginsim.MagCalJob(_ctx(), None, None, R, seg, given=aux._bufs['mag'], keep=True, n=aux.n).run()
    try:
        ids = np.arange(R)
        assert np.array_equal(gen.soft_iron(), giv.soft_iron())
        assert np.array_equal(gen.hard_iron(), giv.hard_iron())
        assert np.array_equal(gen.mag_cal(ids), giv.mag_cal(ids))
        assert np.isfinite(gen.mag_cal(ids)).all()
    finally:
        gen.release()
        giv.release()
        aux.release()


# ------------------------------------------------------------------------------- 3. through the drop-in Sim, against the library
def _sim(algo, runs, **kw):
    from gnss_ins_sim.sim import imu_model, ins_sim
    t = _golden('truth')
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=9, gps=False)
    imu.mag_err = dict(imu.mag_err)
    imu.set_mag_error({'si': t['si'].copy(), 'hi': t['hi'].copy()})
    fs = float(t['fs'])
    sim = ins_sim.Sim([fs, 0.0, fs], CSV, ref_frame=1, imu=imu, algorithm=algo, seed=int(t['seed']), geo_mag_n=t['geo_mag_n'], **kw)
    sim.run(runs)
    return sim


def test_sim_fills_the_data_manager_as_the_reference_does():
    from demo_algorithms.mag_calibrate_device import MagCal
    g, t = _golden('full'), _golden('truth')
    R = int(t['runs'])
    algo = MagCal(segments=_segments('full'))
    sim = _sim(algo, R)
    d = sim.dmgr
    assert np.max(np.abs(d.ref_mag.data - t['ref_mag'])) < 1e-9
    rows = t['mag_rows']
    mag = np.stack([d.mag.data[r][rows] for r in range(R)])
    print('max |mag - reference mag| at the stored rows: %.3g' % np.max(np.abs(mag - t['mag_at_rows'])))
    si = np.stack([d.soft_iron.data['algo0_%d' % r] for r in range(R)])
    hi = np.stack([d.hard_iron.data['algo0_%d' % r] for r in range(R)])
    cal = np.stack([d.mag_cal.data['algo0_%d' % r] for r in range(R)])
    assert si.shape == (R, 3, 3) and hi.shape == (R, 1, 4) and cal.shape == g['mag_cal'].shape
    _check((si, hi, cal), (g['soft_iron'], g['hard_iron'], g['mag_cal']), _tol('full', extra=True), 'Sim against libmagcal.so')
    # the plugin object holds the last run's results, as after the reference's loop
    res = algo.get_results()
    assert np.array_equal(res[0], si[-1]) and np.array_equal(res[1], hi[-1]) and np.array_equal(res[2], cal[-1])
    assert sorted(d.soft_iron.data.keys()) == ['algo0_%d' % r for r in range(R)]


def test_sim_statistics_only_and_segments_from_the_truth():
    from demo_algorithms.mag_calibrate_device import MagCal, segments_from_truth
    t = _golden('truth')
    seg = segments_from_truth(t['ref_gyro'])
    kept = _sim(MagCal(), 40)
    only = _sim(MagCal(), 40, keep_trajectories=False, keep_runs=2)
    assert 'mag' not in only.dmgr.available or len(only.dmgr.mag.data) == 2      # nothing of mag beyond the kept runs
    for r in (0, 1, 39):
        assert np.array_equal(kept.dmgr.soft_iron.data['algo0_%d' % r], only.dmgr.soft_iron.data['algo0_%d' % r])
        assert np.array_equal(kept.dmgr.hard_iron.data['algo0_%d' % r], only.dmgr.hard_iron.data['algo0_%d' % r])
    assert len(only.dmgr.mag_cal.data) == 2 and len(kept.dmgr.mag_cal.data) == 40
    assert np.array_equal(kept.dmgr.mag_cal.data['algo0_1'], only.dmgr.mag_cal.data['algo0_1'])
    # the ranges are those of the truth: the same numbers as a job with them spelled out
    job = None
    try:
        import ginsim
        job = ginsim.MagCalJob(_ctx(), kept.dmgr.ref_mag.data, kept.imu.mag_err, 40, seg, seed=int(t['seed'])).run()
        assert np.array_equal(job.soft_iron()[39], kept.dmgr.soft_iron.data['algo0_39'])
    finally:
        if job is not None:
            job.release()
    none = _sim(MagCal(), 3, keep_trajectories=False)
    assert len(none.dmgr.mag_cal.data) == 0 and len(none.dmgr.soft_iron.data) == 3


def test_plugin_called_directly_on_one_series():
    from demo_algorithms.mag_calibrate_device import MagCal
    seg = _segments('full')
    aux = _aux(2)
    try:
        mag = aux.series('mag', [1])[0]
    finally:
        aux.release()
    m = MagCal(segments=seg)
    m.run([mag])
    si, hi, cal = m.get_results()
    assert si.shape == (3, 3) and hi.shape == (1, 4) and cal.shape == (sum(b - a for a, b in seg), 3)
    want = magcal_ref.calibrate_series(mag, seg)
    _check((si, hi[0], cal), want, _tol('full'), 'MagCal.run on one series')


# ------------------------------------------------------------------------------- 4. full size, statistics only
def test_full_size_statistics_only_without_a_mag_series():
    R, seg = 65536, _segments('full')
    t, _ = _truth()
    n = t['ref_mag'].shape[0]
    job = _job(R, seg).run()
    try:
        si, hi = job.soft_iron(), job.hard_iron()
        assert np.isfinite(si).all() and np.isfinite(hi).all()
        for r in (0, 63, 64, 32767, 65535):
            solo = _job(1, seg, run_offset=r).run()
            try:
                assert np.array_equal(solo.soft_iron()[0], si[r]) and np.array_equal(solo.hard_iron()[0], hi[r]), r
            finally:
                solo.release()
        series_bytes = 3 * n * R * 8                    # one mag plane set for all runs: 22 GB
        assert job.device_bytes == n * 3 * 8 + 13 * R * 8
        assert job.device_bytes < 0.01 * series_bytes
        with pytest.raises(ValueError):
            job.mag_cal([0])                            # nothing was kept
        st = job.stats()
        print('65 536 runs: soft_iron mean\n%s\nstd\n%s\nhard_iron mean %s std %s' % (st['soft_iron']['mean'], st['soft_iron']['std'],
                                                                                  st['hard_iron']['mean'], st['hard_iron']['std']))
        # a sanity bound, not a parity check: the algorithm fixes the x sensitivity at 1, so the estimate is inv(si) up to one
        # common factor; it is exact to first order in si's off-diagonal entries (<= 0.03 here: second order ~1e-3, bound 0.02)
        inv = np.linalg.inv(t['si'])
        scale = st['soft_iron']['mean'][0, 0] / inv[0, 0]
        assert np.max(np.abs(st['soft_iron']['mean'] - scale * inv)) < 0.02
    finally:
        job.release()


# ------------------------------------------------------------------------------- 5. degenerate ranges
def test_range_without_rotation_and_a_singular_range_then_a_normal_launch():
    R, seg = 64, _segments('norot')
    aux = _aux(R)
    job = _job(R, seg, keep=True).run()                     # the launch returns
    try:
        mag = aux.series('mag', np.arange(R))
        want = magcal_ref.calibrate_series(mag, seg)
        for a, b in zip((job.soft_iron(), job.hard_iron(), job.mag_cal(np.arange(R))), want):
            assert np.array_equal(np.isfinite(a), np.isfinite(b))
    finally:
        job.release()
    # an x range of identical rows of small integers: M^T M is singular exactly, the elimination meets 0 / 0 in both
    import ginsim
    rows = mag[:4].copy()
    rows[:, 100:160] = np.array([1.0, 2.0, 2.0])
    rows[3, 100:160] = mag[3, 2007:2067]                    # one run of the launch stays regular
    dseg = ((100, 160), seg[1], (12007, 13007))
    given = _ctx().upload(np.ascontiguousarray(rows.transpose(2, 1, 0)))       # [3][n][4]
    deg = ginsim.MagCalJob(_ctx(), None, None, 4, dseg, given=given, keep=True, n=rows.shape[1]).run()
    try:
        want = magcal_ref.calibrate_series(rows, dseg)
        got = (deg.soft_iron(), deg.hard_iron(), deg.mag_cal(np.arange(4)))
        for a, b in zip(got, want):
            assert np.array_equal(np.isfinite(a), np.isfinite(b))
        assert not np.isfinite(got[0][:3]).any() and not np.isfinite(got[1][:3]).any() and not np.isfinite(got[2][:3]).any()
        assert np.isfinite(got[0][3]).all() and np.isfinite(got[1][3]).all() and np.isfinite(got[2][3]).all()
    finally:
        deg.release()
        given.free()
    # a following normal launch is correct
    nseg = _segments('full')
    nxt = _job(R, nseg, keep=True).run()
    try:
        _check((nxt.soft_iron(), nxt.hard_iron(), nxt.mag_cal(np.arange(R))), magcal_ref.calibrate_series(mag, nseg), _tol('full'),
               'after the degenerate launches')
    finally:
        nxt.release()
        aux.release()


# ------------------------------------------------------------------------------- 6. refusals
def test_argument_errors_of_the_entry_point_and_the_job():
    import ginsim
    from ginsim import _lib
    t, err = _truth()
    n = t['ref_mag'].shape[0]
    ctx = _ctx()
    ref = ctx.upload(np.ascontiguousarray(t['ref_mag']))
    out = ctx.malloc(13 * 8 * 8)
    try:
        def call(seg=(10, 20, 30, 40, 50, 60), runs=8, ref_mag=ref.ptr, in_mag=None):
            p = _lib.MagCalParams()
            p.n, p.runs, p.seed = n, runs, 1
            p.seg[:] = list(seg)
            p.ref_mag, p.in_mag, p.out_si, p.out_hi = ref_mag, in_mag, out.ptr, out.at(9 * 8 * 8)
            return _lib.lib.ginsim_magcal_run(ctx.handle, C.byref(p))
        assert call() == _lib.OK
        ctx.sync()
        for bad in (dict(seg=(10, 20, 30, 40, 50, n + 1)), dict(seg=(-1, 20, 30, 40, 50, 60)), dict(seg=(10, 10, 30, 40, 50, 60)),
                    dict(seg=(10, 20, 40, 30, 50, 60)), dict(ref_mag=None), dict(runs=0)):
            assert call(**bad) == _lib.ERR_ARG, bad
            with pytest.raises(ValueError):
                _lib.check(call(**bad))
    finally:
        ref.free()
        out.free()
    for seg in (((10, 20), (30, 40), (50, n + 1)), ((10, 10), (30, 40), (50, 60)), ((10, 20), (30, 40))):
        with pytest.raises(ValueError):
            _job(8, seg)
    with pytest.raises(ValueError):
        _job(0, _segments('full'))
    with pytest.raises(ValueError):
        ginsim.MagCalJob(ctx, None, None, 8, _segments('full'))


def test_sim_refusals():
    from gnss_ins_sim.sim import imu_model, ins_sim
    from demo_algorithms.mag_calibrate_device import MagCal
    t = _golden('truth')
    fs = float(t['fs'])
    with pytest.raises(ValueError, match='magnetometer'):
        ins_sim.Sim([fs, 0.0, fs], CSV, ref_frame=1, imu=imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=False),
                    algorithm=MagCal(segments=_segments('full')), seed=1).run(2)
    with pytest.raises(NotImplementedError, match='fp64'):
        _sim(MagCal(segments=_segments('full')), 2, precision='f32')
    with pytest.raises(ValueError, match='outside'):
        _sim(MagCal(segments=((10, 20), (30, 40), (50, 10 ** 6))), 2)


@need2
def test_sim_refuses_to_spread_a_magcal_over_devices():
    from demo_algorithms.mag_calibrate_device import MagCal
    with pytest.raises(ValueError, match='several GPUs'):
        _sim(MagCal(segments=_segments('full')), 4, devices=[0, 1])
