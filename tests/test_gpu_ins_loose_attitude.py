"""GPU: the four InsLoose kernels (loose_kernel, loose_aided_kernel, loose_mag_kernel, loose_cons_kernel) away from the level
profile every other test of theirs runs: on tests/golden/ins_loose/motion_def_tilted.csv (41 S 150 W, yaw through +-180 deg twice,
pitch 20 -> -20 -> 20 deg, roll -15 -> 15 -> -15 deg, climbing and descending, the southern field GEO_SOUTH) and on a table of 130
different initial states in one launch (yaw at 0, +-90, +-179.999 and 180 deg, pitch to +-85 deg, roll over +-180 deg, latitude
-80 to 80 deg, longitude to +-179.9 deg, altitude -100 m to 10 km).  tests/test_ins_loose_attitude_oracle.py holds the restatements
these kernels are compared with to the nonlinear model.  Shapes: 65 runs x 800 samples and 130 x 200 at 20 Hz (1024 runs for the
consistency).

Parity bound, as in the other InsLoose files: not a recorded constant.  Every comparison measures, on its own case, the float64
restatement against its np.longdouble evaluation and allows the device ins_loose_cases.PARITY_MARGIN (16) x that; on the sweep over
all 130 runs, since every run is another attitude (the runs near +-85 deg of pitch, whose Euler angles are ill conditioned, set the
bound of the case).  A bound per run was tried first and is printed for information only: the largest rounding error of ONE run
of 200 samples is too noisy a statistic -- the magnetometer kernel exceeded 16 x it by up to 3.8 x in 1e-13-sized entries of single
runs (vel 8.9e-13 against 2.4e-13), the plain kernel stayed below it everywhere.

Measured on the MI355X (largest deviation of the device from the restatement over both frames, and the smallest bound it met):
  tilted profile   loose_kernel        att 1.0e-14 (2.4e-12)  pos 2.7e-15 (6.0e-14)  vel 2.8e-13 (7.7e-11)  wb 1.2e-11 (4.9e-09)  ab 4.6e-12 (2.3e-09)  pdiag_end 3.0e-14 (4.8e-12)
                   loose_aided_kernel  att 1.7e-14 (2.8e-12)  pos 1.1e-15 (5.5e-14)  vel 1.4e-13 (2.0e-11)  wb 2.0e-12 (1.5e-09)  ab 2.3e-12 (8.2e-10)  pdiag_end 2.3e-14 (1.4e-12)
                   loose_mag_kernel    att 5.3e-14 (4.3e-13)  pos 1.0e-14 (8.4e-14)  vel 1.2e-12 (1.4e-11)  wb 4.6e-11 (3.6e-10)  ab 1.9e-11 (7.9e-10)  pdiag_end 5.2e-14 (6.8e-13)
                   loose_cons_kernel   largest column deviation 4.6e-11 (relative to the column's largest value); closest to its bound
                                       P_dr_x 1.5e-15 (1.5e-14)
  sweep            loose_kernel        att 2.7e-15  pos 7.5e-15  vel 1.9e-13  wb 7.8e-12  ab 1.2e-11  pdiag_end 5.8e-15
                   loose_mag_kernel    att 7.8e-14  pos 2.5e-15  vel 8.9e-13  wb 1.0e-10  ab 2.3e-11  pdiag_end 4.3e-14
                   (per run, each relative to its own run; the bounds of the case are printed by the test)
  generated = given and ini_first = 65 against runs 65-129: the same bits.  Consistency: the restatement's ratios to three digits.
"""
import numpy as np
import pytest

import ins_loose_aided_cases as ac
import ins_loose_cases as cs
import ins_loose_mag_cases as mc
import ins_loose_ref as ref
from ins_loose_cons_dump import cons_held, record
from ins_loose_dump import Dump, ctx, held, planes, result, same_bits
from ins_loose_sweep import SWEEP_RUNS, sweep

pytestmark = pytest.mark.gpu

FS, FS_GPS = 20.0, 2.0
RUNS, N = 65, 800


@pytest.fixture(scope='module', params=[0, 1], ids=['rf0', 'rf1'])
def dump(request, ctx):
    """The device's own sensors, fixes, odometer and magnetometer of 65 runs over the whole tilted profile: every kernel's case."""
    d = Dump(ctx, request.param, None, RUNS, truth_fn=mc.outage_truth, profile=cs.TILTED_CSV, geo=mc.GEO_SOUTH, mag_errs=(('skew', mc.MAG_ERR_SKEW),))
    assert d.n == N
    yield d
    d.release()


def wraps(yaw):
    """Indices j with a yaw wrap between samples j and j + 1 of a series (n,)."""
    return np.nonzero(np.abs(np.diff(yaw)) > np.pi)[0]


def restated(d, kernel, mask, every, dtype=np.float64, runs=slice(None)):
    args = (d.rf, d.fs, d.gyro[runs], d.accel[runs], d.ini, d.model, d.gps[runs], d.stamps, d.truth['gps_visibility'])
    aid = ac.aid(mask, every) if mask else None
    if kernel == 'loose':
        return ref.run(*args, dtype=dtype)
    if kernel == 'aided':
        return ref.run(*args, dtype=dtype, odo=d.odo[runs], aid=aid)
    return ref.run(*args, dtype=dtype, odo=d.odo[runs], aid=aid, mag=d.mag['skew'][runs], mag_model=mc.model(mc.MAG_ERR_SKEW, d.rf, 1, d.geo))


def job_of(ctx, d, kernel, mask, every, given, **kw):
    kw = ac.aid_kw(mask, every, **kw)
    if kernel == 'mag':
        kw = mc.mag_kw(mc.MAG_ERR_SKEW, d.geo, **kw)
        given = d.given_with_mag('skew') if given else False
    return d.job(ctx, given, **kw)


CASES = [('loose', 0, 1), ('aided', 7, 7), ('mag', 0, 1), ('mag', 7, 1)]
KERNEL = {'loose': 'loose_kernel', 'aided': 'loose_aided_kernel', 'mag': 'loose_mag_kernel'}


# ------------------------------------------------------------------------------------------------- C1 parity on the tilted profile
@pytest.mark.parametrize('kernel, mask, every', CASES, ids=['loose', 'aided7', 'mag', 'mag7'])
def test_parity_on_the_tilted_profile(ctx, dump, kernel, mask, every):
    job = job_of(ctx, dump, kernel, mask, every, True).run()
    assert job.kernel_name().startswith('ginsim::%s<%d, true,' % (KERNEL[kernel], dump.rf))
    dev = result(job)
    job.release()
    assert all(wraps(dev['att'][r, :, 0]).size >= 2 for r in range(RUNS))        # the estimate passes +-180 deg twice, as the truth
    assert wraps(dump.truth['ref_att'][:, 0]).size == 2
    exp = restated(dump, kernel, mask, every)
    hi = restated(dump, kernel, mask, every, np.longdouble, slice(0, 8))
    err = cs.deviation({k: exp[k][:8] for k in cs.PARITY_KEYS}, hi)
    got = cs.deviation(dev, exp)
    held('tilted parity rf%d %s mask %d' % (dump.rf, kernel, mask), got, {k: cs.PARITY_MARGIN * err[k] for k in got})


def checkpoints(truth):
    """Sample 0, the two samples either side of each yaw wrap, the samples of extreme pitch, the last two."""
    w = wraps(truth['ref_att'][:, 0])
    pitch = truth['ref_att'][:, 1]
    return [0] + [int(j) + s for j in w for s in (0, 1)] + [int(np.argmax(pitch)), int(np.argmin(pitch)), N - 2, N - 1]


@pytest.mark.parametrize('mask, every', [(0, 1), (7, 7)])
def test_checkpoint_parity_on_the_tilted_profile(ctx, dump, mask, every):
    samples = checkpoints(dump.truth)
    assert len(samples) == 9 and samples[1] + 1 == samples[2] and samples[3] + 1 == samples[4]
    job = job_of(ctx, dump, 'cons', mask, every, True, cons_samples=samples, keep_traj=False).run()
    assert job.kernel_name() == 'ginsim::loose_cons_kernel<%d, true, false, %s>' % (dump.rf, 'true' if mask else 'false')
    dev = record(job)
    job.release()
    assert np.all(dev[:, 0] == RUNS)
    cons_held('tilted checkpoints', dev, dump, mask, every, samples)


# ------------------------------------------------------------------------------------------------- C2 generated = given
@pytest.mark.parametrize('kernel, mask, every', [('loose', 0, 1), ('aided', 7, 7), ('mag', 7, 1), ('cons', 7, 7)], ids=['loose', 'aided7', 'mag7', 'cons7'])
def test_generated_form_equals_given_form_bit_for_bit(ctx, dump, kernel, mask, every):
    kw = dict(cons_samples=checkpoints(dump.truth), keep_traj=False) if kernel == 'cons' else {}
    gen, giv = job_of(ctx, dump, kernel, mask, every, False, **kw).run(), job_of(ctx, dump, kernel, mask, every, True, **kw).run()
    name = KERNEL.get(kernel, 'loose_cons_kernel')
    assert gen.kernel_name().startswith('ginsim::%s<%d, false,' % (name, dump.rf)) and giv.kernel_name().startswith('ginsim::%s<%d, true,' % (name, dump.rf))
    if kernel == 'cons':
        a, b = record(gen), record(giv)
        assert a[:, 0].min() == RUNS and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    else:
        same_bits(planes(gen), planes(giv))
    gen.release()
    giv.release()


# ------------------------------------------------------------------------------------------------- C3 a table of initial states
# (the table and the `sweep` fixture: tests/ins_loose_sweep.py, shared with tests/test_gpu_ins_loose_tilted_aids.py)
def upload(ctx, s, runs):
    return {k: ctx.upload(np.ascontiguousarray(s[k][runs].transpose(2, 1, 0))) for k in ('accel', 'gyro', 'gps', 'mag')}


def sweep_job(ctx, s, bufs, runs, with_mag, **kw):
    import ginsim
    if with_mag:
        kw = dict(kw, mag_err=mc.MAG_ERR_SKEW, geo_mag_n=mc.GEO_SOUTH, mag={})
    return ginsim.InsLooseJob(ctx, FS, s['rf'], s['truth'], s['acc_e'], s['gyr_e'], cs.GPS_ERR, s['table'], runs, given=bufs, keep_traj=True, **kw)


@pytest.mark.parametrize('with_mag', [False, True], ids=['loose', 'mag'])
def test_a_table_of_initial_states_in_one_launch(ctx, sweep, with_mag):
    """Run r starts from row r of the table: parity with the restatement given the same table, within 16 x the restatement's own
    float64 error on this case (all 130 runs); and a second launch of 65 runs with ini_first = 65 is runs 65-129 of the first, bit
    for bit."""
    s, rf = sweep, sweep['rf']
    bufs = upload(ctx, s, slice(None))
    job = sweep_job(ctx, s, bufs, SWEEP_RUNS, with_mag).run()
    assert job.kernel_name() == 'ginsim::%s<%d, true, false, false>' % ('loose_mag_kernel' if with_mag else 'loose_kernel', rf)
    dev, whole = result(job), planes(job)
    job.release()
    args = (rf, FS, s['gyro'], s['accel'], s['table'], s['model'], s['gps'], s['stamps'], s['truth']['gps_visibility'])
    kw = dict(mag=s['mag'], mag_model=mc.model(mc.MAG_ERR_SKEW, rf, 1, mc.GEO_SOUTH)) if with_mag else {}
    exp, hi = ref.run(*args, **kw), ref.run(*args, dtype=np.longdouble, **kw)
    assert np.all(np.isfinite(dev['att'])) and np.all(np.isfinite(dev['pdiag_end']))
    got, err = cs.deviation(dev, exp), cs.deviation(exp, hi)
    worst = {k: (0.0, 1.0, -1) for k in cs.PARITY_KEYS}                           # for information: run by run, each against its own bound
    for r in range(SWEEP_RUNS):
        one = lambda o: {k: o[k][r:r + 1] for k in cs.PARITY_KEYS}
        g, e = cs.deviation(one(dev), one(exp)), cs.deviation(one(exp), one(hi))
        for k in g:
            if g[k] / max(cs.PARITY_MARGIN * e[k], 1e-300) > worst[k][0] / worst[k][1]:
                worst[k] = (g[k], max(cs.PARITY_MARGIN * e[k], 1e-300), r)
    print('sweep rf%d %s, run by run, closest to 16 x its own error: ' % (rf, 'mag' if with_mag else 'loose') +
          ', '.join('%s %.2e (%.2e, run %d)' % ((k,) + worst[k]) for k in worst))
    held('sweep rf%d %s' % (rf, 'mag' if with_mag else 'loose'), got, {k: cs.PARITY_MARGIN * err[k] for k in got})
    for b in bufs.values():
        b.free()
    half = slice(65, 130)
    bufs = upload(ctx, s, half)
    second = sweep_job(ctx, s, bufs, 65, with_mag, ini_first=65).run()
    same_bits(whole, planes(second), runs_a=np.arange(65, 130))
    second.release()
    for b in bufs.values():
        b.free()


# ------------------------------------------------------------------------------------------------- C4 consistency on the device
def device_end(ctx, c, name):
    """The filter FILTERS[name] on the device over an ins_loose_mag_cases.consistency_draw: (error state (R, 15), pdiag_end (R, 15)) at
    the last sample.  Nothing is kept: the end state is the truth's last row plus the end-point record."""
    import ginsim
    with_mag, mask = mc.FILTERS[name]
    bufs = {k: ctx.upload(np.ascontiguousarray(c[k].transpose(2, 1, 0))) for k in ('accel', 'gyro', 'gps') + (('mag',) if with_mag else ())}
    kw = {}
    if mask:
        bufs['odo'] = ctx.upload(np.ascontiguousarray(c['odo'].T))
        kw.update(odo_err=ac.ODO_ERR, aid=ac.aid_options(mask))
    if with_mag:
        kw.update(mag_err=c['mag_err'], geo_mag_n=c['geo'], mag={})
    t = c['truth']
    job = ginsim.InsLooseJob(ctx, c['fs'], c['rf'], t, c['acc_e'], c['gyr_e'], cs.GPS_ERR, c['ini'], c['runs'], given=bufs, **kw).run()
    end = job.end_errors()
    wb, ab = job.final_biases()
    pdiag = job.final_pdiag()
    job.release()
    for b in bufs.values():
        b.free()
    e = mc.end_error(c, t['ref_att'][-1] + end[:, 0:3], t['ref_pos'][-1] + end[:, 3:6], t['ref_vel'][-1] + end[:, 6:9], wb, ab)
    return e, pdiag


@pytest.fixture(scope='module')
def drawn():
    cache = {}

    def get(profile, rf):
        if (profile, rf) not in cache:
            cache.clear()                                                     # one draw at a time: 1024 runs of five series
            cache[profile, rf] = mc.consistency_draw(profile, rf, cs.CONSISTENCY_FS, cs.CONSISTENCY_RUNS)
        return cache[profile, rf]
    return get


@pytest.mark.parametrize('name', list(mc.FILTERS))
def test_consistency_on_the_tilted_profile(ctx, drawn, name):
    """ref_frame 1, 1024 x 800: RMS end error over sqrt(mean pdiag_end) within x/: 1.25 of the ratio the restatement gave on the same
    draw (ins_loose_mag_cases.CONSISTENCY_BY_PROFILE; the 1 sigma of an RMS over 1024 runs is 2.2 %, plus correlation)."""
    e, pdiag = device_end(ctx, drawn('tilted', 1), name)
    ratio = mc.end_statistics(e, pdiag)['ratio']
    want = np.array(mc.CONSISTENCY_BY_PROFILE['tilted'][name])
    print("tilted, ref_frame 1, '%s' on the device: " % name + ', '.join('%.3f' % x for x in ratio))
    assert np.all(want <= 1.4) and (name == 'mag7' or np.all(want >= 0.7))
    assert np.all(ratio <= want * 1.25) and np.all(ratio >= want / 1.25), ratio / want


@pytest.mark.parametrize('name', ['gps', 'mag'])
@pytest.mark.parametrize('profile', ['level', 'tilted'])
def test_consistency_in_ref_frame_0(ctx, drawn, profile, name):
    """ref_frame 0, 1024 runs at 20 Hz: the spread of the end error is the covariance's ([0.7, 1.4] for all 15 states) and its mean
    is the error-free offset ins_loose_mag_cases.E0_OVER_SIGMA records, within 4 sigma / sqrt(R) per state."""
    c = drawn(profile, 0)
    e, pdiag = device_end(ctx, c, name)
    s = mc.end_statistics(e, pdiag)
    excess = (s['mean'] - np.array(mc.E0_OVER_SIGMA[profile, name, int(c['fs'])])) * np.sqrt(c['runs'])
    print("ref_frame 0, %s, '%s' on the device: spread %s\n    (mean - e0) in sigma / sqrt(R): %s"
          % (profile, name, ', '.join('%.3f' % x for x in s['spread']), ', '.join('%.2f' % x for x in excess)))
    assert np.all(s['spread'] >= 0.7) and np.all(s['spread'] <= 1.4), s['spread']
    assert np.all(np.abs(excess) <= 4.0), excess
