"""GPU: InsLoose's consistency checkpoints (csrc/ins_loose_cons.hip, InsLooseJob(cons_samples=...).consistency(),
Sim.consistency_curve) against their NumPy restatement (tests/ins_loose_cons_ref.py), against the launch without checkpoints and
against the bands of tests/test_ins_loose_cons_oracle.py.  Shapes: 1-129 runs x 300-700 samples at 20 Hz (1024 x 1200 for the
consistency, 257 x 6000 through Sim).  Every test passes an argument the package did not have before.

Parity bound.  Not a recorded constant: every comparison with the restatement evaluates, on its own case and ALL its runs (the
device's dumped sensors, fixes and odometer), the float64 restatement against its np.longdouble evaluation and allows the device
ins_loose_cases.PARITY_MARGIN (16) x that, column by column of the record; a deviation is relative to the column's largest value
over the case's checkpoints (ins_loose_cons_ref.deviation).  The count column is exact."""
import numpy as np
import pytest

import ins_loose_aided_cases as ac
import ins_loose_cases as cs
import ins_loose_cons_ref as cref
from ins_loose_cons_cases import in_bands
from ins_loose_cons_dump import cons_held, record
from ins_loose_dump import Dump, ctx, planes, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', params=[0, 1], ids=['rf0', 'rf1'])
def dump(request, ctx):
    d = Dump(ctx, request.param, 700, 65)                   # 35 s at 20 Hz: 15 s into the outage
    yield d
    d.release()


SAMPLES = [0, 1, 10, 333, 698, 699]                         # the first two and the last two samples; 10 carries a fix


# ------------------------------------------------------------------------------------------------- 1. parity, 2. generated = given
@pytest.mark.parametrize('mask,every', [(0, 1), (7, 7)])
def test_parity_with_the_restatement(ctx, dump, mask, every):
    assert 10 in dump.stamps
    job = dump.job(ctx, given=True, cons_samples=SAMPLES, keep_traj=False, **ac.aid_kw(mask, every)).run()
    assert job.kernel_name() == 'ginsim::loose_cons_kernel<%d, true, false, %s>' % (dump.rf, 'true' if mask else 'false')
    dev = record(job)
    res = job.consistency()
    job.release()
    lo = cons_held('parity', dev, dump, mask, every, SAMPLES)
    assert np.all(res.count == 65) and res.ratio.shape == (6, 9) and np.all(res.nees[2:] > 0)
    np.testing.assert_allclose(res.sigma, np.sqrt(lo[:, 1:16] / 65), rtol=1e-9)


@pytest.mark.parametrize('mask,every', [(0, 1), (7, 7)])
def test_generated_form_equals_given_form_bit_for_bit(ctx, dump, mask, every):
    gen = dump.job(ctx, cons_samples=SAMPLES, keep_traj=False, **ac.aid_kw(mask, every)).run()
    giv = dump.job(ctx, given=True, cons_samples=SAMPLES, keep_traj=False, **ac.aid_kw(mask, every)).run()
    assert gen.kernel_name() == 'ginsim::loose_cons_kernel<%d, false, false, %s>' % (dump.rf, 'true' if mask else 'false')
    a, b = record(gen), record(giv)
    gen.release()
    giv.release()
    assert a[:, 0].min() == 65 and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ------------------------------------------------------------------------------------------------- 3. tail lanes, run lists
TAIL_SAMPLES = [0, 150, 299]


@pytest.mark.parametrize('runs', [1, 63, 64, 65, 129])
def test_run_counts_around_a_wavefront(ctx, runs):
    d = Dump(ctx, 1, 300, runs, seed=21)
    job = d.job(ctx, given=True, cons_samples=TAIL_SAMPLES, keep_traj=False, **ac.aid_kw(7, 1)).run()
    dev = record(job)
    assert np.all(dev[:, 0] == runs)
    cons_held('%d runs' % runs, dev, d, 7, 1, TAIL_SAMPLES)
    if runs == 129:                                         # 40 scattered runs of the 129: the record is over the listed runs
        ids = np.random.default_rng(3).permutation(129)[:40]
        part = record(job.run(ids))
        assert np.all(part[:, 0] == 40)
        cons_held('40 of 129 runs', part, d, 7, 1, TAIL_SAMPLES, runs=ids)
    job.release()
    d.release()


# ------------------------------------------------------------------------------------------------- 4. perturbs nothing, 5. repeatable
def test_the_checkpoint_perturbs_nothing_and_the_record_repeats(ctx):
    n = 300
    d = Dump(ctx, 0, n, 65, seed=31)
    plain = d.job(ctx, **ac.aid_kw(7, 3)).run()
    want = planes(plain)
    pdiag = plain.final_pdiag()
    plain.release()
    every = d.job(ctx, cons_samples=range(n), **ac.aid_kw(7, 3)).run()
    same_bits(planes(every), want)                          # trajectory, wb, ab, end record, pdiag_end, final biases
    dense = record(every)
    again = record(every.run())
    assert np.array_equal(dense.view(np.uint64), again.view(np.uint64))        # two launches of one job: identical bits
    every.release()
    sparse_at = [0, 7, 64, 150, 298, 299]
    sparse = d.job(ctx, cons_samples=sparse_at, keep_traj=False, **ac.aid_kw(7, 3)).run()
    got = record(sparse)
    sparse.release()
    assert np.array_equal(got.view(np.uint64), dense[sparse_at].view(np.uint64))
    assert np.all(dense[:, 0] == 65)
    np.testing.assert_allclose(dense[-1, 1:16] / 65, pdiag.mean(axis=0), rtol=1e-14, atol=0)
    d.release()


# ------------------------------------------------------------------------------------------------- 6. a non-finite lane
def test_a_non_finite_run_is_left_out_of_every_sum(ctx):
    n, bad_run = 300, 33
    d = Dump(ctx, 1, n, 65, seed=51)
    samples = [50, 100, 101, 200, 299]
    acc = ctx.download(d.mc.buffer('accel'), (3, n, 65))
    acc[1, 100:, bad_run] = np.nan                          # enters the state with the step from sample 100 to 101
    bad = ctx.upload(acc)
    job = d.job(ctx, given=True, cons_samples=samples, keep_traj=False, **ac.aid_kw(0))
    job.mc.in_accel = bad.ptr
    dev = record(job.run())
    job.release()
    bad.free()
    assert list(dev[:, 0]) == [65, 65, 64, 64, 64] and np.all(np.isfinite(dev))
    host = d.accel.copy()
    host[bad_run, 100:, 1] = np.nan
    cons_held('non-finite run, all runs', dev, d, 0, 1, samples, accel=host)        # the restatement leaves it out by the same rule
    keep = np.setdiff1d(np.arange(65), [bad_run])
    cons_held('non-finite run, the others', dev[2:], d, 0, 1, samples[2:], runs=keep)
    d.release()


# ------------------------------------------------------------------------------------------------- 7. consistency on the device
@pytest.mark.parametrize('mask', [0, 1, 7])
def test_consistency_bands_on_the_device(ctx, mask):
    """Generated form, 1024 runs x 1200 samples at 20 Hz, ref_frame 1, a checkpoint every 5 s and at the last sample: the bands of
    tests/test_ins_loose_cons_oracle.py hold for the unaided filter and the odometer; with the constraints (mask 7) only the upper
    ends, as DESIGN 4.11b argues for the end point (the truth obeys the constraints exactly, the pseudo-noise overstates them)."""
    import ginsim
    fs, R = cs.CONSISTENCY_FS, cs.CONSISTENCY_RUNS
    ini, truth, _ = ac.outage_truth(fs, 1, cs.CONSISTENCY_FS_GPS)
    acc_e, gyr_e = cs.imu_errors()
    n = truth['ref_accel'].shape[0]
    samples = list(range(0, n, int(round(5 * fs)))) + [n - 1]
    kw = dict(odo_err=ac.ODO_ERR, aid=ac.aid_options(mask)) if mask else {}
    job = ginsim.InsLooseJob(ctx, fs, 1, truth, acc_e, gyr_e, cs.GPS_ERR, ini, R, seed=cs.CONSISTENCY_SEED, cons_samples=samples, **kw).run()
    res = job.consistency()
    job.release()
    t = np.array(samples) / fs
    for row in zip(t, res.ratio, res.nees):
        print('mask %d %6.2f  ' % (mask, row[0]) + '  '.join(' '.join('%.3f' % x for x in v) for v in (row[1][0:3], row[1][3:6], row[1][6:9], row[2])))
    assert np.all(res.count == R)
    in_bands(t, res.ratio, res.nees, lower=mask != 7)


# ------------------------------------------------------------------------------------------------- 8. through Sim
def test_sim_consistency_curve(ctx):
    from demo_algorithms import free_integration
    from demo_algorithms.ins_loose_device import InsLoose
    from ginsim import InsLooseJob, filter_model, workloads
    from gnss_ins_sim.sim import imu_model, ins_sim
    fs, fs_gps, rf, R = 100.0, 10.0, 1, 257
    ini = workloads.parse_motion(cs.OUTAGE_CSV)[0]

    def sim_of(algos, keep):
        imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=True, odo=True)
        s = ins_sim.Sim([fs, fs_gps, 0.0], cs.OUTAGE_CSV, ref_frame=rf, imu=imu, seed=1234, keep_trajectories=keep, algorithm=algos)
        s.run(R)
        return s
    sim = sim_of([free_integration.FreeIntegration(ini), InsLoose(), InsLoose(odo=True, nhc=True)], False)     # statistics only
    assert not sim.loose_jobs[0][1].keep_traj
    curve = sim.consistency_curve(every=5.0)
    free, plain, aided = sim.mc.nav_names
    n = np.asarray(sim.dmgr.time.data).shape[0]
    samples = np.arange(0, n, 500)
    assert np.array_equal(curve['time'], samples / fs) and curve['states'] == cref.STATES
    assert free not in curve and set(curve) == {'time', 'states', plain, aided}
    d = sim.dmgr
    truth = {'ref_accel': d.ref_accel.data, 'ref_gyro': d.ref_gyro.data, 'ref_pos': d.ref_pos.data, 'ref_vel': d.ref_vel.data,
             'ref_att': d.ref_att_euler.data, 'ref_odo': d.ref_odo.data, 'ref_gps': d.ref_gps.data, 'gps_time': d.gps_time.data,
             'gps_visibility': d.gps_visibility.data}
    imu = sim.imu
    for name, algo in ((plain, sim.amgr.algo[1]), (aided, sim.amgr.algo[2])):
        kw = {} if algo.aid() is None else dict(odo_err=imu.odo_err, aid=algo.aid())
        job = InsLooseJob(ctx, fs, rf, truth, imu.accel_err, imu.gyro_err, imu.gps_err, ini, R, seed=1234, earth_rot=algo.earth_rot,
                          model=filter_model(fs, imu.accel_err, imu.gyro_err, imu.gps_err, algo.q_scale, algo.p0), cons_samples=samples,
                          **kw).run()
        want = job.consistency()
        job.release()
        got = curve[name]
        assert np.all(got['count'] == R)
        for key, exp in (('count', want.count), ('sigma', want.sigma), ('rms', want.rms), ('ratio', want.ratio), ('nees', want.nees)):
            assert np.array_equal(got[key], exp), (name, key)
        assert got['sigma'].shape == (samples.size, 15) and got['rms'].shape == got['ratio'].shape == (samples.size, 9)
    out_end = int(np.nonzero(curve['time'] >= 40.0)[0][0])
    assert curve[aided]['sigma'][out_end, 0] < curve[plain]['sigma'][out_end, 0]       # the aiding shows in the predicted sigma
    # samples= in any order, with repeats
    pick = np.array([3000, 0, 5999, 3000])
    some = sim.consistency_curve(samples=pick)
    assert np.array_equal(some['time'], pick / fs)
    assert np.array_equal(some[plain]['sigma'][0], some[plain]['sigma'][3])
    assert np.array_equal(some[plain]['sigma'][[1, 0]], curve[plain]['sigma'][[0, 6]])
    assert np.array_equal(some[aided]['nees'][[1, 0]], curve[aided]['nees'][[0, 6]])
    with pytest.raises(ValueError, match='not both'):
        sim.consistency_curve(every=5.0, samples=[0])
    with pytest.raises(ValueError, match='indices in'):
        sim.consistency_curve(samples=[n])
    none = sim_of([free_integration.FreeIntegration(ini)], False)
    with pytest.raises(ValueError, match='this Sim has none'):
        none.consistency_curve(every=5.0)
