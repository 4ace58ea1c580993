"""GPU: InsLoose aided by the magnetometer (csrc/ins_loose_mag.hip, InsLooseJob(mag=...), InsLoose(mag=True), the 'loose' role of
Sim) against its NumPy restatement (tests/ins_loose_ref.py), against the unaided and the odometer-aided launch, against
AuxSensorJob's magnetometer series and against the statistics of its own covariance.  Shapes: 1-129 runs x 200-700 samples
(1024 x 1200 for the consistency, 257 x 6000 through Sim).  Every test passes an argument the package did not have before.

Parity bound, as tests/test_gpu_ins_loose_aided.py: not a recorded constant.  Every comparison with the restatement measures, on
its own case (the device's dumped sensors, fixes, odometer and magnetometer, the first 8 runs), the float64 restatement against its
np.longdouble evaluation (ins_loose_cases.restatement_error) and allows the device ins_loose_cases.PARITY_MARGIN (16) x that.
Measured on the MI355X over the twelve parity cases (700 samples, 65 runs, both frames; the largest deviation of the device from
the restatement, and in brackets the smallest bound any case allowed): att 2.8e-14 (3.3e-13), pos 3.0e-14 (5.6e-14), vel 1.7e-13
(5.0e-12), wb 5.7e-11 (5.8e-11, in different cases: the closest single case is 1.7e-11 against 7.2e-11), ab 1.3e-11 (8.1e-10),
pdiag_end 1.4e-13 (3.1e-13); through Sim att 1.2e-13, pos 2.0e-16, vel 9.1e-13, wb 2.9e-10, ab 8.0e-11, pdiag_end 1.4e-13.
Generated = given: the same bits.  Consistency: the restatement's ratios to all three recorded digits, both masks.  Launch times:
profiles/ins_loose_mag_timing.json."""
import numpy as np
import pytest

import ins_loose_aided_cases as ac
import ins_loose_cases as cs
import ins_loose_dump
import ins_loose_mag_cases as mc
import ins_loose_ref as ref
from ins_loose_dump import ctx, held, planes, result, same_bits

pytestmark = pytest.mark.gpu


class Dump(ins_loose_dump.Dump):
    """With one magnetometer series per magnetometer model."""

    def __init__(self, ctx, rf, n, runs, seed=77, run_offset=0, fs=20.0, fs_gps=2.0, mag_errs=(('plain', mc.MAG_ERR), ('skew', mc.MAG_ERR_SKEW)),
                 profile=cs.OUTAGE_CSV, geo=mc.GEO):
        super().__init__(ctx, rf, n, runs, seed, run_offset, fs, fs_gps, truth_fn=mc.outage_truth, profile=profile, geo=geo, mag_errs=mag_errs)

    def job(self, ctx, which, mask=0, every=1, given=False, runs=None, aid_every=1, **kw):
        """which: 'plain' | 'skew', the magnetometer model that generates and that the filter assumes; None: no magnetometer
        argument at all.  mask 0: no aiding argument at all."""
        kw = ac.aid_kw(mask, aid_every, **kw)
        if which is not None:
            kw = mc.mag_kw(self.mag_errs[which], self.geo, every, **kw)
            given = self.given_with_mag(which) if given else False
        return super().job(ctx, given, runs=runs, **kw)

    def _kw(self, which, mask, every):
        return dict(odo=self.odo, mag=self.mag[which]), ac.aid(mask) if mask else None, mc.model(self.mag_errs[which], self.rf, every, self.geo)

    def restate(self, which, mask, every):
        series, aid, model = self._kw(which, mask, every)
        return ref.run(*self._args(), aid=aid, mag_model=model, **series)

    def bound(self, which, mask, every):
        series, aid, model = self._kw(which, mask, every)
        return cs.parity_bound(*self._args(), odo=series['odo'], aid=aid, mag=series['mag'], mag_model=model)


@pytest.fixture(scope='module', params=[0, 1], ids=['rf0', 'rf1'])
def dump(request, ctx):
    d = Dump(ctx, request.param, 700, 65)                   # 35 s at 20 Hz: 15 s into the outage; one wavefront plus one lane
    yield d
    d.release()


# ------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize('every', [1, 7])
@pytest.mark.parametrize('which, mask', [('plain', 0), ('skew', 0), ('skew', 7)])
def test_parity_with_the_restatement(ctx, dump, which, mask, every):
    assert np.any(dump.truth['gps_visibility'] == 0)                           # the outage's start is inside the cut
    job = dump.job(ctx, which, mask, every, given=True).run()
    assert job.kernel_name() == 'ginsim::loose_mag_kernel<%d, true, false, false>' % dump.rf
    dev = result(job)
    job.release()
    held('parity rf%d %s mask %d every %d' % (dump.rf, which, mask, every), cs.deviation(dev, dump.restate(which, mask, every)),
         dump.bound(which, mask, every))
    plain = dump.job(ctx, None, mask, given=True).run()
    assert not np.array_equal(result(plain)['att'], dev['att'])                # the block did something
    plain.release()


# ------------------------------------------------------------------------------------------------- 2. generated = given
@pytest.mark.parametrize('rf, run_offset, which, mask', [(0, 0, 'plain', 0), (1, 2 ** 40, 'skew', 0), (1, 0, 'plain', 1)])
def test_generated_form_equals_given_form_bit_for_bit(ctx, rf, run_offset, which, mask):
    """The lane regenerates the magnetometer sample ginsim_aux_sensors stores for the same seed and run id (given['mag'] is
    AuxSensorJob's out_mag): every output is the same bits, also with a run offset beyond 32 bits and a general calibration."""
    d = Dump(ctx, rf, 300, 65, seed=41, run_offset=run_offset, fs=100.0, fs_gps=10.0, mag_errs=((which, mc.MAG_ERR if which == 'plain' else mc.MAG_ERR_SKEW),))
    gen, giv = d.job(ctx, which, mask, 3, aid_every=2).run(), d.job(ctx, which, mask, 3, given=True, aid_every=2).run()
    assert (gen.variant(), giv.variant()) == (0, 1)
    assert gen.kernel_name() == 'ginsim::loose_mag_kernel<%d, false, false, false>' % rf
    assert giv.kernel_name() == 'ginsim::loose_mag_kernel<%d, true, false, false>' % rf
    same_bits(planes(gen), planes(giv))
    none = d.job(ctx, None, mask, aid_every=2).run()
    assert not np.array_equal(planes(none)['traj'], planes(gen)['traj'])       # and the block fired
    if run_offset:
        other = Dump(ctx, rf, 300, 65, seed=41, fs=100.0, fs_gps=10.0, mag_errs=((which, mc.MAG_ERR_SKEW),))
        assert not np.array_equal(other.mag[which], d.mag[which])              # the run id enters the magnetometer's counter
        other.release()
    for j in (gen, giv, none):
        j.release()
    d.release()


# ------------------------------------------------------------------------------------------------- 3. a block that never fires
@pytest.mark.parametrize('every', ['n', 2 ** 40])
@pytest.mark.parametrize('mask', [0, 7])
def test_a_block_that_never_fires_is_the_launch_without_it(ctx, dump, mask, every):
    """mag_every >= n: the unaided launch (mask 0; the compiled-in odometer block never fires either, not even at sample 0) or the
    odometer-aided launch (mask 7), bit for bit on every output."""
    every = dump.n if every == 'n' else every
    for given in (False, True):
        without, never = dump.job(ctx, None, mask, given=given).run(), dump.job(ctx, 'skew', mask, every, given=given).run()
        assert without.kernel_name().startswith('ginsim::loose_aided_kernel<' if mask else 'ginsim::loose_kernel<')
        assert never.kernel_name().startswith('ginsim::loose_mag_kernel<')
        same_bits(planes(without), planes(never))
        without.release()
        never.release()


# ------------------------------------------------------------------------------------------------- 4. run counts, run lists
@pytest.fixture(scope='module')
def big(ctx):
    d = Dump(ctx, 1, 200, 129, seed=21, mag_errs=(('skew', mc.MAG_ERR_SKEW),))
    job = d.job(ctx, 'skew', 7, 2).run()
    yield d, planes(job)
    job.release()
    d.release()


@pytest.mark.parametrize('runs', [1, 63, 64, 65, 129])
def test_run_counts_around_a_wavefront(ctx, big, runs):
    """Run r of a small launch is run r of the 129-run launch with the same seed (one lane per run, no neighbour in it)."""
    d, whole = big
    small = d.job(ctx, 'skew', 7, 2, runs=runs).run()
    same_bits(whole, planes(small), runs_a=np.arange(runs))
    small.release()


def test_run_list_in_shuffled_order(ctx, big):
    import ginsim
    d, whole = big
    ids = np.random.default_rng(3).permutation(129)[:70]
    part = d.job(ctx, 'skew', 7, 2)
    ctx.sync()
    ginsim._lib.check(ginsim.lib.ginsim_memset(ctx.handle, part.buffer('series').ptr, 0, part.buffer('series').nbytes))
    part.run(ids)
    got = planes(part)
    rest = np.setdiff1d(np.arange(129), ids)
    for k in ('traj', 'wb', 'ab'):
        assert np.array_equal(got[k][..., ids].view(np.uint64), whole[k][..., ids].view(np.uint64)), k
        assert not got[k][..., rest].any(), k               # the other runs' columns were not touched
    assert np.array_equal(got['pdiag'][..., ids].view(np.uint64), whole['pdiag'][..., ids].view(np.uint64))
    part.release()


# ------------------------------------------------------------------------------------------------- 5. statistics only, vibration
def test_online_process_statistics_equal_those_of_the_kept_planes(ctx, dump):
    ned = dump.rf == 0
    job = dump.job(ctx, 'skew', 0, 2, proc_first=100, proc_ned=ned, end_ned=ned).run()
    assert job.kernel_name() == 'ginsim::loose_mag_kernel<%d, false, false, true>' % dump.rf
    online, kept = job.process_stats_online(), job.process_stats(first_sample=100, pos_ned=ned)
    np.testing.assert_allclose(online, kept, rtol=1e-7, atol=1e-12)
    plain = dump.job(ctx, 'skew', 0, 2).run()               # and the statistics variant computes what the plain one does
    same_bits(planes(plain), planes(job))
    only = dump.job(ctx, 'skew', 0, 2, proc_first=100, proc_ned=ned, end_ned=ned, keep_traj=False).run()     # nothing kept at all
    assert only.kernel_name() == job.kernel_name()
    assert np.array_equal(only.end_errors().view(np.uint64), plain.end_errors().view(np.uint64))
    assert np.array_equal(only.process_stats_online().view(np.uint64), online.view(np.uint64))
    for j in (plain, job, only):
        j.release()


def test_vibration_instantiations_launch_under_their_names(ctx, dump):
    vib = {'type': 'random', 'x': 0.05, 'y': 0.05, 'z': 0.05}
    kept = dump.job(ctx, 'skew', 0, 2, vib_accel=vib).run()
    assert kept.kernel_name() == 'ginsim::loose_mag_kernel<%d, false, true, false>' % dump.rf
    stat = dump.job(ctx, 'skew', 0, 2, vib_accel=vib, proc_first=0, keep_traj=False).run()
    assert stat.kernel_name() == 'ginsim::loose_mag_kernel<%d, false, true, true>' % dump.rf
    assert np.array_equal(kept.end_errors().view(np.uint64), stat.end_errors().view(np.uint64))
    assert np.all(np.isfinite(kept.end_errors()))
    calm = dump.job(ctx, 'skew', 0, 2).run()
    assert not np.array_equal(calm.end_errors(), kept.end_errors())            # the vibration term is in the samples
    for j in (kept, stat, calm):
        j.release()


# ------------------------------------------------------------------------------------------------- 6. consistency
@pytest.fixture(scope='module')
def drawn(ctx):
    """The 1024 runs tests/test_ins_loose_mag_oracle.py draws from the filter's own model, on the device."""
    fs, R = cs.CONSISTENCY_FS, cs.CONSISTENCY_RUNS
    ini, truth, stamps = mc.outage_truth(fs, 1, cs.CONSISTENCY_FS_GPS)
    acc_e, gyr_e = cs.imu_errors()
    rng = np.random.default_rng(cs.CONSISTENCY_SEED)
    accel, gyro, tba, tbg = ref.sample_sensors(rng, fs, truth['ref_accel'], truth['ref_gyro'], acc_e, gyr_e, R)
    gps = cs.sample_gps(rng, truth, 1, R)
    odo = ref.sample_odo(rng, truth['ref_odo'], ac.ODO_ERR, R)
    mag = ref.sample_mag(rng, truth['ref_mag'], mc.MAG_ERR, R)
    bufs = {'accel': ctx.upload(np.ascontiguousarray(accel.transpose(2, 1, 0))), 'gyro': ctx.upload(np.ascontiguousarray(gyro.transpose(2, 1, 0))),
            'gps': ctx.upload(np.ascontiguousarray(gps.transpose(2, 1, 0))), 'odo': ctx.upload(np.ascontiguousarray(odo.T)),
            'mag': ctx.upload(np.ascontiguousarray(mag.transpose(2, 1, 0)))}
    yield ini, truth, acc_e, gyr_e, tba, tbg, bufs
    for b in bufs.values():
        b.free()


@pytest.mark.parametrize('mask', [0, 7])
def test_consistency_of_the_covariance(ctx, drawn, mask):
    """For every state the RMS end error over sqrt(mean pdiag_end) is the ratio the restatement gave on the same draws
    (ins_loose_mag_cases.CONSISTENCY_RATIOS), to the 2e-3 the CPU test holds the restatement to."""
    import ginsim
    ini, truth, acc_e, gyr_e, tba, tbg, bufs = drawn
    fs, R = cs.CONSISTENCY_FS, cs.CONSISTENCY_RUNS
    kw = dict(odo_err=ac.ODO_ERR, aid=ac.aid_options(mask)) if mask else {}
    job = ginsim.InsLooseJob(ctx, fs, 1, truth, acc_e, gyr_e, cs.GPS_ERR, ini, R, given=bufs, keep_traj=True, mag_err=mc.MAG_ERR,
                             geo_mag_n=mc.GEO, mag={}, **kw).run()
    assert job.n == 1200
    last, ids = job.n - 1, np.arange(R)
    att, pos, vel = (job.series(k, ids)[:, last] for k in ('att', 'pos', 'vel'))
    wb, ab = job.final_biases()
    e = ref.error_state(1, att, pos, vel, wb, ab, truth['ref_att'][-1], truth['ref_pos'][-1], truth['ref_vel'][-1], tbg[:, -1], tba[:, -1])
    ratio = np.sqrt(np.mean(e * e, axis=0)) / np.sqrt(np.mean(job.final_pdiag(), axis=0))
    job.release()
    want = np.array(mc.CONSISTENCY_RATIOS[mask])
    print('magnetometer, mask %d: consistency ratios on the device:' % mask, np.array2string(ratio, precision=3))
    assert np.all(want <= 1.4) and (mask != 0 or np.all(want >= 0.7))
    np.testing.assert_allclose(ratio, want, rtol=0, atol=2e-3)


# ------------------------------------------------------------------------------------------------- 7. through Sim
def test_sim_runs_the_magnetometer_aided_and_the_unaided_filter_on_one_realisation(ctx):
    """IMU(axis=9, gps=True) with [FreeIntegration, InsLoose(), InsLoose(mag=True)]: the three share the sensors -- InsLoose() is the
    same bits as in a Sim without the third plugin, and the Sim's kept magnetometer series of a run, through the restatement, gives
    that run of the aided plugin; the aided filter's yaw 1 sigma at the end is below the unaided one's; consistency_curve names the
    aided plugin and raises; a statistics-only Sim reports the same statistics."""
    from demo_algorithms import free_integration
    from demo_algorithms.ins_loose_device import InsLoose
    from ginsim import filter_model, mag_model, workloads
    from gnss_ins_sim.sim import imu_model, ins_sim
    fs, fs_gps, rf = 100.0, 10.0, 1
    ini = workloads.parse_motion(cs.OUTAGE_CSV)[0]

    def make(algos, keep=True):
        imu = imu_model.IMU(accuracy='mid-accuracy', axis=9, gps=True)
        sim = ins_sim.Sim([fs, fs_gps, fs], cs.OUTAGE_CSV, ref_frame=rf, imu=imu, seed=1234, keep_trajectories=keep, geo_mag_n=list(mc.GEO),
                          algorithm=algos)
        sim.run(257)
        return sim, imu
    sim, imu = make([free_integration.FreeIntegration(ini), InsLoose(), InsLoose(mag=True)])
    d, res = sim.dmgr, sim.mc
    free, plain, aided = res.nav_names
    assert list(res.loose_names) == [plain, aided]
    (_, job0, kept0), (_, job1, kept1) = sim.loose_jobs
    assert job1 is kept1
    assert job0.kernel_name() == 'ginsim::loose_kernel<1, false, false, false>' and job0.mag is None
    assert job1.kernel_name() == 'ginsim::loose_mag_kernel<1, false, false, false>'
    want = mag_model(imu.mag_err, mc.GEO, rf, {})
    assert sorted(job1.mag) == sorted(want) and all(np.array_equal(job1.mag[k], want[k]) for k in want)
    # the unaided plugin does not see the third one
    two, _ = make([free_integration.FreeIntegration(ini), InsLoose()])
    (_, _, kept_two), = two.loose_jobs
    same_bits(planes(kept0), planes(kept_two))
    # one realisation: the Sim's own kept series of two runs through the restatement
    runs = [3, 65]
    accel, gyro, gps, mag = (np.stack([np.asarray(src.data[r]) for r in runs]) for src in (d.accel, d.gyro, d.gps, d.mag))
    stamps = np.rint(np.asarray(d.gps_time.data) * fs).astype(np.int64)
    vis = np.asarray(d.gps_visibility.data)
    model = filter_model(fs, imu.accel_err, imu.gyro_err, imu.gps_err)
    args = (rf, fs, gyro, accel, ini, model, gps, stamps, vis)
    exp = ref.run(*args, mag=mag, mag_model=job1.mag)
    bound = cs.parity_bound(*args, odo=None, aid=None, mag=mag, mag_model=job1.mag)
    got = {k: np.stack([np.asarray(src.data['%s_%d' % (aided, r)]) for r in runs])
           for k, src in (('att', d.att_euler), ('pos', d.pos), ('vel', d.vel), ('wb', d.wb), ('ab', d.ab))}
    got['pdiag_end'] = job1.final_pdiag()[runs]
    held('Sim pairing', cs.deviation(got, exp), bound)
    # the benefit: yaw at the end, and the curve along the outage
    samples = np.array(ac.outage_samples({'gps_visibility': vis, 'ref_accel': accel[0]}, stamps, fs, fs_gps))
    curve = sim.error_curve(('att_euler', 'pos'), samples=samples)
    yaw = {nm: np.deg2rad(curve['att_euler']['std'][nm][:, 0]) for nm in (free, plain, aided)}
    hor = {nm: np.linalg.norm(curve['pos']['std'][nm][:, 0:2], axis=1) for nm in (free, plain, aided)}
    print('yaw 1 sigma [rad] at outage start / end / +5 s / profile end: ' + ', '.join('%s %s' % (nm, np.array2string(v, precision=3)) for nm, v in yaw.items()))
    print('horizontal 1 sigma [m] at the same instants: ' + ', '.join('%s %s' % (nm, np.array2string(v, precision=3)) for nm, v in hor.items()))
    assert yaw[aided][3] < yaw[plain][3], (yaw[aided][3], yaw[plain][3])
    with pytest.raises(NotImplementedError, match=aided):
        sim.consistency_curve(every=5.0)
    # statistics only: the same numbers in results()
    sim.results(err_stats_start=-1)
    lean, _ = make([free_integration.FreeIntegration(ini), InsLoose(), InsLoose(mag=True)], keep=False)
    (_, lean1, _) = lean.loose_jobs[1]
    assert not lean1.keep_traj and lean1.kernel_name().startswith('ginsim::loose_mag_kernel<1, false, false, ')
    lean.results(err_stats_start=-1)
    for name in ('att_euler', 'pos', 'vel'):
        for key in ('std', 'max', 'avg'):
            for nm in (plain, aided):
                np.testing.assert_allclose(np.asarray(lean.err_stats[name][key][nm]), np.asarray(sim.err_stats[name][key][nm]), rtol=1e-9, atol=1e-12)
