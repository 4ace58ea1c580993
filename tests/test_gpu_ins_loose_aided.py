"""GPU: InsLoose aided by the odometer and the non-holonomic constraints (csrc/ins_loose_aided.hip, InsLooseJob(aid=...),
InsLoose(odo=..., nhc=...), the 'loose' role of Sim) against its NumPy restatement (tests/ins_loose_ref.py), against the
unaided launch, and against the statistics of its own covariance.  Shapes: 1-257 runs x 100-700 samples (1024 x 1200 for the
consistency, 257 x 6000 through Sim).  Every test passes an argument the unaided package does not have.

Parity bound, as tests/test_gpu_ins_loose.py: not a recorded constant.  Every comparison with the restatement measures, on its own
case (the device's dumped sensors, fixes and odometer, the first 8 runs), the float64 aided restatement against its np.longdouble
evaluation (ins_loose_cases.restatement_error) and allows the device ins_loose_cases.PARITY_MARGIN (16) x that.
Measured on the MI355X over the twelve parity cases (700 samples, 65 runs): device against restatement att <= 4.8e-14, pos <= 6.8e-14,
vel <= 1.6e-13, wb <= 4.3e-12, ab <= 1.1e-11, pdiag_end <= 1.2e-13; the smallest bounds att 3.1e-13, pos 5.2e-14, vel 6.3e-12,
wb 3.3e-10, ab 5.3e-10, pdiag_end 4.4e-13.  Consistency ratios on the device: the restatement's to three digits for both masks.
Through Sim (257 runs, 100 Hz, ref_frame 1), horizontal 1 sigma at the outage's start / end / 5 s later / the profile's end:
FreeIntegration 0.392 / 2.351 / 3.207 / 6.906 m, InsLoose() 0.081 / 0.961 / 0.305 / 0.267 m, InsLoose(odo=True, nhc=True)
0.047 / 0.140 / 0.132 / 0.130 m."""
import numpy as np
import pytest

import ins_loose_aided_cases as ac
import ins_loose_cases as cs
import ins_loose_dump
import ins_loose_ref as ref
from ins_loose_dump import ctx, held, planes, result, same_bits

pytestmark = pytest.mark.gpu


class Dump(ins_loose_dump.Dump):
    def job(self, ctx, mask, every=1, given=False, **kw):
        """mask 0: the unaided job (no aiding argument at all)."""
        return super().job(ctx, given, **ac.aid_kw(mask, every, **kw))

    def restate(self, mask, every=1):
        return ref.run(*self._args(), odo=self.odo, aid=ac.aid(mask, every))

    def bound(self, mask, every=1):
        """16 x the aided restatement's own float64 error on this case (its first 8 runs)."""
        return cs.parity_bound(*self._args(), odo=self.odo, aid=ac.aid(mask, every))


def held_to_the_restatement(ctx, d, mask, every, what):
    job = d.job(ctx, mask, every, given=True).run()
    assert job.kernel_name() == 'ginsim::loose_aided_kernel<%d, true, false, false>' % d.rf
    dev = result(job)
    job.release()
    held('%s rf%d mask %d every %d' % (what, d.rf, mask, every), cs.deviation(dev, d.restate(mask, every)), d.bound(mask, every))
    return dev


@pytest.fixture(scope='module', params=[0, 1], ids=['rf0', 'rf1'])
def dump(request, ctx):
    d = Dump(ctx, request.param, 700, 65)                   # 35 s at 20 Hz: 15 s into the outage
    yield d
    d.release()


# ------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize('every', [1, 7])
@pytest.mark.parametrize('mask', [1, 6, 7])
def test_parity_with_the_restatement(ctx, dump, mask, every):
    assert np.any(dump.truth['gps_visibility'] == 0)                           # the outage's start is inside the cut
    dev = held_to_the_restatement(ctx, dump, mask, every, 'parity')
    plain = dump.job(ctx, 0, given=True).run()
    assert not np.array_equal(result(plain)['vel'], dev['vel'])                # the block did something
    plain.release()


# ------------------------------------------------------------------------------------------------- 2. generated = given
@pytest.mark.parametrize('rf, run_offset, mask', [(0, 0, 7), (1, 2 ** 40, 7), (1, 0, 1)])
def test_generated_form_equals_given_form_bit_for_bit(ctx, rf, run_offset, mask):
    """The lane regenerates the odometer sample ginsim_mc_run stores for the same seed and run id (and accel, gyro and the fixes, as
    the unaided kernel does): every output is the same bits, also with a run offset beyond 32 bits."""
    d = Dump(ctx, rf, 300, 65, seed=41, run_offset=run_offset, fs=100.0, fs_gps=10.0)
    gen, giv = d.job(ctx, mask, 3).run(), d.job(ctx, mask, 3, given=True).run()
    assert (gen.variant(), giv.variant()) == (0, 1)
    assert gen.kernel_name() == 'ginsim::loose_aided_kernel<%d, false, false, false>' % rf
    whole = planes(gen)
    same_bits(whole, planes(giv))
    if run_offset:
        other = Dump(ctx, rf, 300, 65, seed=41, fs=100.0, fs_gps=10.0)
        assert not np.array_equal(other.odo, d.odo)                            # the run id enters the odometer's counter
        other.release()
    gen.release()
    giv.release()
    d.release()


# ------------------------------------------------------------------------------------------------- 3. a block that never fires
@pytest.mark.parametrize('every', ['n', 2 ** 40])
def test_a_block_that_never_fires_is_the_unaided_launch(ctx, dump, every):
    every = dump.n if every == 'n' else every
    for given in (False, True):
        plain, aided = dump.job(ctx, 0, given=given).run(), dump.job(ctx, 7, every, given=given).run()
        assert plain.kernel_name().startswith('ginsim::loose_kernel<') and aided.kernel_name().startswith('ginsim::loose_aided_kernel<')
        same_bits(planes(plain), planes(aided))
        plain.release()
        aided.release()


# ------------------------------------------------------------------------------------------------- 4. scheduling edges
@pytest.mark.parametrize('case', ['fix_and_block_on_one_sample', 'block_on_the_last_sample', 'no_gps_at_all', 'stationary_start'])
def test_scheduling_edges(ctx, case):
    if case == 'fix_and_block_on_one_sample':               # fixes at 0, 10, 20, ...: every block falls on a fix
        d, every = Dump(ctx, 0, 300, 65, seed=31), 10
        assert np.all(d.stamps % every == 0) and d.stamps.size == 30
    elif case == 'block_on_the_last_sample':                # blocks at 150 and 300 = n - 1 (also a fix)
        d, every = Dump(ctx, 1, 301, 65, seed=32), 150
        assert d.stamps[-1] == d.n - 1
    elif case == 'no_gps_at_all':                           # m = 0: dead reckoning with a covariance
        d, every = Dump(ctx, 1, 300, 65, seed=33, gps=False), 1
        assert d.stamps.size == 0
    else:                                                   # the filter starts at rest: the psi part of every row (v x D[i,:]) is ~0
        d, every = Dump(ctx, 0, 100, 65, seed=34, vbx0=0.0), 1
        assert d.ini[3] == 0.0
    dev = held_to_the_restatement(ctx, d, 7, every, case)
    if case == 'no_gps_at_all':
        job = d.job(ctx, 7, every, given=True)
        assert job.m == 0
        job.release()
        free = d.job(ctx, 0, given=True).run()              # without aiding it is free integration: P only grows
        assert np.all(dev['pdiag_end'][:, 3:9] < free.final_pdiag()[:, 3:9])
        free.release()
    d.release()


# ------------------------------------------------------------------------------------------------- 5. run counts, run lists
@pytest.fixture(scope='module')
def big(ctx):
    d = Dump(ctx, 1, 200, 129, seed=21)
    job = d.job(ctx, 7, 2).run()
    yield d, planes(job)
    job.release()
    d.release()


@pytest.mark.parametrize('runs', [1, 63, 64, 65, 129])
def test_run_counts_around_a_wavefront(ctx, big, runs):
    """Run r of a small launch is run r of the 129-run launch with the same seed (one lane per run, no neighbour in it)."""
    import ginsim
    d, whole = big
    small = ginsim.InsLooseJob(ctx, d.fs, d.rf, d.truth, d.acc_e, d.gyr_e, cs.GPS_ERR, d.ini, runs, seed=d.seed, keep_traj=True,
                               odo_err=ac.ODO_ERR, aid=ac.aid_options(7, 2)).run()
    same_bits(whole, planes(small), runs_a=np.arange(runs))
    small.release()


def test_run_list_in_shuffled_order(ctx, big):
    import ginsim
    d, whole = big
    ids = np.random.default_rng(3).permutation(129)[:70]
    part = d.job(ctx, 7, 2)
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


# ------------------------------------------------------------------------------------------------- 6. non-finite odometer
@pytest.mark.parametrize('value', [np.inf, np.nan])
def test_a_non_finite_odometer_sample_stays_in_its_run(ctx, dump, value):
    clean = dump.job(ctx, 7, given=True).run()
    want = planes(clean)
    clean.release()
    odo = ctx.download(dump.mc.buffer('odo'), (dump.n, 65))
    odo[100, 33] = value
    bad = ctx.upload(odo)
    job = dump.job(ctx, 7, given=dict(dump.given, odo=bad)).run()
    got = planes(job)
    job.release()
    bad.free()
    keep = np.setdiff1d(np.arange(65), [33])
    same_bits(got, want, runs_a=keep, runs_b=keep)
    assert not np.any(np.isfinite(got['traj'][3:9, -1, 33]))                   # position and velocity of the last row
    assert not np.all(np.isfinite(got['end'][:, 33])) and not np.all(np.isfinite(got['pdiag'][:, 33]))
    assert np.array_equal(got['traj'][:, :100, 33], want['traj'][:, :100, 33])  # rows before the block of sample 100


# ------------------------------------------------------------------------------------------------- 7. online statistics
def test_online_process_statistics_equal_those_of_the_kept_planes(ctx, dump):
    ned = dump.rf == 0
    job = dump.job(ctx, 7, 2, proc_first=100, proc_ned=ned, end_ned=ned).run()
    assert job.kernel_name() == 'ginsim::loose_aided_kernel<%d, false, false, true>' % dump.rf
    online, kept = job.process_stats_online(), job.process_stats(first_sample=100, pos_ned=ned)
    np.testing.assert_allclose(online, kept, rtol=1e-7, atol=1e-12)
    st, ft = job.stats(ned=ned), job.stats_from_traj(pos_ned=ned)
    # the NED position error is a rotated difference of two ECEF vectors of 6.4e6 m: 4e-9 m absolute (tests/test_gpu_ins_loose.py)
    atol = np.array([1e-13] * 3 + [4e-9 if ned else 1e-13] * 3 + [1e-13] * 3)
    assert np.all(np.abs(st.std - ft.std) <= 1e-9 * np.abs(ft.std) + atol)
    assert np.all(np.abs(st.maxabs - ft.maxabs) <= 1e-9 * np.abs(ft.maxabs) + atol)
    plain = dump.job(ctx, 7, 2).run()                       # and the statistics variant computes what the plain one does
    same_bits(planes(plain), planes(job))
    plain.release()
    job.release()


# ------------------------------------------------------------------------------------------------- 8. consistency
@pytest.fixture(scope='module')
def drawn(ctx):
    """The 1024 runs tests/test_ins_loose_aided_oracle.py draws from the filter's own model, on the device."""
    fs, R = cs.CONSISTENCY_FS, cs.CONSISTENCY_RUNS
    ini, truth, stamps = ac.outage_truth(fs, 1, cs.CONSISTENCY_FS_GPS)
    acc_e, gyr_e = cs.imu_errors()
    rng = np.random.default_rng(cs.CONSISTENCY_SEED)
    accel, gyro, tba, tbg = ref.sample_sensors(rng, fs, truth['ref_accel'], truth['ref_gyro'], acc_e, gyr_e, R)
    gps = cs.sample_gps(rng, truth, 1, R)
    odo = ref.sample_odo(rng, truth['ref_odo'], ac.ODO_ERR, R)
    bufs = {'accel': ctx.upload(np.ascontiguousarray(accel.transpose(2, 1, 0))), 'gyro': ctx.upload(np.ascontiguousarray(gyro.transpose(2, 1, 0))),
            'gps': ctx.upload(np.ascontiguousarray(gps.transpose(2, 1, 0))), 'odo': ctx.upload(np.ascontiguousarray(odo.T))}
    yield ini, truth, acc_e, gyr_e, tba, tbg, bufs
    for b in bufs.values():
        b.free()


@pytest.mark.parametrize('mask', [1, 7])
def test_consistency_of_the_covariance(ctx, drawn, mask):
    """For every state the RMS end error over sqrt(mean pdiag_end) lies within x/: 1.25 of the ratio the restatement gave on the same
    draws (ins_loose_aided_cases.CONSISTENCY_RATIOS; the factor of tests/test_gpu_ins_loose.py)."""
    import ginsim
    ini, truth, acc_e, gyr_e, tba, tbg, bufs = drawn
    fs, R = cs.CONSISTENCY_FS, cs.CONSISTENCY_RUNS
    job = ginsim.InsLooseJob(ctx, fs, 1, truth, acc_e, gyr_e, cs.GPS_ERR, ini, R, given=bufs, keep_traj=True, odo_err=ac.ODO_ERR,
                             aid=ac.aid_options(mask)).run()
    last, ids = job.n - 1, np.arange(R)
    att, pos, vel = (job.series(k, ids)[:, last] for k in ('att', 'pos', 'vel'))
    wb, ab = job.final_biases()
    e = ref.error_state(1, att, pos, vel, wb, ab, truth['ref_att'][-1], truth['ref_pos'][-1], truth['ref_vel'][-1], tbg[:, -1], tba[:, -1])
    ratio = np.sqrt(np.mean(e * e, axis=0)) / np.sqrt(np.mean(job.final_pdiag(), axis=0))
    job.release()
    want = np.array(ac.CONSISTENCY_RATIOS[mask])
    print('mask %d consistency ratios on the device:' % mask, np.array2string(ratio, precision=3))
    assert np.all(want <= 1.4) and (mask != 1 or np.all(want >= 0.7))
    assert np.all(ratio <= want * 1.25) and np.all(ratio >= want / 1.25), ratio / want


# ------------------------------------------------------------------------------------------------- 9. through Sim
def test_sim_runs_the_aided_and_the_unaided_filter_on_one_realisation(ctx):
    """IMU(gps=True, odo=True) with [FreeIntegration, InsLoose(), InsLoose(odo=True, nhc=True)]: the aided plugin's summary
    statistics are its job's, its curve is drawn, and at the outage's last sample its horizontal 1 sigma is below half the unaided
    plugin's.  Both filters and the free integration see one sensor realisation per run: the Sim's kept accel / gyro / fixes /
    odometer of a run, fed to the restatement, give that run of the aided plugin."""
    from demo_algorithms import free_integration
    from demo_algorithms.ins_loose_device import InsLoose
    from ginsim import aiding_model, filter_model, workloads
    from gnss_ins_sim.sim import imu_model, ins_sim
    fs, fs_gps, rf = 100.0, 10.0, 1
    ini = workloads.parse_motion(cs.OUTAGE_CSV)[0]
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=True, odo=True)
    sim = ins_sim.Sim([fs, fs_gps, 0.0], cs.OUTAGE_CSV, ref_frame=rf, imu=imu, seed=1234, keep_trajectories=True,
                      algorithm=[free_integration.FreeIntegration(ini), InsLoose(), InsLoose(odo=True, nhc=True)])
    sim.run(257)
    d, mc = sim.dmgr, sim.mc
    free, plain, aided = mc.nav_names
    assert list(mc.loose_names) == [plain, aided]
    (_, job0, _), (_, job1, kept1) = sim.loose_jobs
    assert job1 is kept1
    assert job0.kernel_name() == 'ginsim::loose_kernel<1, false, false, false>' and job0.aid['aid_mask'] == 0
    assert job1.kernel_name() == 'ginsim::loose_aided_kernel<1, false, false, false>'
    assert job1.aid == aiding_model(imu.odo_err, {'odo': True, 'nhc': True})
    # the summary's end-point statistics are the job's
    sim.results(err_stats_start=-1)
    st = job1.stats()
    for name, sl, scale in (('att_euler', slice(0, 3), 180.0 / np.pi), ('pos', slice(3, 6), 1.0), ('vel', slice(6, 9), 1.0)):
        for key, want in (('std', st.std), ('max', st.maxabs), ('avg', st.mean)):
            np.testing.assert_allclose(np.asarray(sim.err_stats[name][key][aided]), want[sl] * scale, rtol=1e-9, atol=1e-12)
    # one realisation: the Sim's own kept series of two runs through the restatement
    runs = [3, 65]
    accel, gyro, gps, odo = (np.stack([np.asarray(src.data[r]) for r in runs]) for src in (d.accel, d.gyro, d.gps, d.odo))
    odo = odo.reshape(len(runs), -1)
    stamps = np.rint(np.asarray(d.gps_time.data) * fs).astype(np.int64)
    vis = np.asarray(d.gps_visibility.data)
    model = filter_model(fs, imu.accel_err, imu.gyro_err, imu.gps_err)
    args = (rf, fs, gyro, accel, ini, model, gps, stamps, vis)
    exp = ref.run(*args, odo=odo, aid=job1.aid)
    bound = cs.parity_bound(*args, odo=odo, aid=job1.aid)
    got = {k: np.stack([np.asarray(src.data['%s_%d' % (aided, r)]) for r in runs])
           for k, src in (('att', d.att_euler), ('pos', d.pos), ('vel', d.vel), ('wb', d.wb), ('ab', d.ab))}
    got['pdiag_end'] = job1.final_pdiag()[runs]
    held('Sim pairing', cs.deviation(got, exp), bound)
    # the curve, and the benefit at the outage's last sample
    samples = np.array(ac.outage_samples({'gps_visibility': vis, 'ref_accel': accel[0]}, stamps, fs, fs_gps))
    curve = sim.error_curve(('pos',), samples=samples)
    direct = job1.error_curve(samples=samples)
    np.testing.assert_array_equal(curve['pos']['std'][aided], direct.std[:, 3:6])
    h = {nm: np.linalg.norm(curve['pos']['std'][nm][:, 0:2], axis=1) for nm in (free, plain, aided)}
    print('horizontal 1 sigma [m] at outage start / end / +5 s / profile end: ' +
          ', '.join('%s %s' % (nm, np.array2string(v, precision=3)) for nm, v in h.items()))
    assert h[aided][1] < 0.5 * h[plain][1], (h[aided][1], h[plain][1])


# ------------------------------------------------------------------------------------------------- 10. the plugin on one series
def test_plugin_run_on_one_logged_series(ctx):
    from demo_algorithms.ins_loose_device import InsLoose
    from gnss_ins_sim.sim import imu_model
    d = Dump(ctx, 1, 600, 1, seed=71)
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=True, odo=True)
    imu.gps_err, imu.odo_err = dict(cs.GPS_ERR), dict(ac.ODO_ERR)
    algo = InsLoose(ini_pos_vel_att=d.ini, ref_frame=1, imu=imu, odo=True, nhc=True, odo_every=3)
    assert algo.input[-1] == 'odo'
    gps7 = np.concatenate([d.gps[0], d.truth['gps_visibility'][:, None]], axis=1)
    series = [d.fs, d.gyro[0], d.accel[0], np.arange(d.n) / d.fs, d.truth['gps_time'], gps7, d.odo[0]]
    with pytest.raises(ValueError, match='seventh'):
        algo.run(series[:6])
    algo.run(series)
    pos, vel, att, wb, ab = algo.get_results()
    job = d.job(ctx, 7, 3, given=True).run()
    want = result(job)
    job.release()
    for k, v in (('pos', pos), ('vel', vel), ('att', att), ('wb', wb), ('ab', ab)):
        assert np.array_equal(v, want[k][0]), k
    d.release()
