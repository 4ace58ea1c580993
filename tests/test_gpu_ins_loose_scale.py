"""GPU: InsLoose with the odometer's scale factor as a 16th state (csrc/ins_loose_scale.hip, InsLooseJob(odo_scale_state=...),
InsLoose(odo_scale_state=True), the 'loose' role of Sim) against its NumPy restatement (tests/ins_loose_scale_ref.py), against the
15-state aided launch in the degenerate case and against the statistics of its own covariance.  Shapes: the outage profile at 20 Hz
(1200 samples) with 257, 64 and 1 runs; 1024 runs for the consistency; 65 runs through Sim.  Every test passes an argument
the package without the state does not have.

Parity bound, as tests/test_gpu_ins_loose_aided.py: not a recorded constant.  Every comparison with the restatement measures, on its
own case (the device's dumped sensors, fixes and odometer, the first 8 runs), the float64 restatement against its np.longdouble
evaluation (ins_loose_cases.restatement_error) and allows the device ins_loose_cases.PARITY_MARGIN (16) x that, per output:
att, pos, vel, wb, ab, pdiag_end, the k_est series, scale_end and pcross_end.

Measured on the MI355X (first run: all pass as written).  Largest deviation from the restatement over the eight 257-run parity
cases, with the smallest bound any of them allowed: att 6.3e-14 (4.9e-12), pos 7.8e-13 in ref_frame 0 (2.1e-10) and 3.4e-16 in
ref_frame 1 (9.0e-14), vel 7.1e-13 (7.1e-11), wb 2.2e-11 (5.8e-9), ab 2.5e-11 (7.5e-9), pdiag_end 1.1e-13 (6.9e-12), k_est 3.0e-13
(3.1e-11), scale_end 2.9e-13 (3.1e-11), pcross_end 8.2e-14 (1.3e-11).  The degenerate launch is loose_aided_kernel's bit for bit in
all four cases.  The consistency ratios on the device are the restatement's to the three recorded digits."""
import numpy as np
import pytest

import ins_loose_aided_cases as ac
import ins_loose_cases as cs
import ins_loose_dump
import ins_loose_ref as ref
import ins_loose_scale_cases as sc
import ins_loose_scale_ref as sref
from ins_loose_dump import ctx, held, planes, result, same_bits

pytestmark = pytest.mark.gpu

FS, FS_GPS, N, RUNS = 20.0, 2.0, 1200, 257
ODO_ERR = {'scale': 0.985, 'stdv': sc.ODO_STDV}        # what the odometer of the dumps reads; the filter starts from 1.0


class Dump(ins_loose_dump.Dump):
    """The odometer of the dump reads ODO_ERR's scale."""

    def __init__(self, ctx, rf, n, runs, seed=77, vib=None):
        super().__init__(ctx, rf, n, runs, seed, fs=FS, fs_gps=FS_GPS, odo_err=ODO_ERR, vib=vib)
        self._restated = {}

    def job(self, ctx, mask, every=1, given=False, state=None, runs=None, **kw):
        """state: the options of the scale-factor state ({}: the defaults); None: the 15-state aided job."""
        kw = dict(dict(keep_traj=True, odo_err=ODO_ERR, aid=ac.aid_options(mask, every)), **kw)
        if state is not None:
            kw = dict(dict(odo_scale_state=state, keep_scale=kw['keep_traj']), **kw)
        return super().job(ctx, given, runs=runs, **kw)

    def restate(self, mask, every=1, scale0=sc.SCALE0, p0=sc.P0_SCALE):
        """The restatement of all runs and 16 x its own float64 error on the first 8, once per case."""
        key = (mask, every, scale0, p0)
        if key not in self._restated:
            kw = dict(odo=self.odo, aid=sc.aid(mask, every, scale0))
            out = sref.run(*self._args(), scale=sc.scale(scale0, p0), **kw)
            bound = cs.parity_bound(*self._args(), run=sref.run, deviation=sc.deviation, odo=self.odo, aid=kw['aid'], scale=sc.scale(scale0, p0))
            for v in out.values():
                v.setflags(write=False)
            self._restated[key] = (out, bound)
        return self._restated[key]


@pytest.fixture(scope='module')
def dumps(ctx):
    made = {}

    def get(rf):
        if rf not in made:
            made[rf] = Dump(ctx, rf, N, RUNS)
        return made[rf]
    yield get
    for d in made.values():
        d.release()


# ------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize('every', [1, 10])
@pytest.mark.parametrize('mask', [1, 7])
@pytest.mark.parametrize('rf', [0, 1])
def test_parity_with_the_restatement(ctx, dumps, rf, mask, every):
    d = dumps(rf)
    assert d.n == 1200 and d.runs == 257 and np.any(d.truth['gps_visibility'] == 0)
    job = d.job(ctx, mask, every, given=True, state={}).run()
    assert job.kernel_name() == 'ginsim::loose_scale_kernel<%d, true, false, false>' % rf
    dev = result(job)
    job.release()
    exp, bound = d.restate(mask, every)
    assert set(bound) == set(sc.PARITY_KEYS)
    held('parity rf%d mask %d every %d' % (rf, mask, every), sc.deviation(dev, exp), bound)
    assert np.all(np.abs(dev['k_est'][:, -1] - ODO_ERR['scale']) < np.abs(sc.SCALE0 - ODO_ERR['scale']))       # it was learnt
    assert np.all(dev['scale_end'][:, 1] < sc.P0_SCALE ** 2)


@pytest.mark.parametrize('rf, runs', [(0, 1), (1, 1), (0, 64), (1, 64)])
def test_one_run_and_one_full_wavefront(ctx, dumps, rf, runs):
    """Run r of a small generated launch is run r of the 257-run case (the same seed): held to the same restatement, mask 7."""
    d = dumps(rf)
    job = d.job(ctx, 7, 1, state={}, runs=runs).run()
    assert job.kernel_name() == 'ginsim::loose_scale_kernel<%d, false, false, false>' % rf
    dev = result(job)
    job.release()
    exp, bound = d.restate(7, 1)
    held('rf%d %d runs' % (rf, runs), sc.deviation(dev, {k: v[:runs] for k, v in exp.items()}), bound)


# ------------------------------------------------------------------------------------------------- 2. generated = given
@pytest.mark.parametrize('rf', [0, 1])
def test_generated_form_equals_given_form_bit_for_bit(ctx, dumps, rf):
    """The lane regenerates the odometer sample ginsim_mc_run stores (MonteCarloJob(keep_sensors)) and accel, gyro and the fixes."""
    d = dumps(rf)
    gen, giv = d.job(ctx, 7, 3, state={}).run(), d.job(ctx, 7, 3, given=True, state={}).run()
    assert (gen.variant(), giv.variant()) == (0, 1)
    a, b = planes(gen), planes(giv)
    assert {'scale', 'scale_end', 'pcross'} <= set(a)
    same_bits(a, b)
    assert np.ptp(a['scale'][-1]) > 0 and np.all(a['scale'][0] == sc.SCALE0)
    gen.release()
    giv.release()


# ------------------------------------------------------------------------------------------------- 3. the degenerate case
@pytest.mark.parametrize('mask', [1, 7])
@pytest.mark.parametrize('rf', [0, 1])
def test_p0_zero_is_the_aided_kernel_with_the_same_scale(ctx, dumps, rf, mask):
    """p0 = 0, q = 0, scale0 = s against loose_aided_kernel told s, within the bound of the degenerate case's own restatement.
    Whether the two launches agree bit for bit is printed; on the MI355X they do, in every output of the four cases (the seventh
    product of a row is a fused multiply-add of zero)."""
    d, s = dumps(rf), 0.99
    deg = d.job(ctx, mask, 1, given=True, state={'scale0': s, 'p0': 0.0, 'q': 0.0}).run()
    aided = d.job(ctx, mask, 1, given=True, aid=ac.aid_options(mask, 1, scale=s, odo_std=sc.ODO_STDV / s)).run()
    assert deg.kernel_name().startswith('ginsim::loose_scale_kernel<') and aided.kernel_name().startswith('ginsim::loose_aided_kernel<')
    assert deg.aid['r_odo'] == aided.aid['r_odo']
    a, b = result(deg), result(aided)
    pa, pb = planes(deg), planes(aided)
    deg.release()
    aided.release()
    assert np.all(a['k_est'] == s) and np.all(a['scale_end'] == [s, 0.0]) and not a['pcross_end'].any()
    bits = all(np.array_equal(pa[k].view(np.uint64), pb[k].view(np.uint64)) for k in pb)
    print('degenerate rf%d mask %d: bit for bit with loose_aided_kernel: %s' % (rf, mask, bits))
    _, bound = d.restate(mask, 1, scale0=s, p0=0.0)
    held('degenerate rf%d mask %d' % (rf, mask), cs.deviation(a, b), {k: bound[k] for k in cs.PARITY_KEYS})


# ------------------------------------------------------------------------------------------------- 4. run_list
def test_run_list_subset(ctx, dumps):
    import ginsim
    d = dumps(1)
    whole_job = d.job(ctx, 7, 2, state={}).run()
    whole = planes(whole_job)
    whole_job.release()
    ids = np.random.default_rng(3).permutation(d.runs)[:70]
    part = d.job(ctx, 7, 2, state={})
    ctx.sync()
    for buf in (part.buffer('series'), part.buffer('scale')):
        ginsim._lib.check(ginsim.lib.ginsim_memset(ctx.handle, buf.ptr, 0, buf.nbytes))
    part.run(ids)
    got = planes(part)
    part.release()
    rest = np.setdiff1d(np.arange(d.runs), ids)
    same_bits(got, whole, ids, ids, keys=('traj', 'wb', 'ab', 'pdiag', 'scale', 'scale_end', 'pcross'))
    for k in ('traj', 'wb', 'ab', 'scale', 'scale_end', 'pcross'):
        assert not got[k][..., rest].any(), k               # the other runs keep what they held


# ------------------------------------------------------------------------------------------------- 5. online statistics
@pytest.mark.parametrize('rf', [0, 1])
def test_online_process_statistics_equal_those_of_the_kept_planes(ctx, dumps, rf):
    d, ned = dumps(rf), rf == 0
    job = d.job(ctx, 7, 2, state={}, proc_first=100, proc_ned=ned).run()
    assert job.kernel_name() == 'ginsim::loose_scale_kernel<%d, false, false, true>' % rf
    online, kept = job.process_stats_online(), job.process_stats(first_sample=100, pos_ned=ned)
    np.testing.assert_allclose(online, kept, rtol=1e-7, atol=1e-12)
    plain = d.job(ctx, 7, 2, state={}).run()                # and the statistics variant computes what the plain one does
    same_bits(planes(plain), planes(job))
    plain.release()
    job.release()


# ------------------------------------------------------------------------------------------------- 6. vibration
def test_vibration_variant_given_equals_generated(ctx):
    vib = {'type': 'random', 'x': 0.05, 'y': 0.05, 'z': 0.05}
    d = Dump(ctx, 1, 400, 65, seed=41, vib=vib)
    gen, giv = d.job(ctx, 7, 1, state={}).run(), d.job(ctx, 7, 1, given=True, state={}).run()
    assert gen.kernel_name() == 'ginsim::loose_scale_kernel<1, false, true, false>'
    assert giv.kernel_name() == 'ginsim::loose_scale_kernel<1, true, false, false>'
    same_bits(planes(gen), planes(giv))
    calm = Dump(ctx, 1, 400, 65, seed=41)
    assert not np.array_equal(calm.accel, d.accel)                             # the vibration term is in the samples
    for x in (gen, giv, calm, d):
        x.release()


# ------------------------------------------------------------------------------------------------- 7. consistency
def test_consistency_of_the_covariance(ctx):
    """The 1024 runs tests/test_ins_loose_scale_oracle.py draws, every run with a true scale of its own, given to the device: for
    every one of the 16 states the RMS end error over sqrt(mean P_kk) lies within x/: 1.25 of the restatement's recorded ratio."""
    import ginsim
    d = sc.draws(cs.CONSISTENCY_RUNS, cs.CONSISTENCY_SEED)
    R, odo = cs.CONSISTENCY_RUNS, sc.odometer(d)
    bufs = {'accel': ctx.upload(np.ascontiguousarray(d['accel'].transpose(2, 1, 0))), 'gyro': ctx.upload(np.ascontiguousarray(d['gyro'].transpose(2, 1, 0))),
            'gps': ctx.upload(np.ascontiguousarray(d['gps'].transpose(2, 1, 0))), 'odo': ctx.upload(np.ascontiguousarray(odo.T))}
    job = ginsim.InsLooseJob(ctx, d['fs'], 1, d['truth'], d['acc_e'], d['gyr_e'], cs.GPS_ERR, d['ini'], R, given=bufs, keep_traj=True,
                             odo_err={'scale': 1.0, 'stdv': sc.ODO_STDV}, aid=ac.aid_options(1), odo_scale_state={}).run()
    ids = np.arange(R)
    o = {k: job.series(k, ids) for k in ('att', 'pos', 'vel')}
    wb, ab = job.final_biases()
    o['wb'], o['ab'] = wb[:, None], ab[:, None]
    k_end, sigma = job.final_scale()
    o['pdiag_end'], o['scale_end'] = job.final_pdiag(), np.stack([k_end, sigma ** 2], axis=1)
    assert job.final_sigmas().shape == (R, 16)
    job.release()
    for b in bufs.values():
        b.free()
    ratio, want = sc.ratios16(d, o, d['scales']), np.array(sc.CONSISTENCY_RATIOS)
    print('consistency ratios on the device, 16 states:', np.array2string(ratio, precision=3))
    assert np.all(want >= sc.CONSISTENCY_BAND[0]) and np.all(want <= sc.CONSISTENCY_BAND[1])
    assert np.all(ratio <= want * 1.25) and np.all(ratio >= want / 1.25), ratio / want


# ------------------------------------------------------------------------------------------------- 8. through Sim
def test_sim_runs_both_filters_on_one_realisation_and_the_plugin_on_one_series(ctx):
    """IMU(gps=True, odo=True) with [InsLoose(odo, nhc), InsLoose(odo, nhc, odo_scale_state)], 65 runs: both plugins see one sensor
    realisation per run (the Sim's kept series of a run, through the two restatements, give that run of either plugin); the
    second plugin's published series are an InsLooseJob's of the same seed, bit for bit; its run() on one logged series gives
    the job's bits."""
    import ginsim
    from demo_algorithms.ins_loose_device import InsLoose
    from ginsim import filter_model, workloads
    from gnss_ins_sim.sim import imu_model, ins_sim
    fs, fs_gps, rf, R = FS, FS_GPS, 1, 65
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=True, odo=True)
    second = InsLoose(odo=True, nhc=True, odo_scale_state=True)
    sim = ins_sim.Sim([fs, fs_gps, 0.0], cs.OUTAGE_CSV, ref_frame=rf, imu=imu, seed=1234, keep_trajectories=True,
                      algorithm=[InsLoose(odo=True, nhc=True), second])
    sim.run(R)
    d, mc = sim.dmgr, sim.mc
    plain, state = mc.loose_names
    (_, job0, _), (_, job1, kept1) = sim.loose_jobs
    assert job1 is kept1
    assert job0.kernel_name() == 'ginsim::loose_aided_kernel<1, false, false, false>' and job0.scale is None
    assert job1.kernel_name() == 'ginsim::loose_scale_kernel<1, false, false, false>'
    assert job1.scale == {'scale0': 1.0, 'p0_scale': 0.02, 'q_k': 0.0}
    assert (job0.mc.seed, job0.mc.run_offset) == (job1.mc.seed, job1.mc.run_offset)
    with pytest.raises(NotImplementedError, match='odo_scale_state'):
        sim.consistency_curve(every=1.0)
    # one realisation: the Sim's own kept series of two runs through the two restatements
    runs = [3, 64]
    accel, gyro, gps, odo = (np.stack([np.asarray(src.data[r]) for r in runs]) for src in (d.accel, d.gyro, d.gps, d.odo))
    odo = odo.reshape(len(runs), -1)
    stamps = np.rint(np.asarray(d.gps_time.data) * fs).astype(np.int64)
    vis = np.asarray(d.gps_visibility.data)
    ini = sim_ini = workloads.parse_motion(cs.OUTAGE_CSV)[0]
    model = filter_model(fs, imu.accel_err, imu.gyro_err, imu.gps_err)
    args = (rf, fs, gyro, accel, ini, model, gps, stamps, vis)
    published = lambda name: {k: np.stack([np.asarray(src.data['%s_%d' % (name, r)]) for r in runs])
                              for k, src in (('att', d.att_euler), ('pos', d.pos), ('vel', d.vel), ('wb', d.wb), ('ab', d.ab))}
    got0 = dict(published(plain), pdiag_end=job0.final_pdiag()[runs])
    held('Sim, the 15-state plugin', cs.deviation(got0, ref.run(*args, odo=odo, aid=job0.aid)),
         cs.parity_bound(*args, odo=odo, aid=job0.aid))
    got1 = dict(published(state), pdiag_end=job1.final_pdiag()[runs], pcross_end=job1.final_pcross()[runs])
    got1['k_est'] = np.stack([np.asarray(d.odo_scale.data['%s_%d' % (state, r)]).reshape(-1) for r in runs])
    k_end, sigma = job1.final_scale()
    got1['scale_end'] = np.stack([k_end, sigma ** 2], axis=1)[runs]
    held('Sim, the 16-state plugin', sc.deviation(got1, sref.run(*args, odo=odo, aid=job1.aid, scale=job1.scale)),
         cs.parity_bound(*args, run=sref.run, deviation=sc.deviation, odo=odo, aid=job1.aid, scale=job1.scale))
    assert np.all(np.abs(k_end - imu.odo_err['scale']) < 4 * sigma + 1e-3)
    # the published series are an InsLooseJob's of the same seed
    t = {'ref_accel': np.asarray(d.ref_accel.data), 'ref_gyro': np.asarray(d.ref_gyro.data), 'ref_att': np.asarray(d.ref_att_euler.data),
         'ref_pos': np.asarray(d.ref_pos.data), 'ref_vel': np.asarray(d.ref_vel.data), 'ref_gps': np.asarray(d.ref_gps.data),
         'gps_time': np.asarray(d.gps_time.data), 'gps_visibility': vis, 'ref_odo': np.asarray(d.ref_odo.data).reshape(-1)}
    own = ginsim.InsLooseJob(ctx, fs, rf, t, imu.accel_err, imu.gyro_err, imu.gps_err, sim_ini, R, seed=job1.mc.seed,
                             run_offset=job1.mc.run_offset, keep_traj=True, odo_err=imu.odo_err, aid={'odo': True, 'nhc': True},
                             odo_scale_state={}, keep_scale=True).run()
    for k, src in (('att', d.att_euler), ('pos', d.pos), ('vel', d.vel), ('wb', d.wb), ('ab', d.ab), ('odo_scale', d.odo_scale)):
        mine = own.series(k, runs)
        for i, r in enumerate(runs):
            assert np.array_equal(np.asarray(src.data['%s_%d' % (state, r)]).reshape(mine[i].shape), mine[i]), (k, r)
    own.release()
    # the plugin on one logged series: the given-form job's bits
    imu2 = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=True, odo=True)
    algo = InsLoose(ini_pos_vel_att=sim_ini, ref_frame=rf, imu=imu2, odo=True, nhc=True, odo_scale_state=True)
    gps7 = np.concatenate([gps[0], vis[:, None]], axis=1)
    algo.run([fs, gyro[0], accel[0], np.asarray(d.time.data), np.asarray(d.gps_time.data), gps7, odo[0]])
    res = algo.get_results()
    assert len(res) == 6 and res[5].shape == (gyro.shape[1],)
    bufs = {'accel': ctx.upload(np.ascontiguousarray(accel[0].T)), 'gyro': ctx.upload(np.ascontiguousarray(gyro[0].T)),
            'gps': ctx.upload(np.ascontiguousarray(gps[0].T)), 'odo': ctx.upload(np.ascontiguousarray(odo[0]))}
    one = ginsim.InsLooseJob(ctx, fs, rf, dict(t, ref_gps=gps[0]), imu.accel_err, imu.gyro_err, imu.gps_err, sim_ini, 1, given=bufs, keep_traj=True,
                             odo_err=imu.odo_err, aid={'odo': True, 'nhc': True}, odo_scale_state={}, keep_scale=True).run()
    for v, k in zip(res, ('pos', 'vel', 'att', 'wb', 'ab', 'odo_scale')):
        assert np.array_equal(v, one.series(k, [0])[0]), k
    one.release()
    for b in bufs.values():
        b.free()
