"""GPU: the loosely coupled GPS/INS filter (csrc/ins_loose.hip, ginsim.InsLooseJob, InsLoose of demo_algorithms.ins_loose_device,
the 'loose' role of Sim) against its NumPy restatement (tests/ins_loose_ref.py), against free integration when no fix is usable,
and against the statistics of its own covariance.  Shapes: 1-257 runs x 300-6000 samples (1024 x 1200 for the consistency).

Parity bound.  Not a recorded constant: every comparison with the restatement measures, on its own case (the device's dumped
sensors and fixes, the first 8 runs), the float64 restatement against its np.longdouble evaluation (ins_loose_cases.restatement_error)
and allows the device 16 x that (MagCal's margin for the freedom in the order of operations).  Measured on the MI355X for the parity
cases (2300 samples, 257 runs): restatement error att 2.6e-13, pos 3.1e-12, vel 5.1e-12, wb 8.4e-10, ab 3.8e-10, pdiag_end 1.9e-13;
device against restatement att 2.0e-14, pos 9.3e-15, vel 4.9e-14, wb 2.9e-12, ab 2.1e-12, pdiag_end 6.4e-14."""
import numpy as np
import pytest

import ins_loose_cases as cs
from conftest import assert_traj_close
import ins_loose_dump
import ins_loose_ref as ref
from ins_loose_dump import ctx, held, planes, result, same_bits

pytestmark = pytest.mark.gpu

FS, FS_GPS = 100.0, 10.0

deviation = cs.deviation


class Dump(ins_loose_dump.Dump):
    """No odometer; the free-integration trajectories of the same launch are kept."""

    def __init__(self, ctx, rf, n, runs, seed=77, run_offset=0, fs=FS, fs_gps=FS_GPS, **bias):
        super().__init__(ctx, rf, n, runs, seed, run_offset, fs, fs_gps, truth_fn=cs.outage_truth, odo_err=None, **bias)

    def restate(self, visible='truth', stamps=None, gps=None):
        vis = self.truth['gps_visibility'] if isinstance(visible, str) else visible
        return ref.run(self.rf, self.fs, self.gyro, self.accel, self.ini, self.model, self.gps if gps is None else gps,
                       self.stamps if stamps is None else stamps, vis)

    def bound(self, visible='truth', stamps=None, gps=None):
        """16 x the restatement's own float64 error on this case (its first 8 runs)."""
        vis = self.truth['gps_visibility'] if isinstance(visible, str) else visible
        return cs.parity_bound(self.rf, self.fs, self.gyro, self.accel, self.ini, self.model, self.gps if gps is None else gps,
                               self.stamps if stamps is None else stamps, vis)


@pytest.fixture(scope='module', params=[0, 1], ids=['rf0', 'rf1'])
def dump(request, ctx):
    d = Dump(ctx, request.param, 2300, 257)                 # 300 samples into the outage
    yield d
    d.release()


# ------------------------------------------------------------------------------------------------- parity, generated = given
def test_parity_with_the_restatement(ctx, dump):
    """Trajectory, wb, ab and pdiag_end of every run against the restatement on the same sensors and fixes, within 16 x the
    restatement's own float64 error on this case."""
    job = dump.job(ctx, given=True).run()
    dev, exp = result(job), dump.restate()
    job.release()
    held('parity rf%d' % dump.rf, deviation(dev, exp), dump.bound())
    assert np.abs(dev['wb'][:, -1]).max() > 0 and np.abs(dev['ab'][:, -1]).max() > 0


def test_generated_form_equals_given_form_bit_for_bit(ctx, dump):
    """The lane regenerates the sensors ginsim_mc_run and the fixes ginsim_aux_sensors store for the same seed and run ids, and
    the two instantiations share the step: every output is the same bits."""
    gen, giv = dump.job(ctx, given=False).run(), dump.job(ctx, given=True).run()
    assert (gen.variant(), giv.variant()) == (0, 1)
    assert gen.kernel_name() == 'ginsim::loose_kernel<%d, false, false, false>' % dump.rf
    same_bits(planes(gen), planes(giv))
    gen.release()
    giv.release()


# ------------------------------------------------------------------------------------------------- no usable fix
@pytest.mark.parametrize('how', ['invisible', 'm0'])
def test_without_a_usable_fix_it_is_free_integration(ctx, dump, how):
    truth = dict(dump.truth)
    if how == 'invisible':
        truth['gps_visibility'] = np.zeros_like(dump.truth['gps_visibility'])
    else:
        truth['ref_gps'], truth['gps_time'], truth['gps_visibility'] = np.zeros((0, 6)), np.zeros(0), np.zeros(0)
    job = dump.job(ctx, truth=truth).run()
    dev = result(job)
    job.release()
    att, pos, vel = dump.mc.trajectories('free', np.arange(dump.runs))
    np.testing.assert_allclose(dev['att'], att, rtol=1e-10, atol=0)
    np.testing.assert_allclose(dev['pos'], pos, rtol=1e-10, atol=0)
    np.testing.assert_allclose(dev['vel'], vel, rtol=1e-10, atol=1e-300)
    assert not dev['wb'].any() and not dev['ab'].any()
    exp = dump.restate(visible=np.zeros(dump.stamps.size))
    d = float(np.max(np.abs(dev['pdiag_end'] - exp['pdiag_end']) / exp['pdiag_end']))
    assert d <= dump.bound(visible=np.zeros(dump.stamps.size))['pdiag_end'], d


# ------------------------------------------------------------------------------------------------- outage
def test_outage_profile(ctx):
    """The whole 60 s profile, ref_frame 0 (NED metres through Sim-like statistics), paired with free integration."""
    d = Dump(ctx, 0, None, 257, seed=5)
    full = d.job(ctx).run()
    out0, out1 = int(d.stamps[np.nonzero(d.truth['gps_visibility'] == 0)[0][0]]), int(d.stamps[np.nonzero(d.truth['gps_visibility'] == 0)[0][-1]])
    m_cut = int(np.count_nonzero(d.stamps < out0))
    cut_truth = dict(d.truth, ref_gps=d.truth['ref_gps'][:m_cut], gps_time=d.truth['gps_time'][:m_cut], gps_visibility=d.truth['gps_visibility'][:m_cut])
    cut = d.job(ctx, truth=cut_truth).run()
    a, b = planes(full), planes(cut)
    stop = out1 + int(FS / FS_GPS)                          # the first visible fix after the outage
    for k in ('traj', 'wb', 'ab'):                          # during the invisible stretch: a run whose fixes stop there
        assert np.array_equal(a[k][:, :stop].view(np.uint64), b[k][:, :stop].view(np.uint64)), k
    assert not np.array_equal(a['traj'][:, stop], b['traj'][:, stop])
    samples = [out0, stop - 1, stop + 500, d.truth['ref_accel'].shape[0] - 1]
    filt = full.error_curve(samples=samples, pos_ned=True).std[:, 3:6]
    free = d.mc.error_curve('free', samples=samples, pos_ned=True).std[:, 3:6]
    h = np.linalg.norm(filt[:, 0:2], axis=1)
    print('horizontal position 1 sigma [m] at outage start / end / +5 s / profile end: filter %s, free %s'
          % (np.array2string(h, precision=3), np.array2string(np.linalg.norm(free[:, 0:2], axis=1), precision=3)))
    assert h[1] > h[0]                                      # it grows through the outage
    assert h[2] < h[1] and h[3] < h[1]                      # and falls again after it
    assert np.all(filt[3] < free[3])                        # at the end below the paired free integration's, on every axis
    full.release()
    cut.release()
    d.release()


# ------------------------------------------------------------------------------------------------- consistency
def test_consistency_of_the_covariance(ctx):
    """1024 runs drawn from the filter's own model on the CPU (the case of tests/test_ins_loose_oracle.py::test_restatement_consistency),
    filtered by the device: for every state the RMS end error over sqrt(mean pdiag_end) lies within x/: 1.25 of the ratio the
    restatement gave (the 1 sigma of an RMS over 1024 runs is 2.2 %, plus correlation), and those lie in [0.7, 1.4]."""
    import ginsim
    fs, R = cs.CONSISTENCY_FS, cs.CONSISTENCY_RUNS
    ini, truth, stamps = cs.outage_truth(fs, 1, cs.CONSISTENCY_FS_GPS)
    acc_e, gyr_e = cs.imu_errors()
    rng = np.random.default_rng(cs.CONSISTENCY_SEED)
    accel, gyro, tba, tbg = ref.sample_sensors(rng, fs, truth['ref_accel'], truth['ref_gyro'], acc_e, gyr_e, R)
    gps = cs.sample_gps(rng, truth, 1, R)
    bufs = {'accel': ctx.upload(np.ascontiguousarray(accel.transpose(2, 1, 0))), 'gyro': ctx.upload(np.ascontiguousarray(gyro.transpose(2, 1, 0))),
            'gps': ctx.upload(np.ascontiguousarray(gps.transpose(2, 1, 0)))}
    job = ginsim.InsLooseJob(ctx, fs, 1, truth, acc_e, gyr_e, cs.GPS_ERR, ini, R, given=bufs, keep_traj=True).run()
    last = job.n - 1
    ids = np.arange(R)
    att, pos, vel = (job.series(k, ids)[:, last] for k in ('att', 'pos', 'vel'))
    wb, ab = job.final_biases()
    e = ref.error_state(1, att, pos, vel, wb, ab, truth['ref_att'][-1], truth['ref_pos'][-1], truth['ref_vel'][-1], tbg[:, -1], tba[:, -1])
    ratio = np.sqrt(np.mean(e * e, axis=0)) / np.sqrt(np.mean(job.final_pdiag(), axis=0))
    job.release()
    for b in bufs.values():
        b.free()
    want = np.array(cs.CONSISTENCY_RATIOS)
    print('consistency ratios on the device:', np.array2string(ratio, precision=3))
    assert np.all(want >= 0.7) and np.all(want <= 1.4)
    assert np.all(ratio <= want * 1.25) and np.all(ratio >= want / 1.25), ratio / want


# ------------------------------------------------------------------------------------------------- bias estimation
def test_constant_biases_are_estimated(ctx):
    """gyro_b = (3, -3, 3)e-4 rad/s, accel_b = (2, -2, 2)e-2 m/s^2 over the whole profile: the across-run mean of wb / ab at the end
    is closer to the injected bias than 0 is on the axes the profile makes observable.  From the restatement (64 runs, same
    profile, ref_frame 1): all six -- mean wb (2.96, -2.96, 2.71)e-4, mean ab (1.99, -1.98, 2.00)e-2, the 1 sigma of the bias states
    down to 3-7 % of its initial value (the horizontal gyro and all accelerometer axes show in the velocity through gravity, the
    gyro z axis through the acceleration and the two turns)."""
    gb, ab_ = np.array([3e-4, -3e-4, 3e-4]), np.array([2e-2, -2e-2, 2e-2])
    d = Dump(ctx, 1, None, 257, seed=9, gyro_b=gb, accel_b=ab_)
    job = d.job(ctx, keep_traj=False).run()
    wb, ab = job.final_biases()
    sig = job.final_sigmas()
    job.release()
    d.release()
    print('wb mean', wb.mean(0), 'ab mean', ab.mean(0), 'sigma bg', sig[:, 9:12].mean(0), 'sigma ba', sig[:, 12:15].mean(0))
    assert np.all(np.abs(wb.mean(0) - gb) < np.abs(gb)), wb.mean(0)
    assert np.all(np.abs(ab.mean(0) - ab_) < np.abs(ab_)), ab.mean(0)


# ------------------------------------------------------------------------------------------------- edges
@pytest.mark.parametrize('runs', [1, 63, 64, 65])
def test_run_counts_around_a_wavefront(ctx, runs):
    """Run r of a small launch is run r of the 257-run launch with the same seed (one lane per run, no neighbour in it)."""
    big, small = Dump(ctx, 1, 300, 257, seed=21), Dump(ctx, 1, 300, runs, seed=21)
    a, b = big.job(ctx).run(), small.job(ctx).run()
    same_bits(planes(a), planes(b), runs_a=np.arange(runs))
    for x in (a, b):
        x.release()
    big.release()
    small.release()


def test_fix_at_the_first_and_at_the_last_sample_and_gps_at_the_imu_rate(ctx):
    n = 300
    d = Dump(ctx, 0, n, 65, seed=31, fs_gps=FS)             # a fix at every sample, the first at sample 0, the last at n - 1
    assert d.stamps[0] == 0 and d.stamps[-1] == n - 1 and d.stamps.size == n
    job = d.job(ctx, given=True).run()
    got, bound = deviation(result(job), d.restate()), d.bound()
    job.release()
    for k in got:
        assert got[k] <= bound[k], (k, got[k], bound[k])
    # two fixes only: sample 0 and the last sample
    ends = np.array([0, n - 1])
    truth = dict(d.truth, ref_gps=d.truth['ref_gps'][ends], gps_time=d.truth['gps_time'][ends], gps_visibility=np.ones(2))
    gps2 = np.ascontiguousarray(d.gps[:, ends])
    buf = ctx.upload(np.ascontiguousarray(gps2.transpose(2, 1, 0)))
    job = d.job(ctx, given=dict(d.given, gps=buf), truth=truth).run()
    got = deviation(result(job), d.restate(visible=np.ones(2), stamps=ends, gps=gps2))
    bound = d.bound(visible=np.ones(2), stamps=ends, gps=gps2)
    job.release()
    buf.free()
    for k in got:
        assert got[k] <= bound[k], (k, got[k], bound[k])
    d.release()


def test_run_offset_2_to_the_40_and_run_lists(ctx):
    d = Dump(ctx, 1, 300, 257, seed=41, run_offset=2 ** 40)
    gen, giv = d.job(ctx).run(), d.job(ctx, given=True).run()
    whole = planes(gen)
    same_bits(whole, planes(giv))
    giv.release()
    other = Dump(ctx, 1, 300, 257, seed=41)
    assert not np.array_equal(other.accel, d.accel)         # the run id enters the counter
    other.release()
    ids = np.random.default_rng(3).permutation(257)[:130]
    part = d.job(ctx)
    part.ctx.sync()
    import ginsim
    ginsim._lib.check(ginsim.lib.ginsim_memset(ctx.handle, part.buffer('series').ptr, 0, part.buffer('series').nbytes))
    part.run(ids)
    got = planes(part)
    for k in ('traj', 'wb', 'ab'):
        assert np.array_equal(got[k][..., ids].view(np.uint64), whole[k][..., ids].view(np.uint64)), k
        rest = np.setdiff1d(np.arange(257), ids)
        assert not got[k][..., rest].any(), k               # the other runs' columns were not touched
    assert np.array_equal(got['pdiag'][..., ids], whole['pdiag'][..., ids])
    part.release()
    gen.release()
    d.release()


def test_a_non_finite_sample_stays_in_its_run(ctx):
    d = Dump(ctx, 0, 300, 65, seed=51)
    clean = d.job(ctx, given=True).run()
    want = planes(clean)
    clean.release()
    acc = ctx.download(d.mc.buffer('accel'), (3, 300, 65))
    acc[1, 100, 33] = np.inf
    bad = ctx.upload(acc)
    job = d.job(ctx, given=True)
    job.mc.in_accel = bad.ptr
    job.run()
    got = planes(job)
    job.release()
    bad.free()
    keep = np.setdiff1d(np.arange(65), [33])
    same_bits(got, want, runs_a=keep, runs_b=keep)
    assert not np.all(np.isfinite(got['traj'][:, -1, 33]))
    assert np.array_equal(got['traj'][:, :101, 33], want['traj'][:, :101, 33])
    d.release()


def test_plain_and_placed_planes_give_the_same_results(ctx):
    assert ctx.placed_reserve(15 * 300 * 257 * 8), ctx.placed_note
    d = Dump(ctx, 1, 300, 257, seed=61)
    plain = d.job(ctx, placed=False).run()
    want = planes(plain)
    assert plain.placement()['placed'] == []
    plain.release()
    placed = d.job(ctx, placed=True).run()
    assert placed.placement()['placed'] == ['series']
    same_bits(planes(placed), want)
    placed.release()
    d.release()


def test_online_process_statistics_equal_those_of_the_kept_planes(ctx, dump):
    job = dump.job(ctx, proc_first=100, proc_ned=dump.rf == 0, end_ned=dump.rf == 0).run()
    online, kept = job.process_stats_online(), job.process_stats(first_sample=100, pos_ned=dump.rf == 0)
    np.testing.assert_allclose(online, kept, rtol=1e-7, atol=1e-12)
    st = job.stats(ned=dump.rf == 0)
    ft = job.stats_from_traj(pos_ned=dump.rf == 0)
    # the NED position error is a rotated difference of two ECEF vectors of 6.4e6 m: an ulp there is 9.3e-10 m, each component of
    # the difference carries up to two of them and the rotation sums three -- 4e-9 m absolute on the position statistics, whichever
    # of the two code paths (the kernel's end record, the reduction over the kept planes) rounds which way
    atol = np.array([1e-13] * 3 + [4e-9 if dump.rf == 0 else 1e-13] * 3 + [1e-13] * 3)
    assert np.all(np.abs(st.std - ft.std) <= 1e-9 * np.abs(ft.std) + atol)
    assert np.all(np.abs(st.maxabs - ft.maxabs) <= 1e-9 * np.abs(ft.maxabs) + atol)
    job.release()


# ------------------------------------------------------------------------------------------------- plugin and Sim
def test_plugin_run_on_one_logged_series(ctx):
    from demo_algorithms.ins_loose_device import InsLoose
    from gnss_ins_sim.sim import imu_model
    d = Dump(ctx, 1, 600, 1, seed=71)
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=True)
    imu.gps_err = dict(cs.GPS_ERR)
    algo = InsLoose(ini_pos_vel_att=d.ini, ref_frame=1, imu=imu)
    gps7 = np.concatenate([d.gps[0], d.truth['gps_visibility'][:, None]], axis=1)
    algo.run([FS, d.gyro[0], d.accel[0], np.arange(600) / FS, d.truth['gps_time'], gps7])
    pos, vel, att, wb, ab = algo.get_results()
    exp, bound = d.restate(), d.bound()
    got = deviation({'att': att[None], 'pos': pos[None], 'vel': vel[None], 'wb': wb[None], 'ab': ab[None], 'pdiag_end': exp['pdiag_end']}, exp)
    for k in ('att', 'pos', 'vel', 'wb', 'ab'):
        assert got[k] <= bound[k], (k, got[k], bound[k])
    d.release()


def _sim(algos, runs, keep, capsys=None, rf=0, **kw):
    from gnss_ins_sim.sim import imu_model, ins_sim
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=True)
    sim = ins_sim.Sim([FS, FS_GPS, 0.0], cs.OUTAGE_CSV, ref_frame=rf, imu=imu, algorithm=algos, seed=1234, keep_trajectories=keep, **kw)
    sim.run(runs)
    return sim


def _printed(text, title):
    """The vectors of one section of Sim's summary text: {'Max error' | 'Avg error' | 'Std of error': [vector, ...]}."""
    import re
    sec = text[text.index('statistics for ' + title):]
    nxt = sec.find('-----------statistics for', 10)
    sec = sec if nxt < 0 else sec[:nxt]
    return {k: [np.array([float(x) for x in v.split()]) for v in re.findall(r'--%s: \[([^\]]*)\]' % k, sec)]
            for k in ('Max error', 'Avg error', 'Std of error')}


def test_sim_summary_equals_the_job_statistics(ctx, capsys):
    """The numbers of the PRINTED summary (end-point statistics, position in NED metres) are InsLooseJob.stats' of the Sim's own job,
    to the digits the text carries."""
    from demo_algorithms.ins_loose_device import InsLoose
    sim = _sim(InsLoose(), 257, False)
    capsys.readouterr()
    sim.results(err_stats_start=-1, extra_opt='ned')
    text = capsys.readouterr().out
    _, job, kept = sim.loose_jobs[0]
    assert kept is None and not job.keep_traj
    st = job.stats(ned=True)
    for title, sl, scale in (('simulation attitude (Euler, ZYX)', slice(0, 3), 180.0 / np.pi), ('simulation position', slice(3, 6), 1.0),
                             ('simulation velocity', slice(6, 9), 1.0)):
        got = _printed(text, title)
        assert len(got['Std of error']) == 1 and len(got['Max error']) == 1, title
        # the text carries eight decimals (fixed notation) or eight decimals of the mantissa: half a unit of the last one
        for key, want in (('Std of error', st.std), ('Max error', st.maxabs), ('Avg error', st.mean)):
            np.testing.assert_allclose(got[key][0], want[sl] * scale, rtol=0, atol=5.1e-9)
    assert len(sim.dmgr.wb.data) == 0                                   # statistics only: names known, nothing kept
    with pytest.raises(ValueError, match='statistics only'):
        sim.error_curve('pos', every=10.0)


def test_sim_pairs_the_filter_with_free_integration_and_draws_its_curve(ctx):
    """A two-plugin Sim: both plugins see ONE sensor realisation per run.  The Sim's own kept accel / gyro of a run (written by the
    FreeIntegration launch) and its kept fixes (its AuxSensorJob), fed to the restatement, give the Sim's InsLoose series of that
    run -- which fails if Sim handed the filter another seed, run offset or initial state than the fused job; and free integration
    of those same samples is the Sim's FreeIntegration series."""
    from demo_algorithms import free_integration
    from demo_algorithms.ins_loose_device import InsLoose
    from ginsim import filter_model, workloads
    from oracle import ins_np
    ini = workloads.parse_motion(cs.OUTAGE_CSV)[0]
    sim = _sim([free_integration.FreeIntegration(ini), InsLoose()], 66, True)
    d, mc = sim.dmgr, sim.mc
    free, loose = mc.nav_names
    assert mc.fused_names == [free] and list(mc.loose_names) == [loose]
    _, job, kept = sim.loose_jobs[0]
    assert job is kept
    runs = [3, 65]                                                      # one in each wavefront
    accel, gyro, gps = (np.stack([np.asarray(src.data[r]) for r in runs]) for src in (d.accel, d.gyro, d.gps))
    stamps = np.rint(np.asarray(d.gps_time.data) * FS).astype(np.int64)
    vis = np.asarray(d.gps_visibility.data)
    model = filter_model(FS, sim.imu.accel_err, sim.imu.gyro_err, sim.imu.gps_err)
    exp = ref.run(0, FS, gyro, accel, ini, model, gps, stamps, vis)
    bound = cs.parity_bound(0, FS, gyro, accel, ini, model, gps, stamps, vis)
    got = {k: np.stack([np.asarray(src.data['%s_%d' % (loose, r)]) for r in runs])
           for k, src in (('att', d.att_euler), ('pos', d.pos), ('vel', d.vel), ('wb', d.wb), ('ab', d.ab))}
    got['pdiag_end'] = job.final_pdiag()[runs]
    held('Sim pairing', cs.deviation(got, exp), bound)
    att, pos, vel = ins_np.free_integration(0, FS, gyro, accel, ini)
    f_att, f_pos, f_vel = (np.stack([np.asarray(d.get_data_all(k).data['%s_%d' % (free, r)]) for r in runs]) for k in ('att_euler', 'pos', 'vel'))
    assert_traj_close(f_att, f_pos, f_vel, att, pos, vel, rtol=1e-10, what='the Sim\'s FreeIntegration')      # as tests/test_gpu_parity.py
    assert np.array_equal(d.wb.data['%s_3' % loose], job.series('wb', [3])[0])
    # the curve of a kept InsLoose is ginsim_error_curve on its planes
    samples = np.array([0, 1999, 3999, 5999])
    curve = sim.error_curve(('pos',), samples=samples, extra_opt='ned')
    direct = job.error_curve(samples=samples, pos_ned=True)
    np.testing.assert_array_equal(curve['pos']['std'][loose], direct.std[:, 3:6])
    np.testing.assert_array_equal(curve['pos']['max'][loose], direct.maxabs[:, 3:6])
    assert np.all(curve['pos']['std'][loose][-1] < curve['pos']['std'][free][-1])
