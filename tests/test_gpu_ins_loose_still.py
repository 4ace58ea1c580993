"""GPU: InsLoose aided at standstill, ZUPT and ZARU (csrc/ins_loose_still.hip, InsLooseJob(still=...), InsLoose(zupt=True, zaru=True),
the 'loose' role of Sim) against its NumPy restatement (tests/ins_loose_ref.py), against the unaided and the odometer-aided
launch and against the statistics of its own covariance.  Shapes: the stops profile at 20 Hz, 1100 samples (600 for the bit
comparisons: the first stop and 13 s after it), 1-257 runs; 1024 runs for the consistency.

Parity bound, as tests/test_gpu_ins_loose_mag.py: not a recorded constant.  Every comparison with the restatement measures, on its
own case (the device's dumped sensors, fixes and odometer, the first 8 runs), the float64 restatement against its np.longdouble
evaluation (ins_loose_cases.restatement_error) and allows the device ins_loose_cases.PARITY_MARGIN (16) x that.
Measured on the MI355X over the twelve 257-run parity cases (the largest deviation of the device from the restatement, and in
brackets the smallest bound any case allowed): att 5.0e-14 (1.7e-12), pos 6.3e-14 in ref_frame 0 (4.7e-12) and 2.0e-16 in ref_frame 1
(7.9e-14), vel 2.7e-13 (1.3e-11), wb 1.0e-11 (5.2e-10), ab 7.9e-12 (8.3e-11), pdiag_end 2.5e-13 (9.3e-13).  Every bit comparison holds.
Consistency: the restatement's ratios to all three recorded digits at both instants.  Launch times:
profiles/ins_loose_still_timing.json."""
import numpy as np
import pytest

import ins_loose_aided_cases as ac
import ins_loose_cases as cs
import ins_loose_dump
import ins_loose_ref as ref
import ins_loose_still_cases as sc
from ins_loose_dump import ctx, held, planes, result, same_bits

pytestmark = pytest.mark.gpu

FS, FS_GPS = 20.0, 2.0
VIB = {'type': 'random', 'x': 0.05, 'y': 0.05, 'z': 0.05}


class Dump(ins_loose_dump.Dump):
    """The stops profile, with the standstill signal of its truth in .flags."""

    def __init__(self, ctx, rf, n, runs, seed=77, run_offset=0, vib=None):
        super().__init__(ctx, rf, n, runs, seed, run_offset, FS, FS_GPS, truth_fn=sc.stops_truth, vib=vib, flags=sc.flags_of)

    def job(self, ctx, smask, mask=0, every=1, given=False, runs=None, flags=None, **kw):
        """smask: the standstill rows (1 ZUPT, 2 ZARU, 3 both); 0: still={zupt: False, zaru: False}; None: no still argument at all.
        mask 0: no aiding argument at all.  flags None: the job derives the signal from the truth."""
        kw = ac.aid_kw(mask, **kw)
        if smask is not None:
            still = sc.options(smask, every) if smask else {'zupt': False, 'zaru': False, 'every': every}
            kw = dict(dict(still=dict(still, flags=flags)), **kw)
        return super().job(ctx, given, runs=runs, **kw)

    def _kw(self, smask, mask, every, flags):
        return dict(odo=self.odo, aid=ac.aid(mask) if mask else None, still=sc.model(self.model, self.fs, smask, every),
                    flags=self.flags if flags is None else flags)

    def restate(self, smask, mask=0, every=1, flags=None):
        return ref.run(*self._args(), **self._kw(smask, mask, every, flags))

    def bound(self, smask, mask=0, every=1, flags=None):
        kw = self._kw(smask, mask, every, flags)
        return cs.parity_bound(*self._args(), odo=kw['odo'], aid=kw['aid'], still=kw['still'], flags=kw['flags'])


@pytest.fixture(scope='module', params=[0, 1], ids=['rf0', 'rf1'])
def dump(request, ctx):
    d = Dump(ctx, request.param, None, 257)                 # the whole profile, 1100 samples; four wavefronts plus one lane
    yield d
    d.release()


@pytest.fixture(scope='module', params=[0, 1], ids=['rf0', 'rf1'])
def short(request, ctx):
    d = Dump(ctx, request.param, 600, 65, seed=41)          # 30 s: the first stop, the turn, 3 s into the outage
    yield d
    d.release()


# ------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize('name, smask, mask, every', [('zupt', 1, 0, 1), ('zaru', 2, 0, 1), ('both', 3, 0, 1), ('both every 3', 3, 0, 3),
                                                      ('both with odo + nhc', 3, 7, 1)])
def test_parity_with_the_restatement(ctx, dump, name, smask, mask, every):
    """The generated form on the whole stops profile, 257 runs: att, pos, vel, wb, ab, pdiag_end.  With mask 7 a GPS fix, an aiding
    block and a standstill block meet on one sample; the restatement holds their order."""
    assert dump.n == 1100 and len(sc.windows(dump.flags)) == 2
    both = [j for j in dump.stamps[np.asarray(dump.truth['gps_visibility']) != 0] if j > 0 and j % every == 0 and dump.flags[j]]
    assert len(both) >= 3                                                      # fixes on flagged samples
    job = dump.job(ctx, smask, mask, every).run()
    assert job.kernel_name() == 'ginsim::loose_still_kernel<%d, false, false, false>' % dump.rf
    dev = result(job)
    job.release()
    held('parity rf%d %s' % (dump.rf, name), cs.deviation(dev, dump.restate(smask, mask, every)), dump.bound(smask, mask, every))
    plain = dump.job(ctx, None, mask).run()
    other = result(plain)
    assert not np.array_equal(other['vel' if smask & 1 else 'wb'], dev['vel' if smask & 1 else 'wb'])      # the block did something
    first = sc.windows(dump.flags)[0][0]
    first += (-first) % every                                                  # the first sample a block fires at
    for k in ('att', 'pos', 'vel', 'wb', 'ab'):
        assert np.array_equal(other[k][:, :first], dev[k][:, :first]), k       # and nothing before the first flagged sample
    plain.release()


@pytest.mark.parametrize('rf', [0, 1])
def test_parity_with_a_vibration_term(ctx, rf):
    d = Dump(ctx, rf, None, 257, seed=9, vib=VIB)
    job = d.job(ctx, 3).run()
    assert job.kernel_name() == 'ginsim::loose_still_kernel<%d, false, true, false>' % rf
    dev = result(job)
    job.release()
    held('parity rf%d both with vibration' % rf, cs.deviation(dev, d.restate(3)), d.bound(3))
    d.release()


def test_a_flag_on_the_last_sample(ctx, short):
    """flags[n - 1] != 0: the block runs on the row that is stored last, from the gyro sample n - 2."""
    n = short.n
    flags = short.flags.copy()                              # the first stop's window, and the last sample (the vehicle is moving there)
    assert flags[n - 1] == 0 and flags.any()
    flags[n - 1] = 1
    job = short.job(ctx, 3, flags=flags).run()
    dev = result(job)
    held('parity rf%d a flag at n - 1' % short.rf, cs.deviation(dev, short.restate(3, flags=flags)), short.bound(3, flags=flags))
    flags[n - 1] = 0
    without = short.job(ctx, 3, flags=flags).run()
    w = result(without)
    for k in ('att', 'pos', 'vel', 'wb', 'ab'):
        assert np.array_equal(w[k][:, :n - 1], dev[k][:, :n - 1]), k
    assert not np.array_equal(w['vel'][:, n - 1], dev['vel'][:, n - 1]) and not np.array_equal(w['pdiag_end'], dev['pdiag_end'])
    job.release()
    without.release()


# ------------------------------------------------------------------------------------------------- 2. bit for bit
@pytest.mark.parametrize('mask', [0, 7])
def test_generated_form_equals_given_form_and_two_launches_are_identical(ctx, short, mask):
    gen, giv = short.job(ctx, 3, mask).run(), short.job(ctx, 3, mask, given=True).run()
    assert (gen.variant(), giv.variant()) == (0, 1)
    assert gen.kernel_name() == 'ginsim::loose_still_kernel<%d, false, false, false>' % short.rf
    assert giv.kernel_name() == 'ginsim::loose_still_kernel<%d, true, false, false>' % short.rf
    a = planes(gen)
    same_bits(a, planes(giv))
    gen.run()
    same_bits(a, planes(gen))
    again = short.job(ctx, 3, mask).run()
    same_bits(a, planes(again))
    for j in (gen, giv, again):
        j.release()


def test_run_offset_above_2_32(ctx):
    d = Dump(ctx, 1, 400, 65, seed=41, run_offset=2 ** 40 + 3)
    gen, giv = d.job(ctx, 3, 1).run(), d.job(ctx, 3, 1, given=True).run()
    a = planes(gen)
    same_bits(a, planes(giv))
    low = Dump(ctx, 1, 400, 65, seed=41, run_offset=3)
    assert not np.array_equal(low.gyro, d.gyro)                                # the high word of the run id enters the counters
    for j in (gen, giv):
        j.release()
    d.release()
    low.release()


@pytest.mark.parametrize('mask', [0, 7])
def test_a_block_that_never_fires_is_the_launch_without_it(ctx, short, mask):
    """still_mask = 0 IS the plain / aided launch (its name says so).  All flags 0, a flag at j = 0 only and still_every >= n launch
    loose_still_kernel and give the plain / aided launch's bits on every output."""
    n = short.n
    at0 = np.zeros(n, dtype=np.int32)
    at0[0] = 1
    for given in (False, True):
        without = short.job(ctx, None, mask, given=given).run()
        want = planes(without)
        assert without.kernel_name().startswith('ginsim::loose_aided_kernel<' if mask else 'ginsim::loose_kernel<')
        degenerate = short.job(ctx, 0, mask, given=given).run()
        assert degenerate.kernel_name() == without.kernel_name()
        same_bits(want, planes(degenerate))
        degenerate.release()
        for name, kw in (('all flags 0', dict(flags=np.zeros(n, dtype=np.int32))), ('a flag at j = 0', dict(flags=at0)), ('every = n', dict(every=n)),
                         ('every = 2^40', dict(every=2 ** 40))):
            never = short.job(ctx, 3, mask, given=given, **kw).run()
            assert never.kernel_name().startswith('ginsim::loose_still_kernel<'), name
            same_bits(want, planes(never))
            never.release()
        without.release()


# ------------------------------------------------------------------------------------------------- 3. run counts, run lists
@pytest.fixture(scope='module')
def big(ctx):
    d = Dump(ctx, 1, 400, 257, seed=21)
    job = d.job(ctx, 3, 7, 2).run()
    yield d, planes(job)
    job.release()
    d.release()


@pytest.mark.parametrize('runs', [1, 63, 64, 65, 257])
def test_run_counts_around_a_wavefront_with_a_shuffled_run_list(ctx, big, runs):
    """Run r of a small launch is run r of the 257-run launch with the same seed (one lane per run, no neighbour in it); and a
    launch of `runs` runs of the 257-run job in shuffled order writes those runs' columns and no other."""
    import ginsim
    d, whole = big
    small = d.job(ctx, 3, 7, 2, runs=runs).run()
    same_bits(whole, planes(small), runs_a=np.arange(runs))
    small.release()
    ids = np.random.default_rng(3).permutation(257)[:runs]
    part = d.job(ctx, 3, 7, 2)
    ctx.sync()
    ginsim._lib.check(ginsim.lib.ginsim_memset(ctx.handle, part.buffer('series').ptr, 0, part.buffer('series').nbytes))
    part.run(ids)
    got = planes(part)
    rest = np.setdiff1d(np.arange(257), ids)
    for k in ('traj', 'wb', 'ab'):
        assert np.array_equal(got[k][..., ids].view(np.uint64), whole[k][..., ids].view(np.uint64)), k
        assert not got[k][..., rest].any(), k               # the other runs' columns were not touched
    assert np.array_equal(got['pdiag'][..., ids].view(np.uint64), whole['pdiag'][..., ids].view(np.uint64))
    part.release()


# ------------------------------------------------------------------------------------------------- 4. statistics only
def test_online_process_statistics_and_the_ned_end_record(ctx, short):
    ned = short.rf == 0
    job = short.job(ctx, 3, 0, 2, proc_first=100, proc_ned=ned, end_ned=ned).run()
    assert job.kernel_name() == 'ginsim::loose_still_kernel<%d, false, false, true>' % short.rf
    online, kept = job.process_stats_online(), job.process_stats(first_sample=100, pos_ned=ned)
    np.testing.assert_allclose(online, kept, rtol=1e-7, atol=1e-12)
    plain = short.job(ctx, 3, 0, 2, end_ned=ned).run()      # and the statistics variant computes what the plain one does
    same_bits(planes(plain), planes(job))
    only = short.job(ctx, 3, 0, 2, proc_first=100, proc_ned=ned, end_ned=ned, keep_traj=False).run()     # nothing kept at all
    assert only.kernel_name() == job.kernel_name()
    assert np.array_equal(only.end_errors().view(np.uint64), plain.end_errors().view(np.uint64))
    assert np.array_equal(only.process_stats_online().view(np.uint64), online.view(np.uint64))
    if ned:
        a, b = only.end_errors(ned=True), plain.end_errors(ned=True)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and np.all(np.isfinite(a))
        assert np.max(np.abs(a[:, 3:6])) > 1e3 * np.max(np.abs(plain.end_errors()[:, 3:5]))       # metres, not radians
        without = short.job(ctx, None, 0, end_ned=True).run()
        assert not np.array_equal(without.end_errors(ned=True), b)
        without.release()
    for j in (plain, job, only):
        j.release()


# ------------------------------------------------------------------------------------------------- 5. consistency
@pytest.mark.parametrize('tag', ['stop', 'end'])
def test_consistency_of_the_covariance(ctx, tag):
    """For every state the RMS error over sqrt(mean pdiag_end) is the ratio the restatement gave on the same 1024 draws
    (ins_loose_still_cases.CONSISTENCY_RATIOS), to the 2e-3 the CPU test holds the restatement to: at the end of the first stop (the
    profile and the draws cut there) and at the profile's end."""
    import ginsim
    R = cs.CONSISTENCY_RUNS
    c = sc.consistency_draw(1, cs.CONSISTENCY_FS, R)
    n = sc.windows(c['flags'])[0][1] + 1 if tag == 'stop' else c['truth']['ref_accel'].shape[0]
    ini, truth, stamps = sc.stops_truth(cs.CONSISTENCY_FS, 1, cs.CONSISTENCY_FS_GPS, n)
    m = stamps.size
    bufs = {'accel': ctx.upload(np.ascontiguousarray(c['accel'][:, :n].transpose(2, 1, 0))),
            'gyro': ctx.upload(np.ascontiguousarray(c['gyro'][:, :n].transpose(2, 1, 0))),
            'gps': ctx.upload(np.ascontiguousarray(c['gps'][:, :m].transpose(2, 1, 0)))}
    job = ginsim.InsLooseJob(ctx, cs.CONSISTENCY_FS, 1, truth, c['acc_e'], c['gyr_e'], cs.GPS_ERR, ini, R, given=bufs, keep_traj=True, still={}).run()
    assert job.n == n and job.kernel_name() == 'ginsim::loose_still_kernel<1, true, false, false>'
    assert np.array_equal(job.still_flags, c['flags'][:n])
    ids = np.arange(R)
    o = {k: job.series(k, ids) for k in ('att', 'pos', 'vel', 'wb', 'ab')}
    ratio = sc.ratios(sc.error_at(c, o, n - 1), job.final_pdiag())
    job.release()
    for b in bufs.values():
        b.free()
    print('standstill, %s: consistency ratios on the device:' % tag, np.array2string(ratio, precision=3))
    np.testing.assert_allclose(ratio, sc.CONSISTENCY_RATIOS['still'][tag], rtol=0, atol=2e-3)


# ------------------------------------------------------------------------------------------------- 6. through Sim
def test_sim_runs_the_standstill_aided_and_the_unaided_filter_on_one_realisation(ctx):
    """IMU(axis=9, gps=True) with [InsLoose(), InsLoose(zupt=True, zaru=True)]: the two share the sensors -- InsLoose() is the same
    bits as in a Sim without the second plugin, and the Sim's kept sensor series of a run, through the restatement with the flags of
    the Sim's truth, gives that run of the aided plugin; consistency_curve names the aided plugin and raises; a statistics-only Sim
    reports the same statistics."""
    from demo_algorithms.ins_loose_device import InsLoose
    from ginsim import filter_model, still_model, workloads
    from gnss_ins_sim.sim import imu_model, ins_sim
    fs, fs_gps, rf = FS, FS_GPS, 1
    ini = workloads.parse_motion(sc.STOPS_CSV)[0]

    def make(algos, keep=True):
        imu = imu_model.IMU(accuracy='mid-accuracy', axis=9, gps=True)
        sim = ins_sim.Sim([fs, fs_gps, fs], sc.STOPS_CSV, ref_frame=rf, imu=imu, seed=1234, keep_trajectories=keep, geo_mag_n=[30.0, -3.0, 40.0],
                          algorithm=algos)
        sim.run(257)
        return sim, imu
    sim, imu = make([InsLoose(), InsLoose(zupt=True, zaru=True)])
    d, res = sim.dmgr, sim.mc
    plain, aided = res.loose_names
    (_, job0, kept0), (_, job1, kept1) = sim.loose_jobs
    assert job0.kernel_name() == 'ginsim::loose_kernel<1, false, false, false>' and job0.still is None
    assert job1.kernel_name() == 'ginsim::loose_still_kernel<1, false, false, false>'
    model = filter_model(fs, imu.accel_err, imu.gyro_err, imu.gps_err)
    want = still_model(model, fs, {})
    assert sorted(job1.still) == sorted(want) and all(np.array_equal(job1.still[k], want[k]) for k in want)
    _, truth, _ = sc.stops_truth(fs, rf, fs_gps)
    assert np.array_equal(job1.still_flags, sc.flags_of(truth)) and len(sc.windows(job1.still_flags)) == 2
    # the unaided plugin does not see the second one
    one, _ = make([InsLoose()])
    (_, _, kept_one), = one.loose_jobs
    same_bits(planes(kept0), planes(kept_one))
    # one realisation: the Sim's own kept series of two runs through the restatement
    runs = [3, 65]
    accel, gyro, gps = (np.stack([np.asarray(src.data[r]) for r in runs]) for src in (d.accel, d.gyro, d.gps))
    stamps = np.rint(np.asarray(d.gps_time.data) * fs).astype(np.int64)
    vis = np.asarray(d.gps_visibility.data)
    args = (rf, fs, gyro, accel, ini, model, gps, stamps, vis)
    exp = ref.run(*args, still=job1.still, flags=job1.still_flags)
    bound = cs.parity_bound(*args, odo=None, aid=None, still=job1.still, flags=job1.still_flags)
    got = {k: np.stack([np.asarray(src.data['%s_%d' % (aided, r)]) for r in runs])
           for k, src in (('att', d.att_euler), ('pos', d.pos), ('vel', d.vel), ('wb', d.wb), ('ab', d.ab))}
    got['pdiag_end'] = job1.final_pdiag()[runs]
    held('parity Sim pairing', cs.deviation(got, exp), bound)
    with pytest.raises(NotImplementedError, match='zupt'):
        sim.consistency_curve(every=5.0)
    # statistics only: the same numbers in results()
    sim.results(err_stats_start=-1)
    lean, _ = make([InsLoose(), InsLoose(zupt=True, zaru=True)], keep=False)
    (_, lean1, _) = lean.loose_jobs[1]
    assert not lean1.keep_traj and lean1.kernel_name().startswith('ginsim::loose_still_kernel<1, false, false, ')
    lean.results(err_stats_start=-1)
    for name in ('att_euler', 'pos', 'vel'):
        for key in ('std', 'max', 'avg'):
            for nm in (plain, aided):
                np.testing.assert_allclose(np.asarray(lean.err_stats[name][key][nm]), np.asarray(sim.err_stats[name][key][nm]), rtol=1e-9, atol=1e-12)
