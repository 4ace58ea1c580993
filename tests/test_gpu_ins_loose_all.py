"""GPU: InsLoose with all its aids in one launch (csrc/ins_loose_all.hip, InsLooseJob(combined=True), InsLoose(combined=True), the
'loose' role of Sim) against its NumPy restatement (tests/ins_loose_all_ref.py), against the single families' launches where a block
never fires and against the statistics of its own covariance.  Shapes: the stops profile at 20 Hz, 1100 samples (600 for the bit
comparisons), 1-257 runs; the tilted stops profile with 65 runs; 1024 runs for the consistency.  Every test passes combined=True,
which the package without the family does not take.

Parity bound, as tests/test_gpu_ins_loose_still.py: not a recorded constant.  Every comparison with the restatement measures, on its
own case (the device's dumped sensors, fixes, odometer and magnetometer, the first 8 runs), the float64 restatement against its
np.longdouble evaluation (ins_loose_cases.restatement_error with run=ins_loose_all_ref.run) and allows the device
ins_loose_cases.PARITY_MARGIN (16) x that, per output: att, pos, vel, wb, ab, pdiag_end and, with 16 states, the k_est series,
scale_end and pcross_end.

Measured on the MI355X (first run: all pass as written).  Largest deviation from the restatement over the sixteen parity cases and the
pairing through Sim, with the smallest bound any of them allowed: att 5.8e-14 (1.5e-13), pos 2.3e-14 in ref_frame 0 (9.7e-14) and
2.0e-16 in ref_frame 1 (8.9e-14), vel 1.2e-12 (8.4e-12), wb 3.9e-11 (1.4e-11 is the bound of the case with a flag on the last sample,
whose own deviation is 1.9e-12; the case of the largest deviation allowed 1.2e-10), ab 1.4e-11 (7.2e-11), pdiag_end 1.8e-13 (1.0e-12),
k_est 1.2e-13 (2.0e-12), scale_end 1.2e-13 (3.0e-12), pcross_end 6.5e-14 (2.3e-13).  Every bit comparison holds.  The consistency
ratios on the device are the restatement's to the three recorded digits at both instants.  Launch times:
profiles/ins_loose_all_timing.json."""
import numpy as np
import pytest

import ins_loose_all_cases as ls
import ins_loose_all_ref as aref
import ins_loose_cases as cs
import ins_loose_dump
import ins_loose_mag_cases as mc
import ins_loose_still_cases as sc
from ins_loose_dump import ctx, held, planes, result, same_bits

pytestmark = pytest.mark.gpu

FS, FS_GPS = 20.0, 2.0
VIB = {'type': 'random', 'x': 0.05, 'y': 0.05, 'z': 0.05}
ALL = ('mag', 'scale', 'still')
NAME = 'ginsim::loose_all_kernel<%d, %s, %s, %s, %d>'


def all_name(rf, given=False, vib=False, ps=False, ns=16):
    return NAME % (rf, str(given).lower(), str(vib).lower(), str(ps).lower(), ns)


class Dump(ins_loose_dump.Dump):
    """A stops profile with the odometer (it reads ls.READS), one magnetometer series and the standstill signal of the truth."""

    def __init__(self, ctx, rf, n, runs, seed=77, run_offset=0, vib=None, profile=sc.STOPS_CSV, geo=mc.GEO, mag_err=mc.MAG_ERR_SKEW):
        super().__init__(ctx, rf, n, runs, seed, run_offset, FS, FS_GPS, truth_fn=ls.stops_truth, profile=profile, geo=geo, odo_err=ls.ODO_ERR,
                         vib=vib, mag_errs=(('m', mag_err),), flags=sc.flags_of)
        self._restated = {}

    def _case(self, which, mask, every, flags, q=0.0):
        return dict(mask=mask, mag=self.mag_errs['m'] if 'mag' in which else None, scale='scale' in which, smask=3 if 'still' in which else 0,
                    every=every, geo=self.geo, flags=flags, q=q)

    def job(self, ctx, which=ALL, mask=ls.MASK, every=1, given=False, runs=None, flags=None, combined=True, mag_every=None, q=0.0, **kw):
        """which: the blocks of {'mag', 'scale', 'still'} the job holds.  flags None: the job derives the signal from the truth.
        mag_every: the magnetometer's own period where it is not `every`.  q: the scale state's random walk [1/sqrt(s)]."""
        case = ls.job_kw(keep=kw.get('keep_traj', True), **self._case(which, mask, every, flags, q))
        if mag_every is not None:
            case['mag'] = {'every': mag_every}
        if combined is not None:
            case['combined'] = combined
        if given and 'mag' in which:
            given = self.given_with_mag('m')
        return super().job(ctx, given, runs=runs, **dict(case, **kw))

    def restate(self, which=ALL, mask=ls.MASK, every=1, flags=None):
        """The restatement of all runs and 16 x its own float64 error on the first 8, once per case."""
        key = (tuple(which), mask, every, None if flags is None else flags.tobytes())
        if key not in self._restated:
            kw = ls.blocks(self.model, self.fs, self.rf, **self._case(which, mask, every, self.flags if flags is None else flags))
            kw.update(odo=self.odo, mag=self.mag['m'] if 'mag' in which else None)
            out = aref.run(*self._args(), **kw)
            bound = cs.parity_bound(*self._args(), run=aref.run, deviation=ls.deviation, **kw)
            self._restated[key] = (out, bound)
        return self._restated[key]


def parity(tag, d, job, which=ALL, mask=ls.MASK, every=1, flags=None):
    dev = result(job)
    exp, bound = d.restate(which, mask, every, flags)
    assert set(bound) == set(ls.kc.PARITY_KEYS if 'scale' in which else cs.PARITY_KEYS)
    held('parity rf%d %s' % (d.rf, tag), ls.deviation(dev, exp), bound)
    return dev


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
@pytest.mark.parametrize('name, which, every', [('mag + still', ('mag', 'still'), 1), ('scale + mag', ('scale', 'mag'), 1),
                                                ('scale + still', ('scale', 'still'), 1), ('all three', ALL, 1), ('all three every 3', ALL, 3)])
def test_parity_with_the_restatement(ctx, dump, name, which, every):
    """The generated form on the whole stops profile, 257 runs.  A GPS fix, an aiding block, a magnetometer block and a standstill
    block meet on one sample; the restatement holds their order."""
    assert dump.n == 1100 and len(sc.windows(dump.flags)) == 2 and np.any(dump.truth['gps_visibility'] == 0)
    job = dump.job(ctx, which, every=every).run()
    assert job.kernel_name() == all_name(dump.rf, ns=16 if 'scale' in which else 15)
    dev = parity(name, dump, job, which, every=every)
    job.release()
    if 'scale' in which:
        assert np.all(np.abs(dev['k_est'][:, -1] - ls.READS) < np.abs(ls.kc.SCALE0 - ls.READS))       # the scale was learnt


@pytest.mark.parametrize('rf', [0, 1])
def test_parity_with_a_vibration_term(ctx, rf):
    d = Dump(ctx, rf, None, 257, seed=9, vib=VIB)
    job = d.job(ctx).run()
    assert job.kernel_name() == all_name(rf, vib=True)
    parity('all three with vibration', d, job)
    job.release()
    d.release()


def test_a_flag_on_the_last_sample(ctx, short):
    """flags[n - 1] != 0: the standstill block runs on the row that is stored last, after that sample's other blocks."""
    n = short.n
    flags = short.flags.copy()
    assert flags[n - 1] == 0 and flags.any()
    flags[n - 1] = 1
    job = short.job(ctx, flags=flags).run()
    dev = parity('a flag at n - 1', short, job, flags=flags)
    flags[n - 1] = 0
    without = short.job(ctx, flags=flags).run()
    w = result(without)
    for k in ('att', 'pos', 'vel', 'wb', 'ab'):
        assert np.array_equal(w[k][:, :n - 1], dev[k][:, :n - 1]), k
    assert not np.array_equal(w['vel'][:, n - 1], dev['vel'][:, n - 1]) and not np.array_equal(w['pdiag_end'], dev['pdiag_end'])
    assert not np.array_equal(w['scale_end'], dev['scale_end'])                # the ZUPT rows move k_est through the cross-covariance
    job.release()
    without.release()


@pytest.mark.parametrize('rf', [0, 1])
def test_parity_on_the_tilted_stops_profile(ctx, rf):
    """41 S, yaw through +-180 deg, parked on a slope: the magnetometer rows and the rest rate are the terms that attitude and
    hemisphere enter.  All three blocks, a southern field, a general calibration."""
    d = Dump(ctx, rf, None, 65, seed=5, profile=sc.TILTED_STOPS_CSV, geo=mc.GEO_SOUTH)
    assert len(sc.windows(d.flags)) == 2
    job = d.job(ctx).run()
    assert job.kernel_name() == all_name(rf)
    parity('tilted stops, all three', d, job)
    job.release()
    d.release()


# ------------------------------------------------------------------------------------------------- 2. bit for bit
@pytest.mark.parametrize('which', [('mag', 'still'), ALL])
def test_generated_form_equals_given_form_and_two_launches_are_identical(ctx, short, which):
    ns = 16 if 'scale' in which else 15
    gen, giv = short.job(ctx, which, every=2).run(), short.job(ctx, which, every=2, given=True).run()
    assert (gen.kernel_name(), giv.kernel_name()) == (all_name(short.rf, ns=ns), all_name(short.rf, given=True, ns=ns))
    a = planes(gen)
    same_bits(a, planes(giv))
    gen.run()
    same_bits(a, planes(gen))
    again = short.job(ctx, which, every=2).run()
    same_bits(a, planes(again))
    for j in (gen, giv, again):
        j.release()


@pytest.mark.parametrize('given', [False, True], ids=['generated', 'given'])
def test_a_block_that_never_fires_leaves_the_single_family_s_bits(ctx, short, given):
    """The combined kernel itself (its name says so) against the single families' launches: a block that is held but never fires
    changes no bit of any output."""
    n, rf = short.n, short.rf
    zero = np.zeros(n, dtype=np.int32)
    cases = [(('mag', 'still'), dict(flags=zero), ('mag',), 15, 'mag + still, all flags 0 = the mag launch'),
             (('mag', 'still'), dict(mag_every=n), ('still',), 15, 'mag + still, mag_every >= n = the still launch'),
             (('scale', 'still'), dict(flags=zero), ('scale',), 16, 'scale + still, all flags 0 = the scale launch'),
             (('scale', 'mag'), dict(mag_every=2 ** 40), ('scale',), 16, 'scale + mag, mag_every >= n = the scale launch')]
    for which, kw, single, ns, name in cases:
        both = short.job(ctx, which, given=given, **kw).run()
        one = short.job(ctx, single, given=given, combined=None).run()
        assert both.kernel_name() == all_name(rf, given=given, ns=ns), name
        assert one.kernel_name() == 'ginsim::loose_%s_kernel<%d, %s, false, false>' % (single[0], rf, str(given).lower()), name
        same_bits(planes(one), planes(both))
        both.release()
        one.release()


@pytest.mark.parametrize('single', ['mag', 'scale', 'still', None])
def test_combined_with_one_block_or_none_is_that_family_s_launch(ctx, short, single):
    which = (single,) if single else ()
    a, b = short.job(ctx, which, combined=True).run(), short.job(ctx, which, combined=None).run()
    assert a.allp is None and a.kernel_name() == b.kernel_name()
    assert a.kernel_name().startswith('ginsim::loose_%s_kernel<' % (single or 'aided'))
    same_bits(planes(b), planes(a))
    a.release()
    b.release()


# ------------------------------------------------------------------------------------------------- 3. lanes and ids
@pytest.fixture(scope='module')
def big(ctx):
    d = Dump(ctx, 1, 400, 257, seed=21)
    job = d.job(ctx, every=2).run()
    yield d, planes(job)
    job.release()
    d.release()


@pytest.mark.parametrize('runs', [1, 63, 64, 65, 257])
def test_run_counts_around_a_wavefront_with_a_shuffled_run_list(ctx, big, runs):
    """Run r of a small launch is run r of the 257-run launch with the same seed (one lane per run, no neighbour in it); and a
    launch of `runs` runs of the 257-run job in shuffled order writes those runs' columns and no other."""
    import ginsim
    d, whole = big
    small = d.job(ctx, every=2, runs=runs).run()
    same_bits(whole, planes(small), runs_a=np.arange(runs))
    small.release()
    ids = np.random.default_rng(3).permutation(257)[:runs]
    part = d.job(ctx, every=2)
    ctx.sync()
    for name in ('series', 'scale'):
        ginsim._lib.check(ginsim.lib.ginsim_memset(ctx.handle, part.buffer(name).ptr, 0, part.buffer(name).nbytes))
    part.run(ids)
    got = planes(part)
    rest = np.setdiff1d(np.arange(257), ids)
    for k in ('traj', 'wb', 'ab', 'scale', 'scale_end', 'pcross'):
        assert np.array_equal(got[k][..., ids].view(np.uint64), whole[k][..., ids].view(np.uint64)), k
        assert not got[k][..., rest].any(), k               # the other runs' columns were not touched
    assert np.array_equal(got['pdiag'][..., ids].view(np.uint64), whole['pdiag'][..., ids].view(np.uint64))
    part.release()


def test_run_offset_above_2_32_and_ini_first(ctx):
    """The high word of the run id enters every sensor's counters (generated = given at an offset of 2^40 + 3); and run r of a launch
    with run_offset = ini_first = 65 is run 65 + r of a launch of 130 runs over a table of 130 initial states."""
    d = Dump(ctx, 1, 400, 65, seed=41, run_offset=2 ** 40 + 3)
    gen, giv = d.job(ctx).run(), d.job(ctx, given=True).run()
    same_bits(planes(gen), planes(giv))
    low = Dump(ctx, 1, 400, 65, seed=41, run_offset=3)
    assert not np.array_equal(low.gyro, d.gyro) and not np.array_equal(low.mag['m'], d.mag['m'])
    for j in (gen, giv):
        j.release()
    table = np.repeat(np.asarray(low.ini, dtype=np.float64).reshape(-1, 1), 130, axis=1)
    table[8] += 1e-3 * np.arange(130)                       # every run its own initial yaw
    table[3] += 1e-2 * np.arange(130)
    import ginsim
    kw = dict(ls.job_kw(ls.MASK, low.mag_errs['m'], True, 3), seed=41, keep_traj=True, combined=True)
    args = (ctx, FS, 1, low.truth, low.acc_e, low.gyr_e, cs.GPS_ERR, table)
    whole = ginsim.InsLooseJob(*args, 130, **kw).run()
    second = ginsim.InsLooseJob(*args, 65, run_offset=65, ini_first=65, **kw).run()
    assert whole.kernel_name() == all_name(1)
    w = planes(whole)
    assert not np.array_equal(w['traj'][..., 0], w['traj'][..., 65])
    same_bits(w, planes(second), runs_a=np.arange(65, 130))
    for j in (whole, second):
        j.release()
    d.release()
    low.release()


@pytest.mark.parametrize('which', [('mag', 'still'), ALL])
def test_online_process_statistics_and_the_ned_end_record(ctx, short, which):
    """The PS instantiations: the online statistics are the kept series', the statistics variant computes what the plain one does,
    and nothing kept at all gives the same end records."""
    ned, ns = short.rf == 0, 16 if 'scale' in which else 15
    job = short.job(ctx, which, every=2, proc_first=100, proc_ned=ned, end_ned=ned).run()
    assert job.kernel_name() == all_name(short.rf, ps=True, ns=ns)
    online, kept = job.process_stats_online(), job.process_stats(first_sample=100, pos_ned=ned)
    np.testing.assert_allclose(online, kept, rtol=1e-7, atol=1e-12)
    plain = short.job(ctx, which, every=2, end_ned=ned).run()
    same_bits(planes(plain), planes(job))
    only = short.job(ctx, which, every=2, proc_first=100, proc_ned=ned, end_ned=ned, keep_traj=False).run()
    assert only.kernel_name() == job.kernel_name() and not only.keep_scale
    assert np.array_equal(only.end_errors().view(np.uint64), plain.end_errors().view(np.uint64))
    assert np.array_equal(only.process_stats_online().view(np.uint64), online.view(np.uint64))
    if 'scale' in which:
        assert np.array_equal(only.final_sigmas().view(np.uint64), plain.final_sigmas().view(np.uint64)) and only.final_sigmas().shape == (65, 16)
        assert np.array_equal(only.final_pcross().view(np.uint64), plain.final_pcross().view(np.uint64))
        assert np.array_equal(only.final_scale()[0].view(np.uint64), plain.final_scale()[0].view(np.uint64))
    if ned:
        a, b = only.end_errors(ned=True), plain.end_errors(ned=True)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and np.all(np.isfinite(a))
        assert np.max(np.abs(a[:, 3:6])) > 1e3 * np.max(np.abs(plain.end_errors()[:, 3:5]))       # metres, not radians
    for j in (plain, job, only):
        j.release()


# ------------------------------------------------------------------------------------------------- 4. consistency
@pytest.mark.parametrize('tag', ['stop', 'end'])
def test_consistency_of_the_covariance(ctx, tag):
    """For every one of the 16 states the RMS error over sqrt(mean P_kk) is the ratio the restatement gave on the same 1024 draws
    (ins_loose_all_cases.CONSISTENCY_RATIOS), to the 2e-3 the CPU test holds the restatement to."""
    import ginsim
    R = cs.CONSISTENCY_RUNS
    c = ls.consistency_draw(1, cs.CONSISTENCY_FS, R)
    n = sc.windows(c['flags'])[0][1] + 1 if tag == 'stop' else c['truth']['ref_accel'].shape[0]
    ini, truth, stamps = ls.stops_truth(cs.CONSISTENCY_FS, 1, cs.CONSISTENCY_FS_GPS, n)
    m = stamps.size
    bufs = {'accel': ctx.upload(np.ascontiguousarray(c['accel'][:, :n].transpose(2, 1, 0))),
            'gyro': ctx.upload(np.ascontiguousarray(c['gyro'][:, :n].transpose(2, 1, 0))),
            'gps': ctx.upload(np.ascontiguousarray(c['gps'][:, :m].transpose(2, 1, 0))),
            'odo': ctx.upload(np.ascontiguousarray(c['odo'][:, :n].T)),
            'mag': ctx.upload(np.ascontiguousarray(c['mag'][:, :n].transpose(2, 1, 0)))}
    kw = ls.job_kw(ls.CONSISTENCY_MASK, mc.MAG_ERR, True, 3)
    job = ginsim.InsLooseJob(ctx, cs.CONSISTENCY_FS, 1, truth, c['acc_e'], c['gyr_e'], cs.GPS_ERR, ini, R, given=bufs, keep_traj=True,
                             combined=True, **kw).run()
    assert job.n == n and job.kernel_name() == all_name(1, given=True)
    ids = np.arange(R)
    o = {k: job.series(k, ids) for k in ('att', 'pos', 'vel', 'wb', 'ab')}
    o['pdiag_end'] = job.final_pdiag()
    o['scale_end'] = job.ctx.download(job.scalep.out_scale_end, (2, R)).T.copy()
    ratio = ls.ratios16(c, o, n - 1)
    job.release()
    for b in bufs.values():
        b.free()
    print('combined, %s: consistency ratios on the device:' % tag, np.array2string(ratio, precision=3))
    np.testing.assert_allclose(ratio, ls.CONSISTENCY_RATIOS[tag], rtol=0, atol=2e-3)


# ------------------------------------------------------------------------------------------------- 5. through Sim
def test_sim_runs_the_plugin_with_every_aid_next_to_the_plain_one(ctx):
    """IMU(axis=9, gps=True, odo=True) with [InsLoose(), InsLoose(every aid, combined=True)]: the combined plugin launches
    loose_all_kernel with 16 states; the Sim's kept sensor series of two runs, through the restatement with the flags of the Sim's
    truth and the Sim's field, give those runs of the plugin; 'odo_scale' is among the data; consistency_curve names the plugin and
    raises."""
    from demo_algorithms.ins_loose_device import InsLoose
    from ginsim import filter_model
    from gnss_ins_sim.sim import imu_model, ins_sim
    rf, geo = 1, [30.0, -3.0, 40.0]
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=9, gps=True, odo=True)
    imu.odo_err = dict(imu.odo_err, scale=0.99)
    algo = InsLoose(odo=True, nhc=True, odo_scale_state=True, mag=True, zupt=True, zaru=True, combined=True)
    assert algo.output[-1] == 'odo_scale' and algo.input[-2:] == ['odo', 'mag']
    sim = ins_sim.Sim([FS, FS_GPS, FS], sc.STOPS_CSV, ref_frame=rf, imu=imu, seed=1234, keep_trajectories=True, geo_mag_n=geo,
                      algorithm=[InsLoose(), algo])
    sim.run(65)
    d = sim.dmgr
    plain, aided = sim.mc.loose_names
    (_, job0, _), (_, job1, _) = sim.loose_jobs
    assert job0.kernel_name() == 'ginsim::loose_kernel<1, false, false, false>' and job0.allp is None
    assert job1.kernel_name() == all_name(1) and job1.allp is not None
    ini = __import__('ginsim').workloads.parse_motion(sc.STOPS_CSV)[0]
    model = filter_model(FS, imu.accel_err, imu.gyro_err, imu.gps_err)
    runs = [3, 64]
    accel, gyro, gps, odo, mag = (np.stack([np.asarray(src.data[r]) for r in runs]) for src in (d.accel, d.gyro, d.gps, d.odo, d.mag))
    stamps = np.rint(np.asarray(d.gps_time.data) * FS).astype(np.int64)
    args = (rf, FS, gyro, accel, ini, model, gps, stamps, np.asarray(d.gps_visibility.data))
    kw = dict(odo=odo, aid=dict(job1.aid), mag=mag, mag_model=job1.mag, scale=job1.scale, still=job1.still, flags=job1.still_flags)
    exp = aref.run(*args, **kw)
    bound = cs.parity_bound(*args, run=aref.run, deviation=ls.deviation, **kw)
    got = {k: np.stack([np.asarray(src.data['%s_%d' % (aided, r)]) for r in runs])
           for k, src in (('att', d.att_euler), ('pos', d.pos), ('vel', d.vel), ('wb', d.wb), ('ab', d.ab), ('k_est', d.odo_scale))}
    got['pdiag_end'] = job1.final_pdiag()[runs]
    got['scale_end'] = job1.ctx.download(job1.scalep.out_scale_end, (2, job1.runs)).T[runs]
    got['pcross_end'] = job1.final_pcross()[runs]
    held('parity Sim pairing', ls.deviation(got, exp), bound)
    assert np.all(np.abs(got['k_est'][:, -1] - 0.99) < 0.005)
    with pytest.raises(NotImplementedError, match='combined=True'):
        sim.consistency_curve(every=5.0)
