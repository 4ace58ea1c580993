"""GPU: consistency checkpoints for every InsLoose family (csrc/ins_loose_all_cons.hip, InsLooseJob(checkpoints=..., scale_truth=...),
Sim.consistency_curve_any_family()) against their NumPy restatement (tests/ins_loose_all_cons_ref.py), against the launch without
checkpoints, against cons_samples= where both exist and against the recorded ratios of the combined filter.  Shapes: the stops
profile at 20 Hz cut to 300-1100 samples, 65 runs (1-129 around a wavefront, 1024 for the ratios).  Every test passes checkpoints=
or calls consistency_curve_any_family, which the package without the family does not take.

Parity bound, DESIGN 4.11c's rule.  Not a recorded constant: every comparison with the restatement evaluates, on its own case and ALL
its runs (the device's dumped sensors, fixes, odometer and magnetometer), the float64 restatement against its np.longdouble
evaluation and allows the device ins_loose_cases.PARITY_MARGIN (16) x that, column by column of the record's 43; a deviation is
relative to the column's largest value over the case's checkpoints (ins_loose_all_cons_ref.deviation).  The count column is exact.
The run-count cases add the order of the sum over the runs to it; the comment at TAIL_SAMPLES has the reasoning and the figures of
the two runs in which the 129-run case missed the rule as it stands.

Measured on the MI355X (52 tests, 31 s).  Parity, 16 cases: the device's largest deviation in any column 3.1e-12 ... 3.3e-11 where the
restatement's own is 2.2e-8 ... 2.0e-7; the tightest column of every case a bias variance P_dba, 1.0e-14 against bounds of 2.5e-14 ...
3.1e-14; no case uses more than 0.40 of a bound.  Run counts: the largest use of the bound is 0.63 (129 runs, nes_psi_z 4.5e-14 of
7.1e-14).  Every bit comparison holds.  The ratios of the 1024-run launch are the table's to its three digits at both instants.
Launch times: profiles/ins_loose_all_cons_timing.json."""
import itertools

import numpy as np
import pytest

import ins_loose_all_cases as ls
import ins_loose_all_cons_ref as acons
import ins_loose_cases as cs
import ins_loose_mag_cases as mc
import ins_loose_still_cases as sc
from ins_loose_cons_dump import COLUMNS, nav_of, record
from ins_loose_dump import ctx, planes, same_bits
from test_gpu_ins_loose_all import ALL, Dump, all_name

pytestmark = pytest.mark.gpu

FS = 20.0
SUBSETS = [w for k in range(4) for w in itertools.combinations(ALL, k)]
IDS = ['+'.join(w) or 'none' for w in SUBSETS]
COLS = COLUMNS + ['P_scale', 'e2_scale', 'nes_scale', 'zero_40', 'zero_41', 'zero_42']
NAME = 'ginsim::loose_all_cons_kernel<%d, %s, false, %d>'


def cons_name(rf, which, given=False):
    return NAME % (rf, str(given).lower(), 16 if 'scale' in which else 15)


def restated(d, which, samples, mask=ls.MASK, every=1, flags=None, runs=None, accel=None, dtype=np.float64, scale_truth=None, q=0.0):
    """The restatement's record of Dump d over `runs` (None: all) at `samples`.  q: the scale state's random walk [1/sqrt(s)]."""
    r = np.arange(d.runs) if runs is None else np.asarray(runs)
    kw = ls.blocks(d.model, d.fs, d.rf, **d._case(which, mask, every, d.flags if flags is None else flags, q))
    kw.update(odo=d.odo[r], mag=d.mag['m'][r] if 'mag' in which else None)
    if scale_truth is not None and np.ndim(scale_truth):
        scale_truth = np.asarray(scale_truth)[r]
    acc = d.accel if accel is None else accel
    with np.errstate(all='ignore'):
        return acons.run(d.rf, d.fs, d.gyro[r], acc[r], d.ini, d.model, nav_of(d.truth), samples, d.gps[r], d.stamps, d.truth['gps_visibility'],
                         dtype=dtype, scale_truth=scale_truth if 'scale' in which else None, **kw)


def cons_held(what, dev, d, which, samples, order=False, **kw):
    """Assert the device record dev (m, 43) against the restatement within 16 x the restatement's own float64 error; print both.
    order: the run-count cases (see TAIL_SAMPLES) add what the ORDER of a sum of R non-negative doubles can move it by."""
    lo, hi = restated(d, which, samples, **kw), restated(d, which, samples, dtype=np.longdouble, **kw)
    own = acons.deviation(lo, hi)
    bound = cs.PARITY_MARGIN * own
    if order:
        bound = np.where(own > 0, bound + (int(lo[:, 0].max()) - 1) * np.finfo(np.float64).eps, bound)
    got = acons.deviation(dev, lo)
    worst = int(np.argmax(got / np.maximum(bound, 1e-300)))
    print('%s rf%d %s: restatement f64 - long double: largest %.2e; device: largest deviation %.2e, tightest column %s %.2e (bound %.2e)'
          % (what, d.rf, '+'.join(which) or 'none', own.max(), got.max(), COLS[worst], got[worst], bound[worst]))
    assert not dev[:, 40:].any() and ('scale' in which or not dev[:, 37:].any())
    assert np.array_equal(dev[:, 0], lo[:, 0])
    for k in range(43):
        assert got[k] <= bound[k], (what, COLS[k], got[k], bound[k])
    return lo


@pytest.fixture(scope='module', params=[0, 1], ids=['rf0', 'rf1'])
def dump(request, ctx):
    d = Dump(ctx, request.param, ls.SCHEDULE_N, 65, seed=41)   # 30 s: the first stop, the turn, 3 s into the outage
    yield d
    d.release()


def held_job(d, ctx, which, **kw):
    """The job of Dump d with the blocks `which` (combined=True: what two blocks need and one does not notice)."""
    if 'scale' in which and kw.get('given') and 'scale_truth' not in kw:
        kw['scale_truth'] = ls.READS
    return d.job(ctx, which, **kw)


# ------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize('which', SUBSETS, ids=IDS)
def test_parity_with_the_restatement(ctx, dump, which):
    """The given form, a period of its own per block (ins_loose_all_cases.SCHEDULE): checkpoints at the first two samples, at a sample
    where a fix, the aiding, the magnetometer and the standstill block all fire, and at the last two."""
    n = dump.n
    fires = ls.schedule(n, ls.SCHEDULE, dump.stamps, dump.truth['gps_visibility'], dump.flags)
    everything = ls.FIX | ls.AID | ls.MAG | ls.STILL
    for bit in (ls.AID, ls.MAG, ls.STILL):
        assert np.any(fires & (ls.FIX | bit) == (ls.FIX | bit))            # every block fires on a fix's sample at least once
    meet = int(np.nonzero(fires == everything)[0][0])
    samples = [0, 1, meet, n - 2, n - 1]
    job = held_job(dump, ctx, which, every=ls.SCHEDULE, given=True, checkpoints=samples, keep_traj=False).run()
    assert job.kernel_name() == cons_name(dump.rf, which, given=True)
    res = job.consistency()
    dev = res.pack()
    job.release()
    lo = cons_held('parity', dev, dump, which, samples, every=ls.SCHEDULE, scale_truth=ls.READS)
    assert np.all(res.count == 65) and res.ratio.shape == (5, 9) and res.pbar.shape == (5, 15) and res.ratio_scale.shape == (5,)
    np.testing.assert_allclose(res.sigma, np.sqrt(lo[:, 1:16] / 65), rtol=1e-9)
    if 'scale' in which:
        assert np.all(res.pbar_scale > 0) and np.all(res.e2_scale > 0) and res.sigma_scale[-1] < 0.5 * res.sigma_scale[0]
        np.testing.assert_allclose(res.ratio_scale, np.sqrt(lo[:, 38] / lo[:, 37]), rtol=1e-9)


# ------------------------------------------------------------------------------------------------- 2. the checkpoint perturbs nothing
@pytest.mark.parametrize('which', SUBSETS, ids=IDS)
def test_same_bits_with_and_without_checkpoints(ctx, dump, which):
    """A checkpoint at every sample against the launch without checkpoints (the single family's kernel, or loose_all_kernel): every
    kept series and every end record bit for bit; the dense record at the samples of a sparse one; two launches."""
    n = dump.n
    plain = dump.job(ctx, which, every=2).run()
    assert '_cons_' not in plain.kernel_name()
    assert plain.kernel_name() == (all_name(dump.rf, ns=16 if 'scale' in which else 15) if len(which) >= 2 else
                                   'ginsim::loose_%s_kernel<%d, false, false, false>' % (which[0] if which else 'aided', dump.rf))
    want, sig = planes(plain), plain.final_sigmas()
    plain.release()
    every = dump.job(ctx, which, every=2, checkpoints=range(n)).run()
    assert every.kernel_name() == cons_name(dump.rf, which)
    same_bits(planes(every), want)          # traj, wb, ab, the end record, pdiag_end, biases; k_est, scale_end, pcross_end with 16 states
    assert np.array_equal(every.final_sigmas().view(np.uint64), sig.view(np.uint64))
    dense = record(every)
    again = record(every.run())
    assert np.array_equal(dense.view(np.uint64), again.view(np.uint64))
    every.release()
    sparse_at = [0, 7, 64, 333, n - 2, n - 1]
    sparse = dump.job(ctx, which, every=2, checkpoints=sparse_at, keep_traj=False).run()
    got = record(sparse)
    sparse.release()
    assert np.array_equal(got.view(np.uint64), dense[sparse_at].view(np.uint64)) and np.all(dense[:, 0] == 65)


# ------------------------------------------------------------------------------------------------- 3. the record of cons_samples=
@pytest.mark.parametrize('mask', [0, 7])
def test_without_a_block_the_record_is_that_of_cons_samples_bit_for_bit(ctx, dump, mask):
    samples = [0, 1, 10, 333, dump.n - 2, dump.n - 1]
    new = dump.job(ctx, (), mask=mask, every=3, checkpoints=samples, keep_traj=False).run()
    old = dump.job(ctx, (), mask=mask, every=3, cons_samples=samples, keep_traj=False, combined=None).run()
    assert new.kernel_name() == cons_name(dump.rf, ())
    assert old.kernel_name() == 'ginsim::loose_cons_kernel<%d, false, false, %s>' % (dump.rf, 'true' if mask else 'false')
    a, b = record(new), record(old)
    new.release()
    old.release()
    assert a[:, 0].min() == 65 and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ------------------------------------------------------------------------------------------------- 4. generated = given
@pytest.mark.parametrize('which', [(), ('mag', 'still'), ALL], ids=['none', 'mag+still', 'all'])
def test_generated_form_equals_given_form_bit_for_bit(ctx, dump, which):
    """The generated form's truth of the scale factor is its own odometer's scale (odo_err['scale']); the given form is told it."""
    samples = [0, 1, 10, 333, dump.n - 1]
    gen = dump.job(ctx, which, every=2, checkpoints=samples, keep_traj=False).run()
    giv = held_job(dump, ctx, which, every=2, given=True, checkpoints=samples, keep_traj=False).run()
    assert (gen.kernel_name(), giv.kernel_name()) == (cons_name(dump.rf, which), cons_name(dump.rf, which, given=True))
    a, b = record(gen), record(giv)
    gen.release()
    giv.release()
    assert a[:, 0].min() == 65 and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert ('scale' in which) == bool(a[:, 38].any())


# ------------------------------------------------------------------------------------------------- 5. tail lanes, run lists
# A column's bound is 16 x the MAX over the checkpoints of the restatement's own deviation.  With [0, 150, 299] (the list of
# tests/test_gpu_ins_loose_cons.py) two checkpoints carry an error at all -- every run sits on the truth at sample 0 -- and one
# fortunate cancellation in a sum over the runs sets the bound: on the first run on an MI355X the 129-run case had e2_dv_y at 1.24e-14
# against a bound of 8.4e-15, the float64 restatement lying within 5.2e-16 (2.4 ulp) of its long-double evaluation there, while the same
# column of the 65-run case had 1.37e-14 against 4.2e-14.  The list is longer since, so that the maximum is taken over nine
# checkpoints and both sides of the comparison see more of the run.  On the second run the same case had nes_psi_y at 2.66e-14 against
# 1.78e-14 (the restatement within 1.1e-15 of its long-double evaluation; the 63-, 64- and 65-run cases 3.8e-14 against 8e-14 in the
# sister column e2_psi_x); every other column of every case held.
# What the rule does not measure: both evaluations of the restatement add the R runs in NumPy's order; the device adds them in the
# butterfly's order within a wavefront and the wavefronts ascending.  Every column is a sum of R non-negative terms (P_kk, e^2,
# e^2 / P_kk, a positive definite form), and two orders of such a sum differ by at most (R - 1) eps of it.  The run-count cases, whose
# subject is which lanes enter the sums and with what weight (a lane lost or counted twice moves a sum by the order of 1 / R), allow
# that on top: 16 x the restatement's own deviation + (R - 1) eps, column by column (1.78e-14 + 2.84e-14 for the column above).
# The parity cases of section 1 and the non-finite run keep the rule as it stands.
TAIL_SAMPLES = [0, 1, 50, 100, 150, 200, 250, 298, 299]


def tail_flags(d):
    flags = np.array(d.flags, dtype=np.int32)
    flags[100:160] = 1                      # constructed: parity does not need the signal to be physical
    return flags


@pytest.mark.parametrize('runs', [1, 63, 64, 65, 129])
def test_run_counts_around_a_wavefront(ctx, runs):
    d = Dump(ctx, 1, 300, runs, seed=21)
    flags = tail_flags(d)
    truth = ls.READS + 1e-3 * np.arange(runs)                                   # a truth per run: the run id indexes it, not the lane
    job = d.job(ctx, ALL, every=2, given=True, flags=flags, checkpoints=TAIL_SAMPLES, scale_truth=truth, keep_traj=False).run()
    dev = record(job)
    assert np.all(dev[:, 0] == runs)
    cons_held('%d runs' % runs, dev, d, ALL, TAIL_SAMPLES, order=True, every=2, flags=flags, scale_truth=truth)
    if runs == 129:                                         # 40 scattered runs of the 129: the record is over the listed runs
        ids = np.random.default_rng(3).permutation(129)[:40]
        part = record(job.run(ids))
        assert np.all(part[:, 0] == 40)
        cons_held('40 of 129 runs', part, d, ALL, TAIL_SAMPLES, order=True, every=2, flags=flags, scale_truth=truth, runs=ids)
    job.release()
    d.release()


def test_a_non_finite_run_is_left_out_of_every_sum(ctx):
    n, bad_run = 300, 33
    d = Dump(ctx, 1, n, 65, seed=51)
    flags = tail_flags(d)
    samples = [50, 100, 101, 200, 299]
    acc = ctx.download(d.mc.buffer('accel'), (3, n, 65))
    acc[1, 100:, bad_run] = np.nan                          # enters the state with the step from sample 100 to 101
    bad = ctx.upload(acc)
    job = d.job(ctx, ALL, every=2, given=True, flags=flags, checkpoints=samples, scale_truth=ls.READS, keep_traj=False)
    job.mc.in_accel = bad.ptr
    dev = record(job.run())
    job.release()
    bad.free()
    assert list(dev[:, 0]) == [65, 65, 64, 64, 64] and np.all(np.isfinite(dev))
    host = d.accel.copy()
    host[bad_run, 100:, 1] = np.nan
    cons_held('non-finite run, all runs', dev, d, ALL, samples, every=2, flags=flags, scale_truth=ls.READS, accel=host)
    keep = np.setdiff1d(np.arange(65), [bad_run])
    cons_held('non-finite run, the others', dev[2:], d, ALL, samples[2:], every=2, flags=flags, scale_truth=ls.READS, runs=keep)
    d.release()


# ------------------------------------------------------------------------------------------------- 6. the last checkpoint
def test_the_last_checkpoint_is_the_end_record(ctx, dump):
    n = dump.n
    job = held_job(dump, ctx, ALL, every=2, given=True, checkpoints=[n - 1]).run()
    rec = record(job)[0]
    sig2 = job.final_sigmas() ** 2
    k_est = job.series('odo_scale', np.arange(65))[:, n - 1]
    job.release()
    assert rec[0] == 65 and sig2.shape == (65, 16)
    np.testing.assert_allclose(rec[1:16] / 65, sig2[:, :15].mean(axis=0), rtol=1e-14, atol=0)
    np.testing.assert_allclose(rec[37] / 65, sig2[:, 15].mean(), rtol=1e-14, atol=0)
    want = np.sum((k_est - ls.READS) ** 2)
    print('sum of (k_est - k)^2 at the last sample: record %.17g, from the kept series %.17g' % (rec[38], want))
    np.testing.assert_allclose(rec[38], want, rtol=64 * np.finfo(np.float64).eps, atol=0)      # a 65-term sum in another order
    blind = dump.job(ctx, ALL, every=2, given=True, checkpoints=[n - 1], keep_traj=False).run()    # the given form has no truth of its own
    got = record(blind)[0]
    blind.release()
    assert got[38] == 0.0 and got[39] == 0.0 and np.array_equal(got[:38].view(np.uint64), rec[:38].view(np.uint64))


# ------------------------------------------------------------------------------------------------- 7. the recorded ratios
def test_one_launch_gives_the_recorded_ratios_at_both_instants(ctx):
    """ins_loose_all_cases.consistency_draw, 1024 runs, every block, the true scale of every run as scale_truth: the ratios at the
    last sample of the first stop and at the profile's end are CONSISTENCY_RATIOS' (the nine navigation states, and ratio_scale
    against entry 15) to the 2e-3 the CPU test holds the table to -- one launch, nothing kept."""
    import ginsim
    R = cs.CONSISTENCY_RUNS
    c = ls.consistency_draw(1, cs.CONSISTENCY_FS, R)
    n = c['truth']['ref_accel'].shape[0]
    at = [sc.windows(c['flags'])[0][1], n - 1]
    bufs = {'accel': ctx.upload(np.ascontiguousarray(c['accel'].transpose(2, 1, 0))), 'gyro': ctx.upload(np.ascontiguousarray(c['gyro'].transpose(2, 1, 0))),
            'gps': ctx.upload(np.ascontiguousarray(c['gps'].transpose(2, 1, 0))), 'odo': ctx.upload(np.ascontiguousarray(c['odo'].T)),
            'mag': ctx.upload(np.ascontiguousarray(c['mag'].transpose(2, 1, 0)))}
    kw = ls.job_kw(ls.CONSISTENCY_MASK, mc.MAG_ERR, True, 3, keep=False)
    job = ginsim.InsLooseJob(ctx, cs.CONSISTENCY_FS, 1, c['truth'], c['acc_e'], c['gyr_e'], cs.GPS_ERR, c['ini'], R, given=bufs, combined=True,
                             checkpoints=at, scale_truth=c['scales'], **kw).run()
    assert job.kernel_name() == cons_name(1, ALL, given=True)
    res = job.consistency()
    job.release()
    for b in bufs.values():
        b.free()
    assert np.all(res.count == R)
    for k, tag in enumerate(('stop', 'end')):
        print('combined, %s: ratios on the device' % tag, np.array2string(res.ratio[k], precision=3), 'scale %.3f' % res.ratio_scale[k],
              'nees', np.array2string(res.nees[k], precision=3))
    for k, tag in enumerate(('stop', 'end')):
        np.testing.assert_allclose(res.ratio[k], ls.CONSISTENCY_RATIOS[tag][:9], rtol=0, atol=2e-3)
        np.testing.assert_allclose(res.ratio_scale[k], ls.CONSISTENCY_RATIOS[tag][15], rtol=0, atol=2e-3)


# ------------------------------------------------------------------------------------------------- 8. through Sim
def test_sim_consistency_curve_of_any_family(ctx):
    """Sim.consistency_curve_any_family() is the job-level record for the plain plugin, for each single-aid plugin and for the
    combined one; the scale-state plugins have 'scale' against the Sim's odometer scale; consistency_curve keeps its refusals."""
    from demo_algorithms.ins_loose_device import InsLoose
    from ginsim import InsLooseJob, filter_model, workloads
    from gnss_ins_sim.sim import imu_model, ins_sim
    rf, R, geo, fs_gps = 1, 65, [30.0, -3.0, 40.0], 2.0
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=9, gps=True, odo=True)
    imu.odo_err = dict(imu.odo_err, scale=0.99)
    algos = [InsLoose(), InsLoose(mag=True, mag_every=3), InsLoose(odo=True, odo_scale_state=True), InsLoose(zupt=True, zaru=True, still_every=2),
             InsLoose(odo=True, nhc=True, odo_scale_state=True, mag=True, zupt=True, zaru=True, combined=True)]
    sim = ins_sim.Sim([FS, fs_gps, FS], sc.STOPS_CSV, ref_frame=rf, imu=imu, seed=1234, keep_trajectories=False, geo_mag_n=geo, algorithm=algos)
    sim.run(R)
    names = sim.mc.loose_names
    with pytest.raises(NotImplementedError, match='not built'):
        sim.consistency_curve(every=5.0)
    curve = sim.consistency_curve_any_family(every=5.0)
    n = np.asarray(sim.dmgr.time.data).shape[0]
    samples = np.arange(0, n, 100)
    assert np.array_equal(curve['time'], samples / FS) and set(curve) == {'time', 'states'} | set(names)
    d = sim.dmgr
    truth = {'ref_accel': d.ref_accel.data, 'ref_gyro': d.ref_gyro.data, 'ref_pos': d.ref_pos.data, 'ref_vel': d.ref_vel.data,
             'ref_att': d.ref_att_euler.data, 'ref_odo': d.ref_odo.data, 'ref_mag': d.ref_mag.data, 'ref_gps': d.ref_gps.data,
             'gps_time': d.gps_time.data, 'gps_visibility': d.gps_visibility.data}
    ini = workloads.parse_motion(sc.STOPS_CSV)[0]
    for name, algo in zip(names, algos):
        kw = {}
        if algo.aid() is not None:
            kw.update(odo_err=imu.odo_err, aid=algo.aid())
        if algo.mag_options() is not None:
            kw.update(mag_err=imu.mag_err, geo_mag_n=geo, mag=algo.mag_options())
        if algo.scale_options() is not None:
            kw.update(odo_scale_state=algo.scale_options())
        if algo.still_options() is not None:
            kw.update(still=algo.still_options())
        job = InsLooseJob(ctx, FS, rf, truth, imu.accel_err, imu.gyro_err, imu.gps_err, ini, R, seed=1234, earth_rot=algo.earth_rot,
                          model=filter_model(FS, imu.accel_err, imu.gyro_err, imu.gps_err, algo.q_scale, algo.p0), checkpoints=samples,
                          combined=algo.combined, **kw).run()
        want = job.consistency()
        job.release()
        got = curve[name]
        assert np.all(got['count'] == R), name
        for key, exp in (('count', want.count), ('sigma', want.sigma), ('rms', want.rms), ('ratio', want.ratio), ('nees', want.nees)):
            assert np.array_equal(got[key], exp), (name, key)
        assert ('scale' in got) == algo.odo_scale_state, name
        if algo.odo_scale_state:
            for key, exp in (('sigma', want.sigma_scale), ('rms', want.rms_scale), ('ratio', want.ratio_scale)):
                assert got['scale'][key].shape == (samples.size,) and np.array_equal(got['scale'][key], exp), (name, key)
            assert got['scale']['sigma'][0] == pytest.approx(0.02, rel=1e-12) and got['scale']['rms'][0] == pytest.approx(0.01, rel=1e-12)  # |1.0 - 0.99|
            assert got['scale']['sigma'][-1] < 0.005
    some = sim.consistency_curve_any_family(samples=[n - 1, 0])         # samples= in any order
    assert some[names[-1]]['sigma'].shape == (2, 15) and some[names[-1]]['scale']['sigma'].shape == (2,)
    assert np.array_equal(some[names[-1]]['sigma'][1], curve[names[-1]]['sigma'][0])
