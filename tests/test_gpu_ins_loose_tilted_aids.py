"""GPU: the two newest InsLoose kernel families away from level.  loose_scale_kernel (the 16-state filter, csrc/ins_loose_scale.hip) runs
on tests/golden/ins_loose/motion_def_tilted.csv (41 S 150 W, yaw through +-180 deg twice, pitch 20 -> -20 -> 20 deg, roll -15 -> 15 -> -15
deg, climbing and descending) and on the table of 130 initial states of tests/ins_loose_sweep.py; loose_still_kernel (ZUPT and ZARU,
csrc/ins_loose_still.hip) on tests/golden/ins_loose/motion_def_tilted_stops.csv (41 S, parked twice on a slope at (170, 12, -10) deg
and (-160, -8, 5) deg, the second time inside a GPS outage, yaw through +-180 deg between the stops) and on the same table with every
vehicle parked.  Every other test of the two families runs a level profile at 32 N, where the terms of body_to_nav that sin(pitch),
sin(roll), a vertical velocity or the hemisphere multiply vanish: the rest rate w_rest = D (W cos lat, 0, -W sin lat) of the ZARU
innovation, the cross-covariances of state 15 with psi and dv, and the ini table path of both families.
tests/test_ins_loose_attitude_oracle.py holds the restatements these kernels are compared with to the nonlinear model (B5', B6') and
shows that a wrong rest rate moves wb on the new profile by far more than the bound below (B7').  Shapes: 65 runs x 800 / 960 samples
and 130 x 200 at 20 Hz; 1024 runs for the consistency.

Parity bound, as in the other InsLoose files: not a recorded constant.  Every comparison measures, on its own case, the float64
restatement against its np.longdouble evaluation and allows the device ins_loose_cases.PARITY_MARGIN (16) x that, per output: on the
profiles over the first 8 runs, on the tables over all 130 runs, since every run there is another attitude and one short run's largest
rounding error is too noisy a statistic (tests/test_gpu_ins_loose_attitude.py); the run-by-run figure is printed for information.

Measured on the MI355X (first run: all pass as written; largest deviation of the device from the restatement over both frames and
all cases of the line, and the smallest bound any of them allowed):
  loose_scale_kernel   tilted profile   att 5.2e-14 (1.5e-12)  pos 2.4e-14 in ref_frame 0 (2.0e-12), 1.9e-16 in ref_frame 1 (3.7e-14)
                                        vel 9.0e-13 (1.4e-11)  wb 4.0e-11 (1.7e-09)  ab 2.7e-11 (1.9e-09)  pdiag_end 3.5e-14 (1.3e-12)
                                        k_est 4.9e-14 (5.0e-12)  scale_end 4.9e-14 (5.0e-12)  pcross_end 2.5e-14 (1.1e-12)
                       table            att 4.2e-14 (2.1e-13)  pos 1.5e-15 (5.9e-14)  vel 6.2e-13 (4.1e-12)  wb 5.2e-11 (3.8e-10)
                                        ab 4.2e-11 (4.0e-10)  pdiag_end 1.8e-14 (2.7e-13)  k_est 1.1e-14 (5.3e-13)  scale_end 4.8e-14 (5.5e-13)
                                        pcross_end 2.0e-14 (1.4e-13)
  loose_still_kernel   tilted stops     att 8.4e-14 (5.6e-13)  pos 1.5e-15 (4.8e-14)  vel 4.5e-13 (2.1e-11)  wb 8.4e-12 (1.9e-10)
                                        ab 2.1e-12 (3.2e-10)  pdiag_end 1.3e-13 (5.7e-13)
                       earth_rot False  att 3.0e-14 (2.5e-11)  pos 2.6e-15 (2.1e-12)  vel 3.2e-13 (9.8e-10)  wb 5.1e-12 (1.5e-08)
                                        ab 1.6e-12 (7.6e-10)  pdiag_end 3.3e-14 (1.2e-11)
                       parked table     att 4.6e-14 (1.2e-13)  pos 4.1e-16 (6.5e-14)  vel 1.9e-13 (8.3e-13)  wb 1.1e-11 (3.2e-11)
                                        ab 2.2e-11 (6.5e-11)  pdiag_end 7.2e-15 (1.2e-13)
  On the tables single runs exceed 16 x their OWN run's error in 1e-11-sized entries (wb 3.9e-11 against 8.9e-12, scale_end 3.2e-14
  against 1.4e-14), as tests/test_gpu_ins_loose_attitude.py found for loose_mag_kernel: printed, not asserted.
  Every bit comparison holds (generated = given = a second launch; ini_first = 65 against runs 65-129; earth_rot in ref_frame 1).
  Parked table, ref_frame 0: the mean wb of the runs at 80 N and 80 S lie 0.11 of the largest |wb| apart, +W sin lat for -W sin lat
  moves them by 1.2 of it; the bound there is 4.9e-11.  Consistency: the restatement's ratios to the three recorded digits.
"""
import numpy as np
import pytest

import ins_loose_aided_cases as ac
import ins_loose_cases as cs
import ins_loose_dump
import ins_loose_ref as ref
import ins_loose_scale_cases as sc
import ins_loose_scale_ref as sref
import ins_loose_still_cases as stc
from ins_loose_dump import ctx, held, planes, result, same_bits
from ins_loose_sweep import FS, FS_GPS, SWEEP_N, SWEEP_RUNS, make_sweep, sweep, sweep_table
from oracle import ins_np

pytestmark = pytest.mark.gpu

RUNS = 65                                               # one wavefront plus one lane
ODO_ERR = {'scale': 0.985, 'stdv': sc.ODO_STDV}        # what the odometer of the scale-state cases reads; the filter starts from 1.0
HALF = np.arange(65, 130)


def wraps(yaw):
    """Indices j with a yaw wrap between samples j and j + 1 of a series (n,)."""
    return np.nonzero(np.abs(np.diff(yaw)) > np.pi)[0]


def run_by_run(what, dev, exp, hi, deviation, keys):
    """For information: each run against 16 x the restatement's own error on that run alone; the one closest to it, per output."""
    worst = {k: (0.0, 1.0, -1) for k in keys}
    for r in range(SWEEP_RUNS):
        one = lambda o: {k: o[k][r:r + 1] for k in keys}
        g, e = deviation(one(dev), one(exp)), deviation(one(exp), one(hi))
        for k in g:
            b = max(cs.PARITY_MARGIN * e[k], 1e-300)
            if g[k] / b > worst[k][0] / worst[k][1]:
                worst[k] = (g[k], b, r)
    print(what + ', run by run, closest to 16 x its own error: ' + ', '.join('%s %.2e (%.2e, run %d)' % ((k,) + worst[k]) for k in worst))


def upload(ctx, s, runs, odo=None):
    bufs = {k: ctx.upload(np.ascontiguousarray(s[k][runs].transpose(2, 1, 0))) for k in ('accel', 'gyro', 'gps')}
    if odo is not None:
        bufs['odo'] = ctx.upload(np.ascontiguousarray(odo[runs].T))
    return bufs


def free(bufs):
    for b in bufs.values():
        b.free()


# ================================================================================================= the scale-factor state
class ScaleDump(ins_loose_dump.Dump):
    """The tilted profile; the odometer of the dump reads ODO_ERR's scale."""

    def __init__(self, ctx, rf):
        super().__init__(ctx, rf, None, RUNS, fs=FS, fs_gps=FS_GPS, profile=cs.TILTED_CSV, odo_err=ODO_ERR)

    def job(self, ctx, mask, every=1, given=False, **kw):
        kw = dict(dict(keep_traj=True, keep_scale=True, odo_err=ODO_ERR, aid=ac.aid_options(mask, every), odo_scale_state={}), **kw)
        return super().job(ctx, given, **kw)

    def restate(self, mask, every=1):
        """The restatement of all runs and 16 x its own float64 error on the first 8."""
        kw = dict(odo=self.odo, aid=sc.aid(mask, every), scale=sc.scale())
        return sref.run(*self._args(), **kw), cs.parity_bound(*self._args(), run=sref.run, deviation=sc.deviation, **kw)


@pytest.fixture(scope='module', params=[0, 1], ids=['rf0', 'rf1'])
def scale_dump(request, ctx):
    d = ScaleDump(ctx, request.param)
    assert d.n == 800 and d.runs == RUNS
    yield d
    d.release()


# ------------------------------------------------------------------------------------------------- S1
@pytest.mark.parametrize('mask, every', [(1, 1), (7, 1), (7, 7)])
def test_scale_state_parity_on_the_tilted_profile(ctx, scale_dump, mask, every):
    d = scale_dump
    job = d.job(ctx, mask, every, given=True).run()
    assert job.kernel_name() == 'ginsim::loose_scale_kernel<%d, true, false, false>' % d.rf
    dev = result(job)
    job.release()
    assert wraps(d.truth['ref_att'][:, 0]).size == 2
    assert all(wraps(dev['att'][r, :, 0]).size >= 2 for r in range(RUNS))        # the estimate passes +-180 deg twice, as the truth
    exp, bound = d.restate(mask, every)
    assert set(bound) == set(sc.PARITY_KEYS)
    held('scale state, tilted parity rf%d mask %d every %d' % (d.rf, mask, every), sc.deviation(dev, exp), bound)
    assert np.all(np.abs(dev['k_est'][:, -1] - ODO_ERR['scale']) < np.abs(dev['k_est'][:, -1] - sc.SCALE0))      # it was learnt
    assert np.all(dev['scale_end'][:, 1] < sc.P0_SCALE ** 2)


# ------------------------------------------------------------------------------------------------- S2
def test_scale_state_generated_form_equals_given_form_bit_for_bit(ctx, scale_dump):
    d = scale_dump
    gen, giv = d.job(ctx, 7, 3).run(), d.job(ctx, 7, 3, given=True).run()
    assert gen.kernel_name() == 'ginsim::loose_scale_kernel<%d, false, false, false>' % d.rf
    assert giv.kernel_name() == 'ginsim::loose_scale_kernel<%d, true, false, false>' % d.rf
    a, b = planes(gen), planes(giv)
    assert {'scale', 'scale_end', 'pcross'} <= set(a)
    same_bits(a, b)
    assert np.ptp(a['scale'][-1]) > 0 and np.all(a['scale'][0] == sc.SCALE0)
    gen.release()
    giv.release()


# ------------------------------------------------------------------------------------------------- S3
def scale_sweep_job(ctx, s, bufs, runs, **kw):
    import ginsim
    return ginsim.InsLooseJob(ctx, FS, s['rf'], s['truth'], s['acc_e'], s['gyr_e'], cs.GPS_ERR, s['table'], runs, given=bufs, keep_traj=True,
                              keep_scale=True, odo_err=ODO_ERR, aid=ac.aid_options(7), odo_scale_state={}, **kw)


def test_scale_state_on_a_table_of_initial_states_in_one_launch(ctx, sweep):
    """Run r starts from row r of the table and has an odometer of its own truth speed: parity with the restatement given the same
    table, within 16 x the restatement's own float64 error on this case (all 130 runs); every output finite; and a second launch of 65
    runs with ini_first = 65 is runs 65-129 of the first, bit for bit."""
    s, rf = sweep, sweep['rf']
    odo = np.concatenate([ref.sample_odo(np.random.default_rng(600 + r), s['ref_odo'][r], ODO_ERR, 1) for r in range(SWEEP_RUNS)])
    assert odo.shape == (SWEEP_RUNS, SWEEP_N) and np.ptp(np.mean(s['ref_odo'], axis=1)) > 5.0
    bufs = upload(ctx, s, slice(None), odo)
    job = scale_sweep_job(ctx, s, bufs, SWEEP_RUNS).run()
    assert job.kernel_name() == 'ginsim::loose_scale_kernel<%d, true, false, false>' % rf
    dev, whole = result(job), planes(job)
    job.release()
    free(bufs)
    args = (rf, FS, s['gyro'], s['accel'], s['table'], s['model'], s['gps'], s['stamps'], s['truth']['gps_visibility'])
    kw = dict(odo=odo, aid=sc.aid(7), scale=sc.scale())
    exp, hi = sref.run(*args, **kw), sref.run(*args, dtype=np.longdouble, **kw)
    assert all(np.all(np.isfinite(dev[k])) for k in sc.PARITY_KEYS)
    got, err = sc.deviation(dev, exp), sc.deviation(exp, hi)
    run_by_run('scale state, sweep rf%d' % rf, dev, exp, hi, sc.deviation, sc.PARITY_KEYS)
    held('scale state, sweep rf%d' % rf, got, {k: cs.PARITY_MARGIN * err[k] for k in got})
    bufs = upload(ctx, s, HALF, odo)
    second = scale_sweep_job(ctx, s, bufs, 65, ini_first=65).run()
    same_bits(whole, planes(second), runs_a=HALF)
    second.release()
    free(bufs)


# ================================================================================================= the standstill block
class StillDump(ins_loose_dump.Dump):
    """The tilted stops profile, with the standstill signal of its truth in .flags."""

    def __init__(self, ctx, rf):
        super().__init__(ctx, rf, None, RUNS, fs=FS, fs_gps=FS_GPS, truth_fn=stc.stops_truth, profile=stc.TILTED_STOPS_CSV, flags=stc.flags_of)

    def job(self, ctx, smask, mask=0, every=1, given=False, **kw):
        """smask: the standstill rows (1 ZUPT, 2 ZARU, 3 both); None: no still argument at all.  mask 0: no aiding argument at all."""
        kw = ac.aid_kw(mask, **kw)
        if smask is not None:
            kw = dict(dict(still=stc.options(smask, every)), **kw)
        return super().job(ctx, given, **kw)

    def _kw(self, smask, mask, every, **kw):
        return dict(dict(odo=self.odo, aid=ac.aid(mask) if mask else None, still=stc.model(self.model, self.fs, smask, every), flags=self.flags),
                    **kw)

    def restate(self, smask, mask=0, every=1, **kw):
        return ref.run(*self._args(), **self._kw(smask, mask, every, **kw))

    def bound(self, smask, mask=0, every=1, **kw):
        return cs.parity_bound(*self._args(), **self._kw(smask, mask, every, **kw))


@pytest.fixture(scope='module', params=[0, 1], ids=['rf0', 'rf1'])
def still_dump(request, ctx):
    d = StillDump(ctx, request.param)
    assert d.n == 960 and d.runs == RUNS and stc.windows(d.flags) == [(180, 301), (600, 721)]
    yield d
    d.release()


# ------------------------------------------------------------------------------------------------- T1
@pytest.mark.parametrize('name, smask, mask, every', [('zupt', 1, 0, 1), ('zaru', 2, 0, 1), ('both', 3, 0, 1), ('both every 3', 3, 0, 3),
                                                      ('both with odo + nhc', 3, 7, 1)])
def test_standstill_parity_on_the_tilted_stops_profile(ctx, still_dump, name, smask, mask, every):
    """The generated form on the whole profile, 65 runs: att, pos, vel, wb, ab, pdiag_end."""
    d = still_dump
    both = [j for j in d.stamps[np.asarray(d.truth['gps_visibility']) != 0] if j > 0 and j % every == 0 and d.flags[j]]
    assert len(both) >= 3                                                      # fixes on flagged samples
    job = d.job(ctx, smask, mask, every).run()
    assert job.kernel_name() == 'ginsim::loose_still_kernel<%d, false, false, false>' % d.rf
    dev = result(job)
    job.release()
    held('standstill, tilted parity rf%d %s' % (d.rf, name), cs.deviation(dev, d.restate(smask, mask, every)), d.bound(smask, mask, every))
    plain = d.job(ctx, None, mask).run()
    other = result(plain)
    plain.release()
    first = stc.windows(d.flags)[0][0]
    assert first == 180 and first % every == 0                                 # the first sample a block fires at
    for k in ('att', 'pos', 'vel', 'wb', 'ab'):
        assert np.array_equal(other[k][:, :first], dev[k][:, :first]), k       # nothing before the first flagged sample
    k = 'vel' if smask & 1 else 'wb'
    assert not np.array_equal(other[k][:, first:], dev[k][:, first:])          # and the block did something after it


# ------------------------------------------------------------------------------------------------- T2
def test_standstill_without_earth_rotation(ctx, still_dump):
    """earth_rot = False, ZARU alone.  ref_frame 0: w_rest is zero; the launch is held to the restatement with earth_rot = False, and
    its wb differs from that of the launch with earth_rot = True on the same inputs.  ref_frame 1 has no earth rate at all: the two
    launches are the same bits."""
    d = still_dump
    off, on = d.job(ctx, 2, earth_rot=False).run(), d.job(ctx, 2).run()
    assert off.kernel_name() == 'ginsim::loose_still_kernel<%d, false, false, false>' % d.rf
    dev, a, b = result(off), planes(off), planes(on)
    off.release()
    on.release()
    if d.rf == 1:
        same_bits(a, b)
        return
    held('standstill, earth_rot = False rf0 zaru', cs.deviation(dev, d.restate(2, earth_rot=False)), d.bound(2, earth_rot=False))
    assert not np.array_equal(a['wb'][:, 181:], b['wb'][:, 181:])


# ------------------------------------------------------------------------------------------------- T3
@pytest.mark.parametrize('mask', [0, 7])
def test_standstill_generated_form_equals_given_form_and_two_launches_are_identical(ctx, still_dump, mask):
    d = still_dump
    gen, giv = d.job(ctx, 3, mask).run(), d.job(ctx, 3, mask, given=True).run()
    assert gen.kernel_name() == 'ginsim::loose_still_kernel<%d, false, false, false>' % d.rf
    assert giv.kernel_name() == 'ginsim::loose_still_kernel<%d, true, false, false>' % d.rf
    a = planes(gen)
    same_bits(a, planes(giv))
    again = d.job(ctx, 3, mask).run()
    same_bits(a, planes(again))
    for j in (gen, giv, again):
        j.release()


# ------------------------------------------------------------------------------------------------- T4
PARKED = ((1.0, 0, 0, 0, 0, 0, 0, SWEEP_N / FS, 1.0),)                       # 10 s of nothing: with a speed of zero, at rest


@pytest.fixture(scope='module', params=[0, 1], ids=['rf0', 'rf1'])
def parked(request):
    """The table of 130 initial states with the speed column zero: every run's truth is 10 s at rest from its row."""
    table = sweep_table()
    table[3] = 0.0
    s = make_sweep(request.param, table, PARKED)
    assert np.max(np.abs(s['ref_vel'])) == 0.0 and np.max(np.linalg.norm(s['ref_gyro'], axis=2)) <= ins_np.W_IE * (1 + 1e-9)
    return s


def still_sweep_job(ctx, s, bufs, runs, flags, **kw):
    import ginsim
    return ginsim.InsLooseJob(ctx, FS, s['rf'], s['truth'], s['acc_e'], s['gyr_e'], cs.GPS_ERR, s['table'], runs, given=bufs, keep_traj=True,
                              still=dict(stc.options(3), flags=flags), **kw)


def turned_rest_rate(f):
    """LooseFilter.rest_rate with +W sin lat for -W sin lat: D (W cos lat, 0, +W sin lat)."""
    return ref.LooseFilter.rest_rate(f) + f.D[:, :, 2] * (2 * ins_np.W_IE * np.sin(f.pos[:, 0]))[:, None]


def test_standstill_on_a_table_of_parked_vehicles(ctx, parked):
    """130 vehicles parked at the table's attitudes and latitudes, every sample flagged, ZUPT and ZARU: parity with the restatement
    within 16 x its own float64 error on this case (all 130 runs); a launch of 65 runs with ini_first = 65 is runs 65-129, bit for bit.
    ref_frame 0: the hemisphere matters here -- the bias the ZARU rows learn differs between the northernmost and the southernmost
    run by more than the bound, and with the sign of W sin lat turned the restatement of those two runs leaves it by far."""
    s, rf = parked, parked['rf']
    flags = np.ones(SWEEP_N, dtype=np.int32)
    bufs = upload(ctx, s, slice(None))
    job = still_sweep_job(ctx, s, bufs, SWEEP_RUNS, flags).run()
    assert job.kernel_name() == 'ginsim::loose_still_kernel<%d, true, false, false>' % rf
    dev, whole = result(job), planes(job)
    job.release()
    free(bufs)
    args = (rf, FS, s['gyro'], s['accel'], s['table'], s['model'], s['gps'], s['stamps'], s['truth']['gps_visibility'])
    kw = dict(still=stc.model(s['model'], FS, 3), flags=flags)
    exp, hi = ref.run(*args, **kw), ref.run(*args, dtype=np.longdouble, **kw)
    assert all(np.all(np.isfinite(dev[k])) for k in cs.PARITY_KEYS)
    got, err = cs.deviation(dev, exp), cs.deviation(exp, hi)
    bound = {k: cs.PARITY_MARGIN * err[k] for k in got}
    run_by_run('standstill, parked sweep rf%d' % rf, dev, exp, hi, cs.deviation, cs.PARITY_KEYS)
    held('standstill, parked sweep rf%d' % rf, got, bound)
    bufs = upload(ctx, s, HALF)
    second = still_sweep_job(ctx, s, bufs, 65, flags, ini_first=65).run()
    same_bits(whole, planes(second), runs_a=HALF)
    second.release()
    free(bufs)
    if rf == 0:
        lat = s['table'][0]
        north, south = int(np.argmax(lat)), int(np.argmin(lat))
        assert np.rad2deg(lat[north]) == pytest.approx(80.0) and np.rad2deg(lat[south]) == pytest.approx(-80.0)
        scale = np.max(np.abs(exp['wb']))                                      # cs.deviation's metric of wb
        apart = np.max(np.abs(np.mean(exp['wb'][north], axis=0) - np.mean(exp['wb'][south], axis=0))) / scale
        two = [north, south]
        turned = type('TurnedHemisphere', (ref.LooseFilter,), {'rest_rate': turned_rest_rate})
        args2 = (rf, FS, s['gyro'][two], s['accel'][two], s['table'][:, two], s['model'], s['gps'][two], s['stamps'], s['truth']['gps_visibility'])
        wrong = ref.run(*args2, filt=turned(rf, FS, s['table'][:, two], 2, s['model']), **kw)
        moved = np.max(np.abs(wrong['wb'] - exp['wb'][two])) / scale
        print('standstill, parked sweep rf0: mean wb of run %d (80 N) and run %d (80 S) apart by %.2e, +W sin lat moves them by %.2e (bound %.2e)'
              % (north, south, apart, moved, bound['wb']))
        assert apart > bound['wb'] and moved > 100.0 * bound['wb']


# ================================================================================================= C consistency on the tilted profiles
def test_scale_state_consistency_on_the_tilted_profile(ctx):
    """ref_frame 1, 1024 x 800, the odometer row alone, every run with a true scale of its own ~ N(1, 0.02^2): for every one of the 16
    states the RMS end error over sqrt(mean P_kk) lies within x/: 1.25 of the ratio the restatement gave on the same draw
    (ins_loose_scale_cases.CONSISTENCY_BY_PROFILE; the 1 sigma of an RMS over 1024 runs is 2.2 %, plus correlation)."""
    import ginsim
    d = sc.draws(cs.CONSISTENCY_RUNS, cs.CONSISTENCY_SEED, profile=cs.TILTED_CSV)
    R, odo = cs.CONSISTENCY_RUNS, sc.odometer(d)
    bufs = {'accel': ctx.upload(np.ascontiguousarray(d['accel'].transpose(2, 1, 0))), 'gyro': ctx.upload(np.ascontiguousarray(d['gyro'].transpose(2, 1, 0))),
            'gps': ctx.upload(np.ascontiguousarray(d['gps'].transpose(2, 1, 0))), 'odo': ctx.upload(np.ascontiguousarray(odo.T))}
    job = ginsim.InsLooseJob(ctx, d['fs'], 1, d['truth'], d['acc_e'], d['gyr_e'], cs.GPS_ERR, d['ini'], R, given=bufs, keep_traj=True,
                             odo_err={'scale': 1.0, 'stdv': sc.ODO_STDV}, aid=ac.aid_options(1), odo_scale_state={}).run()
    assert job.n == 800 and job.kernel_name() == 'ginsim::loose_scale_kernel<1, true, false, false>'
    ids = np.arange(R)
    o = {k: job.series(k, ids) for k in ('att', 'pos', 'vel')}
    wb, ab = job.final_biases()
    o['wb'], o['ab'] = wb[:, None], ab[:, None]
    k_end, sigma = job.final_scale()
    o['pdiag_end'], o['scale_end'] = job.final_pdiag(), np.stack([k_end, sigma ** 2], axis=1)
    job.release()
    free(bufs)
    ratio, want = sc.ratios16(d, o, d['scales']), np.array(sc.CONSISTENCY_BY_PROFILE['tilted'])
    print('scale state, tilted profile: consistency ratios on the device, 16 states:', np.array2string(ratio, precision=3))
    assert np.all(want >= sc.CONSISTENCY_BAND[0]) and np.all(want <= sc.CONSISTENCY_BAND[1])
    assert np.all(ratio <= want * 1.25) and np.all(ratio >= want / 1.25), ratio / want


@pytest.mark.parametrize('tag', ['stop', 'end'])
def test_standstill_consistency_on_the_tilted_stops_profile(ctx, tag):
    """ref_frame 1, 1024 runs, both rows: for every state the RMS error over sqrt(mean pdiag_end) lies within x/: 1.25 of the ratio the
    restatement gave on the same draw (ins_loose_still_cases.CONSISTENCY_BY_PROFILE), at the last sample of the first stop (the
    profile and the draws cut there) and at the profile's end."""
    import ginsim
    R = cs.CONSISTENCY_RUNS
    c = stc.consistency_draw(1, cs.CONSISTENCY_FS, R, profile=stc.TILTED_STOPS_CSV)
    n = stc.windows(c['flags'])[0][1] + 1 if tag == 'stop' else c['truth']['ref_accel'].shape[0]
    ini, truth, stamps = stc.stops_truth(cs.CONSISTENCY_FS, 1, cs.CONSISTENCY_FS_GPS, n, stc.TILTED_STOPS_CSV)
    m = stamps.size
    bufs = {'accel': ctx.upload(np.ascontiguousarray(c['accel'][:, :n].transpose(2, 1, 0))),
            'gyro': ctx.upload(np.ascontiguousarray(c['gyro'][:, :n].transpose(2, 1, 0))),
            'gps': ctx.upload(np.ascontiguousarray(c['gps'][:, :m].transpose(2, 1, 0)))}
    job = ginsim.InsLooseJob(ctx, cs.CONSISTENCY_FS, 1, truth, c['acc_e'], c['gyr_e'], cs.GPS_ERR, ini, R, given=bufs, keep_traj=True, still={}).run()
    assert job.n == n == (302 if tag == 'stop' else 960) and job.kernel_name() == 'ginsim::loose_still_kernel<1, true, false, false>'
    assert np.array_equal(job.still_flags, c['flags'][:n])
    ids = np.arange(R)
    o = {k: job.series(k, ids) for k in ('att', 'pos', 'vel', 'wb', 'ab')}
    ratio = stc.ratios(stc.error_at(c, o, n - 1), job.final_pdiag())
    job.release()
    free(bufs)
    want = np.array(stc.CONSISTENCY_BY_PROFILE['tilted']['still'][tag])
    print('standstill, tilted stops, %s: consistency ratios on the device:' % tag, np.array2string(ratio, precision=3))
    assert np.all(ratio <= want * 1.25) and np.all(ratio >= want / 1.25), ratio / want
