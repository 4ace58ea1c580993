"""GPU: what tests/test_gpu_ins_loose_all.py leaves open of InsLoose with all its aids in one launch (csrc/ins_loose_all.hip,
csrc/ins_loose_all16.hip; loose_body and loose_propagate of csrc/ins_loose.hpp): a period of its own for every block, the aiding masks
next to the other blocks, a block that fires on the last stored row only, the scale state's random walk q_k > 0 (also on
loose_scale_kernel), every one of the 24 instantiations, and non-finite aids in the combined given form.  CPU side:
tests/test_ins_loose_all_schedule_oracle.py.

Shapes: the schedule case of ins_loose_all_cases (the first 600 samples of the stops profile at 20 Hz with 2 Hz GPS, aid / mag / still
every 4 / 3 / 5 samples and with the roles rotated, 5 / 4 / 3; schedule_flags) with 65 runs, one wavefront plus one lane; 400 (and 401)
samples with 65 runs where only bits are compared; three runs through Sim.

Parity bound, as tests/test_gpu_ins_loose_all.py: not a recorded constant.  Every comparison with the restatement
(tests/ins_loose_all_ref.py) measures, on its own case (the device's dumped sensors, the first 8 runs), the float64 restatement against
its np.longdouble evaluation and allows the device ins_loose_cases.PARITY_MARGIN (16) x that, per output.

One reading is this file's own.  The period edge "period n - 1 on n samples equals the longer series cut back" is held as: the SAME
period n - 1 on a series of n + 1 samples (the block then fires on the row before the last) gives, in its first n rows, the bits of the
n-sample launch, last row included; and a period of exactly n on n samples is the launch whose block never fires.  (A period of n on
n + 1 samples fires on row n, which the cut removes: that launch has no block in its first n rows and cannot equal one that has.)  The
generated form is used, so the two series agree by construction of the streams; the end records of the two lengths are not compared.

Measured on the MI355X (first run: all 44 pass as written, 0.65 s the slowest; no kernel changed).  Largest deviation from the restatement
over the 18 parity cases, with the smallest bound any of them allowed: att 8.7e-15 (1.6e-13), pos 8.2e-15 in ref_frame 0 (9.0e-13) and
1.4e-16 in ref_frame 1 (4.8e-14), vel 1.1e-13 (1.2e-11), wb 1.2e-12 (4.0e-12), ab 4.7e-12 (1.4e-11), pdiag_end 1.5e-14 (2.0e-13), k_est
6.2e-15 (9.8e-13), scale_end 1.7e-14 (9.7e-13), pcross_end 5.0e-15 (2.0e-13); no case used more than 0.07 of its own bound.  The closed
form: P[15][15] after 399 additions of q_k = 5e-8 to 4e-4 is 0.00041994999999998969 on the device in all four launches (both kernels,
both frames), BIT-EQUAL to the Python loop.  End sigma of the scale state, mean over the 65 runs of the schedule case, q = 0 against
q = 1e-3 /sqrt(s): all three blocks with mask 7 0.002536 -> 0.003809 (ref_frame 0) and 0.002530 -> 0.003797 (ref_frame 1); the scale
family alone 0.002660 -> 0.003910 and 0.002660 -> 0.003912; larger in every run.  The set of kernel names launched by the instantiation
test is the 24.  Every bit comparison holds.
"""
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

FS, FS_GPS, RUNS, BAD_RUN = 20.0, 2.0, 65, 33
VIB = {'type': 'random', 'x': 0.05, 'y': 0.05, 'z': 0.05}
ALL, MS = ('mag', 'scale', 'still'), ('mag', 'still')
NAME = 'ginsim::loose_all_kernel<%d, %s, %s, %s, %d>'
NEVER = 2 ** 40
Q = ls.SCALE_Q
ROWS = ('traj', 'wb', 'ab', 'scale')                    # the planes that hold one row per sample


def all_name(rf, given=False, vib=False, ps=False, ns=16):
    return NAME % (rf, str(given).lower(), str(vib).lower(), str(ps).lower(), ns)


def states(which):
    return 16 if 'scale' in which else 15


class Dump(ins_loose_dump.Dump):
    """The first n samples of the stops profile with the odometer (it reads ls.READS), one magnetometer series (a general calibration)
    and the standstill signal of the truth; every: a period for all blocks or one per block (ls.periods); q: the scale state's random walk."""

    def __init__(self, ctx, rf, n, runs=RUNS, seed=41, vib=None):
        super().__init__(ctx, rf, n, runs, seed, 0, FS, FS_GPS, truth_fn=ls.stops_truth, profile=sc.STOPS_CSV, geo=mc.GEO, odo_err=ls.ODO_ERR,
                         vib=vib, mag_errs=(('m', mc.MAG_ERR_SKEW),), flags=sc.flags_of)
        self._restated, self._altered = {}, []

    def _case(self, which, mask, every, flags, q):
        return dict(mask=mask, mag=self.mag_errs['m'] if 'mag' in which else None, scale='scale' in which, smask=3 if 'still' in which else 0,
                    every=every, geo=self.geo, flags=flags, q=q)

    def job(self, ctx, which=ALL, mask=ls.MASK, every=1, given=False, flags=None, q=0.0, combined=True, **kw):
        """which: the blocks of {'mag', 'scale', 'still'} the job holds.  flags None: the job derives the signal from the truth.
        given: True for the dumped series, a dict for other buffers.  combined None: the keyword is not passed (a single family)."""
        case = ls.job_kw(keep=kw.get('keep_traj', True), **self._case(which, mask, every, flags, q))
        if combined is not None:
            case['combined'] = combined
        if given is True and 'mag' in which:
            given = self.given_with_mag('m')
        return super().job(ctx, given, **dict(case, **kw))

    def restate(self, which=ALL, mask=ls.MASK, every=1, flags=None, q=0.0):
        """The restatement of all runs and 16 x its own float64 error on the first 8, once per case."""
        key = (tuple(which), mask, str(every), None if flags is None else np.asarray(flags).tobytes(), q)
        if key not in self._restated:
            kw = ls.blocks(self.model, self.fs, self.rf, **self._case(which, mask, every, self.flags if flags is None else flags, q))
            kw.update(odo=self.odo, mag=self.mag['m'] if 'mag' in which else None)
            out = aref.run(*self._args(), **kw)
            bound = cs.parity_bound(*self._args(), run=aref.run, deviation=ls.deviation, **kw)
            self._restated[key] = (out, bound)
        return self._restated[key]

    def altered(self, ctx, name, change):
        """A device copy, in the layout `given` takes, of the dumped 'mag' (R, n, 3), 'gps' (R, m, 6) or 'odo' (R, n) after change(host)."""
        host = {'mag': self.mag['m'], 'gps': self.gps, 'odo': self.odo}[name].copy()
        change(host)
        buf = ctx.upload(np.ascontiguousarray(host.T if name == 'odo' else host.transpose(2, 1, 0)))
        self._altered.append(buf)
        return buf

    def release(self):
        for b in self._altered:
            b.free()
        super().release()


def parity(tag, d, job, which=ALL, mask=ls.MASK, every=1, flags=None, q=0.0):
    dev = result(job)
    exp, bound = d.restate(which, mask, every, flags, q)
    assert set(bound) == set(ls.kc.PARITY_KEYS if 'scale' in which else cs.PARITY_KEYS)
    held('parity rf%d %s' % (d.rf, tag), ls.deviation(dev, exp), bound)
    return dev


def rows(p, upto, run=None):
    """The first `upto` rows of the planes that hold one per sample (of one run where given)."""
    out = {k: (p[k][:upto] if k == 'scale' else p[k][:, :upto]) for k in ROWS if k in p}
    return out if run is None else {k: np.ascontiguousarray(v[..., run]) for k, v in out.items()}


def scale_end(job):
    """(k_est, P[15][15]) at the last sample, each (runs,), as the kernel stored them."""
    a = job.ctx.download(job.scalep.out_scale_end, (2, job.runs))
    return a[0].copy(), a[1].copy()


@pytest.fixture(scope='module', params=[0, 1], ids=['rf0', 'rf1'])
def short(request, ctx):
    """The schedule case: 30 s, the first stop, the turn, 3 s into the outage; sflags: ls.schedule_flags."""
    d = Dump(ctx, request.param, ls.SCHEDULE_N)
    d.sflags = ls.schedule_flags(d.truth, d.stamps, d.n)
    yield d
    d.release()


@pytest.fixture(scope='module', params=[0, 1], ids=['rf0', 'rf1'])
def edge(request, ctx):
    d = Dump(ctx, request.param, 400)
    yield d
    d.release()


# ------------------------------------------------------------------------------------------------- 1. a period of its own per block
@pytest.mark.parametrize('every', [ls.SCHEDULE, ls.ROTATED], ids=['aid4 mag3 still5', 'aid5 mag4 still3'])
def test_parity_with_a_period_of_its_own_for_every_block(ctx, short, every):
    """The three counters of the lane out of lockstep: every non-empty subset of {fix, aid, mag, still} fires on some sample (shown for
    SCHEDULE by the CPU file and again here on the dump's own stamps), a standstill block follows an aiding block with no magnetometer
    block between them, blocks fire without a fix inside the outage.  The given form gives the generated form's bits."""
    flags = short.sflags
    assert short.n == 600 and short.runs == 65
    count = np.bincount(ls.schedule(short.n, ls.SCHEDULE, short.stamps, short.truth['gps_visibility'], flags)[1:], minlength=16)
    assert np.all(count[1:] > 0)
    gen = short.job(ctx, every=every, flags=flags).run()
    assert gen.kernel_name() == all_name(short.rf)
    parity('all three, %s' % (every,), short, gen, every=every, flags=flags)
    giv = short.job(ctx, every=every, flags=flags, given=True).run()
    assert giv.kernel_name() == all_name(short.rf, given=True)
    same_bits(planes(gen), planes(giv))
    gen.release()
    giv.release()


# ------------------------------------------------------------------------------------------------- 2. the aiding masks
@pytest.mark.parametrize('which, mask', [(MS, 0), (MS, 6), (ALL, 1)], ids=['mag + still, mask 0', 'mag + still, mask 6', 'all three, mask 1'])
def test_parity_with_every_aiding_mask_next_to_the_other_blocks(ctx, short, which, mask):
    """Mask 0 fires no aiding block at all, mask 6 the constraint rows without an odometer read, mask 1 the odometer row of the
    16-state lane alone.  Masks 0 and 6, given form: the whole odometer column of one run is NaN and the launch is handed that buffer
    (in_odo itself, which the job leaves NULL for these masks) -- bit 0 of the mask is all that keeps the lane from the load."""
    flags, every = short.sflags, ls.SCHEDULE
    gen = short.job(ctx, which, mask, every, flags=flags).run()
    assert gen.kernel_name() == all_name(short.rf, ns=states(which))
    parity('%s, mask %d' % (' + '.join(which), mask), short, gen, which, mask, every, flags)
    if not mask & 1:
        def poison(odo):
            odo[BAD_RUN] = np.nan
        bad = short.altered(ctx, 'odo', poison)
        giv = short.job(ctx, which, mask, every, flags=flags, given=dict(short.given_with_mag('m'), odo=bad))
        assert not giv.mc.in_odo
        giv.mc.in_odo = bad.ptr
        giv.run()
        assert giv.kernel_name() == all_name(short.rf, given=True, ns=15)
        same_bits(planes(gen), planes(giv))
        giv.release()
    gen.release()


# ------------------------------------------------------------------------------------------------- 3. period edges
@pytest.mark.parametrize('block', ['mag', 'still'])
def test_a_block_with_period_n_minus_1_fires_once_on_the_last_stored_row(ctx, edge, block):
    """Rows 0 .. n - 2 are those of the launch whose block never fires, the last row and pdiag_end are not; a period of exactly n
    never fires; and the same period on a series one sample longer, cut back, gives every one of the n rows (the module docstring
    says how the issue's sentence is read)."""
    n, rf = edge.n, edge.rf
    flags = edge.flags.copy()
    assert n == 400 and flags[n - 1] == 0 and flags.any()
    if block == 'still':
        flags[n - 1] = 1
    period = lambda p: dict(ls.SCHEDULE, **{block: p})
    once, never, exact = (edge.job(ctx, every=period(p), flags=flags).run() for p in (n - 1, NEVER, n))
    assert once.kernel_name() == never.kernel_name() == exact.kernel_name() == all_name(rf)
    a, b = planes(once), planes(never)
    same_bits(rows(a, n - 1), rows(b, n - 1))
    moved = 'att' if block == 'mag' else 'vel'
    k = 3 * ('att', 'pos', 'vel').index(moved)
    assert not np.array_equal(a['traj'][k:k + 3, n - 1], b['traj'][k:k + 3, n - 1]) and not np.array_equal(a['pdiag'], b['pdiag'])
    assert not np.array_equal(a['scale'][n - 1], b['scale'][n - 1])            # k_est moves through the cross-covariance
    same_bits(b, planes(exact))
    parity('%s fires on the last row only' % block, edge, once, every=period(n - 1), flags=flags)
    longer = Dump(ctx, rf, n + 1)
    assert longer.n == n + 1 and np.array_equal(longer.truth['ref_gyro'][:n], edge.truth['ref_gyro'])
    cut = longer.job(ctx, every=period(n - 1), flags=np.append(flags, 0)).run()
    same_bits(rows(a, n), rows(planes(cut), n))
    for j in (once, never, exact, cut, longer):
        j.release()


# ------------------------------------------------------------------------------------------------- 4. q_k > 0
def closed_form(p0, q_k, n):
    p = p0 * p0
    for _ in range(n - 1):
        p += q_k
    return p


@pytest.mark.parametrize('family', ['scale', 'all'])
def test_closed_form_of_the_random_walk_on_the_device(ctx, edge, family):
    """No aiding block ever fires (aid_every = n), so nothing observes state 15: P[15][15] is p0^2 and n - 1 additions of q_k, within
    (n - 1) 2^-53 relative of the Python loop (the a-priori bound of n - 1 additions; whether it is bit-equal is printed), k_est is
    scale0 to the bit on every row and the cross column is exactly 0 -- on loose_scale_kernel and on loose_all_kernel<.., 16> with a
    magnetometer block that never fires and all flags 0."""
    n, rf = edge.n, edge.rf
    if family == 'scale':
        job = edge.job(ctx, ('scale',), every={'aid': n, 'mag': 1, 'still': 1}, q=Q, combined=None).run()
        assert job.kernel_name() == 'ginsim::loose_scale_kernel<%d, false, false, false>' % rf
    else:
        job = edge.job(ctx, ALL, every={'aid': n, 'mag': n, 'still': 1}, flags=np.zeros(n, dtype=np.int32), q=Q).run()
        assert job.kernel_name() == all_name(rf)
    q_k = job.scale['q_k']
    assert q_k == Q * Q / FS == job.scalep.q_k > 0.0
    want = closed_form(ls.kc.P0_SCALE, q_k, n)
    k_end, p = scale_end(job)
    rel = float(np.max(np.abs(p - want)) / want)
    print('closed form rf%d %s: P[15][15] %.17g, the loop %.17g, relative %.2e (bound %.2e), bit-equal: %s'
          % (rf, family, p[0], want, rel, (n - 1) * 2.0 ** -53, bool(np.all(p == want))))
    assert want > ls.kc.P0_SCALE ** 2 and rel <= (n - 1) * 2.0 ** -53
    assert np.all(job.series('odo_scale', np.arange(job.runs)) == ls.kc.SCALE0) and np.all(k_end == ls.kc.SCALE0)
    assert np.array_equal(job.final_scale()[1], np.sqrt(p)) and not job.final_pcross().any()
    job.release()


@pytest.mark.parametrize('family', ['scale', 'all'])
def test_parity_with_a_random_walk_of_the_scale_state(ctx, short, family):
    """q = 1e-3 /sqrt(s): mask 7 with all three blocks at the schedule's periods, and the scale family alone with the same q.  The end
    sigma of the scale state exceeds the q = 0 launch's in every run, as the CPU file finds for the restatement."""
    which, kw = (ALL, dict(flags=short.sflags)) if family == 'all' else (('scale',), dict(combined=None))
    walk, fixed = (short.job(ctx, which, every=ls.SCHEDULE, q=q, **kw).run() for q in (Q, 0.0))
    name = all_name(short.rf) if family == 'all' else 'ginsim::loose_scale_kernel<%d, false, false, false>' % short.rf
    assert walk.kernel_name() == fixed.kernel_name() == name and walk.scalep.q_k == Q * Q / FS and fixed.scalep.q_k == 0.0
    parity('%s, q = 1e-3' % family, short, walk, which, every=ls.SCHEDULE, flags=kw.get('flags'), q=Q)
    sw, sf = walk.final_scale()[1], fixed.final_scale()[1]
    print('rf%d %s: end sigma of the scale state, mean over the runs: q = 0 %.6f, q = 1e-3 %.6f' % (short.rf, family, sf.mean(), sw.mean()))
    assert np.all(sw > sf) and np.all(sf < ls.kc.P0_SCALE)
    assert not np.array_equal(walk.final_scale()[0], fixed.final_scale()[0])
    walk.release()
    fixed.release()


def test_the_plugin_passes_the_random_walk_to_both_families(ctx):
    """InsLoose(odo=True, odo_scale_state=True, odo_scale_q=1e-3) alone and with every other aid and combined=True under one Sim:
    q_k = q^2 / fs reaches the scale family's block and the combined family's."""
    from demo_algorithms.ins_loose_device import InsLoose
    from gnss_ins_sim.sim import imu_model, ins_sim
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=9, gps=True, odo=True)
    alone = InsLoose(odo=True, odo_scale_state=True, odo_scale_q=Q)
    every = InsLoose(odo=True, nhc=True, odo_scale_state=True, odo_scale_q=Q, mag=True, zupt=True, zaru=True, combined=True)
    sim = ins_sim.Sim([FS, FS_GPS, FS], sc.STOPS_CSV, ref_frame=1, imu=imu, seed=99, geo_mag_n=list(mc.GEO), algorithm=[alone, every])
    sim.run(3)
    (_, job0, _), (_, job1, _) = sim.loose_jobs
    assert job0.kernel_name() == 'ginsim::loose_scale_kernel<1, false, false, false>' and job1.kernel_name() == all_name(1)
    for job in (job0, job1):
        assert job.scale['q_k'] == 1e-6 / FS == job.scalep.q_k
        assert np.all(job.final_scale()[1] > 0.0) and np.all(np.isfinite(job.final_sigmas()))


# ------------------------------------------------------------------------------------------------- 5. every instantiation
def test_every_one_of_the_24_instantiations_runs_and_agrees_with_its_neighbours(ctx):
    """One 400-sample launch per name of loose_all_kernel<RF, GIVEN, VIB, PS, NS>, each held to another variant's bits: a statistics
    variant to the plain one in every kept plane and end record, the given variant to the generated one, a vibration variant to the
    given launch fed with its own dumped sensors (so the vibration variant with statistics holds both comparisons)."""
    table = set(all_name(rf, g, v, ps, ns) for rf in (0, 1) for g, v in ((False, False), (True, False), (False, True)) for ps in (False, True)
                for ns in (15, 16))
    assert len(table) == 24
    seen = set()

    def launch(d, which, want, given=False, ps=False):
        job = d.job(ctx, which, every=ls.SCHEDULE, given=given, **(dict(proc_first=100) if ps else {})).run()
        assert job.kernel_name() == want and want in table
        seen.add(want)
        out = planes(job), (job.process_stats_online() if ps else None)
        job.release()
        return out

    for rf in (0, 1):
        calm, shaken = Dump(ctx, rf, 400), Dump(ctx, rf, 400, vib=VIB)
        assert not np.array_equal(calm.accel, shaken.accel)                     # the vibration term is in the samples
        for which in (MS, ALL):
            ns = states(which)
            gen, _ = launch(calm, which, all_name(rf, ns=ns))
            gen_ps, online = launch(calm, which, all_name(rf, ps=True, ns=ns), ps=True)
            giv, _ = launch(calm, which, all_name(rf, given=True, ns=ns), given=True)
            giv_ps, online_g = launch(calm, which, all_name(rf, given=True, ps=True, ns=ns), given=True, ps=True)
            vib, _ = launch(shaken, which, all_name(rf, vib=True, ns=ns))
            vib_ps, online_v = launch(shaken, which, all_name(rf, vib=True, ps=True, ns=ns), ps=True)
            fed, _ = launch(shaken, which, all_name(rf, given=True, ns=ns), given=True)
            assert ('scale' in gen) == (ns == 16) and np.all(np.isfinite(gen['traj'])) and np.all(np.isfinite(vib['traj']))
            same_bits(gen, gen_ps)
            same_bits(gen, giv)
            same_bits(giv, giv_ps)
            same_bits(fed, vib)
            same_bits(vib, vib_ps)
            same_bits(fed, vib_ps)
            assert not np.array_equal(gen['traj'], vib['traj'])
            assert np.array_equal(online.view(np.uint64), online_g.view(np.uint64)) and np.all(np.isfinite(online_v))
        calm.release()
        shaken.release()
    assert seen == table, sorted(table - seen)


# ------------------------------------------------------------------------------------------------- 6. non-finite aids, given form
J_BAD = 300             # a magnetometer block (300 % 3 == 0) and a visible fix (stamp 30) fall on this sample


@pytest.fixture(scope='module')
def given_base(ctx, short):
    job = short.job(ctx, every=ls.SCHEDULE, flags=short.sflags, given=True).run()
    assert job.kernel_name() == all_name(short.rf, given=True)
    p = planes(job)
    job.release()
    assert all(np.all(np.isfinite(v)) for v in p.values())
    return p


def given_with(ctx, short, name, change):
    buf = short.altered(ctx, name, change)
    job = short.job(ctx, every=ls.SCHEDULE, flags=short.sflags, given=dict(short.given_with_mag('m'), **{name: buf})).run()
    p = planes(job)
    job.release()
    return p


@pytest.mark.parametrize('value', [np.nan, np.inf], ids=['nan', 'inf'])
@pytest.mark.parametrize('what', ['mag', 'fix'])
def test_a_non_finite_aid_that_is_read_stays_in_its_run_and_after_its_sample(ctx, short, given_base, what, value):
    """One magnetometer component at a sample whose block fires / one component of a visible fix, run 33 of 65: every other run and
    the bad run's earlier rows keep their bits; its last row, pdiag_end and scale_end are not all finite."""
    n = short.n
    kf = int(np.nonzero(short.stamps == J_BAD)[0][0])
    assert J_BAD % ls.SCHEDULE['mag'] == 0 and short.truth['gps_visibility'][kf] != 0

    def change(a):
        if what == 'mag':
            a[BAD_RUN, J_BAD, 1] = value
        else:
            a[BAD_RUN, kf, 4] = value
    got = given_with(ctx, short, 'mag' if what == 'mag' else 'gps', change)
    others = np.setdiff1d(np.arange(short.runs), [BAD_RUN])
    same_bits(given_base, got, others, others)
    same_bits(rows(given_base, J_BAD, BAD_RUN), rows(got, J_BAD, BAD_RUN))
    for k, v in (('last row', got['traj'][:, n - 1, BAD_RUN]), ('pdiag_end', got['pdiag'][:, BAD_RUN]), ('scale_end', got['scale_end'][:, BAD_RUN])):
        assert not np.all(np.isfinite(v)), k


@pytest.mark.parametrize('value', [np.nan, np.inf], ids=['nan', 'inf'])
@pytest.mark.parametrize('what', ['mag off its period', 'mag at sample 0', 'hidden fix'])
def test_a_non_finite_aid_that_is_not_read_changes_no_bit(ctx, short, given_base, what, value):
    hidden = np.nonzero(np.asarray(short.truth['gps_visibility']) == 0)[0]
    assert (J_BAD + 1) % ls.SCHEDULE['mag'] != 0 and hidden.size

    def change(a):
        if what == 'hidden fix':
            a[BAD_RUN, hidden[1], :] = value
        else:
            a[BAD_RUN, J_BAD + 1 if what == 'mag off its period' else 0, :] = value
    same_bits(given_base, given_with(ctx, short, 'gps' if what == 'hidden fix' else 'mag', change))
