"""GPU: what tests/test_gpu_ins_loose_all_cons.py leaves open of the checkpoint kernels loose_all_cons_kernel<RF, GIVEN, VIB, NS>
(csrc/ins_loose_all_cons.hpp) and loose_cons_kernel<RF, GIVEN, VIB, AID> (csrc/ins_loose_cons.hip): the tilted stops
profile in the southern hemisphere (A), the vibration variants (B), run offsets and the merge of records (C), every branch of the
inclusion rule (D), the scale state's random walk under checkpoints (E) and the caller's order (F).  CPU side: the last two tests of
tests/test_ins_loose_all_cons_oracle.py hold section A's choice of checkpoints and section D1's truth vector on the restatement alone.

Shapes.  A: tests/golden/ins_loose/motion_def_tilted_stops.csv whole (960 samples at 20 Hz, 41 S 150 W, yaw 170 -> 200 deg through
+-180, pitch 12 -> 8 -> 12 deg, roll -10 -> -7 -> -10 deg, parked twice on the slope, the second stop inside the GPS outage) with the
field GEO_SOUTH, 65 runs, both frames.  B: 400 samples, 65 runs, both frames.  C, D: 300 samples, 65 or 129 runs, ref_frame 1.
E: the schedule case (600 samples), 65 runs, ref_frame 1.

Parity bound, DESIGN 4.11c's rule as tests/test_gpu_ins_loose_all_cons.py states it (cons_held): column by column of the 43 the device
may deviate from the float64 restatement by ins_loose_cases.PARITY_MARGIN (16) x the restatement's own float64 - np.longdouble
deviation on that case and all its runs; the count column is exact.  Section D, whose subject is which lanes enter a sum, adds the
order of a sum of R non-negative doubles, (R - 1) eps (order=True; the comment at TAIL_SAMPLES there).  Section C's bound is derived
at its test.  Sections A, B and E hold the rule as it stands on eight checkpoints each, spread over the run; section D's five are those
of the sibling file's non-finite run.

The 24 names of the two checkpoint kernels and a test that launches each (rf = 0 and 1 in every line):
  loose_all_cons_kernel<rf, true,  false, 15>   test_tilted_parity_of_the_given_form[none, mag+still]
  loose_all_cons_kernel<rf, true,  false, 16>   test_tilted_parity_of_the_given_form[scale, all]
  loose_all_cons_kernel<rf, false, false, 15>   test_tilted_generated_form_equals_given_form[mag+still]
  loose_all_cons_kernel<rf, false, false, 16>   test_tilted_generated_form_equals_given_form[all], test_tilted_checkpoints_perturb_nothing
  loose_all_cons_kernel<rf, false, true,  15>   test_vibration_variant_of_the_combined_checkpoint_kernel[mag+still]
  loose_all_cons_kernel<rf, false, true,  16>   test_vibration_variant_of_the_combined_checkpoint_kernel[all]
  loose_cons_kernel<rf, false, true,  false>    test_vibration_variant_of_the_plain_checkpoint_kernel[mask0]
  loose_cons_kernel<rf, false, true,  true>     test_vibration_variant_of_the_plain_checkpoint_kernel[mask7]
  loose_cons_kernel<rf, true,  false, false | true>   tests/test_gpu_ins_loose_cons.py::test_parity_with_the_restatement[0-1, 7-7]
  loose_cons_kernel<rf, false, false, false | true>   tests/test_gpu_ins_loose_cons.py::test_generated_form_equals_given_form_bit_for_bit

Measured on the MI355X (28 tests, 31 s, the slowest 2.8 s; no kernel changed, and ConsistencyResult needed no fix: count 0 gives NaN
means without a warning).  Per section, the device's largest deviation in any column, and the column closest to its bound:
  A  8 parity cases: 3.3e-12 ... 1.0e-9 where the restatement's own float64 error is 2.8e-8 ... 3.5e-7; closest P_dr_y of the scale
     filter in ref_frame 0, 5.77e-15 against 5.91e-15 (0.98 of the bound); every other case uses 0.69 of a bound or less
     (P_dv_x 1.61e-14 of 2.33e-14, all three blocks, ref_frame 0).  Generated = given and dense = sparse = no checkpoints: the same bits.
  B  loose_all_cons_kernel 2.0e-13 ... 2.8e-13, closest nees_v 1.48e-13 of 1.27e-12; loose_cons_kernel 1.4e-12 ... 5.7e-12, closest
     P_dr_x 3.71e-16 of 2.60e-15.  Fed = generated bit for bit in all eight; none equals the calm dump's record.
  C  |whole - (a + b)| / whole 2.19e-16 (bound 4.44e-16); merged ratio 3.28e-16 (1.55e-15), nees 2.15e-16 (6.66e-16), ratio_scale
     1.59e-16 (1.55e-15); run 64 alone: the same bits from both jobs.
  D  non-finite truth 6.8e-13, closest nees_v 1.49e-14 of 6.46e-14; a wavefront left out 6.8e-13, closest e2_psi_z 6.46e-14 of 1.28e-13;
     no run included: 43 x +0.0 at the last three checkpoints.
  E  q = 1e-3: 1.0e-12, closest e2_psi_z 2.14e-13 of 5.67e-13; q = 0: P_dba_z 9.87e-15 of 5.81e-14; the sum of P[15][15] over the 65
     runs at n - 1 4.161e-4 with q = 0, 9.372e-4 with q = 1e-3.
"""
import warnings

import numpy as np
import pytest

import ins_loose_aided_cases as ac
import ins_loose_all_cases as ls
import ins_loose_cons_dump as cdump
import ins_loose_dump
import ins_loose_mag_cases as mc
import ins_loose_still_cases as sc
from ins_loose_cons_dump import record
from ins_loose_dump import ctx, planes, same_bits
from test_gpu_ins_loose_all import ALL, VIB, Dump
from test_gpu_ins_loose_all_cons import TAIL_SAMPLES, cons_held, cons_name, tail_flags

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
MS = ('mag', 'still')
BLOCKS = {'none': (), 'scale': ('scale',), 'mag+still': MS, 'all': ALL}
VIB_ALL_NAME = 'ginsim::loose_all_cons_kernel<%d, false, true, %d>'
VIB_CONS_NAME = 'ginsim::loose_cons_kernel<%d, false, true, %s>'
VIB_SAMPLES = [0, 1, 50, 120, 200, 300, 398, 399]
BAD_SAMPLES = [50, 100, 101, 200, 299]              # an accelerometer that is NaN from sample 100 on enters the state with the step to 101


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def job_of(d, ctx, which, **kw):
    """The job of Dump d with the blocks `which`; the given form of a filter with the scale state is told what the odometer reads."""
    if 'scale' in which and kw.get('given') and 'scale_truth' not in kw:
        kw['scale_truth'] = ls.READS
    return d.job(ctx, which, **kw)


def record_of(job):
    rec = record(job.run())
    job.release()
    return rec


# ------------------------------------------------------------------------------------------------- A. the tilted stops profile
@pytest.fixture(scope='module', params=[0, 1], ids=['rf0', 'rf1'])
def tilted(request, ctx):
    d = Dump(ctx, request.param, None, 65, seed=5, profile=sc.TILTED_STOPS_CSV, geo=mc.GEO_SOUTH)
    d.samples = ls.edge_checkpoints(d.ini, d.truth, d.stamps, d.flags)          # asserts the preconditions and that each sample exists
    yield d
    d.release()


@pytest.mark.parametrize('blocks', list(BLOCKS))
def test_tilted_parity_of_the_given_form(ctx, tilted, blocks):
    """41 S, pitch and roll away from 0, yaw through +-180 deg: psi from the antisymmetric part of C_est C^T, the position error in
    metres through geo_param of the truth row (ref_frame 0), after the magnetometer and the standstill block of the same sample;
    columns 37-39 after the ZUPT rows have moved k_est through the cross-covariance.  A period of its own per block."""
    d, which, n = tilted, BLOCKS[blocks], tilted.n
    assert n == 960 and d.runs == 65 and d.ini[0] < 0 and len(sc.windows(d.flags)) == 2
    assert np.max(np.abs(d.truth['ref_att'][:, 1])) >= np.radians(10.0) and d.samples[-1] == n - 1 and len(d.samples) == 8
    job = job_of(d, ctx, which, every=ls.SCHEDULE, given=True, checkpoints=d.samples, keep_traj=False).run()
    assert job.kernel_name() == cons_name(d.rf, which, given=True)
    dev = record(job)
    job.release()
    assert np.all(dev[:, 0] == 65) and np.all(np.isfinite(dev))
    cons_held('tilted stops', dev, d, which, d.samples, every=ls.SCHEDULE, scale_truth=ls.READS)
    if 'scale' in which:
        assert np.all(dev[:, 37:40] > 0) and dev[-1, 37] < 0.25 * dev[0, 37]     # the scale state is learnt on the slope too


@pytest.mark.parametrize('blocks', ['mag+still', 'all'])
def test_tilted_generated_form_equals_given_form(ctx, tilted, blocks):
    d, which = tilted, BLOCKS[blocks]
    kw = dict(every=ls.SCHEDULE, checkpoints=d.samples, keep_traj=False)
    gen, giv = job_of(d, ctx, which, **kw), job_of(d, ctx, which, given=True, **kw)
    assert (gen.kernel_name(), giv.kernel_name()) == (cons_name(d.rf, which), cons_name(d.rf, which, given=True))
    a, b = record_of(gen), record_of(giv)
    assert a[:, 0].min() == 65 and np.array_equal(bits(a), bits(b)) and ('scale' in which) == bool(a[:, 38].any())


def test_tilted_checkpoints_perturb_nothing(ctx, tilted):
    """A checkpoint at every one of the 960 samples leaves every kept plane and end record of the launch without checkpoints bit for
    bit; the dense record at a sparse list's samples is the sparse launch's."""
    d, n = tilted, tilted.n
    plain = d.job(ctx, ALL, every=ls.SCHEDULE).run()
    assert '_cons_' not in plain.kernel_name()
    want, sig = planes(plain), plain.final_sigmas()
    plain.release()
    every = d.job(ctx, ALL, every=ls.SCHEDULE, checkpoints=range(n)).run()
    assert every.kernel_name() == cons_name(d.rf, ALL)
    same_bits(planes(every), want)
    assert np.array_equal(bits(every.final_sigmas()), bits(sig))
    dense = record(every)
    every.release()
    sparse = record_of(d.job(ctx, ALL, every=ls.SCHEDULE, checkpoints=d.samples, keep_traj=False))
    assert np.all(dense[:, 0] == 65) and np.array_equal(bits(sparse), bits(dense[d.samples]))


# ------------------------------------------------------------------------------------------------- B. the vibration variants
@pytest.fixture(scope='module', params=[0, 1], ids=['rf0', 'rf1'])
def shaken(request, ctx):
    """(calm, shaken): the same seed without and with a vibration term of the accelerometer, every aid dumped."""
    pair = Dump(ctx, request.param, 400, 65, seed=41), Dump(ctx, request.param, 400, 65, seed=41, vib=VIB)
    assert not np.array_equal(pair[0].accel, pair[1].accel)
    yield pair
    for d in pair:
        d.release()


@pytest.mark.parametrize('blocks', ['mag+still', 'all'])
def test_vibration_variant_of_the_combined_checkpoint_kernel(ctx, shaken, blocks):
    """loose_all_cons_kernel<rf, false, true, NS>: the record of the generated form with a vibration term is, bit for bit, that of the
    given form fed the shaken dump's own buffers; it is held to the restatement on those buffers; it is not the calm dump's."""
    calm, d = shaken
    which = BLOCKS[blocks]
    kw = dict(every=ls.SCHEDULE, checkpoints=VIB_SAMPLES, keep_traj=False)
    gen = job_of(d, ctx, which, **kw).run()
    assert gen.kernel_name() == VIB_ALL_NAME % (d.rf, 16 if 'scale' in which else 15)
    rec = record(gen)
    gen.release()
    fed = job_of(d, ctx, which, given=True, **kw)
    assert fed.kernel_name() == cons_name(d.rf, which, given=True)
    assert np.array_equal(bits(rec), bits(record_of(fed))) and np.all(rec[:, 0] == 65)
    cons_held('vibration', rec, d, which, VIB_SAMPLES, every=ls.SCHEDULE, scale_truth=ls.READS)
    still = job_of(calm, ctx, which, **kw)
    assert still.kernel_name() == cons_name(d.rf, which)
    quiet = record_of(still)
    assert np.array_equal(quiet[:, 0], rec[:, 0]) and not np.array_equal(quiet[1:], rec[1:])


@pytest.fixture(scope='module', params=[0, 1], ids=['rf0', 'rf1'])
def shaken_plain(request, ctx):
    """(calm, shaken) for loose_cons_kernel: the outage profile with the odometer alone, as tests/test_gpu_ins_loose_cons.py dumps it."""
    pair = ins_loose_dump.Dump(ctx, request.param, 400, 65, seed=41), ins_loose_dump.Dump(ctx, request.param, 400, 65, seed=41, vib=VIB)
    assert not np.array_equal(pair[0].accel, pair[1].accel)
    yield pair
    for d in pair:
        d.release()


@pytest.mark.parametrize('mask, every', [(0, 1), (7, 3)], ids=['mask0', 'mask7'])
def test_vibration_variant_of_the_plain_checkpoint_kernel(ctx, shaken_plain, mask, every):
    """loose_cons_kernel<rf, false, true, AID> through cons_samples=: the same three assertions."""
    calm, d = shaken_plain
    kw = ac.aid_kw(mask, every, cons_samples=VIB_SAMPLES, keep_traj=False)
    gen = d.job(ctx, **kw).run()
    assert gen.kernel_name() == VIB_CONS_NAME % (d.rf, 'true' if mask else 'false')
    rec = record(gen)
    gen.release()
    fed = d.job(ctx, given=True, **kw)
    assert fed.kernel_name() == 'ginsim::loose_cons_kernel<%d, true, false, %s>' % (d.rf, 'true' if mask else 'false')
    assert np.array_equal(bits(rec), bits(record_of(fed))) and np.all(rec[:, 0] == 65)
    cdump.cons_held('vibration', rec, d, mask, every, VIB_SAMPLES)
    quiet = record_of(calm.job(ctx, **kw))
    assert np.array_equal(quiet[:, 0], rec[:, 0]) and not np.array_equal(quiet[1:], rec[1:])


# ------------------------------------------------------------------------------------------------- C. run offsets and the merge
@pytest.fixture(scope='module')
def wide(ctx):
    d = Dump(ctx, 1, 300, 129, seed=21)
    yield d
    d.release()


def test_records_of_disjoint_runs_at_a_run_offset_merge_by_addition(ctx, wide):
    """One job of 129 runs against run_offset = 0, runs = 64 and run_offset = 64, runs = 65 in the generated form: the lane regenerates
    sensors, fixes, odometer and magnetometer from run_offset + r and indexes the truth of the scale factor by the local r.
    The bound.  The split is on a wavefront boundary, so the three wavefronts' partial records w0, w1, w2 are the same bits in both
    arrangements (the butterfly's order within a wavefront does not depend on the launch).  The whole job's record is fl(fl(w0 + w1)
    + w2), the sum of the parts' fl(w0 + fl(w1 + w2)): two roundings each of non-negative terms, each within eps / 2 of a partial sum
    no larger than the total S, so each side lies within eps S (1 + eps / 4) of S and the two within 2 eps S of each other.
    The means divide by the same count; ratio = sqrt(e2) / sqrt(pbar) carries half of each sum's 2 eps, 2 eps together, and each side's
    evaluation rounds five times (two divisions by the count, two roots, one quotient: 5 eps / 2 a side): 7 eps.  nees is one sum
    and one division a side: 3 eps."""
    import ginsim
    d = wide
    flags, truth = tail_flags(d), ls.READS + 1e-3 * np.arange(129)
    kw = dict(every=2, flags=flags, checkpoints=TAIL_SAMPLES, keep_traj=False)
    whole = d.job(ctx, ALL, scale_truth=truth, **kw).run()
    a = d.job(ctx, ALL, runs=64, run_offset=0, scale_truth=truth[:64], **kw).run()
    b = d.job(ctx, ALL, runs=65, run_offset=64, scale_truth=truth[64:], **kw).run()
    assert whole.kernel_name() == a.kernel_name() == b.kernel_name() == cons_name(1, ALL)
    w, ra, rb = whole.consistency(), a.consistency(), b.consistency()
    rw, pa, pb = w.pack(), ra.pack(), rb.pack()
    assert np.all(rw[:, 0] == 129) and np.all(pa[:, 0] == 64) and np.all(pb[:, 0] == 65)
    rel = np.abs(rw - (pa + pb)) / np.where(rw != 0, np.abs(rw), 1.0)
    print('129 runs against 64 + 65 at an offset: largest |whole - (a + b)| / whole %.2e (bound %.2e)' % (rel.max(), 2 * EPS))
    assert np.all(np.abs(rw - (pa + pb)) <= 2 * EPS * np.abs(rw)) and not rw[:, 40:].any() and np.all(rw[1:, 1:40] > 0)
    m = ginsim.ConsistencyResult.merge([pa, pb])
    assert np.array_equal(m.count, w.count) and np.array_equal(m.records, pa + pb)
    for name, bound in (('ratio', 7 * EPS), ('nees', 3 * EPS), ('ratio_scale', 7 * EPS)):
        got, want = getattr(m, name), getattr(w, name)
        some = want != 0                                                        # psi is exactly 0 at sample 0: 0 on both sides
        dev = float(np.max(np.abs(got - want)[some] / np.abs(want)[some]))
        print('    merged %s against the whole job\'s: %.2e (bound %.2e)' % (name, dev, bound))
        assert np.all(np.isfinite(want)) and np.array_equal(got != 0, some) and np.all(some[1:]) and dev <= bound, name
    # run 64 of the whole job alone, and lane 0 of the offset job alone: the same run, the same truth, the same bits
    one, other = record(whole.run([64])), record(b.run([0]))
    assert np.all(one[:, 0] == 1) and np.array_equal(bits(one), bits(other))
    first = record(a.run([0]))
    assert not np.array_equal(first[1:, 16:40], one[1:, 16:40])
    for j in (whole, a, b):
        j.release()


# ------------------------------------------------------------------------------------------------- D. the inclusion rule
@pytest.fixture(scope='module')
def level(ctx):
    d = Dump(ctx, 1, 300, 65, seed=51)
    yield d
    d.release()


def poisoned(ctx, d, runs):
    """(a device copy of the dumped accelerometer with NaN in `runs` from sample 100 on, the same on the host as the restatement reads it)"""
    acc = ctx.download(d.mc.buffer('accel'), (3, d.n, d.runs))
    acc[1, 100:, runs] = np.nan
    host = d.accel.copy()
    host[runs, 100:, 1] = np.nan
    return ctx.upload(acc), host


def test_a_non_finite_truth_of_the_scale_factor_leaves_its_run_out(ctx, level):
    """NaN in run 7 and +inf in run 40 of scale_truth: the branch of the inclusion rule that 16 states alone have."""
    d, flags, truth = level, tail_flags(level), ls.bad_scale_truth(65)
    dev = record_of(d.job(ctx, ALL, every=2, given=True, flags=flags, checkpoints=BAD_SAMPLES, scale_truth=truth, keep_traj=False))
    assert np.all(dev[:, 0] == 63) and np.all(np.isfinite(dev))
    keep = np.setdiff1d(np.arange(65), [7, 40])
    kw = dict(order=True, every=2, flags=flags, scale_truth=truth)
    cons_held('non-finite truth, the other 63', dev, d, ALL, BAD_SAMPLES, runs=keep, **kw)
    cons_held('non-finite truth, all 65', dev, d, ALL, BAD_SAMPLES, **kw)


def test_a_whole_wavefront_left_out_adds_nothing(ctx, wide):
    """Runs 64 ... 127, the second of three wavefronts, are NaN from sample 100 on: cons_final_kernel adds a partial record whose 43
    numbers are all 0."""
    d, flags = wide, tail_flags(wide)
    bad_runs = np.arange(64, 128)
    bad, host = poisoned(ctx, d, bad_runs)
    job = d.job(ctx, ALL, every=2, given=True, flags=flags, checkpoints=BAD_SAMPLES, scale_truth=ls.READS, keep_traj=False)
    job.mc.in_accel = bad.ptr
    dev = record_of(job)
    bad.free()
    assert list(dev[:, 0]) == [129, 129, 65, 65, 65] and np.all(np.isfinite(dev))
    keep = np.setdiff1d(np.arange(129), bad_runs)
    kw = dict(order=True, every=2, flags=flags, scale_truth=ls.READS)
    cons_held('a wavefront left out, the other 65', dev[2:], d, ALL, BAD_SAMPLES[2:], runs=keep, **kw)
    cons_held('a wavefront left out, all 129', dev, d, ALL, BAD_SAMPLES, accel=host, **kw)


def test_no_run_included_gives_zeros_and_nan_means_without_a_warning(ctx, level):
    d, flags = level, tail_flags(level)
    kw = dict(every=2, given=True, flags=flags, checkpoints=BAD_SAMPLES, scale_truth=ls.READS, keep_traj=False)
    clean = record_of(d.job(ctx, ALL, **kw))
    bad, _ = poisoned(ctx, d, np.arange(65))
    job = d.job(ctx, ALL, **kw)
    job.mc.in_accel = bad.ptr
    job.run()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = job.consistency()
        derived = {k: getattr(res, k) for k in ('pbar', 'ratio', 'nees', 'ratio_scale', 'sigma', 'rms', 'sigma_scale', 'rms_scale')}
    dev = res.pack()
    job.release()
    bad.free()
    assert np.all(clean[:, 0] == 65) and np.array_equal(bits(dev[:2]), bits(clean[:2]))
    assert dev[2:].shape == (3, 43) and not bits(dev[2:]).any()                  # +0.0 in all 43 columns: no bit set, the sign neither
    assert not np.signbit(dev[2:]).any() and list(res.count) == [65, 65, 0, 0, 0]
    for k, v in derived.items():
        assert np.all(np.isnan(v[2:])) and np.all(np.isfinite(v[:2])), k


# ------------------------------------------------------------------------------------------------- E. the random walk
def test_the_scale_random_walk_under_checkpoints(ctx):
    """q = 1e-3 /sqrt(s) on the schedule case: P[15][15] grows between the odometer updates, which a checkpoint inside the outage
    sees and one with q = 0 cannot.  Seven checkpoints and more: the four of OUTAGE_FLAGS among them."""
    d = Dump(ctx, 1, ls.SCHEDULE_N, 65, seed=41)
    n, flags = d.n, ls.schedule_flags(d.truth, d.stamps, d.n)
    samples = [0, 1, 300] + list(ls.OUTAGE_FLAGS) + [n - 1]
    assert len(samples) == 8 and n == 600
    kw = dict(every=ls.SCHEDULE, given=True, flags=flags, checkpoints=samples, scale_truth=ls.READS, keep_traj=False)
    walk, fixed = d.job(ctx, ALL, q=ls.SCALE_Q, **kw).run(), d.job(ctx, ALL, **kw).run()
    assert walk.kernel_name() == fixed.kernel_name() == cons_name(1, ALL, given=True)
    assert walk.scalep.q_k == ls.SCALE_Q * ls.SCALE_Q / d.fs > 0.0 == fixed.scalep.q_k
    a, b = record(walk), record(fixed)
    walk.release()
    fixed.release()
    assert np.all(a[:, 0] == 65) and np.all(b[:, 0] == 65)
    cons_held('random walk', a, d, ALL, samples, every=ls.SCHEDULE, flags=flags, q=ls.SCALE_Q, scale_truth=ls.READS)
    cons_held('no random walk', b, d, ALL, samples, every=ls.SCHEDULE, flags=flags, scale_truth=ls.READS)
    print('sum of P[15][15] over 65 runs at n - 1: q = 0 %.6e, q = 1e-3 %.6e' % (b[-1, 37], a[-1, 37]))
    assert a[-1, 37] > b[-1, 37] and np.all(a[1:, 37] > b[1:, 37])
    assert np.array_equal(bits(a[0, 1:37]), bits(b[0, 1:37])) and not np.array_equal(a[-1, 1:37], b[-1, 1:37])
    d.release()


# ------------------------------------------------------------------------------------------------- F. the caller's order
def test_the_records_come_back_in_the_caller_s_order(ctx, level):
    d, n = level, level.n
    kw = dict(every=2, given=True, scale_truth=ls.READS, keep_traj=False)
    asked = record_of(d.job(ctx, ALL, checkpoints=[n - 1, 0, 0, 7], **kw))
    ordered = record_of(d.job(ctx, ALL, checkpoints=[0, 7, n - 1], **kw))
    assert asked.shape == (4, 43) and np.all(asked[:, 0] == 65)
    assert np.array_equal(bits(asked[1]), bits(asked[2])) and np.array_equal(bits(asked[[1, 3, 0]]), bits(ordered))
    assert not np.array_equal(ordered[0], ordered[1]) and not np.array_equal(ordered[1], ordered[2])
