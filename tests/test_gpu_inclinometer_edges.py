"""GPU: the inclinometer kernel (csrc/inclinometer.hip) where the vehicle of the other goldens never goes -- attitudes over the
whole sphere and the records of tests/inclinometer_records.py against the unmodified reference's golden (incl_sphere.npz) and
the NumPy restatement, the +-pi wrap of the att_euler error, non-finite runs and their wavefront neighbours, process windows,
launch shapes (block sizes, 64-bit run offsets, algorithm subsets, the compacted chain) and seeded random configurations.
Every comparison is against the golden or the restatement evaluated on the host, except where bit-identity under another launch
shape is the property."""
import numpy as np
import pytest

from conftest import GOLDEN, PKG, REPO  # noqa: F401  (the suite's paths)
import inclinometer_ref as iref
import inclinometer_records as rec
from test_gpu_full_size import _record
from test_inclinometer_oracle import ILL_MEASURED, quat_diff, sphere_golden

pytestmark = pytest.mark.gpu
SEED = 4242
G = 9.8


def _ctx():
    import ginsim
    return ginsim.default_context()


def _turn(n=None, fs=100.0):
    from ginsim import workloads
    ini, truth, _ = workloads.truth_from_profile('turn_90deg', fs, 1)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    if n is not None:
        truth = {k: v[:n] for k, v in truth.items()}
    return truth, acc, gyr


def _job(runs, truth, acc, gyr, fs=100.0, **kw):
    import ginsim
    kw.setdefault('seed', SEED)
    return ginsim.InclinometerJob(_ctx(), fs, truth, acc, gyr, runs, **kw)


def _given(accel, gyro, fs=100.0, ref_att=None, **kw):
    ctx = _ctx()
    R, n, _ = accel.shape
    bufs = {'accel': ctx.upload(np.ascontiguousarray(accel.transpose(2, 1, 0))),
            'gyro': ctx.upload(np.ascontiguousarray(gyro.transpose(2, 1, 0)))}
    truth = {'ref_accel': np.zeros((n, 3)), 'ref_gyro': np.zeros((n, 3)), 'ref_att': np.zeros((n, 3)) if ref_att is None else ref_att}
    kw.setdefault('start_bias', np.zeros((R, 3)))
    job = _job(R, truth, None, None, fs=fs, given=bufs, **kw).run()
    job._bufs.update({'given_accel': bufs['accel'], 'given_gyro': bufs['gyro']})     # freed with the job
    return job


def _wrapped(a, b):
    """|a - b| modulo 2 pi (a last-place difference at the +-pi seam must not count as 2 pi)."""
    return np.abs(np.mod(a - b + np.pi, 2 * np.pi) - np.pi)


def _worst(d):
    return float(np.nanmax(d)) if np.isfinite(d).any() else 0.0


# ------------------------------------------------------------------------------------------------- 1. the sphere records
def test_sphere_records_against_the_golden_and_the_restatement():
    """The records of inclinometer_records.sphere_batches() as given sensors: quaternions (up to sign) 1e-12, wb / ab / final bias
    1e-14 against the golden's rows and the restatement's every row, NaN patterns equal; the ill-conditioned groups (within 1e-6 /
    1e-9 rad of +-x) at 4 x the bound measured on the CPU for reference vs restatement, which is 0.0: bit-identical.  Euler angles:
    the device's against iref.quat2euler of the device's own quaternions everywhere (1e-12), against the golden where the
    restatement has |cos pitch| >= 0.02, NaN where the golden says the reference raises.
    Measured on the MI355X (the margins file of _record, entry incl_edges_sphere): quaternions 1.2e-15 from the golden and 1.0e-15
    from the restatement (both in the group with cos(theta / 2) < 0), wb 5.5e-16, ab 1.1e-15, Euler angles 4.4e-15 from the
    golden and 4.4e-16 from the restatement of the device's own quaternions; the ill-conditioned groups 0.0 for every output."""
    g = sphere_golden()
    worst = {}
    for b in rec.sphere_batches():
        p, R = b['name'] + '_', b['accel'].shape[0]
        k, ids = g[p + 'rows'], np.arange(R)
        job = _given(b['accel'], b['gyro'], fs=b['fs'], gains=b['gains'], stats=True, keep=True)
        assert job.kernel_name() == 'ginsim::incl_kernel<3, true, false>'
        q, wb, ab, fin = iref.mahony(b['gyro'], b['accel'], 1.0 / b['fs'], np.zeros((R, 3)), b['gains'])
        want = {'mahony_quat': q, 'tilt_quat': iref.tilt(b['accel']), 'wb': wb, 'ab': ab, 'bias_after': fin}
        got = {'mahony_quat': job.series('quat_mahony', ids), 'tilt_quat': job.series('quat_tilt', ids), 'wb': job.series('wb', ids),
               'ab': job.series('ab', ids), 'bias_after': job.final_biases()}
        eul = {a: job.series('euler_' + a, ids) for a in ('mahony', 'tilt')}
        job.release()
        for nm in want:
            assert np.array_equal(np.isnan(got[nm]), np.isnan(want[nm])), (b['name'], nm)
            gold = got[nm] if nm == 'bias_after' else got[nm][:, k]
            assert np.array_equal(np.isnan(gold), np.isnan(g[p + nm])), (b['name'], nm)
            for gn, gi in b['groups'].items():
                for tag, x, y in (('restatement', got[nm][gi], want[nm][gi]), ('golden', gold[gi], g[p + nm][gi])):
                    d = _worst(quat_diff(x, y) if nm.endswith('quat') else np.abs(x - y))
                    key = '%s_%s_%s' % (gn, nm, tag)
                    worst[key] = max(worst.get(key, 0.0), d)
                    tol = 4.0 * ILL_MEASURED[gn] if gn in rec.ILL_GROUPS else (1e-12 if nm.endswith('quat') else 1e-14)
                    assert d <= tol, (key, d)
        for a in ('mahony', 'tilt'):
            dq = got[a + '_quat']
            own = iref.quat2euler(dq)
            assert np.array_equal(np.isnan(eul[a]), np.isnan(own)), (b['name'], a)
            worst['euler_own_' + a] = max(worst.get('euler_own_' + a, 0.0), _worst(_wrapped(eul[a], own)))
            assert worst['euler_own_' + a] < 1e-12
            raises = g[p + a + '_asin_raises']
            assert np.isnan(eul[a][:, k][raises][:, 1]).all()
            rq = want[a + '_quat'][:, k]
            with np.errstate(invalid='ignore'):
                ok = np.abs(np.cos(iref.quat2euler(rq)[..., 1])) >= 0.02
            d = _wrapped(eul[a][:, k], g[p + a + '_euler'])[ok]
            worst['euler_golden_' + a] = max(worst.get('euler_golden_' + a, 0.0), _worst(d))
            assert worst['euler_golden_' + a] < 1e-12
    print(worst)
    _record('incl_edges_sphere', **{k: v for k, v in worst.items() if v > 0.0 or k.startswith('euler')})


# ------------------------------------------------------------------------------------------------- 2. the wrap
@pytest.mark.parametrize('yaw', [np.pi, -np.pi, np.nextafter(np.pi, 0), np.nextafter(np.pi, 4), np.nextafter(-np.pi, 0),
                                 np.nextafter(-np.pi, -4)], ids=['+pi', '-pi', '+pi-', '+pi+', '-pi-', '-pi+'])
def test_wrap_of_an_exact_error(yaw):
    """The level, zero-rate record has yaw == 0 exactly; against a truth of +-pi and its neighbouring doubles the error is what
    attitude.angle_range_pi gives (+pi for both exact values) at the end point, in the window mean and max, with std == 0."""
    R, n = 3, 8
    accel, gyro = np.zeros((R, n, 3)), np.zeros((R, n, 3))
    accel[:, :, 2] = -G
    ref = np.zeros((n, 3))
    ref[:, 0] = yaw
    job = _given(accel, gyro, ref_att=ref, stats=True, keep=True, proc_first=2)
    want = float(iref.angle_range_pi(np.array(0.0 - yaw)))
    if abs(yaw) == np.pi:
        assert want == np.pi
    for a in ('mahony', 'tilt'):
        assert np.array_equal(job.series('euler_' + a, np.arange(R)), np.zeros((R, n, 3)))
        end, proc, st = job.end_errors(a), job.process_stats_online(a), job.stats(a)
        assert np.array_equal(end, np.tile([want, 0.0, 0.0], (R, 1)))
        assert np.array_equal(proc[:, 0, 0:3], np.tile([abs(want), 0.0, 0.0], (R, 1)))
        assert np.array_equal(proc[:, 1, 0:3], np.tile([want, 0.0, 0.0], (R, 1)))
        assert np.array_equal(proc[:, 2], np.zeros((R, 9)))
        assert st.maxabs[0] == abs(want) and st.mean[0] == want and np.array_equal(st.std, np.zeros(9))
    job.release()


@pytest.mark.parametrize('offset', [0.0, np.pi], ids=['truth_from_170_degrees', 'error_about_pi'])
def test_wrap_with_a_heading_that_sweeps_through_180_degrees(offset):
    """A constant yaw rate of 2 rad/s for 15 s (almost five turns); the truth starts at 170 degrees, or half a turn from the
    estimate with a wiggle so that the error itself changes sign at +-pi: online statistics against iref.stats of the kept series."""
    R, n, first = 2, 1500, 100
    accel, gyro = np.zeros((R, n, 3)), np.zeros((R, n, 3))
    accel[:, :, 2] = -G
    gyro[:, :, 2] = 2.0
    gyro[1, :, 2] = -1.3
    t = 0.01 * (np.arange(n) + 1)
    ref = np.zeros((n, 3))
    ref[:, 0] = iref.angle_range_pi(170 * np.pi / 180 + 2.0 * t) if offset == 0.0 else iref.angle_range_pi(np.pi + 2.0 * t + 0.02 * np.sin(0.7 * t))
    job = _given(accel, gyro, ref_att=ref, stats=True, keep=True, proc_first=first)
    for a in ('mahony', 'tilt'):
        e = job.series('euler_' + a, np.arange(R))
        if a == 'mahony':
            assert np.sum(np.abs(np.diff(e[0, :, 0])) > 6.0) >= 4          # the estimate really went through +-180 degrees
        end, proc = iref.stats(e, ref, first)
        assert np.array_equal(job.end_errors(a), end) or np.max(_wrapped(job.end_errors(a), end)) < 1e-12
        assert np.allclose(job.process_stats_online(a)[:, :, 0:3], proc, rtol=1e-9, atol=1e-13)
    if offset:
        err = iref.angle_err(job.series('euler_mahony', [0])[0, first:, 0], ref[first:, 0])
        assert err.max() > 3.0 and err.min() < -3.0                         # both sides of the wrap inside the window
    job.release()


# ------------------------------------------------------------------------------------------------- 3. non-finite runs
def test_nan_runs_follow_numpy_and_leave_their_neighbours_alone():
    """132 given records (three wavefronts).  Lane 0 of the batch and its last run are TiltAcc's +x record (NaN quaternions in the
    reference too); the last lane of the first wavefront, the first of the second and the last of the second carry a NaN in the
    gyro before, at and after proc_first.  Statistics as NumPy's (np.max(np.abs()), np.mean, np.std of the wrapped error): NaN in
    exactly those runs; every other run bit-identical to the batch with clean records in their place."""
    from oracle import ins_np
    R, n, first = 132, 50, 20
    rng = np.random.RandomState(11)
    accel = np.array([0.0, 0.0, -G]) + 0.3 * rng.standard_normal((R, n, 3))
    gyro = 0.05 * rng.standard_normal((R, n, 3))
    ref = 0.01 * rng.standard_normal((n, 3))
    bad_a, bad_g = accel.copy(), gyro.copy()
    bad_a[[0, R - 1]] = [G, 0.0, 0.0]
    for r, j in ((63, 10), (64, first), (127, 35)):
        bad_g[r, j, 1] = np.nan
    nan_tilt, nan_mah = [0, R - 1], [63, 64, 127]
    clean = _given(accel, gyro, ref_att=ref, stats=True, keep=True, proc_first=first)
    job = _given(bad_a, bad_g, ref_att=ref, stats=True, keep=True, proc_first=first)
    ids = np.arange(R)
    q, wb, ab, fin = iref.mahony(bad_g, bad_a, 0.01, np.zeros((R, 3)))
    with np.errstate(invalid='ignore'):
        want = {'mahony': iref.stats(iref.quat2euler(q), ref, first), 'tilt': iref.stats(iref.quat2euler(iref.tilt(bad_a)), ref, first)}
    for a, nan_runs in (('mahony', nan_mah), ('tilt', nan_tilt)):
        end, proc = job.end_errors(a), job.process_stats_online(a)[:, :, 0:3]
        isn = np.zeros(R, dtype=bool)
        isn[nan_runs] = True
        assert np.array_equal(np.isnan(end), np.repeat(isn[:, None], 3, 1)) and np.array_equal(np.isnan(proc), np.broadcast_to(isn[:, None, None], (R, 3, 3)))
        assert np.array_equal(np.isnan(end), np.isnan(want[a][0])) and np.array_equal(np.isnan(proc), np.isnan(want[a][1]))
        assert np.allclose(proc, want[a][1], rtol=1e-7, atol=1e-11, equal_nan=True)
        with np.errstate(invalid='ignore'):
            st, np_st = job.stats(a), ins_np.array_stats(end)
        for x, y in ((st.maxabs, np_st['max']), (st.mean, np_st['avg']), (st.std, np_st['std'])):
            assert np.isnan(x[0:3]).all() and np.isnan(y).all() and not np.isnan(x[3:9]).any()
        # the runs that share a record with the clean batch: bit-identical
        same = np.ones(R, dtype=bool)
        same[nan_mah if a == 'mahony' else nan_tilt] = False
        if a == 'mahony':
            same[nan_tilt] = False                      # another accelerometer record: Mahony's outputs differ legitimately
        assert np.array_equal(end[same], clean.end_errors(a)[same])
        assert np.array_equal(proc[same], clean.process_stats_online(a)[same][:, :, 0:3])
        names = ('quat_' + a, 'euler_' + a) + (('wb', 'ab') if a == 'mahony' else ())
        for nm in names:
            assert np.array_equal(job.series(nm, ids[same]), clean.series(nm, ids[same])), nm
    assert np.isfinite(job.series('quat_mahony', nan_tilt)).all()           # Mahony on +x is finite
    assert np.array_equal(np.isnan(job.series('quat_mahony', ids)), np.isnan(q))
    assert np.array_equal(job.final_biases()[~np.isin(ids, nan_mah + nan_tilt)], clean.final_biases()[~np.isin(ids, nan_mah + nan_tilt)])
    job.release()
    clean.release()


# ------------------------------------------------------------------------------------------------- 4. windows
def test_process_windows_from_the_first_sample_to_past_the_end():
    """Generated sensors, the turn cut to 300 samples, the truth's yaw moved 3.0 rad below the heading the filters report (zero:
    neither has a heading reference), so the error is a large positive constant plus a noise-sized wiggle and never wraps:
    proc_first 0, 1, n-2, n-1 against iref.stats of the kept series; n-1: std == 0 and mean == max; >= n: zeros."""
    truth, acc, gyr = _turn(300)
    ref = truth['ref_att'].copy()
    ref[:, 0] += -3.0 - ref[0, 0]
    truth = dict(truth, ref_att=ref)
    n, R = 300, 5
    for first in (0, 1, n - 2, n - 1, n, n + 10):
        job = _job(R, truth, acc, gyr, keep=True, stats=True, proc_first=first, start_bias=np.zeros((R, 3))).run()
        for a in ('mahony', 'tilt'):
            got = job.process_stats_online(a)
            if first >= n:
                assert np.array_equal(got, np.zeros((R, 3, 9)))
                continue
            end, proc = iref.stats(job.series('euler_' + a, np.arange(R)), truth['ref_att'], first)
            assert np.all(proc[:, 0, 0] > 2.0) and np.all(proc[:, 0, 0] < 3.1)          # large, and short of the wrap
            assert np.allclose(got[:, :, 0:3], proc, rtol=1e-9, atol=1e-13), (first, a)
            # the reference wraps every error (x % 2 pi, then - 2 pi): a negative one loses its last bits there, the kernel keeps
            # |e| < pi as it is -- the bound test_online_statistics_equal_those_of_the_kept_series has for the end point
            assert np.max(_wrapped(job.end_errors(a), end)) < 1e-12
            if first == n - 1:      # a window of one sample: no spread, and its mean is the end-point error itself
                assert np.array_equal(got[:, 2], np.zeros((R, 9))) and np.array_equal(got[:, 1, 0], got[:, 0, 0])
                assert np.array_equal(got[:, 1, 0:3], job.end_errors(a))
        job.release()


# ------------------------------------------------------------------------------------------------- 5. launch shapes
def _outputs(job, ids):
    out = {'fin': job.final_biases()[ids]} if 'mahony' in job.algos else {}
    for a in job.algos:
        out['end_' + a], out['proc_' + a] = job.end_errors(a)[ids], job.process_stats_online(a)[ids]
        out['quat_' + a], out['euler_' + a] = job.series('quat_' + a, ids), job.series('euler_' + a, ids)
    if 'mahony' in job.algos:
        out['wb'], out['ab'] = job.series('wb', ids), job.series('ab', ids)
    return out


@pytest.mark.parametrize('R', [1, 63, 64, 65, 255, 256, 257, 1023])
def test_block_sizes_and_single_run_launches_give_the_same_bits(R):
    truth, acc, gyr = _turn(200)
    start = 1e-4 * np.random.RandomState(R).standard_normal((R, 3))
    off = 1000
    kw = dict(keep=True, stats=True, proc_first=40, run_offset=off)
    ids = np.arange(R)
    base = None
    for bt in (0, 64, 128, 256):
        job = _job(R, truth, acc, gyr, start_bias=start, block_threads=bt, **kw).run()
        assert job.passes == 1
        out = _outputs(job, ids)
        job.release()
        if base is None:
            base = out
            assert all(np.isfinite(v).all() for v in out.values())
            continue
        for nm in base:
            assert np.array_equal(out[nm], base[nm]), (bt, nm)
    for r in sorted({0, R // 2, R - 1}):
        one = _job(1, truth, acc, gyr, start_bias=start[r:r + 1], **dict(kw, run_offset=off + r)).run()
        out = _outputs(one, np.arange(1))
        one.release()
        for nm in base:
            assert np.array_equal(out[nm][0], base[nm][r]), (r, nm)


@pytest.mark.parametrize('off', [2 ** 32 - 3, 2 ** 40 + 17])
def test_run_offsets_past_32_bits(off):
    """The batch at 2^32 - 3 straddles the high word of the RNG key: sensors through the filter against ins_np.mc_sensors +
    iref.mahony (1e-9 on quaternions, 1e-10 on wb), and not the runs of offset 0."""
    from oracle import ins_np
    truth, acc, gyr = _turn(200)
    R = 8
    ids = np.arange(R)
    job = _job(R, truth, acc, gyr, keep=True, stats=False, run_offset=off).run()
    accel, gyro = ins_np.mc_sensors(SEED, off + ids, 100.0, truth['ref_accel'], truth['ref_gyro'], acc, gyr)
    q, wb, ab, fin = iref.mahony(gyro, accel, 0.01, job.initial_biases())
    dq, dwb = job.series('quat_mahony', ids), job.series('wb', ids)
    assert np.max(quat_diff(dq, q)) < 1e-9 and np.max(np.abs(dwb - wb)) < 1e-10
    assert np.max(quat_diff(job.series('quat_tilt', ids), iref.tilt(accel))) < 1e-9
    _record('incl_edges_offset_%d' % off, quat=np.max(quat_diff(dq, q)), wb=np.max(np.abs(dwb - wb)))
    dacc = job.series('quat_tilt', ids)
    zero = _job(R, truth, acc, gyr, keep=True, stats=False, run_offset=0).run()
    assert np.all(np.max(quat_diff(zero.series('quat_tilt', ids), dacc), axis=1) > 1e-9)
    zero.release()
    for r in (3, R - 1):            # past 2^32: not the run that has the same LOW word
        low = _job(1, truth, acc, gyr, keep=True, stats=False, run_offset=(off + r) & 0xFFFFFFFF).run()
        assert np.max(quat_diff(low.series('quat_tilt', [0])[0], dacc[r])) > 1e-9
        low.release()
    job.release()


def test_algorithm_subsets_give_the_same_bits_alone_and_together():
    truth, acc, gyr = _turn(200)
    R = 70
    start = 1e-4 * np.random.RandomState(3).standard_normal((R, 3))
    ids = np.arange(R)
    outs = {}
    for algos, mask in ((('mahony',), 1), (('tilt',), 2), (('mahony', 'tilt'), 3)):
        job = _job(R, truth, acc, gyr, algos=algos, start_bias=start, keep=True, stats=True, proc_first=30).run()
        assert job.kernel_name() == 'ginsim::incl_kernel<%d, false, false>' % mask and job.passes == 1
        outs[algos] = _outputs(job, ids)
        job.release()
    both = outs[('mahony', 'tilt')]
    for algos in (('mahony',), ('tilt',)):
        assert len(outs[algos]) >= 4
        for nm, v in outs[algos].items():
            assert np.array_equal(v, both[nm]), nm


def test_compacted_chain_of_257_runs_against_the_restated_chain():
    from oracle import ins_np
    truth, acc, gyr = _turn(100)
    R = 257
    b0 = np.array([2e-4, -1e-4, 5e-5])
    job = _job(R, truth, acc, gyr, bias0=b0, stats=True).run()
    print('R=%d passes=%d launched=%s' % (R, job.passes, job.launched[:12]))
    assert job.passes > 1 and job.launched[0] == R and any(x < R for x in job.launched[1:])      # compaction really happened
    accel, gyro = ins_np.mc_sensors(SEED, np.arange(R), 100.0, truth['ref_accel'], truth['ref_gyro'], acc, gyr)
    q, wb, ab, starts, last = iref.chain(gyro, accel, 0.01, b0)
    d_ini, d_fin = np.max(np.abs(job.initial_biases() - starts)), np.max(np.abs(job.final_biases()[-1] - last))
    _record('incl_edges_chain_257', initial=d_ini, final=d_fin)
    assert d_ini < 1e-11 and d_fin < 1e-11
    assert np.max(np.abs(job.final_biases()[:-1] - starts[1:])) < 1e-11
    end, _ = iref.stats(iref.quat2euler(q), truth['ref_att'])
    assert np.max(_wrapped(job.end_errors('mahony'), end)) < 1e-9
    job.release()


# ------------------------------------------------------------------------------------------------- 6. seeded random configurations
FUZZ_CASES = list(range(200, 224))
_FUZZ = {}                  # case -> runs sampled / dropped from the statistics comparison (the cap test reads it)


def _fuzz_config(i):
    """tests/test_gpu_fuzz.py's random profile / IMU model / vibration / rate / frame / run count / 64-bit offset, plus the
    filter's own parameters: gains within a decade of their defaults, bias0 <= 1e-3 rad/s, dt = 1 / fs except in a quarter of the
    cases, a random window; every sixth case has at most 8 runs (the whole chain is then restated)."""
    from test_gpu_fuzz import _random_case
    c = _random_case(i)
    rng = np.random.RandomState(12000 + i)
    c['gains'] = {k: float(v * 10.0 ** rng.uniform(-1, 1)) for k, v in sorted(iref.GAINS.items())}
    c['bias0'] = rng.uniform(-1e-3, 1e-3, 3)
    c['dt'] = 1.0 / c['fs'] if rng.rand() >= 0.25 else float(rng.uniform(0.5, 2.0) / c['fs'])
    c['first'] = int(rng.randint(0, c['truth']['ref_accel'].shape[0] - 1))
    if i % 6 == 0:
        c['runs'] = 1 + int(rng.randint(0, 8))
    return c


def _fuzz_reference(c, ids, start):
    """Restated quaternions, wb, ab, Euler angles, statistics of runs `ids` from initial biases `start`, and which (run, algorithm)
    pairs keep |cos pitch| >= 0.02 over the whole window (asin's slope: the line tests/test_gpu_fuzz.py draws)."""
    from oracle import ins_np
    accel, gyro = ins_np.mc_sensors(c['seed'], c['off'] + ids, c['fs'], c['truth']['ref_accel'], c['truth']['ref_gyro'], c['acc'], c['gyr'],
                                    vib_accel=c['va'], vib_gyro=c['vg'])
    q, wb, ab, fin = iref.mahony(gyro, accel, c['dt'], start, c['gains'])
    out = {'accel': accel, 'gyro': gyro, 'quat_mahony': q, 'wb': wb, 'ab': ab, 'fin': fin, 'quat_tilt': iref.tilt(accel)}
    for a in ('mahony', 'tilt'):
        e = iref.quat2euler(out['quat_' + a])
        out['euler_' + a] = e
        with np.errstate(invalid='ignore'):
            out['ok_' + a] = np.abs(np.cos(e[..., 1])) >= 0.02
            out['stats_' + a] = iref.stats(e, c['truth']['ref_att'], c['first'])
        out['keep_' + a] = out['ok_' + a][:, c['first']:].all(axis=1)
    return out


@pytest.mark.parametrize('i', FUZZ_CASES)
def test_random_configuration_against_the_restatement(i):
    """Three runs (first, middle, last) of every case through ins_np.mc_sensors + iref.mahony from job.initial_biases(), and
    iref.tilt: quaternions 1e-9 up to sign, wb / ab 1e-10 on every sample; Euler angles 1e-9 on the samples where the restatement
    has |cos pitch| >= 0.02; statistics (rtol 1e-7, atol 1e-11) for the runs whose window has no excluded sample.  Cases of at most
    8 runs: the whole chain against iref.chain (1e-11 on the biases)."""
    c = _fuzz_config(i)
    R = c['runs']
    job = _job(R, c['truth'], c['acc'], c['gyr'], fs=c['fs'], gains=c['gains'], dt=c['dt'], bias0=c['bias0'], seed=c['seed'],
               run_offset=c['off'], stats=True, proc_first=c['first'], keep=True, vib_accel=c['va'], vib_gyro=c['vg']).run()
    assert job.passes <= R + 1
    ids = np.unique([0, R // 2, R - 1])
    ref = _fuzz_reference(c, ids, job.initial_biases()[ids])
    worst = {}
    for nm, tol in (('quat_mahony', 1e-9), ('quat_tilt', 1e-9), ('wb', 1e-10), ('ab', 1e-10)):
        x = job.series(nm, ids)
        d = _worst(quat_diff(x, ref[nm]) if nm.startswith('quat') else np.abs(x - ref[nm]))
        assert np.array_equal(np.isnan(x), np.isnan(ref[nm])) and d < tol, 'case %d %s %.3e' % (i, nm, d)
        worst[nm] = d
    assert np.max(np.abs(job.final_biases()[ids] - ref['fin'])) < 1e-10
    sampled = dropped = 0
    for a in ('mahony', 'tilt'):
        ok, keep = ref['ok_' + a], ref['keep_' + a]
        d = _worst(_wrapped(job.series('euler_' + a, ids), ref['euler_' + a])[ok])
        assert d < 1e-9, 'case %d euler %s %.3e' % (i, a, d)
        worst['euler_' + a] = d
        sampled, dropped = sampled + keep.size, dropped + int((~keep).sum())
        end, proc = ref['stats_' + a]
        last_ok = ok[:, -1]
        assert np.all(_wrapped(job.end_errors(a)[ids], end)[last_ok] < 1e-9)
        got = job.process_stats_online(a)[ids][:, :, 0:3]
        assert np.allclose(got[keep], proc[keep], rtol=1e-7, atol=1e-11), 'case %d statistics %s' % (i, a)
    _FUZZ[i] = (sampled, dropped)
    if R <= 8:
        from oracle import ins_np
        accel, gyro = ins_np.mc_sensors(c['seed'], c['off'] + np.arange(R), c['fs'], c['truth']['ref_accel'], c['truth']['ref_gyro'], c['acc'], c['gyr'],
                                        vib_accel=c['va'], vib_gyro=c['vg'])
        q, wb, ab, starts, last = iref.chain(gyro, accel, c['dt'], c['bias0'], c['gains'])
        assert np.max(np.abs(job.initial_biases() - starts)) < 1e-11 and np.max(np.abs(job.final_biases()[-1] - last)) < 1e-11
    job.release()
    _record('incl_edges_fuzz_case_%d' % i, **worst)


def test_random_configurations_keep_most_of_their_runs():
    """The share of (run, algorithm) pairs that drop out of the statistics comparison because their window holds a sample with
    |cos pitch| < 0.02, from the restatement alone: at most 5 % over the whole set (a later change of the generator cannot empty the
    comparison silently).  Measured for cases 200-223: 2 of 140 pairs (1.4 %), both in case 203; worst differences over the set:
    quaternions, wb, ab and the compared Euler angles 2.2e-14 (the margins file of _record, entries incl_edges_fuzz_*)."""
    assert sorted(_FUZZ) == FUZZ_CASES, 'runs after the cases of test_random_configuration_against_the_restatement'
    sampled, dropped = (sum(v[k] for v in _FUZZ.values()) for k in (0, 1))
    print('fuzz: %d of %d sampled (run, algorithm) pairs dropped' % (dropped, sampled))
    _record('incl_edges_fuzz_excluded', sampled=sampled, dropped=dropped)
    assert sampled >= 2 * 2 * len(FUZZ_CASES) and dropped <= 0.05 * sampled
