"""Error-growth curves on the device (csrc/error_curve.hip, ginsim_error_curve*, MonteCarloJob.error_curve, Sim.error_curve)
against the NumPy restatement tests/error_curve_ref.py.

Tolerances are the project's own (tests/test_gpu_size_edges.py): mean and max rtol 1e-12, std rtol 1e-9, atol 1e-9 (2e-8 for
NED positions) -- or the per-record bound of the restatement (16 x max(long-double distance, spread over eight permutations of
the run order, eps |q|)) where that is larger.  No record is left out of a comparison.
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, PKG, load_golden
import error_curve_ref

pytestmark = pytest.mark.gpu

FS = 100.0
RTOL = {'max': 1e-12, 'avg': 1e-12, 'std': 1e-9}


@pytest.fixture(scope='module')
def ctx():
    import ginsim
    c = ginsim.Context(0)
    yield c
    c.close()


def _job(ctx, rf, runs, precision='f64', algos=('free',), seed=20261017, **kw):
    import ginsim
    from ginsim import workloads
    ini, truth, _ = workloads.truth_from_profile('turn_90deg', FS, rf)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    job = ginsim.MonteCarloJob(ctx, FS, rf, truth, acc, gyr, ini, runs=runs, algos=algos, odo_err={'scale': 0.999, 'stdv': 0.1},
                               seed=seed, keep_traj=True, precision=precision, **kw)
    ref_nav = np.ascontiguousarray(np.concatenate([truth['ref_att'], truth['ref_pos'], truth['ref_vel']], axis=1))
    return job, ref_nav


def _series(job, algo='free'):
    """(runs, n, 9) of the job's own trajectories, as the device holds them (fp32: origin + displacement, formed in fp64)."""
    att, pos, vel = job.trajectories(algo, np.arange(job.runs))
    return np.concatenate([att, pos, vel], axis=2)


def _atol(ned):
    a = np.full(9, 1e-9)
    if ned:
        a[3:6] = 2e-8
    return a


def _assert_curve(got, want, rows, ned, extra=None, what=''):
    """Every record of `got` (a CurveResult over samples rows) against rows `rows` of the restatement `want`.  extra: (9,) added
    to every tolerance (a propagated series tolerance)."""
    rows = np.arange(want['max'].shape[0]) if rows is None else np.asarray(rows)
    assert got.mean.shape == (rows.size, 9), (got.mean.shape, rows.size)
    with np.errstate(invalid='ignore'):
        for key, dev in (('max', got.maxabs), ('avg', got.mean), ('std', got.std)):
            ref = want[key][rows]
            tol = np.maximum(_atol(ned) + RTOL[key] * np.abs(ref), want['tol_' + key][rows])
            if extra is not None:
                tol = tol + extra
            np.testing.assert_array_equal(np.isnan(dev), np.isnan(ref), err_msg='%s %s: NaN mask' % (what, key))
            np.testing.assert_array_equal(np.isposinf(dev), np.isposinf(ref), err_msg='%s %s: +inf mask' % (what, key))
            np.testing.assert_array_equal(np.isneginf(dev), np.isneginf(ref), err_msg='%s %s: -inf mask' % (what, key))
            fin = np.isfinite(ref)
            excess = np.where(fin, np.abs(np.where(fin, dev, 0.0) - np.where(fin, ref, 0.0)) - np.where(fin, tol, 0.0), -1.0)
            worst = np.unravel_index(np.argmax(excess), excess.shape)
            print('%s %s: largest |d| / tol = %.3g' % (what, key, np.max(np.where(fin, np.abs(dev - ref) / tol, 0.0))))
            assert excess[worst] <= 0.0, '%s %s: record %s is %.3e beyond its tolerance %.3e' % (what, key, worst, excess[worst], tol[worst])


def _bits(c):
    return c.pack().tobytes()


# ------------------------------------------------------------------------------------------ 1. the device's own trajectories
@pytest.mark.parametrize('frame', ['rf1', 'rf0', 'rf0_ned'])
@pytest.mark.parametrize('precision', ['f64', 'f32'])
@pytest.mark.parametrize('runs', [1, 63, 64, 65, 1000, 4096])
def test_curve_against_the_restatement_on_the_downloaded_trajectories(ctx, runs, precision, frame):
    """Every sample, a stride, a shuffled subset with repeats and the single last sample, on both sides of a wavefront (63 / 64 /
    65 runs), with the two-runs-per-lane loads (1000, 4096) and with the run axis cut into slices (the sparse sets at 4096)."""
    rf, ned = (1 if frame == 'rf1' else 0), frame == 'rf0_ned'
    job, ref_nav = _job(ctx, rf, runs, precision)
    job.run()
    n = job.n
    assert n == 1000
    want = error_curve_ref.curve(_series(job), ref_nav, None, ned)
    rng = np.random.RandomState(runs)
    shuffled = rng.randint(0, n, size=37)
    shuffled[5], shuffled[20] = shuffled[4], shuffled[0]                   # repeats
    for name, rows in (('all', None), ('stride', np.arange(3, n, 7)), ('shuffled', shuffled), ('last', np.array([n - 1]))):
        got = job.error_curve('free', rows, pos_ned=ned)
        assert np.all(got.count == runs)
        _assert_curve(got, want, rows, ned, what='%s %d %s %s' % (frame, runs, precision, name))
        assert _bits(job.error_curve('free', rows, pos_ned=ned)) == _bits(got), 'two launches of the same shape differ'
    job.release()


def test_bad_arguments_are_refused(ctx):
    job, _ = _job(ctx, 1, 8)
    job.run()
    for bad in ([], [-1], [job.n], [0, 5, job.n]):
        with pytest.raises(ValueError):
            job.error_curve('free', bad)
    job.release()
    import ginsim
    from ginsim import workloads
    ini, truth, _ = workloads.truth_from_profile('turn_90deg', FS, 1)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    nokeep = ginsim.MonteCarloJob(ctx, FS, 1, truth, acc, gyr, ini, runs=8).run()
    with pytest.raises(ValueError, match='keep_traj=True'):
        nokeep.error_curve('free')
    nokeep.release()


# ------------------------------------------------------------------------------------------ 2. the C oracle's series
@pytest.mark.parametrize('rf,algo', [(1, 'free'), (1, 'odo'), (0, 'free')])
def test_curve_against_the_restatement_on_the_c_oracle_series(ctx, rf, algo):
    """1024 runs, Philox parity: the restatement on the C oracle's trajectories.  The series tolerances of the parity tests (1e-9
    rad, 2e-8 m in ref_frame 1 / 1e-12 rad and 1e-8 m in ref_frame 0, 1e-9 m/s) bound what a per-sample difference of that size
    can move max |e|, the mean and the std by, and are added to every record's tolerance."""
    from ginsim import workloads
    from oracle import c_oracle
    runs, seed = 1024, 777
    job, ref_nav = _job(ctx, rf, runs, algos=('free', 'odo'), seed=seed)
    job.run()
    ini, truth, _ = workloads.truth_from_profile('turn_90deg', FS, rf)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    _, traj, _ = c_oracle.mc_run(seed, 0, runs, FS, rf, truth, acc, gyr, ini, algo=algo, odo_err={'scale': 0.999, 'stdv': 0.1}, keep=runs)
    want = error_curve_ref.curve(traj, ref_nav, None, False)
    series = np.array([1e-9] * 3 + ([2e-8] * 3 if rf == 1 else [1e-12, 1e-12, 1e-8]) + [1e-9] * 3)
    _assert_curve(job.error_curve(algo), want, None, False, extra=series, what='oracle rf%d %s' % (rf, algo))
    job.release()


# ------------------------------------------------------------------------------------------ 3. the end-point record
@pytest.mark.parametrize('precision', ['f64', 'f32'])
@pytest.mark.parametrize('frame', ['rf1', 'rf0', 'rf0_ned'])
def test_last_row_is_the_end_point_record(ctx, frame, precision):
    """The last row of the curve against the job's end-point record recomputed from the same trajectories (stats_from_traj).
    With 64 runs -- one wavefront, one run per lane, the same shuffle butterfly about the same shift -- bit for bit."""
    rf, ned = (1 if frame == 'rf1' else 0), frame == 'rf0_ned'
    for runs in (64, 1000):
        job, _ = _job(ctx, rf, runs, precision)
        job.run()
        end = job.stats_from_traj('free', pos_ned=ned)
        got = job.error_curve('free', [job.n - 1], pos_ned=ned)
        assert got.count[0] == end.count == runs
        if runs == 64:
            assert got.mean[0].tobytes() == end.mean.tobytes()
            assert got.m2[0].tobytes() == end.m2.tobytes()
            assert got.maxabs[0].tobytes() == end.maxabs.tobytes()
        a = _atol(ned)
        np.testing.assert_array_equal(got.maxabs[0], end.maxabs)
        assert np.all(np.abs(got.mean[0] - end.mean) <= a + 1e-12 * np.abs(end.mean))
        assert np.all(np.abs(got.std[0] - end.std) <= a + 1e-9 * np.abs(end.std))
        job.release()


# ------------------------------------------------------------------------------------------ 5. non-finite values
def test_a_poisoned_run_marks_its_records_and_no_other(ctx):
    """One run's accelerometer is NaN at one sample and another run's is +inf later (through given_sensors).  Every record carries
    the masks NumPy gives on the same trajectories; every record before the first poisoned sample keeps the bits of the launch
    whose runs are all clean."""
    import ginsim
    from ginsim import workloads
    rf, runs, j_nan, j_inf = 1, 130, 400, 700
    ini, truth, _ = workloads.truth_from_profile('turn_90deg', FS, rf)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    src = ginsim.MonteCarloJob(ctx, FS, rf, truth, acc, gyr, ini, runs=runs, seed=5, keep_sensors=True).run()
    n = src.n
    accel = ctx.download(src.buffer('accel'), (3, n, runs))
    gyro = ctx.download(src.buffer('gyro'), (3, n, runs))
    ref_nav = np.ascontiguousarray(np.concatenate([truth['ref_att'], truth['ref_pos'], truth['ref_vel']], axis=1))
    curves = {}
    for tag in ('clean', 'poisoned'):
        a = accel.copy()
        if tag == 'poisoned':
            a[0, j_nan, 77] = np.nan
            a[2, j_inf, 64] = np.inf
        given = {'accel': ctx.upload(a), 'gyro': ctx.upload(gyro)}
        job = ginsim.MonteCarloJob(ctx, FS, rf, truth, None, None, ini, runs=runs, given=given, keep_traj=True).run()
        curves[tag] = job.error_curve('free')
        if tag == 'poisoned':
            with np.errstate(invalid='ignore', over='ignore'):
                want = error_curve_ref.curve(_series(job), ref_nav, None, False)
            _assert_curve(curves[tag], want, None, False, what='poisoned')
            bad = ~np.isfinite(want['avg'])
            assert bad[j_nan + 1:].any() and not bad[:j_nan].any()
            assert np.isnan(want['std'][bad]).all()
        job.release()
        for b in given.values():
            b.free()
    clean, pois = curves['clean'].pack(), curves['poisoned'].pack()
    assert clean[:j_nan].tobytes() == pois[:j_nan].tobytes()
    assert np.isfinite(clean).all()
    # a component the poison has not reached yet keeps its bits as well
    untouched = np.isfinite(pois).all(axis=2) & (np.arange(n) >= j_nan)[:, None]
    assert np.array_equal(clean[untouched], pois[untouched])
    src.release()


# ------------------------------------------------------------------------------------------ 4. / 6. / 7. through Sim
def _sim(runs, rf=1, seed=99, algos=('free',), **kw):
    sys.path[:0] = [PKG] if PKG not in sys.path else []
    from gnss_ins_sim.sim import imu_model, ins_sim
    from demo_algorithms import free_integration, free_integration_odo
    csv = os.path.join(PKG, 'motion_profiles', 'turn_90deg.csv')
    ini = np.genfromtxt(csv, delimiter=',', skip_header=1, max_rows=1)
    ini[0:2] *= np.pi / 180
    ini[6:9] *= np.pi / 180
    odo = 'odo' in algos
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=False, odo=odo, odo_opt={'scale': 0.999, 'stdv': 0.1} if odo else None)
    objs = [(free_integration_odo if a == 'odo' else free_integration).FreeIntegration(ini.copy()) for a in algos]
    sim = ins_sim.Sim([FS, 0.0, 0.0], csv, ref_frame=rf, imu=imu, algorithm=objs if len(objs) > 1 else objs[0], seed=seed, **kw)
    sim.run(runs)
    return sim


def _assert_same_curve(a, b, what):
    """Two Sim.error_curve results agree to rounding: rtol 1e-12 mean / max, 1e-9 std (and the project's atol)."""
    assert sorted(a) == sorted(b)
    for name in a:
        np.testing.assert_array_equal(a[name]['time'], b[name]['time'])
        for stat, rtol in (('max', 1e-12), ('avg', 1e-12), ('std', 1e-9)):
            assert sorted(a[name][stat]) == sorted(b[name][stat])
            for algo in a[name][stat]:
                np.testing.assert_allclose(a[name][stat][algo], b[name][stat][algo], rtol=rtol, atol=1e-9, err_msg='%s %s %s' % (what, name, stat))


BLOCK_BYTES = 16384 * 9 * 8 * 1000          # max_device_bytes that makes _blocks re-integrate 16 384 runs at a time


@pytest.fixture(scope='module')
def kept_c2():
    """BASELINE config 2 (65 536 runs x 1000 samples, fp64), every trajectory kept."""
    sim = _sim(65536, keep_trajectories=True)
    yield sim
    sim.mc.jobs[0].release()


def test_c2_every_sample_against_the_restatement_on_256_time_rows(kept_c2):
    """The curve of C2 over every sample; 256 time rows of the planes are downloaded ([9][n][runs]: a row of one component is
    contiguous), never the 4.7 GB."""
    sim = kept_c2
    job = sim.mc.jobs[0]
    runs, n = job.runs, job.n
    rows = np.unique(np.concatenate([[0, 1, n - 1], np.random.RandomState(2).randint(0, n, size=300)]))[:256]
    rows[-1] = n - 1
    rows = np.unique(rows)
    base = job.buffer('traj_free').ptr
    traj = np.empty((runs, rows.size, 9))
    for c in range(9):
        for k, j in enumerate(rows):
            traj[:, k, c] = job.ctx.download(base + (c * n + int(j)) * runs * 8, (runs,))
    ref_nav = job._ref_nav
    want = error_curve_ref.curve(traj, ref_nav[rows], None, False)
    got = job.error_curve('free')
    assert got.m == n and np.all(got.count == runs)
    import ginsim
    sub = ginsim.CurveResult(got.pack()[rows])
    _assert_curve(sub, want, None, False, what='C2')
    assert _bits(job.error_curve('free')) == _bits(got)


def test_blocked_statistics_only_sim_equals_the_kept_job(kept_c2):
    """A 65 536-run statistics-only Sim re-integrated through _blocks (four blocks of 16 384 runs) against the kept job."""
    whole = kept_c2.error_curve()
    sim = _sim(65536, keep_trajectories=False, max_device_bytes=BLOCK_BYTES)
    assert sim.mc.jobs[0].keep_traj is False and sim.mc._block_runs == 16384
    blocked = sim.error_curve()
    _assert_same_curve(blocked, whole, 'blocked')
    assert blocked['pos']['max']['algo0'].shape == (1000, 3)
    again = sim.error_curve()
    assert again is not blocked and np.array_equal(again['vel']['std']['algo0'], blocked['vel']['std']['algo0'])


@pytest.mark.parametrize('rf', [1, 0])
def test_blocked_fp32_statistics_only_sim_equals_the_kept_fp32_sim(rf):
    """The statistics-only fp32 path: the runs integrated again by the fp32 kernel in four blocks of 2048, each block's float
    series (position as displacement from the origin table, every block with its own first run) reduced by
    ginsim_error_curve_f32 and merged -- against the fp32 Sim that keeps all 8192 trajectories; NED in ref_frame 0."""
    runs, opt = 8192, ('ned' if rf == 0 else '')
    kept = _sim(runs, rf=rf, precision='f32', keep_trajectories=True)
    assert kept.mc.jobs[0].precision == 'f32' and kept.mc.jobs[0].keep_traj
    sim = _sim(runs, rf=rf, precision='f32', keep_trajectories=False, max_device_bytes=2048 * 9 * 4 * 1000)
    assert sim.mc.jobs[0].precision == 'f32' and sim.mc.jobs[0].keep_traj is False and sim.mc._block_runs == 2048
    whole, blocked = kept.error_curve(extra_opt=opt), sim.error_curve(extra_opt=opt)
    _assert_same_curve(blocked, whole, 'fp32 blocked rf%d' % rf)
    assert blocked['pos']['units'] == ['m', 'm', 'm'] and np.all(blocked['pos']['std']['algo0'][-1] > 0.0)
    kept.mc.jobs[0].release()


def test_four_contexts_on_one_device_equal_the_kept_job(kept_c2):
    whole = kept_c2.error_curve(every=0.5)
    sim = _sim(65536, keep_trajectories=False, max_device_bytes=BLOCK_BYTES, devices=[0, 0, 0, 0])
    _assert_same_curve(sim.error_curve(every=0.5), whole, 'devices=[0, 0, 0, 0] blocked')
    kept = _sim(65536, keep_trajectories=True, devices=[0, 0, 0, 0])
    _assert_same_curve(kept.error_curve(every=0.5), whole, 'devices=[0, 0, 0, 0] kept')


def _port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


_WORKER = r'''
import os, sys
sys.path[:0] = [%(pkg)r, %(repo)r]
import numpy as np, torch.distributed as dist
dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%(port)d', rank=int(sys.argv[1]), world_size=2)
os.environ['LOCAL_RANK'] = '0'
from gnss_ins_sim.sim import imu_model, ins_sim
from demo_algorithms import free_integration
csv = os.path.join(%(pkg)r, 'motion_profiles', 'turn_90deg.csv')
ini = np.genfromtxt(csv, delimiter=',', skip_header=1, max_rows=1)
ini[0:2] *= np.pi / 180; ini[6:9] *= np.pi / 180
imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=False)
sim = ins_sim.Sim([100.0, 0.0, 0.0], csv, ref_frame=1, imu=imu, algorithm=free_integration.FreeIntegration(ini), seed=99,
                  keep_trajectories=False, max_device_bytes=%(bytes)d)
sim.run(%(runs)d)
c = sim.error_curve(every=0.5)
np.save(sys.argv[2], np.stack([np.concatenate([c[k][s]['algo0'] for k in ('att_euler', 'pos', 'vel')], axis=1) for s in ('max', 'avg', 'std')]))
dist.barrier(); dist.destroy_process_group()
'''


@pytest.mark.parametrize('runs', [65536, 1])
def test_two_gloo_ranks_sharing_the_device(tmp_path, kept_c2, runs):
    """Two ranks over gloo, each re-integrating its half in blocks; the gathered records give the same curve on both ranks, equal
    to the one-process curve to rounding.  runs = 1: rank 1 holds no run and contributes the empty record."""
    script = tmp_path / 'w.py'
    script.write_text(_WORKER % {'pkg': PKG, 'repo': REPO, 'port': _port(), 'bytes': BLOCK_BYTES, 'runs': runs})
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    procs = [subprocess.Popen([sys.executable, str(script), str(r), str(tmp_path / ('r%d.npy' % r))], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, env=env) for r in range(2)]
    outs = [p.communicate(timeout=600)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    a, b = np.load(tmp_path / 'r0.npy'), np.load(tmp_path / 'r1.npy')
    np.testing.assert_array_equal(a, b)
    one = (kept_c2 if runs == 65536 else _sim(1, keep_trajectories=True)).error_curve(every=0.5)
    for k, (stat, rtol) in enumerate((('max', 1e-12), ('avg', 1e-12), ('std', 1e-9))):
        ref = np.concatenate([one[name][stat]['algo0'] for name in ('att_euler', 'pos', 'vel')], axis=1)
        np.testing.assert_allclose(a[k], ref, rtol=rtol, atol=1e-9)


@pytest.mark.parametrize('rf', [0, 1])
def test_sim_error_curve_units_and_keys(rf):
    """Keys, shapes, time axis and units; the last sample equals what Sim.results(err_stats_start=-1) reports (output units:
    the attitude in degrees), with extra_opt='ned' too; every= and samples= pick the same rows."""
    sim = _sim(1000, rf=rf, algos=('free', 'odo'), keep_trajectories=True)
    assert sim.error_curve.__kwdefaults__ == {'every': None, 'samples': None, 'extra_opt': ''}
    n = sim.dmgr.time.data.shape[0]
    for opt in ('', 'ned'):
        c = sim.error_curve(extra_opt=opt)
        assert sorted(c) == ['att_euler', 'pos', 'vel']
        sim.results(err_stats_start=-1, extra_opt=opt)
        for name in c:
            assert sorted(c[name]) == ['avg', 'max', 'std', 'time', 'units']
            assert c[name]['units'] == eval(sim.err_stats[name]['units'])
            np.testing.assert_array_equal(c[name]['time'], sim.dmgr.time.data)
            for stat, rtol in (('max', 1e-12), ('avg', 1e-12), ('std', 1e-9)):
                assert sorted(c[name][stat]) == ['algo0', 'algo1']
                for algo in ('algo0', 'algo1'):
                    assert c[name][stat][algo].shape == (n, 3)
                    np.testing.assert_allclose(c[name][stat][algo][-1], sim.err_stats[name][stat][algo], rtol=rtol, atol=1e-9)
        assert c['att_euler']['units'] == ['deg', 'deg', 'deg']
        assert c['pos']['units'] == (['m', 'm', 'm'] if rf == 1 or opt == 'ned' else ['deg', 'deg', 'm'])
    one_hz = sim.error_curve(('pos',), every=1.0)
    picked = sim.error_curve('pos', samples=np.arange(0, n, 100))
    assert sorted(one_hz) == ['pos'] and one_hz['pos']['time'].shape == (10,)
    np.testing.assert_array_equal(one_hz['pos']['std']['algo1'], picked['pos']['std']['algo1'])
    np.testing.assert_array_equal(one_hz['pos']['std']['algo1'], sim.error_curve()['pos']['std']['algo1'][::100])
    with pytest.raises(ValueError):
        sim.error_curve(every=1.0, samples=[0])
    with pytest.raises(ValueError):
        sim.error_curve(samples=[n])
    with pytest.raises(ValueError):
        sim.error_curve(('att_quat',))


def test_sim_error_curve_before_run_and_without_fused_plugins(capsys):
    sys.path[:0] = [PKG] if PKG not in sys.path else []
    from gnss_ins_sim.sim import imu_model, ins_sim
    from demo_algorithms import inclinometer_device
    csv = os.path.join(PKG, 'motion_profiles', 'turn_90deg.csv')
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=False)
    sim = ins_sim.Sim([FS, 0.0, 0.0], csv, ref_frame=1, imu=imu, algorithm=inclinometer_device.TiltAcc(), seed=1)
    assert sim.error_curve() is None and 'Call Sim.run()' in capsys.readouterr().out
    sim.run(8)
    with pytest.raises(ValueError, match='inclinometer'):
        sim.error_curve(('att_euler',))


@pytest.mark.parametrize('case', ['turn_rf1', 'turn_rf0_ned', 'wrap_rf1'])
def test_sim_error_curve_against_the_reference_goldens(case):
    """The reference's own calc_data_err + __array_stats at every stored sample (tests/golden/error_curve/*.npz, 16 runs with the
    reference's normals replaced by the engine's Philox normals) through the drop-in Sim with the same seed.  The tolerance of a
    record is the file's (rtol 1e-12 mean / max, 1e-9 std, atol 1e-9, 2e-8 for NED metres, here in the output units) or the
    golden's own bound where that is larger; nothing is added for the device's series against the reference's."""
    import error_curve_cases
    g = load_golden(os.path.join('error_curve', case))
    sim = error_curve_cases.dropin_sim(g, PKG)
    sim.run(int(g['R']))
    rows = g['rows']
    c = sim.error_curve(samples=rows, extra_opt=str(g['extra_opt']))
    ned = int(g['ref_frame']) == 0 and str(g['extra_opt']) == 'ned'
    for name in ('att_euler', 'pos', 'vel'):
        for stat, rtol in (('max', 1e-12), ('avg', 1e-12), ('std', 1e-9)):
            for a, algo in enumerate(error_curve_cases.ALGOS[case]):
                ref = g['%s_%s_algo%d' % (name, stat, a)]
                tol = np.maximum((2e-8 if ned and name == 'pos' else 1e-9) + rtol * np.abs(ref), g['%s_tol_%s_algo%d' % (name, stat, a)])
                got = c[name][stat]['algo%d' % a]
                worst = np.max((np.abs(got - ref) - tol))
                print('%s %s %s %s: largest |d| / tol = %.3g' % (case, name, stat, algo, np.max(np.abs(got - ref) / tol)))
                assert worst <= 0.0, (case, name, stat, algo, worst)
