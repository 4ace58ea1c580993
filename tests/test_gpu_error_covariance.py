"""Error covariance across runs on the device (csrc/error_cov.hip, ginsim_error_cov*, BatchJob.error_cov, JobSet.error_cov,
distributed.allgather_cov, Sim.error_covariance) against the NumPy restatement tests/error_covariance_ref.py.

The parity bound is the record's own, measured on the CPU per case (error_covariance_ref.bounded): per entry |dC_ab| /
sqrt(C_aa C_bb) and |dmean_a| / max(|mean_a|, sigma_a) at most 16 x max(distance of the float64 two-pass record from its long-double
evaluation, spread over eight run orders, eps).  Where the inputs themselves may differ (NED metres, the fp32 origin) what the
component tolerance of tests/test_gpu_error_curve.py (1e-9 max(1, |x|), 2e-8 m for NED) moves an entry by is added
(error_covariance_ref.input_slack).  Every comparison prints its largest |d| / bound.  The jobs run a 64-sample cut of the turn
profile, the Sims a 64-sample motion definition of their own.  Measured on the MI355X: 522 comparisons, every one within 0.125 of
its bound (16 eps in most); the conditioning case bit-equal in ref_frame 1 and at 0.0013 of the bound in ref_frame 0."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, PKG
import error_covariance_cases as cc
import error_covariance_ref as ref

pytestmark = pytest.mark.gpu

FS = cc.FS


@pytest.fixture(scope='module')
def ctx():
    import ginsim
    c = ginsim.Context(0)
    yield c
    c.close()


def _job(ctx, rf, runs, precision='f64', seed=20261019, ini=None, **kw):
    import ginsim
    from ginsim import workloads
    ini0, truth, ref_nav = cc.turn_truth(rf)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    job = ginsim.MonteCarloJob(ctx, FS, rf, truth, acc, gyr, ini0 if ini is None else ini, runs=runs, seed=seed, keep_traj=True,
                               precision=precision, **kw).run()
    return job, ref_nav


def _series(job, algo='free'):
    att, pos, vel = job.trajectories(algo, np.arange(job.runs))
    return np.concatenate([att, pos, vel], axis=2)


def _bounded(job, ref_nav, algo, which, ned, loose_inputs):
    """bounded() of the job's own downloaded trajectories at every sample, and the input slack where the inputs may differ."""
    e = ref.errors3(_series(job, algo), ref_nav, None, which, ned)
    b = ref.bounded(e)
    slack = ref.input_slack(b['rec'], ref.component_tolerance(e, which, ned)) if loose_inputs else None
    return b, slack


def _rows(b, slack, rows):
    if rows is None:
        return b, slack
    rows = np.asarray(rows)
    return {k: v[rows] for k, v in b.items()}, None if slack is None else (slack[0][rows], slack[1][rows])


def _sample_sets(n, seed):
    shuffled = np.random.RandomState(seed).randint(0, n, size=23)
    shuffled[5], shuffled[20] = shuffled[4], shuffled[0]                   # repeats
    return (('all', None), ('one', np.array([n // 3])), ('last', np.array([n - 1])), ('shuffled', shuffled))


# ------------------------------------------------------------------------------------------ 1. the record
@pytest.mark.parametrize('frame', ['rf1', 'rf0', 'rf0_ned'])
@pytest.mark.parametrize('precision', ['f64', 'f32'])
@pytest.mark.parametrize('runs', [1, 2, 63, 64, 65, 127, 128, 129, 257, 1000])
def test_record_against_the_restatement_on_the_downloaded_trajectories(ctx, runs, precision, frame):
    """Position and velocity; every sample, one sample, the last sample and an unordered set with repeats, on both sides of one and
    of two wavefront steps; one sample of 65 runs and more takes the sliced path.  Two launches give the same bytes."""
    rf, ned = (1 if frame == 'rf1' else 0), frame == 'rf0_ned'
    job, ref_nav = _job(ctx, rf, runs, precision)
    assert job.n == cc.CUT
    for which in (0, 1):
        b, slack = _bounded(job, ref_nav, 'free', which, ned, ned or precision == 'f32')
        assert np.all(b['rec'][:, 0] == runs)
        for name, rows in _sample_sets(job.n, runs):
            got = job.error_cov('free', rows, which, pos_ned=ned)
            bb, ss = _rows(b, slack, rows)
            ref.assert_record(got.pack(), bb, '%s %s %d which %d %s' % (frame, precision, runs, which, name), ss)
            assert job.error_cov('free', rows, which, pos_ned=ned).pack().tobytes() == got.pack().tobytes(), 'two launches differ'
        if runs == 1:
            one = job.error_cov('free', None, which, pos_ned=ned)
            assert np.all(one.comoment == 0.0) and np.all(one.cov == 0.0)
    job.release()


@pytest.mark.parametrize('precision,frame', [('f64', 'rf1'), ('f32', 'rf0_ned')])
def test_sliced_path_at_4096_runs(ctx, precision, frame):
    """4096 runs x 1 sample and x 3 samples: 64 slices of the run axis per sample, folded by cov_final_kernel; the record of the same
    sample does not depend on how many others are asked for beyond the bound, and two launches give the same bytes."""
    rf, ned = (1 if frame == 'rf1' else 0), frame == 'rf0_ned'
    job, ref_nav = _job(ctx, rf, 4096, precision)
    for which in (0, 1):
        b, slack = _bounded(job, ref_nav, 'free', which, ned, ned or precision == 'f32')
        for rows in ([job.n - 1], [7, job.n - 1, 30]):
            got = job.error_cov('free', rows, which, pos_ned=ned)
            assert np.all(got.count == 4096)
            bb, ss = _rows(b, slack, rows)
            ref.assert_record(got.pack(), bb, 'sliced %s %s which %d m %d' % (frame, precision, which, len(rows)), ss)
            assert job.error_cov('free', rows, which, pos_ned=ned).pack().tobytes() == got.pack().tobytes()
    job.release()


@pytest.mark.parametrize('rf', [1, 0])
def test_runs_that_all_start_1000_m_off_the_truth(ctx, rf):
    """The conditioning case: 64 runs whose initial altitude is 1000 m off (the ini table), samples 1 and 2, where the spread is
    far below a millimetre and |mean| / sigma beyond 1e6.  The same bound, relative to sqrt(C_aa C_bb); the frame's own axes in
    both frames, so that nothing is added for the inputs."""
    ini0, _, _ = cc.turn_truth(rf)
    ini = np.array(ini0, dtype=np.float64)
    ini[2] += 1000.0
    job, ref_nav = _job(ctx, rf, 64, ini=ini)
    ned = False
    b, slack = _bounded(job, ref_nav, 'free', 0, ned, False)
    rows = [1, 2]
    rec = b['rec'][rows]
    sigma = np.sqrt(np.array([rec[:, 4], rec[:, 7], rec[:, 9]]).T / 64.0)
    print('rf%d: |mean| %s, sigma %s' % (rf, np.abs(rec[:, 1:4]).max(axis=0), sigma.max(axis=0)))
    assert np.linalg.norm(rec[:, 1:4], axis=1).min() > 999.0 and 0.0 < sigma.max() < 1e-3
    got = job.error_cov('free', rows, 0, pos_ned=ned)
    bb, ss = _rows(b, slack, rows)
    ref.assert_record(got.pack(), bb, 'conditioning rf%d' % rf, ss)
    job.release()


# ------------------------------------------------------------------------------------------ 2. non-finite values
def test_runs_that_are_not_finite_are_counted_out_at_their_samples_only(ctx):
    """Through given sensors: run 77's accelerometer is NaN at sample 10, run 64's is +inf at sample 20, every run but run 5 is NaN
    at sample 40 and run 5 at sample 55.  The counts are the restatement's on the same trajectories: 130, 129, 128, then the one
    surviving run (its error, an exactly zero covariance), then none (NaN, count 0); every record of a sample that no poisoned run
    has reached is bit for bit that of the clean launch."""
    import ginsim
    from ginsim import workloads
    rf, runs = 1, 130
    ini, truth, ref_nav = cc.turn_truth(rf)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    src = ginsim.MonteCarloJob(ctx, FS, rf, truth, acc, gyr, ini, runs=runs, seed=5, keep_sensors=True).run()
    n = src.n
    accel = ctx.download(src.buffer('accel'), (3, n, runs))
    gyro = ctx.download(src.buffer('gyro'), (3, n, runs))
    got = {}
    for tag in ('clean', 'poisoned'):
        a = accel.copy()
        if tag == 'poisoned':
            a[0, 10, 77] = np.nan
            a[2, 20, 64] = np.inf
            a[1, 40, :] = np.nan
            a[1, 40, 5] = accel[1, 40, 5]
            a[0, 55, 5] = np.nan
        given = {'accel': ctx.upload(a), 'gyro': ctx.upload(gyro)}
        job = ginsim.MonteCarloJob(ctx, FS, rf, truth, None, None, ini, runs=runs, given=given, keep_traj=True).run()
        got[tag] = [job.error_cov('free', None, which).pack() for which in (0, 1)]
        if tag == 'poisoned':
            series = _series(job)
            for which in (0, 1):
                b = ref.bounded(ref.errors3(series, ref_nav, None, which, False))
                ref.assert_record(got[tag][which], b, 'poisoned which %d' % which)
                assert sorted(set(b['rec'][:, 0].tolist())) == [0.0, 1.0, 128.0, 129.0, 130.0]
        job.release()
        for buf in given.values():
            buf.free()
    for which in (0, 1):
        clean, pois = got['clean'][which], got['poisoned'][which]
        assert np.all(clean[:, 0] == runs) and np.isfinite(clean).all()
        full = pois[:, 0] == runs
        assert full[:10].all() and not full[12:].any()
        assert clean[full].tobytes() == pois[full].tobytes()
        assert np.all(np.diff(pois[:, 0]) <= 0)
        none = pois[:, 0] == 0
        assert none[-1] and np.isnan(pois[none][:, 1:]).all()
        single = pois[:, 0] == 1
        assert single.any() and np.all(pois[single][:, 4:] == 0.0) and np.isfinite(pois[single][:, 1:4]).all()
    src.release()


def test_bad_arguments_are_refused(ctx):
    import ginsim
    from ginsim import workloads
    job, _ = _job(ctx, 1, 8)
    for bad in ([], [-1], [job.n], [0, 5, job.n]):
        with pytest.raises(ValueError, match='error_cov'):
            job.error_cov('free', bad)
    with pytest.raises(ValueError, match='which=2'):
        job.error_cov('free', [0], 2)
    job.release()
    ini, truth, _ = cc.turn_truth(1)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    nokeep = ginsim.MonteCarloJob(ctx, FS, 1, truth, acc, gyr, ini, runs=8).run()
    with pytest.raises(ValueError, match='keep_traj=True'):
        nokeep.error_cov('free')
    nokeep.release()


# ------------------------------------------------------------------------------------------ 3. an InsLoose job
@pytest.mark.parametrize('rf', [1, 0])
def test_record_of_an_ins_loose_job(ctx, rf):
    """InsLooseJob(keep_traj=True), 65 runs, 10 Hz GPS, the first 64 samples of the outage profile."""
    import ginsim
    import ins_loose_cases as cs
    ini, truth, _ = cs.outage_truth(FS, rf, 10.0, 64)
    acc_e, gyr_e = cs.imu_errors()
    job = ginsim.InsLooseJob(ctx, FS, rf, truth, acc_e, gyr_e, cs.GPS_ERR, ini, 65, seed=11, keep_traj=True).run()
    ned = rf == 0
    for which in (0, 1):
        b, slack = _bounded(job, job._ref_nav, 'loose', which, ned, ned)
        for rows in (None, [job.n - 1], [40, 3, 3]):
            bb, ss = _rows(b, slack, rows)
            ref.assert_record(job.error_cov(None, rows, which, pos_ned=ned).pack(), bb, 'InsLoose rf%d which %d' % (rf, which), ss)
    job.release()


# ------------------------------------------------------------------------------------------ 4. blocks, contexts, ranks
RUNS = 4096
ROWS = np.array([1, 20, 63, 40])


def _block_bytes(esize):
    return 1024 * 9 * esize * cc.CUT        # max_device_bytes that makes _blocks re-integrate 1024 runs at a time


def _kept_bounds(sim, loose_inputs):
    """{which: (bounded rows, slack rows)} from the kept Sim's own trajectories at ROWS."""
    job = sim.mc.jobs[0]
    assert job.keep_traj and job.n == cc.CUT
    ned = sim.ref_frame == 0
    out = {}
    for which in (0, 1):
        b, slack = _bounded(job, job._ref_nav, 'free', which, ned, loose_inputs or ned)
        out[which] = _rows(b, slack, ROWS)
    return out


def _record_of(sim, which):
    return sim.mc.error_covariance(sim.mc.nav_names[0], ROWS, cc.CUT, which, ned=sim.ref_frame == 0).pack()


@pytest.fixture(scope='module')
def kept_f64():
    sim = cc.short_sim(PKG, RUNS, keep_trajectories=True)
    yield sim, _kept_bounds(sim, False)
    sim.mc.jobs[0].release()


def test_blocked_statistics_only_sim_equals_whole(kept_f64):
    """Statistics only, integrated again in four blocks of 1024 whose records are merged on the host -- and the kept Sim in one
    call -- against the restatement on the kept trajectories."""
    kept, bounds = kept_f64
    sim = cc.short_sim(PKG, RUNS, keep_trajectories=False, max_device_bytes=_block_bytes(8))
    assert sim.mc.jobs[0].keep_traj is False and sim.mc._block_runs == 1024
    for which in (0, 1):
        bb, ss = bounds[which]
        ref.assert_record(_record_of(kept, which), bb, 'kept which %d' % which, ss)
        ref.assert_record(_record_of(sim, which), bb, 'blocked which %d' % which, ss)


@pytest.mark.parametrize('rf', [1, 0])
def test_blocked_fp32_statistics_only_sim_equals_the_kept_fp32_sim(rf):
    """The statistics-only fp32 path: four blocks of 1024 float series (position as displacement from the origin table, every block
    with its own first run) through ginsim_error_cov_f32, merged -- against the restatement on the kept fp32 Sim's trajectories;
    NED in ref_frame 0."""
    kept = cc.short_sim(PKG, RUNS, rf=rf, precision='f32', keep_trajectories=True)
    assert kept.mc.jobs[0].precision == 'f32'
    bounds = _kept_bounds(kept, True)
    sim = cc.short_sim(PKG, RUNS, rf=rf, precision='f32', keep_trajectories=False, max_device_bytes=_block_bytes(4))
    assert sim.mc.jobs[0].precision == 'f32' and sim.mc.jobs[0].keep_traj is False and sim.mc._block_runs == 1024
    for which in (0, 1):
        bb, ss = bounds[which]
        ref.assert_record(_record_of(kept, which), bb, 'fp32 kept rf%d which %d' % (rf, which), ss)
        ref.assert_record(_record_of(sim, which), bb, 'fp32 blocked rf%d which %d' % (rf, which), ss)
    kept.mc.jobs[0].release()


def test_two_contexts_on_one_device_equal_whole(kept_f64):
    _, bounds = kept_f64
    spread = cc.short_sim(PKG, RUNS, keep_trajectories=True, devices=[0, 0])
    blocked = cc.short_sim(PKG, RUNS, keep_trajectories=False, max_device_bytes=_block_bytes(8), devices=[0, 0])
    assert spread.mc.devices == [0, 0] and blocked.mc.jobs[0].keep_traj is False
    for which in (0, 1):
        bb, ss = bounds[which]
        ref.assert_record(_record_of(spread, which), bb, 'devices=[0, 0] kept which %d' % which, ss)
        ref.assert_record(_record_of(blocked, which), bb, 'devices=[0, 0] blocked which %d' % which, ss)
    spread.mc.jobs[0].release()


def _port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


_WORKER = r'''
import os, sys
sys.path[:0] = [%(pkg)r, %(repo)r, %(tests)r]
import numpy as np, torch.distributed as dist
dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%(port)d', rank=int(sys.argv[1]), world_size=2)
os.environ['LOCAL_RANK'] = '0'
import error_covariance_cases as cc
rows = np.array(%(rows)r, dtype=np.int64)
out = []
for runs in (%(runs)d, 1):
    sim = cc.short_sim(%(pkg)r, runs, keep_trajectories=False, max_device_bytes=%(bytes)d)
    out.append(np.stack([sim.mc.error_covariance(sim.mc.nav_names[0], rows, cc.CUT, which).pack() for which in (0, 1)]))
np.save(sys.argv[2], np.stack(out))
dist.barrier(); dist.destroy_process_group()
'''


def test_two_gloo_ranks_sharing_the_device(tmp_path, kept_f64):
    """Two ranks over gloo, each re-integrating its half in blocks; the gathered records give the same record on both ranks, within
    the bound of the restatement on the one-process kept trajectories.  Then one run in all: rank 1 holds none and contributes the
    empty record to the same collective."""
    _, bounds = kept_f64
    script = tmp_path / 'w.py'
    script.write_text(_WORKER % {'pkg': PKG, 'repo': REPO, 'tests': os.path.join(REPO, 'tests'), 'port': _port(), 'bytes': _block_bytes(8),
                                 'runs': RUNS, 'rows': ROWS.tolist()})
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    procs = [subprocess.Popen([sys.executable, str(script), str(r), str(tmp_path / ('r%d.npy' % r))], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, env=env) for r in range(2)]
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    a, b = np.load(tmp_path / 'r0.npy'), np.load(tmp_path / 'r1.npy')
    assert a.tobytes() == b.tobytes()
    for which in (0, 1):
        bb, ss = bounds[which]
        ref.assert_record(a[0, which], bb, 'two ranks which %d' % which, ss)
    one = cc.short_sim(PKG, 1, keep_trajectories=True)
    for which in (0, 1):
        want = _record_of(one, which)
        assert np.all(want[:, 0] == 1) and np.all(want[:, 4:] == 0.0)
        assert a[1, which].tobytes() == want.tobytes()
    one.mc.jobs[0].release()


# ------------------------------------------------------------------------------------------ 5. through Sim
@pytest.mark.parametrize('rf', [1, 0])
def test_sim_error_covariance_against_sim_error_curve(rf):
    """257 kept runs: keys, shapes, axes, units and time; sqrt(diag(cov)) and mean in 'nav' against Sim.error_curve's std and avg at
    the same samples (rtol 1e-9, atol 1e-9, 2e-8 for NED metres); 'track' is the rotation of 'nav' by the truth's yaw; corr and
    ellipse follow from cov; cached, and copies are handed out; the refusals."""
    import ginsim
    sim = cc.short_sim(PKG, 257, rf=rf, keep_trajectories=True)
    assert sim.error_covariance.__kwdefaults__ == {'every': None, 'samples': None, 'frame': 'track'}
    t = np.asarray(sim.dmgr.time.data)
    n = t.shape[0]
    rows = np.arange(0, n, 10)
    name = sim.mc.nav_names[0]
    nav = sim.error_covariance(('pos', 'vel'), every=0.1, frame='nav')
    trk = sim.error_covariance(('pos', 'vel'), samples=rows)
    curve = sim.error_curve(('pos', 'vel'), samples=rows, extra_opt='ned' if rf == 0 else '')
    yaw = np.asarray(sim.dmgr.ref_att_euler.data)[rows, 0]
    assert sorted(nav) == ['pos', 'vel']
    for nm in ('pos', 'vel'):
        r, k = nav[nm], trk[nm]
        assert sorted(r) == ['axes', 'corr', 'count', 'cov', 'ellipse', 'frame', 'mean', 'time', 'units']
        assert r['units'] == (['m'] if nm == 'pos' else ['m/s']) and r['frame'] == 'nav' and k['frame'] == 'track'
        assert r['axes'] == (('north', 'east', 'down') if rf == 0 else ('x', 'y', 'z')) and k['axes'] == ('along', 'cross', 'down')
        np.testing.assert_array_equal(r['time'], t[rows])
        assert r['count'][name].shape == (rows.size,) and np.all(r['count'][name] == 257)
        assert r['mean'][name].shape == (rows.size, 3) and r['cov'][name].shape == (rows.size, 3, 3)
        assert r['corr'][name].shape == (rows.size, 3, 3) and r['ellipse'][name].shape == (rows.size, 3)
        atol = 2e-8 if (rf == 0 and nm == 'pos') else 1e-9
        std = np.sqrt(np.einsum('kaa->ka', r['cov'][name]))
        np.testing.assert_allclose(std, curve[nm]['std'][name], rtol=1e-9, atol=atol)
        np.testing.assert_allclose(r['mean'][name], curve[nm]['avg'][name], rtol=1e-9, atol=atol)
        wm, wc = ref.track_frame(r['mean'][name], r['cov'][name], yaw)
        np.testing.assert_allclose(k['mean'][name], wm, rtol=1e-12, atol=1e-14 * np.abs(wm).max())
        np.testing.assert_allclose(k['cov'][name], wc, rtol=1e-12, atol=1e-14 * np.abs(wc).max())
        for res in (r, k):
            cov = res['cov'][name]
            for s in range(1, rows.size):
                want = ref.error_ellipse(cov[s, :2, :2])
                np.testing.assert_allclose(res['ellipse'][name][s], want, rtol=1e-12, atol=1e-9)
                sd = np.sqrt(np.diag(cov[s]))
                np.testing.assert_allclose(res['corr'][name][s], cov[s] / np.outer(sd, sd), rtol=1e-12)
                assert np.allclose(np.diag(res['corr'][name][s]), 1.0) and np.all(np.abs(res['corr'][name][s]) <= 1.0 + 1e-12)
        assert np.isnan(r['corr'][name][0]).all() and np.all(r['cov'][name][0] == 0.0)       # sample 0: every run is at the truth
    again = sim.error_covariance('pos', samples=rows)['pos']
    assert again['cov'][name] is not trk['pos']['cov'][name]
    np.testing.assert_array_equal(again['cov'][name], trk['pos']['cov'][name])
    every = sim.error_covariance('vel', frame='nav')['vel']
    assert every['time'].shape == (n,) and every['cov'][name].shape == (n, 3, 3)
    np.testing.assert_array_equal(every['cov'][name][rows], nav['vel']['cov'][name])
    with pytest.raises(ValueError, match="'att_euler' has no error covariance"):
        sim.error_covariance(('att_euler',))
    with pytest.raises(ValueError, match="frame='body'"):
        sim.error_covariance(frame='body')
    with pytest.raises(ValueError, match='not both'):
        sim.error_covariance(every=1.0, samples=[0])
    with pytest.raises(ValueError, match='samples must be indices'):
        sim.error_covariance(samples=[n])
    with pytest.raises(ValueError, match='shorter than one sample'):
        sim.error_covariance(every=1e-4)
    sim.mc.jobs[0].release()


def _outage_sim(algos, runs, keep, fs=20.0, fs_gps=2.0, **kw):
    sys.path[:0] = [PKG] if PKG not in sys.path else []
    import ins_loose_cases as cs
    from gnss_ins_sim.sim import imu_model, ins_sim
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=True, odo=True)
    sim = ins_sim.Sim([fs, fs_gps, 0.0], cs.OUTAGE_CSV, ref_frame=1, imu=imu, algorithm=algos, seed=1234, keep_trajectories=keep, **kw)
    sim.run(runs)
    return sim


def test_statistics_only_ins_loose_and_sims_without_a_navigation_plugin_are_refused(capsys):
    sys.path[:0] = [PKG] if PKG not in sys.path else []
    from demo_algorithms.ins_loose_device import InsLoose
    sim = _outage_sim([InsLoose()], 64, False)
    with pytest.raises(ValueError, match=r'error_covariance: .* \(InsLoose\) kept statistics only'):
        sim.error_covariance()
    from gnss_ins_sim.sim import imu_model, ins_sim
    from demo_algorithms import inclinometer_device
    csv = os.path.join(PKG, 'motion_profiles', 'turn_90deg.csv')
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=False)
    sim = ins_sim.Sim([FS, 0.0, 0.0], csv, ref_frame=1, imu=imu, algorithm=inclinometer_device.TiltAcc(), seed=1)
    assert sim.error_covariance() is None and 'Call Sim.run()' in capsys.readouterr().out
    sim.run(8)
    with pytest.raises(ValueError, match='inclinometer'):
        sim.error_covariance()


def test_the_odometer_leaves_a_strip_across_the_track_on_the_device():
    """Sim.error_covariance of [InsLoose(odo=True)] on the outage profile, 257 runs at 20 Hz with 2 Hz GPS: at the outage's last
    sample the along-track sigma is below a quarter of the cross-track sigma, and the ellipse says the same in the nav frame."""
    sys.path[:0] = [PKG] if PKG not in sys.path else []
    import ins_loose_aided_cases as ac
    from demo_algorithms.ins_loose_device import InsLoose
    sim = _outage_sim([InsLoose(odo=True)], 257, True)
    _, truth, stamps = ac.outage_truth(20.0, 1, 2.0)
    j = ac.outage_samples(truth, stamps, 20.0, 2.0)[1]
    name = sim.mc.nav_names[0]
    trk = sim.error_covariance('pos', samples=[j])['pos']
    nav = sim.error_covariance('pos', samples=[j], frame='nav')['pos']
    along, cross = np.sqrt(trk['cov'][name][0, 0, 0]), np.sqrt(trk['cov'][name][0, 1, 1])
    sx, sy = np.sqrt(nav['cov'][name][0, 0, 0]), np.sqrt(nav['cov'][name][0, 1, 1])
    print('InsLoose(odo=True), %d runs at the outage end: sx %.3f sy %.3f along %.3f cross %.3f, ellipse %s (nav) %s (track)'
          % (257, sx, sy, along, cross, nav['ellipse'][name][0], trk['ellipse'][name][0]))
    assert trk['count'][name][0] == 257
    assert along < 0.25 * cross, (along, cross)
    assert trk['ellipse'][name][0, 1] <= along * (1 + 1e-9) and abs(abs(trk['ellipse'][name][0, 2]) - 90.0) < 15.0
    for _, job, _ in sim.loose_jobs:
        job.release()
