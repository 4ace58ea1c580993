"""GPU: MahonyFilter / TiltAcc of demo_algorithms.inclinometer_device on the inclinometer kernel (csrc/inclinometer.hip) --
against the unmodified reference's goldens through the drop-in Sim, the exactness of the run chain, the sensors of the
free-integration kernel, the statistics, kept runs, 65 536 runs against the NumPy restatement, edge cases, refusals."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest

from conftest import GOLDEN
import inclinometer_ref as iref


def load_golden(name):
    import os
    return dict(np.load(os.path.join(GOLDEN, 'inclinometer', name + '.npz'), allow_pickle=False))

pytestmark = pytest.mark.gpu
SEED = 4242


def _ctx():
    import ginsim
    return ginsim.default_context()


def _turn(fs=100.0, rf=1):
    from ginsim import workloads
    ini, truth, _ = workloads.truth_from_profile('turn_90deg', fs, rf)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    return truth, acc, gyr


def _job(runs, truth, acc, gyr, **kw):
    import ginsim
    kw.setdefault('seed', SEED)
    return ginsim.InclinometerJob(_ctx(), 100.0, truth, acc, gyr, runs, **kw)


def _quat_close(a, b, tol):
    d = np.minimum(np.max(np.abs(a - b), axis=-1), np.max(np.abs(a + b), axis=-1))
    assert np.max(d) < tol, np.max(d)


def _ang_close(a, b, tol):
    d = np.mod(a - b + np.pi, 2 * np.pi) - np.pi
    assert np.max(np.abs(d)) < tol, np.max(np.abs(d))


# --------------------------------------------------------------------------------------------- 1. goldens through the Sim
@pytest.mark.parametrize('name', ['incl_mahony_tilt_rf1', 'incl_mag9_gps_rf0', 'incl_chain_rf1'])
def test_goldens_through_the_dropin_sim(name):
    from gnss_ins_sim.sim import imu_model, ins_sim
    from demo_algorithms.inclinometer_device import MahonyFilter, TiltAcc
    g = load_golden(name)
    R, fs, axis, rf = int(g['R']), float(g['fs']), int(g['axis']), int(g['ref_frame'])
    gps = float(g['fs_gps']) > 0
    imu = imu_model.IMU(accuracy='mid-accuracy' if axis == 6 else 'low-accuracy', axis=axis, gps=gps)
    mah = MahonyFilter()
    algos = [mah, TiltAcc()] if name != 'incl_chain_rf1' else [mah]
    for call in range(int(g['calls'])):
        p = 'c%d_' % call
        assert np.max(np.abs(mah.gyro_bias - g[p + 'bias_before'])) < 1e-12
        sim = ins_sim.Sim([fs, float(g['fs_gps']), fs if axis == 9 else 0.0], str(g['profile']), ref_frame=rf, imu=imu,
                          algorithm=algos, seed=int(g['seed']), geo_mag_n=g['geo_mag_n'] if axis == 9 else None)
        sim.run(R)
        assert sim.passes and sim.passes[0] <= R + 1
        d = sim.dmgr
        k = g[p + 'rows']
        names = ['algo0'] + (['StaticTilt'] if len(algos) > 1 else [])
        for nm in names:
            q = np.stack([d.att_quat.data[nm + '_%d' % r] for r in range(R)])
            _quat_close(q[:, k], g[p + nm + '_att_quat'], 1e-9)
            e = np.stack([d.att_euler.data[nm + '_%d' % r] for r in range(R)])
            _ang_close(e[:, k], g[p + nm + '_att_euler'], 1e-9)
        wb = np.stack([d.wb.data['algo0_%d' % r] for r in range(R)])
        ab = np.stack([d.ab.data['algo0_%d' % r] for r in range(R)])
        assert np.max(np.abs(wb[:, k] - g[p + 'wb'])) < 1e-9 and np.max(np.abs(ab[:, k] - g[p + 'ab'])) < 1e-9
        assert np.max(np.abs(mah.gyro_bias - g[p + 'bias_after'])) < 1e-12
        assert np.max(np.abs(mah.wb[-1] - g[p + 'wb_last'][-1])) < 1e-12
        st = d.get_error_stats('att_euler', err_stats_start=-1, angle=True, use_output_units=False)
        for s in ('max', 'avg', 'std'):
            for nm in names:
                got = st[s][nm] if isinstance(st[s], dict) else st[s]
                assert np.allclose(got, g['%send_%s_%s' % (p, s, nm)], rtol=1e-7, atol=1e-10)
        st = d.get_error_stats('att_euler', err_stats_start=2.0, angle=True, use_output_units=False)
        for s in ('max', 'avg', 'std'):
            got = np.stack([st[s][kk] for kk in g[p + 'proc_keys']])
            assert np.allclose(got, g[p + 'proc_' + s], rtol=1e-7, atol=1e-10)
        buf = io.StringIO()
        with redirect_stdout(buf):
            sim.results()
        # the reference's att_euler description has two spaces before 'from algo' (ins_data_manager.py:183); the drop-in's
        # registry has always printed one, and tests/test_gpu_reference_script.py pins that
        assert sim.sum == str(g[p + 'summary']).replace('(Euler, ZYX)  from algo', '(Euler, ZYX) from algo')


def test_statistics_only_sim_matches_the_kept_one():
    from gnss_ins_sim.sim import imu_model, ins_sim
    from demo_algorithms.inclinometer_device import MahonyFilter, TiltAcc
    g = load_golden('incl_mahony_tilt_rf1')
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=False)
    sums = []
    for keep in (True, False):
        sim = ins_sim.Sim([100.0, 0.0, 0.0], str(g['profile']), ref_frame=1, imu=imu, algorithm=[MahonyFilter(), TiltAcc()],
                          seed=int(g['seed']), keep_trajectories=keep, keep_runs=0 if keep else 2)
        sim.run(5)
        with redirect_stdout(io.StringIO()):
            sim.results()
        sums.append(sim.sum)
        if not keep:        # the kept runs of a statistics-only Sim are the same records
            assert len(sim.dmgr.att_quat.data) == 4
    assert sums[0] == sums[1]


# --------------------------------------------------------------------------------------------- 2. the chain
@pytest.mark.parametrize('R', [64, 1000])
def test_chain_is_exact(R):
    truth, acc, gyr = _turn()
    truth = {k: v[:400] for k, v in truth.items()}          # 4 s: the runs forget little of their start
    b0 = np.array([1e-4, -2e-4, 3e-5])
    job = _job(R, truth, acc, gyr, bias0=b0, stats=True, proc_first=50).run()
    assert 1 < job.passes <= R + 1
    print('R=%d passes=%d launched=%s' % (R, job.passes, job.launched))
    fin, ini, end, proc = job.final_biases(), job.initial_biases(), job.end_errors('mahony'), job.process_stats_online('mahony')
    step = 1 if R <= 64 else 97
    prev = b0
    for r in range(R):
        one = _job(1, truth, acc, gyr, start_bias=prev.reshape(1, 3), run_offset=r, stats=True, proc_first=50).run()
        if r % step == 0 or r == R - 1:
            assert np.array_equal(ini[r], prev)
            assert np.array_equal(one.final_biases()[0], fin[r])
            assert np.array_equal(one.end_errors('mahony')[0], end[r])
            assert np.array_equal(one.process_stats_online('mahony')[0], proc[r])
        prev = one.final_biases()[0]
        one.release()
    job.release()


# --------------------------------------------------------------------------------------------- 3. the engine's sensors
def test_given_sensors_of_a_free_integration_job_give_the_same_bits():
    import ginsim
    truth, acc, gyr = _turn()
    ini = np.zeros(9)
    R = 300
    mc = ginsim.MonteCarloJob(_ctx(), 100.0, 1, truth, acc, gyr, ini, runs=R, seed=SEED, keep_sensors=True).run()
    gen = _job(R, truth, acc, gyr, keep=True, stats=True).run()
    giv = _job(R, truth, None, None, keep=True, stats=True, given={'accel': mc.buffer('accel'), 'gyro': mc.buffer('gyro')}).run()
    assert gen.kernel_name().endswith('<3, false, false>') and giv.kernel_name().endswith('<3, true, false>')
    assert gen.passes == giv.passes
    ids = [0, 1, 63, 64, 299]
    for nm in ('quat_mahony', 'quat_tilt', 'euler_mahony', 'euler_tilt', 'wb', 'ab'):
        assert np.array_equal(gen.series(nm, ids), giv.series(nm, ids)), nm
    assert np.array_equal(gen.final_biases(), giv.final_biases())
    for a in ('mahony', 'tilt'):
        assert np.array_equal(gen.process_stats_online(a), giv.process_stats_online(a))
    for j in (mc, gen, giv):
        j.release()


# --------------------------------------------------------------------------------------------- 4. statistics, 5. kept runs
def test_online_statistics_equal_those_of_the_kept_series():
    truth, acc, gyr = _turn()
    R, first = 200, 120
    job = _job(R, truth, acc, gyr, keep=True, stats=True, proc_first=first).run()
    ids = np.arange(R)
    for a in ('mahony', 'tilt'):
        e = job.series('euler_' + a, ids)
        end, proc = iref.stats(e, truth['ref_att'], first)
        _ang_close(job.end_errors(a), end, 1e-12)
        assert np.allclose(job.process_stats_online(a)[:, :, 0:3], proc, rtol=1e-9, atol=1e-13)
        st = job.stats(a)
        assert np.allclose(st.maxabs[0:3], np.max(np.abs(end), 0), rtol=1e-12)
        assert np.allclose(st.mean[0:3], np.mean(end, 0), rtol=1e-9, atol=1e-15)
    job.release()


def test_kept_runs_are_the_runs_of_the_full_launch():
    truth, acc, gyr = _turn()
    R, K = 700, 9
    full = _job(R, truth, acc, gyr, keep=True, stats=True).run()
    stats = _job(R, truth, acc, gyr, stats=True).run()
    kept = _job(K, truth, acc, gyr, keep=True, stats=False, start_bias=stats.initial_biases()[:K]).run()
    assert np.array_equal(stats.initial_biases(), full.initial_biases())
    for nm in ('quat_mahony', 'quat_tilt', 'euler_mahony', 'wb', 'ab'):
        assert np.array_equal(kept.series(nm, np.arange(K)), full.series(nm, np.arange(K))), nm
    for a in ('mahony', 'tilt'):
        assert np.array_equal(stats.process_stats_online(a), full.process_stats_online(a))
    for j in (full, stats, kept):
        j.release()


# --------------------------------------------------------------------------------------------- 6. full size
def test_full_size_against_the_numpy_restatement():
    from oracle import ins_np
    truth, acc, gyr = _turn()
    R = 65536
    job = _job(R, truth, acc, gyr, stats=True).run()
    print('65536 runs of the 90-degree turn: passes=%d launched=%s' % (job.passes, job.launched))
    assert job.passes <= R + 1
    ids = np.array([0, R // 2, R - 1])
    accel, gyro = ins_np.mc_sensors(SEED, ids, 100.0, truth['ref_accel'], truth['ref_gyro'], acc, gyr)
    ini = job.initial_biases()[ids]
    q, wb, ab, fin = iref.mahony(gyro, accel, 0.01, ini)
    assert np.max(np.abs(fin - job.final_biases()[ids])) < 1e-11
    end, proc = iref.stats(iref.quat2euler(q), truth['ref_att'])
    _ang_close(job.end_errors('mahony')[ids], end, 1e-9)
    assert np.allclose(job.process_stats_online('mahony')[ids][:, :, 0:3], proc, rtol=1e-7, atol=1e-11)
    tend, _ = iref.stats(iref.quat2euler(iref.tilt(accel)), truth['ref_att'])
    _ang_close(job.end_errors('tilt')[ids], tend, 1e-9)
    job.release()


# --------------------------------------------------------------------------------------------- 7. edge cases
def test_one_run_one_sample_and_a_window_after_the_end():
    truth, acc, gyr = _turn()
    one = _job(1, truth, acc, gyr, keep=True, stats=True).run()
    assert one.passes == 1
    short = {k: v[:1] for k, v in truth.items()}
    s = _job(5, short, acc, gyr, keep=True, stats=True).run()
    assert s.series('wb', [4]).shape == (1, 1, 3)
    late = _job(5, truth, acc, gyr, stats=True, proc_first=truth['ref_accel'].shape[0] + 10).run()
    assert np.array_equal(late.process_stats_online('mahony'), np.zeros((5, 3, 9)))
    for j in (one, s, late):
        j.release()


@pytest.mark.parametrize('env', [('random', {'type': 'random', 'x': 0.05, 'y': 0.02, 'z': 0.03}),
                                 ('sinusoidal', {'type': 'sinusoidal', 'x': 0.01, 'y': 0.02, 'z': 0.005, 'freq': 2.5})])
def test_vibration_environments(env):
    from oracle import ins_np
    truth, acc, gyr = _turn()
    R = 70
    job = _job(R, truth, acc, gyr, keep=True, stats=False, vib_accel=env[1], vib_gyro=env[1]).run()
    ids = np.array([0, 69])
    accel, gyro = ins_np.mc_sensors(SEED, ids, 100.0, truth['ref_accel'], truth['ref_gyro'], acc, gyr, vib_accel=env[1], vib_gyro=env[1])
    q, wb, ab, _ = iref.mahony(gyro, accel, 0.01, job.initial_biases()[ids])
    assert np.max(np.abs(job.series('wb', ids) - wb)) < 1e-10
    _quat_close(job.series('quat_mahony', ids), q, 1e-9)
    job.release()


def _given(accel, gyro, **kw):
    ctx = _ctx()
    R, n, _ = accel.shape
    bufs = {'accel': ctx.upload(np.ascontiguousarray(accel.transpose(2, 1, 0))),
            'gyro': ctx.upload(np.ascontiguousarray(gyro.transpose(2, 1, 0)))}
    truth = {'ref_accel': np.zeros((n, 3)), 'ref_gyro': np.zeros((n, 3)), 'ref_att': np.zeros((n, 3))}
    return _job(R, truth, None, None, given=bufs, keep=True, **kw).run()


def test_given_records_that_reach_the_rare_branches():
    n = 40
    accel, gyro = np.zeros((4, n, 3)), np.zeros((4, n, 3))
    accel[0, :, 2] = -9.8                                   # level, no rate: theta == 0 after the first step
    accel[1, :, 0] = 9.8                                    # +x: acc[0] >= 1.0 initialisation
    accel[2, :, 1] = -9.8                                   # -y: acc[1] <= -1.0 initialisation
    accel[3, :, 2] = -9.8
    gyro[3, :, 2] = 0.5 * np.pi / 0.01 / 10                 # yaw through 180 degrees: q0 changes sign
    job = _given(accel, gyro, start_bias=np.zeros((4, 3)), stats=True)
    q, wb, ab, fin = iref.mahony(gyro, accel, 0.01, np.zeros((4, 3)))
    dq = job.series('quat_mahony', np.arange(4))
    _quat_close(dq, q, 1e-12)
    assert np.max(np.abs(job.series('wb', np.arange(4)) - wb)) < 1e-14
    assert np.array_equal(dq[0, -1], [1.0, 0.0, 0.0, 0.0])
    assert np.all(np.isfinite(dq))
    # TiltAcc on an accelerometer along its pseudo-magnetometer (+x) divides 0 by 0 in the reference too: NaN where it has NaN
    tq, rq = job.series('quat_tilt', np.arange(4)), iref.tilt(accel)
    assert np.array_equal(np.isnan(tq), np.isnan(rq)) and np.isnan(tq[1]).all() and not np.isnan(tq[[0, 2, 3]]).any()
    _quat_close(tq[[0, 2, 3]], rq[[0, 2, 3]], 1e-14)
    job.release()


# --------------------------------------------------------------------------------------------- 8. plugin surface, 9. refusals
def test_plugin_run_on_a_given_record_and_reset_keeps_the_bias():
    from demo_algorithms.inclinometer_device import MahonyFilter, TiltAcc
    truth, acc, gyr = _turn()
    from oracle import ins_np
    accel, gyro = ins_np.mc_sensors(SEED, np.array([3]), 100.0, truth['ref_accel'], truth['ref_gyro'], acc, gyr)
    m = MahonyFilter()
    m.run([100.0, gyro[0], accel[0]])
    q, wb, ab, fin = iref.mahony(gyro, accel, 0.01, np.zeros((1, 3)))
    _quat_close(m.get_results()[0], q[0], 1e-9)
    assert np.max(np.abs(m.gyro_bias - fin[0])) < 1e-12
    kept = m.gyro_bias.copy()
    m.reset()
    assert m.ini == 0 and np.array_equal(m.gyro_bias, kept)
    m.run([100.0, gyro[0], accel[0]])                   # the second run starts from the bias the first ended with
    q2, _, _, fin2 = iref.mahony(gyro, accel, 0.01, kept.reshape(1, 3))
    assert np.max(np.abs(m.gyro_bias - fin2[0])) < 1e-12
    t = TiltAcc()
    t.run([accel[0]])
    _quat_close(t.get_results()[0], iref.tilt(accel)[0], 1e-12)


_DIST_WORKER = r'''
import sys, json
sys.path[:0] = [%(pkg)r, %(repo)r]
import torch.distributed as dist
dist.init_process_group('gloo', init_method='file://%(pg)s', rank=0, world_size=1)
from gnss_ins_sim.sim import imu_model, ins_sim
from demo_algorithms.inclinometer_device import MahonyFilter
imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=False)
try:
    ins_sim.Sim([100.0, 0.0, 0.0], %(prof)r, imu=imu, algorithm=[MahonyFilter()], seed=1).run(2)
    err = ''
except ValueError as e:
    err = str(e)
print('RESULT ' + json.dumps({'error': err}))
dist.destroy_process_group()
'''


def test_refusals(tmp_path):
    from gnss_ins_sim.sim import imu_model, ins_sim
    from demo_algorithms.inclinometer_device import MahonyFilter
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=False)
    prof = str(load_golden('incl_mahony_tilt_rf1')['profile'])
    with pytest.raises(NotImplementedError, match='fp64'):
        ins_sim.Sim([100.0, 0.0, 0.0], prof, imu=imu, algorithm=[MahonyFilter()], seed=1, precision='f32').run(2)
    with pytest.raises(ValueError, match='does not cross devices'):
        ins_sim.Sim([100.0, 0.0, 0.0], prof, imu=imu, algorithm=[MahonyFilter()], seed=1, devices=[0, 0]).run(2)
    # under torch.distributed: in a process of its own, as the other process-group tests do
    import json
    import subprocess
    import sys
    from conftest import PKG, REPO
    script = tmp_path / 'd.py'
    script.write_text(_DIST_WORKER % dict(pkg=PKG, repo=REPO, pg=str(tmp_path / 'pg'), prof=prof))
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300)
    line = [x for x in out.stdout.splitlines() if x.startswith('RESULT ')]
    assert line, out.stdout + out.stderr
    assert 'torch.distributed' in json.loads(line[0][7:])['error']
    with pytest.raises(NotImplementedError, match='psd'):
        truth, acc, gyr = _turn()
        _job(2, truth, acc, gyr, vib_accel={'type': 'psd'})
