#!/usr/bin/env python3
"""Golden vectors of the error-growth curve by EXECUTING the unmodified reference through the normal-injection harness of
make_golden.py (np.random.randn replaced by oracle.ref_shim: the engine's Philox normals in the reference's call order), so that
the C oracle and the device reproduce the same series from `seed`.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_error_curve.py [CASE ..]   -> tests/golden/error_curve/

Needs the reference checkout make_golden.py names.  One interpreter per case, as make_golden.py
does and for its reason (IMU(accuracy=dict) aliases module-level dicts of the reference).

Per case (tests/error_curve_cases.py): the reference's own calc_data_err arrays of att_euler / pos / vel, reduced over the 16 runs
by its own __array_stats at every sample and converted by its own sim_data.convert_unit to the output units
get_error_stats(use_output_units=True) reports -- `<name>_<max|avg|std>_<plugin>` (n, 3); the last row is asserted to equal
get_error_stats(..., err_stats_start=-1).  `<name>_tol_<stat>_<plugin>`: the bound of every record, measured on the reference's
series only (tests/error_curve_ref.py: 16 x max(long-double distance, spread over eight permutations of the run order, eps |q|)),
in the same units.  Plus seed, configuration, the truth, the IMU error dicts and `wraps`: how many attitude errors array_error had to wrap.
"""
import os
import subprocess
import sys

sys.dont_write_bytecode = True

import numpy as np      # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(HERE))
import make_golden as mg            # noqa: E402  (the harness: reference on sys.path, RandnShim, injected, SEED, MOTION, read_ini)
import error_curve_cases as cases   # noqa: E402
import error_curve_ref              # noqa: E402

OUT = os.path.join(os.environ.get('GINSIM_GOLDEN_OUT') or HERE, 'error_curve')


def make(case):
    from gnss_ins_sim.sim import sim_data
    motion, rf, extra_opt, algos = cases.CASES[case]
    R, fs = cases.RUNS, cases.FS
    if motion is None:
        csv = mg.MOTION + 'motion_def-90deg_turn.csv'
        ini = mg.read_ini(csv)
    else:
        csv = motion
        ini = np.array([float(v) for v in motion.strip().split('\n')[1].split(',')])
        ini[0:2] *= mg.D2R
        ini[6:9] *= mg.D2R
    imu = mg.imu_model.IMU(accuracy={k: v.copy() for k, v in cases.DEMO_IMU.items()}, axis=6, gps=False, odo=True, odo_opt=dict(cases.ODO))
    objs = [(mg.free_integration_odo if a == 'odo' else mg.free_integration).FreeIntegration(ini.copy()) for a in algos]
    sim = mg.ins_sim.Sim([fs, 0.0, 0.0], csv, ref_frame=rf, imu=imu, algorithm=objs)
    n = 1000
    shim = mg.RandnShim(mg.SEED, n, imu.accel_err['b_corr'], imu.gyro_err['b_corr'], odo=True)
    with mg.injected(shim):
        sim.run(R)
    assert shim.run == R and not shim.queue
    d = sim.dmgr
    assert d.time.data.shape[0] == n
    out = dict(case=case, seed=mg.SEED, R=R, fs=fs, n=n, ref_frame=rf, extra_opt=extra_opt, ini=ini, rows=np.arange(n),
               ref_att=d.ref_att_euler.data, ref_pos=d.ref_pos.data, ref_vel=d.ref_vel.data,
               ref_accel=d.ref_accel.data, ref_gyro=d.ref_gyro.data, ref_odo=d.ref_odo.data)
    out.update(mg.err_dict_arrays('accel_', imu.accel_err))
    out.update(mg.err_dict_arrays('gyro_', imu.gyro_err))
    ref_nav = np.concatenate([d.ref_att_euler.data, d.ref_pos.data, d.ref_vel.data], axis=1)
    wraps = 0
    for a in range(len(algos)):
        g = 'algo%d' % a
        traj = np.stack([np.concatenate([d.att_euler.data['%s_%d' % (g, r)], d.pos.data['%s_%d' % (g, r)], d.vel.data['%s_%d' % (g, r)]], axis=1)
                         for r in range(R)])
        wraps += int(np.sum(np.abs(traj[:, :, 0:3] - ref_nav[None, :, 0:3]) > np.pi))
        bound = error_curve_ref.curve(traj, ref_nav, None, extra_opt == 'ned' and rf == 0)
        for k, (name, ang) in enumerate((('att_euler', True), ('pos', False), ('vel', False))):
            d._InsDataMgr__err = {}
            err = d.calc_data_err(name, 'ref_' + name, ang, extra_opt)
            e = np.stack([err.data['%s_%d' % (g, r)] for r in range(R)])
            st = d._InsDataMgr__array_stats(e)              # over the runs, at every sample: (n, 3) each
            end = d.get_error_stats(name, err_stats_start=-1, angle=ang, use_output_units=True, extra_opt=extra_opt)
            scale = sim_data.unit_conversion_scale(err.units, err.output_units)
            for s in ('max', 'avg', 'std'):
                q = sim_data.convert_unit(st[s], err.units, err.output_units)
                want = end[s][g] if isinstance(end[s], dict) else end[s]
                assert np.array_equal(q[-1], want), (case, name, s, q[-1], want)
                # the restatement on the reference's series is the reference's reduction, to the restatement's own bound
                assert np.all(np.abs(st[s] - bound[s][:, 3 * k:3 * k + 3]) <= bound['tol_' + s][:, 3 * k:3 * k + 3]), (case, name, s)
                out['%s_%s_%s' % (name, s, g)] = q
                out['%s_tol_%s_%s' % (name, s, g)] = bound['tol_' + s][:, 3 * k:3 * k + 3] * scale
    out['wraps'] = wraps
    if case.startswith('wrap'):
        assert wraps > 0, 'no attitude error of this case crosses +-pi'
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, case + '.npz')
    np.savez_compressed(path, **out)
    print('%-24s %7.1f KB, %d wrapped attitude errors' % (case + '.npz', os.path.getsize(path) / 1024, wraps))


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--case':
        make(sys.argv[2])
        sys.exit(0)
    for name in (sys.argv[1:] or list(cases.CASES)):
        subprocess.check_call([sys.executable, os.path.abspath(__file__), '--case', name],
                              env=dict(os.environ, PYTHONDONTWRITEBYTECODE='1', MPLBACKEND='Agg'))
