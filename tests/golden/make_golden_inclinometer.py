#!/usr/bin/env python3
"""Golden vectors of the inclinometer plugins by EXECUTING the unmodified reference (MahonyFilter, TiltAcc through its Sim,
with np.random.randn replaced by oracle.ref_shim: the engine's Philox normals in the reference's call order, as the t3 cases of
make_golden.py do).  Needs a checkout of the reference (argument or $GNSS_INS_SIM_REFERENCE); one interpreter per case.

    python tests/golden/make_golden_inclinometer.py /path/to/reference      -> tests/golden/inclinometer/

  incl_mahony_tilt_rf1.npz   (a) 65 s cut of motion_def.csv (static start, the 45 degree pitch climb, a turn): 3 runs of
                             [MahonyFilter(), TiltAcc()], ref_frame 1, 6-axis 'mid-accuracy'
  incl_mag9_gps_rf0.npz      (b) the same profile, 9-axis with GPS, ref_frame 0, 2 runs (the demo_multiple_algorithms.py recipe)
  incl_chain_rf1.npz         (c) two Sim(...).run(2) calls with ONE MahonyFilter object: the chain goes on across calls
"""
import io
import math
import os
import subprocess
import sys
from contextlib import redirect_stdout

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
# a directory of their own: every .npz directly under tests/golden/ belongs to make_golden.py's recipe
OUT = os.path.join(HERE, 'inclinometer')
SEED = 20261016
D2R = math.pi / 180
# a cut of the reference's demo_motion_def_files/motion_def.csv: 10 s static, the climb to 45 degrees pitch at 10 m/s, 5 s
# straight, the 90 degree turn with the pitch back to level, 5 s straight
PROFILE = """ini lat (deg),ini lon (deg),ini alt (m),ini vx_body (m/s),ini vy_body (m/s),ini vz_body (m/s),ini yaw (deg),ini pitch (deg),ini roll (deg)
32,120,0,0,0,0,0,0,0
command type,yaw (deg),pitch (deg),roll (deg),vx_body (m/s),vy_body (m/s),vz_body (m/s),command duration (s),GPS visibility
1,0,0,0,0,0,0,10,1
5,0,45,0,10,0,0,20,1
1,0,0,0,0,0,0,5,1
3,90,-45,0,0,0,0,25,1
1,0,0,0,0,0,0,5,1
"""


def rows(n, stride):
    idx = set(range(0, n, stride)) | {n - 2, n - 1}
    return np.array(sorted(k for k in idx if k >= 0))


def case(name, ref):
    sys.path.insert(0, ref)
    sys.path.insert(1, REPO)
    from gnss_ins_sim.sim import imu_model, ins_sim
    from demo_algorithms import inclinometer_mahony, inclinometer_acc
    from oracle.ref_shim import RandnShim, injected
    csv = os.path.join(os.environ.get('TMPDIR', '/tmp'), 'incl_profile_%d.csv' % os.getpid())
    with open(csv, 'w') as f:
        f.write(PROFILE)
    rf, R, axis, gps, fs_gps, calls = {'incl_mahony_tilt_rf1': (1, 3, 6, False, 0.0, 1), 'incl_mag9_gps_rf0': (0, 2, 9, True, 10.0, 1),
                                       'incl_chain_rf1': (1, 2, 6, False, 0.0, 2)}[name]
    fs = 100.0
    imu = imu_model.IMU(accuracy='mid-accuracy' if axis == 6 else 'low-accuracy', axis=axis, gps=gps)
    mah = inclinometer_mahony.MahonyFilter()
    algos = [mah, inclinometer_acc.TiltAcc()] if name != 'incl_chain_rf1' else [mah]
    out = dict(seed=SEED, R=R, fs=fs, ref_frame=rf, axis=axis, fs_gps=fs_gps, calls=calls, profile=np.array(PROFILE))
    for call in range(calls):
        # a new Sim per call on the SAME plugin objects: a second run() of one reference Sim keeps the first call's att_euler
        # (__add_associated_data_to_results adds only keys that are not there yet)
        sim = ins_sim.Sim([fs, fs_gps, fs if axis == 9 else 0.0], csv, ref_frame=rf, imu=imu, mode=None, env=None, algorithm=algos)
        bias_before = mah.gyro_bias.copy()
        probe = ins_sim.Sim([fs, fs_gps, 0.0], csv, ref_frame=rf, imu=None)
        ini_pva, motion_def = probe._Sim__parse_motion()
        from gnss_ins_sim.pathgen import pathgen
        r = pathgen.path_gen(ini_pva.copy(), motion_def.copy(), np.array([[1.0, fs], [1.0, fs_gps if gps else 10.0], [1.0, fs]]),
                             probe._Sim__parse_mode(None), ref_frame=rf, magnet=False)
        n, m = r['imu'].shape[0], (r['gps'].shape[0] if gps else 0)
        shim = RandnShim(SEED, n, imu.accel_err['b_corr'], imu.gyro_err['b_corr'], gps_m=m, mag=(axis == 9))
        with injected(shim):
            sim.run(R)
        assert shim.run == R and not shim.queue
        d = sim.dmgr
        k = rows(n, 25)
        p = 'c%d_' % call
        out[p + 'bias_before'] = bias_before
        out[p + 'bias_after'] = mah.gyro_bias.copy()
        out[p + 'rows'] = k
        out[p + 'n'] = n
        out['ref_att'] = d.ref_att_euler.data
        out[p + 'accel'] = np.stack([d.accel.data[i] for i in range(R)])[:, k]
        out[p + 'gyro'] = np.stack([d.gyro.data[i] for i in range(R)])[:, k]
        names = [sim.amgr.get_algo_name(i) for i in range(len(algos))]
        for nm in names:
            out[p + nm + '_att_quat'] = np.stack([d.att_quat.data[nm + '_' + str(i)][k] for i in range(R)])
            out[p + nm + '_att_euler'] = np.stack([d.att_euler.data[nm + '_' + str(i)][k] for i in range(R)])
            out[p + nm + '_quat_last'] = np.stack([d.att_quat.data[nm + '_' + str(i)][-1] for i in range(R)])
        out[p + 'wb'] = np.stack([d.wb.data['algo0_' + str(i)][k] for i in range(R)])
        out[p + 'ab'] = np.stack([d.ab.data['algo0_' + str(i)][k] for i in range(R)])
        out[p + 'wb_last'] = np.stack([d.wb.data['algo0_' + str(i)][-1] for i in range(R)])
        st = d.get_error_stats('att_euler', err_stats_start=-1, angle=True, use_output_units=False)
        for s in ('max', 'avg', 'std'):
            for g, v in (st[s].items() if isinstance(st[s], dict) else [('algo0', st[s])]):
                out['%send_%s_%s' % (p, s, g)] = v
        st = d.get_error_stats('att_euler', err_stats_start=2.0, angle=True, use_output_units=False)
        keys = [nm + '_' + str(i) for nm in names for i in range(R)]
        out[p + 'proc_keys'] = np.array(keys)
        for s in ('max', 'avg', 'std'):
            out[p + 'proc_' + s] = np.stack([st[s][kk] for kk in keys])
        if axis == 9:
            from gnss_ins_sim.geoparams import geomag
            gm = geomag.GeoMag("WMM.COF")
            f = gm.GeoMag(32.0, 120.0, 0.0)
            out['geo_mag_n'] = np.array([f.bx, f.by, f.bz]) / 1000.0
        buf = io.StringIO()
        with redirect_stdout(buf):
            sim.results()
        out[p + 'summary'] = np.array(sim.sum)
    os.remove(csv)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, name + '.npz'), **out)
    print('%-28s %7.1f KB' % (name + '.npz', os.path.getsize(os.path.join(OUT, name + '.npz')) / 1024))


if __name__ == '__main__':
    if len(sys.argv) >= 3 and sys.argv[1] == '--case':
        case(sys.argv[2], sys.argv[3])
    else:
        ref = sys.argv[1] if len(sys.argv) > 1 else os.environ['GNSS_INS_SIM_REFERENCE']
        # the reference's motion_def.csv as it is: the workload of examples/demo_inclinometer.py
        os.makedirs(OUT, exist_ok=True)
        with open(os.path.join(ref, 'demo_motion_def_files', 'motion_def.csv')) as f, open(os.path.join(OUT, 'motion_def.csv'), 'w') as g:
            g.write(f.read())
        for nm in ('incl_mahony_tilt_rf1', 'incl_mag9_gps_rf0', 'incl_chain_rf1'):
            subprocess.run([sys.executable, os.path.abspath(__file__), '--case', nm, ref], check=True,
                           env=dict(os.environ, PYTHONDONTWRITEBYTECODE='1', MPLBACKEND='Agg'))
