#!/usr/bin/env python3
"""Golden vectors of the inclinometer plugins by EXECUTING the unmodified reference (MahonyFilter, TiltAcc through its Sim,
with np.random.randn replaced by oracle.ref_shim: the engine's Philox normals in the reference's call order, as the t3 cases of
make_golden.py do).  Needs a checkout of the reference (argument or $GNSS_INS_SIM_REFERENCE); one interpreter per case.

    python tests/golden/make_golden_inclinometer.py /path/to/reference      -> tests/golden/inclinometer/

  incl_mahony_tilt_rf1.npz   (a) 65 s cut of motion_def.csv (static start, the 45 degree pitch climb, a turn): 3 runs of
                             [MahonyFilter(), TiltAcc()], ref_frame 1, 6-axis 'mid-accuracy'
  incl_mag9_gps_rf0.npz      (b) the same profile, 9-axis with GPS, ref_frame 0, 2 runs (the demo_multiple_algorithms.py recipe)
  incl_chain_rf1.npz         (c) two Sim(...).run(2) calls with ONE MahonyFilter object: the chain goes on across calls
  incl_sphere.npz            (d) no Sim, no profile: MahonyFilter / TiltAcc objects driven directly on the hand-built records of
                             tests/inclinometer_records.py (attitudes over the whole sphere, the neighbourhoods of +-x and of
                             dcm2quat's tr == 0, rates past cos(theta / 2) = 0, zero accelerometers, other gains and rate),
                             attitude.quat2euler of their quaternions (a mask where it raises), attitude.angle_range_pi at the wrap

    python tests/golden/make_golden_inclinometer.py --check /path/to/reference   -> regenerates (d) in memory and compares it
                                                                                    with the committed file, array by array
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


def sphere(ref):
    """(d): every array of incl_sphere.npz, by the unmodified reference objects."""
    sys.path.insert(0, ref)
    sys.path.insert(1, os.path.join(REPO, 'tests'))
    from gnss_ins_sim.attitude import attitude
    from demo_algorithms import inclinometer_mahony, inclinometer_acc
    import inclinometer_records as rec
    names = dict(kp_high='kp_acc_high', kp_low='kp_acc_low', ki_high='ki_acc_high', ki_low='ki_acc_low', innovation_limit='innovationLimit')

    def euler(q):
        e, bad = np.full(q.shape[:-1] + (3,), np.nan), np.zeros(q.shape[:-1], dtype=bool)
        for i in np.ndindex(*q.shape[:-1]):
            try:
                e[i] = attitude.quat2euler(q[i])
            except ValueError:                          # math.asin domain error
                bad[i] = True
        return e, bad
    out = dict(seed=rec.SEED, batches=np.array([b['name'] for b in rec.sphere_batches()]))
    for b in rec.sphere_batches():
        R, n, _ = b['accel'].shape
        k = rows(n, 12)
        p = b['name'] + '_'
        mq, tq, wb, ab, fin = [], [], [], [], []
        for r in range(R):
            m = inclinometer_mahony.MahonyFilter()      # a new object per record: zero gyro_bias
            for key, attr in names.items():
                if b['gains'] is not None:
                    setattr(m, attr, b['gains'][key])
            m.run([b['fs'], b['gyro'][r], b['accel'][r]])
            t = inclinometer_acc.TiltAcc()
            with np.errstate(invalid='ignore', divide='ignore'):
                t.run([b['accel'][r]])
            mq.append(m.quat[k]); wb.append(m.wb[k]); ab.append(m.ab[k]); fin.append(m.gyro_bias.copy()); tq.append(t.results[k])
        out[p + 'rows'], out[p + 'n'], out[p + 'fs'] = k, n, b['fs']
        out[p + 'accel0'], out[p + 'gyro0'] = b['accel'][:, 0], b['gyro'][:, 0]
        out[p + 'mahony_quat'], out[p + 'tilt_quat'] = np.stack(mq), np.stack(tq)
        out[p + 'wb'], out[p + 'ab'], out[p + 'bias_after'] = np.stack(wb), np.stack(ab), np.stack(fin)
        for a in ('mahony', 'tilt'):
            out[p + a + '_euler'], out[p + a + '_asin_raises'] = euler(out[p + a + '_quat'])
        for g, ids in b['groups'].items():
            out[p + 'group_' + g] = ids
    out['wrap_x'] = rec.WRAP_VALUES
    out['wrap_y'] = np.array([attitude.angle_range_pi(float(x)) for x in rec.WRAP_VALUES])
    return out


if __name__ == '__main__':
    if len(sys.argv) >= 3 and sys.argv[1] == '--case':
        case(sys.argv[2], sys.argv[3])
    elif len(sys.argv) >= 3 and sys.argv[1] == '--sphere':
        os.makedirs(OUT, exist_ok=True)
        np.savez_compressed(os.path.join(OUT, 'incl_sphere.npz'), **sphere(sys.argv[2]))
        print('%-28s %7.1f KB' % ('incl_sphere.npz', os.path.getsize(os.path.join(OUT, 'incl_sphere.npz')) / 1024))
    elif len(sys.argv) >= 3 and sys.argv[1] == '--check':
        new, old = sphere(sys.argv[2]), dict(np.load(os.path.join(OUT, 'incl_sphere.npz'), allow_pickle=False))
        bad = [k for k in sorted(set(new) | set(old)) if k not in new or k not in old or not np.array_equal(np.asarray(new[k]), old[k], equal_nan=np.asarray(new[k]).dtype.kind == 'f')]
        print('incl_sphere.npz: %d arrays, %s' % (len(old), 'reproduced' if not bad else 'DIFFERENT: %s' % bad))
        sys.exit(1 if bad else 0)
    else:
        ref = sys.argv[1] if len(sys.argv) > 1 else os.environ['GNSS_INS_SIM_REFERENCE']
        # the reference's motion_def.csv as it is: the workload of examples/demo_inclinometer.py
        os.makedirs(OUT, exist_ok=True)
        with open(os.path.join(ref, 'demo_motion_def_files', 'motion_def.csv')) as f, open(os.path.join(OUT, 'motion_def.csv'), 'w') as g:
            g.write(f.read())
        for nm in ('incl_mahony_tilt_rf1', 'incl_mag9_gps_rf0', 'incl_chain_rf1'):
            subprocess.run([sys.executable, os.path.abspath(__file__), '--case', nm, ref], check=True,
                           env=dict(os.environ, PYTHONDONTWRITEBYTECODE='1', MPLBACKEND='Agg'))
        subprocess.run([sys.executable, os.path.abspath(__file__), '--sphere', ref], check=True,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE='1', MPLBACKEND='Agg'))
