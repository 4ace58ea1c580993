#!/usr/bin/env python3
"""What a filter may assume while the vehicle stands still, on an MI355X: the loosely coupled GPS/INS Kalman filter of
demo_algorithms.ins_loose_device twice over the same Monte-Carlo runs of a 55 s ground-vehicle profile with two stops -- one with
GPS, one inside an 18 s GPS outage -- once on GPS alone, once with the zero-velocity update (the velocity is zero) and the
zero-angular-rate update (the gyroscope reads its own bias) at every sample of a stop (InsLoose(zupt=True, zaru=True)).
The standstill signal comes from the Sim's truth: |velocity| <= 0.01 m/s and |angular rate| <= 2e-4 rad/s.  Both filters see the
same sensor realisation per run, and every run is a lane of one launch that makes its own IMU samples and GPS fixes.

    PYTHONPATH=gnss-ins-sim_amd python examples/demo_ins_loose_still.py [runs]

Printed, for both filters: the filter's own 1 sigma of the yaw-gyro bias at the end of the first stop, and the across-run 1 sigma of
the yaw and of the horizontal position error at the end of the outage (runs: default 4096).
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, 'gnss-ins-sim_amd'))

from gnss_ins_sim.sim import imu_model, ins_sim                # noqa: E402
from demo_algorithms.ins_loose_device import InsLoose          # noqa: E402

MOTION = os.path.join(REPO, 'tests', 'golden', 'ins_loose', 'motion_def_stops.csv')
fs = 100.0          # IMU sample frequency
fs_gps = 10.0       # GPS sample frequency


def bias_sigma_at(sim, algo, n, runs):
    """The filter's own 1 sigma of the yaw-gyro bias (state dbg_z) after the first n samples: the plugin's job on the cut profile."""
    import ginsim
    from ginsim import workloads
    d = sim.dmgr
    m = int(np.count_nonzero(np.rint(np.asarray(d.gps_time.data) * fs) < n))
    truth = {'ref_accel': d.ref_accel.data[:n], 'ref_gyro': d.ref_gyro.data[:n], 'ref_att': d.ref_att_euler.data[:n], 'ref_pos': d.ref_pos.data[:n],
             'ref_vel': d.ref_vel.data[:n], 'ref_gps': d.ref_gps.data[:m], 'gps_time': d.gps_time.data[:m], 'gps_visibility': d.gps_visibility.data[:m]}
    truth = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in truth.items()}
    kw = {} if algo.still_options() is None else {'still': algo.still_options()}
    job = ginsim.InsLooseJob(ginsim.default_context(), fs, sim.ref_frame, truth, sim.imu.accel_err, sim.imu.gyro_err, sim.imu.gps_err,
                             workloads.parse_motion(MOTION)[0], runs, seed=2026, **kw).run()
    sigma = float(np.sqrt(np.mean(job.final_pdiag()[:, 11])))
    job.release()
    return sigma


def main(runs):
    from ginsim.ins_loose import standstill_flags
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=True)
    algos = [InsLoose(), InsLoose(zupt=True, zaru=True)]
    sim = ins_sim.Sim([fs, fs_gps, 0.0], MOTION, ref_frame=1, imu=imu, mode=None, env=None, algorithm=algos, seed=2026, keep_trajectories=True)
    t0 = time.perf_counter()
    sim.run(runs)
    n = len(sim.dmgr.time.data)
    print('%d runs x %d samples, two filters, everything kept: %.1f ms' % (runs, n, (time.perf_counter() - t0) * 1e3))
    flags = standstill_flags({'ref_vel': sim.dmgr.ref_vel.data, 'ref_gyro': sim.dmgr.ref_gyro.data})
    edges = np.flatnonzero(np.diff(np.concatenate([[0], flags, [0]])))
    stops = list(zip(edges[0::2], edges[1::2] - 1))
    print('standstill: ' + ', '.join('%.2f-%.2f s' % (a / fs, b / fs) for a, b in stops))
    vis, gt = np.asarray(sim.dmgr.gps_visibility.data), np.asarray(sim.dmgr.gps_time.data)
    hidden = gt[vis == 0]
    last = int(round((hidden.max() + 1.0 / fs_gps) * fs)) - 1         # the sample before the first fix after the outage
    print('GPS outage: %.1f-%.1f s' % (hidden.min(), (last + 1) / fs))
    curve = sim.error_curve(('att_euler', 'pos'), samples=np.array([last]))
    gps_only, aided = sim.mc.nav_names
    bias = [bias_sigma_at(sim, a, int(stops[0][1]) + 1, min(runs, 256)) for a in algos]
    yaw = [float(curve['att_euler']['std'][a][0, 0]) for a in (gps_only, aided)]
    hor = [float(np.hypot(*curve['pos']['std'][a][0, 0:2])) for a in (gps_only, aided)]
    print('\n                                                             InsLoose()   InsLoose(zupt=True, zaru=True)')
    print('yaw-gyro bias, the filter\'s 1 sigma at the end of the first stop [rad/s]   %10.3e   %10.3e' % tuple(bias))
    print('yaw, across-run 1 sigma at the end of the outage [deg]                    %10.4f   %10.4f' % tuple(yaw))
    print('horizontal position, across-run 1 sigma at the end of the outage [m]      %10.3f   %10.3f' % tuple(hor))


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 4096)
