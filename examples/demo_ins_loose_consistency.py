#!/usr/bin/env python3
"""Is the filter's covariance honest along the run?  On an MI355X: the loosely coupled GPS/INS Kalman filter of
demo_algorithms.ins_loose_device on GPS alone and aided by the odometer and the non-holonomic constraints, over the Monte-Carlo
runs of a 60 s ground-vehicle profile with 20 s without GPS -- and, every 5 s, what each filter PREDICTS of its own error (the
1 sigma of its covariance, averaged over the runs) next to the error it actually makes (the RMS over the runs, in the filter's own
error coordinates), and the normalised error of the position, velocity and attitude block (NEES: 3 for a consistent filter).
The sums are taken inside the filter's launch (Sim.consistency_curve): nothing is kept, so the Sim is statistics-only.

    PYTHONPATH=gnss-ins-sim_amd python examples/demo_ins_loose_consistency.py [runs]

Printed per filter (runs: default 4096): horizontal position and velocity sigma and RMS, their largest ratio over the nine
navigation states, and the three block NEES.
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

MOTION = os.path.join(REPO, 'tests', 'golden', 'ins_loose', 'motion_def_outage.csv')
fs = 100.0          # IMU sample frequency
fs_gps = 10.0       # GPS sample frequency


def main(runs):
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=True, odo=True)
    algos = [InsLoose(), InsLoose(odo=True, nhc=True)]
    sim = ins_sim.Sim([fs, fs_gps, 0.0], MOTION, ref_frame=1, imu=imu, mode=None, env=None, algorithm=algos, seed=2026,
                      keep_trajectories=False)
    sim.run(runs)
    t0 = time.perf_counter()
    curve = sim.consistency_curve(every=5.0)
    print('%d runs x %d samples, two filters, %d checkpoints each: %.1f ms' % (runs, len(sim.dmgr.time.data), len(curve['time']),
                                                                             (time.perf_counter() - t0) * 1e3))
    vis = np.asarray(sim.dmgr.gps_visibility.data)
    gt = np.asarray(sim.dmgr.gps_time.data)
    for name, label in zip(sim.mc.loose_names, ('InsLoose()', 'InsLoose(odo=True, nhc=True)')):
        c = curve[name]
        print('\n%s over %d runs (* = no GPS)' % (label, int(c['count'].min())))
        print('   t [s]   horizontal position [m]   horizontal velocity [m/s]   largest     NEES')
        print('            sigma      RMS            sigma      RMS             RMS/sigma   position velocity attitude')
        for k, t in enumerate(curve['time']):
            out = vis[np.argmin(np.abs(gt - t))] == 0
            hp = [float(np.hypot(*c[key][k, 0:2])) for key in ('sigma', 'rms')]
            hv = [float(np.hypot(*c[key][k, 3:5])) for key in ('sigma', 'rms')]
            print('%s %6.1f   %8.3f  %8.3f         %8.4f  %8.4f         %6.2f      %6.2f   %6.2f   %6.2f'
                  % ('*' if out else ' ', t, hp[0], hp[1], hv[0], hv[1], c['ratio'][k].max(), c['nees'][k, 0], c['nees'][k, 1], c['nees'][k, 2]))


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 4096)
