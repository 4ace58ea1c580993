#!/usr/bin/env python3
"""What the odometer buys during a GPS outage, on an MI355X: the loosely coupled GPS/INS Kalman filter of
demo_algorithms.ins_loose_device twice over the same Monte-Carlo runs of a 60 s ground-vehicle profile (an acceleration, a turn,
20 s without GPS, the turn back, braking) -- once on GPS alone, once aided by the wheel speed and by the fact that the vehicle does
not slide sideways or leave the road (InsLoose(odo=True, nhc=True)).  Both filters see the same sensor realisation
per run, and every run is a lane of one launch that makes its own IMU samples, GPS fixes and odometer samples.

    PYTHONPATH=gnss-ins-sim_amd python examples/demo_ins_loose_odo.py [runs]

Printed: the across-run 1 sigma of the horizontal position error of both filters every 2.5 s (runs: default 4096).
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
    sim = ins_sim.Sim([fs, fs_gps, 0.0], MOTION, ref_frame=0, imu=imu, mode=None, env=None, algorithm=algos, seed=2026,
                      keep_trajectories=True)
    t0 = time.perf_counter()
    sim.run(runs)
    print('%d runs x %d samples, two filters, everything kept: %.1f ms' % (runs, len(sim.dmgr.time.data), (time.perf_counter() - t0) * 1e3))
    print('odometer: scale %(scale)g, 1 sigma %(stdv)g m/s' % imu.odo_err)
    curve = sim.error_curve('pos', every=2.5, extra_opt='ned')['pos']
    gps_only, aided = sim.mc.nav_names
    vis = np.asarray(sim.dmgr.gps_visibility.data)
    gt = np.asarray(sim.dmgr.gps_time.data)
    print('\nhorizontal position error, across-run 1 sigma [m] over %d runs (* = no GPS)' % runs)
    print('   t [s]   InsLoose()   InsLoose(odo=True, nhc=True)')
    for k, t in enumerate(curve['time']):
        out = vis[np.argmin(np.abs(gt - t))] == 0
        h = [float(np.hypot(*curve['std'][a][k, 0:2])) for a in (gps_only, aided)]
        print('%s %6.1f   %10.3f   %10.3f' % ('*' if out else ' ', t, h[0], h[1]))


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 4096)
