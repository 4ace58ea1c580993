#!/usr/bin/env python3
"""What the magnetometer buys the heading, on an MI355X: the loosely coupled GPS/INS Kalman filter of
demo_algorithms.ins_loose_device twice over the same Monte-Carlo runs of a 60 s ground-vehicle profile (an acceleration, a turn,
20 s without GPS, the turn back, braking) -- once on GPS alone, once with the three axes of the magnetometer as a measurement of the
attitude error (InsLoose(mag=True)).  GPS shows the yaw only while the vehicle accelerates horizontally; on a
straight stretch and in the outage it drifts with the gyro, and the position goes with it.  Both filters see the same sensor
realisation per run, and every run is a lane of one launch that makes its own IMU samples, GPS fixes and magnetometer samples.

    PYTHONPATH=gnss-ins-sim_amd python examples/demo_ins_loose_mag.py [runs]

Printed: the across-run 1 sigma of the yaw and of the horizontal position error of both filters every 2.5 s (runs: default 4096).
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
fs = 100.0          # IMU and magnetometer sample frequency
fs_gps = 10.0       # GPS sample frequency
GEO_MAG_N = [30.0, -3.0, 40.0]      # the geomagnetic field at the start [uT, NED]


def main(runs):
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=9, gps=True)
    algos = [InsLoose(), InsLoose(mag=True)]
    sim = ins_sim.Sim([fs, fs_gps, fs], MOTION, ref_frame=1, imu=imu, mode=None, env=None, algorithm=algos, seed=2026,
                      keep_trajectories=True, geo_mag_n=GEO_MAG_N)
    t0 = time.perf_counter()
    sim.run(runs)
    print('%d runs x %d samples, two filters, everything kept: %.1f ms' % (runs, len(sim.dmgr.time.data), (time.perf_counter() - t0) * 1e3))
    print('magnetometer: 1 sigma %s uT in a field of %s uT' % (np.asarray(imu.mag_err['std']) * np.ones(3), GEO_MAG_N))
    curve = sim.error_curve(('att_euler', 'pos'), every=2.5)
    gps_only, aided = sim.mc.nav_names
    vis = np.asarray(sim.dmgr.gps_visibility.data)
    gt = np.asarray(sim.dmgr.gps_time.data)
    print('\nacross-run 1 sigma over %d runs (* = no GPS)' % runs)
    print('            yaw [deg]                    horizontal position [m]')
    print('   t [s]   InsLoose()   InsLoose(mag=True)   InsLoose()   InsLoose(mag=True)')
    for k, t in enumerate(curve['pos']['time']):
        out = vis[np.argmin(np.abs(gt - t))] == 0
        y = [float(curve['att_euler']['std'][a][k, 0]) for a in (gps_only, aided)]
        h = [float(np.hypot(*curve['pos']['std'][a][k, 0:2])) for a in (gps_only, aided)]
        print('%s %6.1f   %10.4f   %10.4f           %10.3f   %10.3f' % ('*' if out else ' ', t, y[0], y[1], h[0], h[1]))


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 4096)
