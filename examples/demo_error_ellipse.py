#!/usr/bin/env python3
"""Which way the error points through a GPS outage, on an MI355X: the along-track and cross-track 1 sigma and the horizontal error
ellipse of the position error across the Monte-Carlo runs of a 60 s ground-vehicle profile (an acceleration, a turn, 20 s without
GPS, the turn back, braking), for FreeIntegration, for the loosely coupled GPS/INS filter InsLoose(), for the filter aided by the
wheel speed (InsLoose(odo=True)) and by the wheel speed and the non-holonomic constraints (InsLoose(odo=True, nhc=True)).  The
odometer takes the along-track error away and leaves a narrow strip across the track; the per-axis sigmas of ``error_curve`` and the
radius of ``error_quantiles`` do not show it.  The mean vector and the 3x3 covariance are reduced on the device from the kept
trajectory planes (Sim.error_covariance, csrc/error_cov.hip); all four plugins see the same sensor realisation per run.

    PYTHONPATH=gnss-ins-sim_amd python examples/demo_error_ellipse.py [runs]
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, 'gnss-ins-sim_amd'))

from gnss_ins_sim.sim import imu_model, ins_sim                # noqa: E402
from demo_algorithms import free_integration                   # noqa: E402
from demo_algorithms.ins_loose_device import InsLoose          # noqa: E402
from ginsim import workloads                                   # noqa: E402

MOTION = os.path.join(REPO, 'tests', 'golden', 'ins_loose', 'motion_def_outage.csv')
fs = 20.0           # IMU sample frequency
fs_gps = 2.0        # GPS sample frequency
LABELS = ('FreeIntegration', 'InsLoose()', 'InsLoose(odo=True)', 'InsLoose(odo=True, nhc=True)')


def main(runs):
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=True, odo=True)
    ini = workloads.parse_motion(MOTION)[0]
    algos = [free_integration.FreeIntegration(ini), InsLoose(), InsLoose(odo=True), InsLoose(odo=True, nhc=True)]
    sim = ins_sim.Sim([fs, fs_gps, 0.0], MOTION, ref_frame=1, imu=imu, mode=None, env=None, algorithm=algos, seed=2026,
                      keep_trajectories=True)
    t0 = time.perf_counter()
    sim.run(runs)
    t = np.asarray(sim.dmgr.time.data)
    print('%d runs x %d samples, four plugins, everything kept: %.1f ms' % (runs, len(t), (time.perf_counter() - t0) * 1e3))
    # the instants: the first fix that is missing, the sample before the first fix that is back, the end of the profile
    vis = np.asarray(sim.dmgr.gps_visibility.data)
    gt = np.asarray(sim.dmgr.gps_time.data)
    hidden = np.nonzero(vis == 0)[0]
    start = int(np.argmin(np.abs(t - gt[hidden[0]])))
    end = int(np.argmin(np.abs(t - gt[hidden[-1] + 1]))) - 1
    rows = [start, end, len(t) - 1]
    t0 = time.perf_counter()
    trk = sim.error_covariance('pos', samples=rows)['pos']
    nav = sim.error_covariance('pos', samples=rows, frame='nav')['pos']
    print('covariance of four plugins at %d instants, two frames: %.1f ms' % (len(rows), (time.perf_counter() - t0) * 1e3))
    yaw = np.degrees(np.asarray(sim.dmgr.ref_att_euler.data)[rows, 0])
    print('\nposition error over %d runs, 1 sigma [m]: x / y | rho xy | along / cross | ellipse semi-major x semi-minor, azimuth from x' % runs)
    for k, what in enumerate(('outage start', 'outage end', 'profile end')):
        print('\n%s, t = %.2f s, truth heading %.0f deg' % (what, t[rows[k]], yaw[k] % 360.0))
        for a, label in zip(sim.mc.nav_names, LABELS):
            cov, tc, el = nav['cov'][a][k], trk['cov'][a][k], nav['ellipse'][a][k]
            print('  %-30s %8.3f /%8.3f | %6.2f | %8.3f /%8.3f | %8.3f x %7.3f, %6.1f deg'
                  % (label, np.sqrt(cov[0, 0]), np.sqrt(cov[1, 1]), nav['corr'][a][k, 0, 1], np.sqrt(tc[0, 0]), np.sqrt(tc[1, 1]), el[0], el[1], el[2]))
    print('\nThe ellipse is the 1 sigma one (39.3 % of a Gaussian error); times 2.4477 it holds 95 %.')


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 4096)
