#!/usr/bin/env python3
"""A GPS outage on an MI355X: the loosely coupled GPS/INS Kalman filter (InsLoose of demo_algorithms.ins_loose_device) next to
FreeIntegration over 65 536 Monte-Carlo runs of a 60 s profile -- an acceleration, a turn, 20 s without GPS, the turn back, braking.
The reference declares InsLoose and leaves its prediction and correction empty; here every run is a lane of one launch that makes
its own IMU samples and GPS fixes, so nothing but statistics is stored for the 65 536 runs.  Both plugins see the same sensor
realisation per run.

    PYTHONPATH=gnss-ins-sim_amd python examples/demo_ins_loose.py [runs] [curve_runs]

Printed: the summary of the big statistics-only Sim (end-point statistics of both plugins), and from a second Sim over
curve_runs runs (default 4096) with the trajectories kept, the across-run 1 sigma of the horizontal position error every 5 s.
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
fs = 100.0          # IMU sample frequency
fs_gps = 10.0       # GPS sample frequency


def make_sim(runs, keep):
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=True)
    ini = workloads.parse_motion(MOTION)[0]
    algos = [free_integration.FreeIntegration(ini), InsLoose()]
    sim = ins_sim.Sim([fs, fs_gps, 0.0], MOTION, ref_frame=0, imu=imu, mode=None, env=None, algorithm=algos, seed=2026,
                      keep_trajectories=keep)
    t0 = time.perf_counter()
    sim.run(runs)
    return sim, time.perf_counter() - t0


def main(runs, curve_runs):
    sim, dt = make_sim(runs, False)
    print('%d runs x %d samples, two plugins, statistics only: %.1f ms' % (runs, len(sim.dmgr.time.data), dt * 1e3))
    sim.results(err_stats_start=-1, extra_opt='ned')
    wb, ab = sim.loose_jobs[0][1].final_biases()
    print('bias estimates at the end, across-run std: wb %s rad/s, ab %s m/s^2' % (wb.std(0), ab.std(0)))
    sim, dt = make_sim(curve_runs, True)
    curve = sim.error_curve('pos', every=5.0, extra_opt='ned')['pos']
    free, loose = sim.mc.nav_names
    vis = np.asarray(sim.dmgr.gps_visibility.data)
    gt = np.asarray(sim.dmgr.gps_time.data)
    print('\nhorizontal position error, across-run 1 sigma [m] over %d runs (* = no GPS)' % curve_runs)
    print('   t [s]   FreeIntegration   InsLoose')
    for k, t in enumerate(curve['time']):
        out = vis[np.argmin(np.abs(gt - t))] == 0
        h = [float(np.hypot(*curve['std'][a][k, 0:2])) for a in (free, loose)]
        print('%s %6.1f   %12.3f   %10.3f' % ('*' if out else ' ', t, h[0], h[1]))


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 65536, int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
