#!/usr/bin/env python3
"""CEP50 / CEP95 through a GPS outage, on an MI355X: the horizontal radius that holds 50 % and 95 % of the Monte-Carlo runs, every
5 s of a 60 s ground-vehicle profile (an acceleration, a turn, 20 s without GPS, the turn back, braking), for FreeIntegration, for the
loosely coupled GPS/INS filter InsLoose() and for the filter aided by the wheel speed and the non-holonomic constraints
(InsLoose(odo=True, nhc=True)) -- next to the horizontal 1 sigma that ``error_curve`` gives.  The radial error is not Gaussian and
in ref_frame 0 its across-run mean is not zero, so the quantiles do not follow from the moments: they are selected on the device
from the kept trajectory planes (Sim.error_quantiles, csrc/error_quantile.hip).  All three plugins see the same sensor realisation
per run.

    PYTHONPATH=gnss-ins-sim_amd python examples/demo_cep.py [runs]
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
LABELS = ('FreeIntegration', 'InsLoose()', 'InsLoose(odo=True, nhc=True)')


def main(runs):
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=True, odo=True)
    ini = workloads.parse_motion(MOTION)[0]
    algos = [free_integration.FreeIntegration(ini), InsLoose(), InsLoose(odo=True, nhc=True)]
    sim = ins_sim.Sim([fs, fs_gps, 0.0], MOTION, ref_frame=0, imu=imu, mode=None, env=None, algorithm=algos, seed=2026,
                      keep_trajectories=True)
    t0 = time.perf_counter()
    sim.run(runs)
    print('%d runs x %d samples, three plugins, everything kept: %.1f ms' % (runs, len(sim.dmgr.time.data), (time.perf_counter() - t0) * 1e3))
    t0 = time.perf_counter()
    q = sim.error_quantiles('pos', (0.5, 0.95), every=5.0)['pos']
    print('CEP50 / CEP95 of three plugins at %d instants: %.1f ms' % (len(q['time']), (time.perf_counter() - t0) * 1e3))
    curve = sim.error_curve('pos', every=5.0, extra_opt='ned')['pos']
    vis = np.asarray(sim.dmgr.gps_visibility.data)
    gt = np.asarray(sim.dmgr.gps_time.data)
    print('\nhorizontal position error over %d runs [m]: 1 sigma | CEP50 | CEP95 (* = no GPS)' % runs)
    print('   t [s]   ' + '   '.join('%-28s' % s for s in LABELS))
    for k, t in enumerate(q['time']):
        out = vis[np.argmin(np.abs(gt - t))] == 0
        cols = []
        for a in sim.mc.nav_names:
            sigma = float(np.hypot(*curve['std'][a][k, 0:2]))
            cols.append('%8.3f |%8.3f |%8.3f ' % (sigma, q['horizontal'][a][k, 0], q['horizontal'][a][k, 1]))
        print('%s %6.1f   %s' % ('*' if out else ' ', t, '   '.join(cols)))
    print('\nFor a circular Gaussian error with 1 sigma s per axis, CEP50 = 1.177 s and CEP95 = 2.448 s; the horizontal 1 sigma printed'
          '\nhere is sqrt(s_n^2 + s_e^2) = 1.414 s, so CEP50 / sigma = 0.83 and CEP95 / sigma = 1.73 would be the Gaussian ratios.')


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 4096)
