#!/usr/bin/env python3
"""How the position error of a free-integrating INS grows with time, over 65 536 Monte-Carlo runs: the across-run 1 sigma and
max |e| of each position axis at 1 Hz (Sim.error_curve), for the free integration and the odometer-aided one.  Printed are the
norms of the two three-axis vectors; the norm of the per-axis max |e| is an UPPER BOUND of the largest error norm of any run,
not that norm itself.

The reference's answer is one error line per run (``sim.plot(['pos'], opt={'pos': 'error'})``, ins_sim.py:253-337), which is not
usable at this run count; the curve is the same statistic the reference prints for the end point
(``results(err_stats_start=-1)``), at every instant.  It is shown twice: from a Sim that keeps every trajectory in device memory
(one reduction) and from a statistics-only Sim, whose runs are integrated again in blocks that fit ``max_device_bytes`` and
folded block by block -- so the curve exists at run counts whose trajectories would never fit.

    PYTHONPATH=gnss-ins-sim_amd python examples/demo_error_growth.py [runs]
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'gnss-ins-sim_amd'))

from gnss_ins_sim.sim import imu_model, ins_sim                      # noqa: E402
from demo_algorithms import free_integration, free_integration_odo   # noqa: E402

MOTION = os.path.join(os.path.dirname(HERE), 'gnss-ins-sim_amd', 'motion_profiles', 'turn_90deg.csv')


def main(runs):
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=False, odo=True, odo_opt={'scale': 0.999, 'stdv': 0.1})
    ini = np.genfromtxt(MOTION, delimiter=',', skip_header=1, max_rows=1)
    ini[0:2] *= np.pi / 180
    ini[6:9] *= np.pi / 180
    for keep, budget in ((True, 64 * 2 ** 30), (False, 2 * 2 ** 30)):       # bytes of materialised series one GPU may hold
        algos = [free_integration.FreeIntegration(ini.copy()), free_integration_odo.FreeIntegration(ini.copy())]
        sim = ins_sim.Sim([100.0, 0.0, 0.0], MOTION, ref_frame=1, imu=imu, algorithm=algos, seed=1, keep_trajectories=keep,
                          max_device_bytes=budget, device=0)
        t0 = time.perf_counter()
        sim.run(runs)
        t_run = time.perf_counter() - t0
        t0 = time.perf_counter()
        pos = sim.error_curve(('pos',), every=1.0)['pos']
        t_curve = time.perf_counter() - t0
        print('\n%d runs, %s: Sim.run %.3f s, the 1 Hz curve %.3f s' % (
            runs, 'every trajectory kept' if keep else 'statistics only (runs integrated again in blocks within %d GiB)' % (budget >> 30),
            t_run, t_curve))
        names = sorted(pos['std'])
        print('  t [s]  ' + '  '.join('%s: |1 sigma|  bound of max |e| [%s]' % (nm, pos['units'][0]) for nm in names))
        for k, t in enumerate(pos['time']):
            # the norms of the per-axis 1 sigma and of the per-axis max |e| (the latter bounds the largest error norm of any run)
            print('  %5.1f  ' % t + '  '.join('%s  %10.4f  %16.4f' % (' ' * len(nm), np.linalg.norm(pos['std'][nm][k]),
                                                                    np.linalg.norm(pos['max'][nm][k])) for nm in names))


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 65536)
