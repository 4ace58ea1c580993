#!/usr/bin/env python3
"""The reference's demo_mag_cal.py on an MI355X: the soft / hard-iron calibration of a 9-axis IMU's magnetometer (MagCal of
demo_algorithms.mag_calibrate_device) over 65 536 Monte-Carlo runs of motion_def_mag_cal.csv (140 s at 100 Hz: a rotation about x,
about y, about z), statistics only.  The reference calibrates ONE run, after six prompts for the rows of the three rotations; here
the rows come from the true angular rate, every run is a lane of one launch, and no magnetometer series is stored: each lane makes
its samples again from the counter RNG.

    PYTHONPATH=gnss-ins-sim_amd python examples/demo_mag_cal.py [runs]

What is printed next to the estimates: the algorithm fixes the x sensitivity at 1, so `soft_iron` estimates inv(si) up to ONE common
factor (printed: about soft_iron[0][0] / inv(si)[0][0], within some 20 % of 1 for matrices like the one below), and hard_iron[:3] is
hi times that factor.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, 'gnss-ins-sim_amd'))

from gnss_ins_sim.sim import imu_model, ins_sim                # noqa: E402
from demo_algorithms.mag_calibrate_device import MagCal        # noqa: E402

MOTION = os.path.join(REPO, 'tests', 'golden', 'magcal', 'motion_def_mag_cal.csv')
fs = 100.0          # IMU sample frequency
fs_gps = 10.0       # GPS sample frequency
fs_mag = fs         # magnetometer sample frequency, not used for now
GEO_MAG_N = [33.0, -3.2, 36.5]      # uT, N frame, near 32 N 120 E (the reference evaluates the WMM of the day here)


def test_mag_cal(runs):
    #### IMU model, typical for IMU381
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=9, gps=False)
    np.random.seed(2026)
    mag_error = {'si': np.eye(3) + np.random.randn(3, 3) * 0.1,
                 'hi': np.array([10.0, 10.0, 10.0]) * 1.0}
    imu.set_mag_error(mag_error)
    #### Algorithm
    algo = MagCal()
    #### start simulation
    for label in ('first Sim.run (library loads, truth)', 'second Sim.run'):
        sim = ins_sim.Sim([fs, fs_gps, fs_mag], MOTION, ref_frame=1, imu=imu, mode=None, env=None, algorithm=algo, seed=2026,
                          keep_trajectories=False, geo_mag_n=GEO_MAG_N)
        t0 = time.perf_counter()
        sim.run(runs)
        dt = time.perf_counter() - t0
        n = len(sim.dmgr.time.data)
        print('%s: %d runs x %d samples in %.1f ms' % (label, runs, n, dt * 1e3))
    sim.results()
    sim.plot(['mag', 'mag_cal'], opt={'mag': 'projection', 'mag_cal': 'projection'}, extra_opt='.')
    name, job, _ = sim.magcal_jobs[0]
    st = job.stats()
    inv = np.linalg.inv(mag_error['si'])
    factor = st['soft_iron']['mean'][0, 0] / inv[0, 0]
    np.set_printoptions(precision=5, suppress=True)
    print('rows of the three rotations (from the true angular rate): %s' % (job.segments,))
    print('device memory of the calibration job: %.2f MB (one mag series set for these runs: %.2f GB, never stored)' % (
        job.device_bytes / 1e6, 3.0 * n * runs * 8 / 1e9))
    print('true soft iron is:')
    print(inv)
    print('estimated soft iron, mean over %d runs (common factor %.4f):' % (runs, factor))
    print(st['soft_iron']['mean'])
    print('  +- std over the runs:')
    print(st['soft_iron']['std'])
    print('true hard iron is:')
    print(mag_error['hi'])
    print('estimated hard iron [x y z radius], mean +- std over the runs (hi x the factor: %s):' % (mag_error['hi'] * factor,))
    print(st['hard_iron']['mean'], '+-', st['hard_iron']['std'])
    print('run 0, as the reference prints them:')
    print(sim.dmgr.soft_iron.data['%s_0' % name])
    print(sim.dmgr.hard_iron.data['%s_0' % name])


if __name__ == '__main__':
    test_mag_cal(int(sys.argv[1]) if len(sys.argv) > 1 else 65536)
