#!/usr/bin/env python3
"""The two Allan estimators side by side on the device: one static profile, 32 runs, the kept gyro series analysed with the
reference's non-overlapping bins and with the overlapping estimator (every window shift) at the same averaging times.  Printed
per tau: both deviations (mean over the runs and axes) and their across-run scatter; the scatter ratio at the longest tau is the
point -- the same data, read more steadily where bias instability and rate random walk are read.

    PYTHONPATH=gnss-ins-sim_amd python examples/demo_allan_overlapping.py [runs] [seconds]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'gnss-ins-sim_amd'))

import ginsim                                        # noqa: E402
from ginsim import workloads                         # noqa: E402


def main(runs, seconds):
    fs = 100.0
    text = open(workloads.profile_path('static_1800s')).read().split('\n')
    ini, _ = workloads.parse_motion('\n'.join(text[:4]))
    raw = ginsim.pathgen(ini, np.array([[1.0, 0, 0, 0, 0, 0, 0, seconds, 0.0]]), fs, 0.0, workloads.HIGH_MOBILITY, 1)
    truth = {'ref_accel': np.ascontiguousarray(raw['imu'][:, 1:4]), 'ref_gyro': np.ascontiguousarray(raw['imu'][:, 4:7]),
             'ref_pos': raw['nav'][:, 1:4], 'ref_vel': raw['nav'][:, 4:7], 'ref_att': raw['nav'][:, 7:10]}
    acc, gyr = workloads.imu_grade('mid-accuracy')
    ctx = ginsim.Context(0)
    job = ginsim.MonteCarloJob(ctx, fs, 1, truth, acc, gyr, None, runs=runs, algos=(), seed=1, keep_sensors=True).run()
    tau, binned = job.allan(fs)
    tau_o, over = job.allan(fs, overlapping=True)
    assert np.array_equal(tau, tau_o)                # the two curves share their tau
    b, o = binned['gyro'], over['gyro']              # (runs, ntau, 3)
    print('%d runs x %d samples @ %g Hz, gyro Allan deviation [rad/s], mean and scatter over runs x axes' % (runs, job.n, fs))
    print('%10s  %12s %10s   %12s %10s   %s' % ('tau [s]', 'binned', 'scatter', 'overlapping', 'scatter', 'scatter ratio'))
    for k in range(tau.size):
        sb, so = b[:, k, :].std(), o[:, k, :].std()
        print('%10.3f  %12.4e %10.2e   %12.4e %10.2e   %.3f' % (tau[k], b[:, k, :].mean(), sb, o[:, k, :].mean(), so, so / sb))
    print('scatter ratio at the longest tau (%.0f s): %.3f' % (tau[-1], o[:, -1, :].std() / b[:, -1, :].std()))
    job.release()
    ctx.close()


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 32, float(sys.argv[2]) if len(sys.argv) > 2 else 1800.0)
