#!/usr/bin/env python3
"""An odometer whose scale factor nobody told the filter, on an MI355X: the loosely coupled GPS/INS Kalman filter three times over
the same Monte-Carlo runs of a ground-vehicle profile, up to the last sample of its 20 s GPS outage.  The wheel-speed sensor reads
0.99 of the true speed.  One filter assumes 1.0 (InsLoose(odo=True, nhc=True, odo_scale=1.0)), one is told 0.99, and one estimates
the scale factor as its 16th state while GPS is visible and uses the estimate through the outage
(InsLoose(odo=True, nhc=True, odo_scale_state=True)).  The three launches share seed and run ids, so every run sees
one sensor realisation; each is the ginsim.InsLooseJob that Sim makes for the plugin.

    PYTHONPATH=gnss-ins-sim_amd python examples/demo_ins_loose_odo_scale.py [runs]

Printed at the outage's last sample, per filter: the horizontal position 1 sigma the filter claims and the across-run RMS of its
horizontal error; and the estimated scale factor with its 1 sigma (runs: default 4096).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, 'gnss-ins-sim_amd'))

import ginsim                                                   # noqa: E402
from ginsim import workloads                                    # noqa: E402
from demo_algorithms.ins_loose_device import InsLoose          # noqa: E402

MOTION = os.path.join(REPO, 'tests', 'golden', 'ins_loose', 'motion_def_outage.csv')
fs = 100.0          # IMU sample frequency
fs_gps = 10.0       # GPS sample frequency
rf = 1
ODO_ERR = {'scale': 0.99, 'stdv': 0.1}
GPS_ERR = {'stdp': np.array([5.0, 5.0, 7.0]), 'stdv': np.array([0.05, 0.05, 0.05])}


def main(runs):
    ini, seg = workloads.parse_motion(MOTION)
    raw = ginsim.pathgen(ini, seg, fs, fs_gps, workloads.HIGH_MOBILITY, rf, gps=True)
    stamps = np.rint(raw['gps'][:, 0]).astype(np.int64)
    hidden = np.nonzero(raw['gps'][:, 7] == 0)[0]
    n = int(stamps[hidden[-1]]) + int(round(fs / fs_gps))       # up to the sample before the first fix after the outage
    m = int(np.count_nonzero(stamps < n))
    truth = {'ref_accel': np.ascontiguousarray(raw['imu'][:n, 1:4]), 'ref_gyro': np.ascontiguousarray(raw['imu'][:n, 4:7]),
             'ref_pos': np.ascontiguousarray(raw['nav'][:n, 1:4]), 'ref_vel': np.ascontiguousarray(raw['nav'][:n, 4:7]),
             'ref_att': np.ascontiguousarray(raw['nav'][:n, 7:10]), 'ref_gps': np.ascontiguousarray(raw['gps'][:m, 1:7]),
             'gps_time': raw['gps'][:m, 0] / fs, 'gps_visibility': raw['gps'][:m, 7].copy(),
             'ref_odo': np.ascontiguousarray(raw['odo'][:n, 2])}
    acc, gyr = workloads.imu_grade('mid-accuracy')
    plugins = [('assumes 1.0', InsLoose(odo=True, nhc=True, odo_scale=1.0)), ('told 0.99', InsLoose(odo=True, nhc=True, odo_scale=0.99)),
               ('estimates it', InsLoose(odo=True, nhc=True, odo_scale_state=True))]
    ctx = ginsim.Context(0)
    print('%d runs x %d samples (%.1f s, the last %.1f s without GPS); the odometer reads %g of the speed, 1 sigma %g m/s'
          % (runs, n, n / fs, (n - stamps[hidden[0]]) / fs, ODO_ERR['scale'], ODO_ERR['stdv']))
    print('\nhorizontal position at the outage\'s last sample')
    print('   filter          1 sigma claimed [m]   across-run RMS error [m]')
    ids = np.arange(runs)
    for label, algo in plugins:
        job = ginsim.InsLooseJob(ctx, fs, rf, truth, acc, gyr, GPS_ERR, ini, runs, seed=2026, keep_traj=True, odo_err=ODO_ERR,
                                 aid=algo.aid(), odo_scale_state=algo.scale_options()).run()
        sig = job.final_sigmas()
        e = job.series('pos', ids)[:, -1, 0:2] - truth['ref_pos'][-1, 0:2]
        print('   %-14s  %18.3f   %18.3f' % (label, float(np.sqrt(np.mean(sig[:, 0] ** 2 + sig[:, 1] ** 2))),
                                             float(np.sqrt(np.mean(np.sum(e * e, axis=1))))))
        if algo.odo_scale_state:
            k_est, k_sigma = job.final_scale()
            scale_line = ('estimated scale factor: %.4f +- %.4f (mean over the runs and RMS of the filter\'s 1 sigma; across-run std %.4f)'
                          % (float(np.mean(k_est)), float(np.sqrt(np.mean(k_sigma ** 2))), float(np.std(k_est))))
        job.release()
    print('\n' + scale_line)
    ctx.close()


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 4096)
