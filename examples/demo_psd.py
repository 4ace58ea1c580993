#!/usr/bin/env python3
"""The two curves of IEEE Std 952 from the same device-resident series on an MI355X: a few runs of static_1800s.csv with a
sinusoidal vibration of 25 Hz on the accelerometer, analysed by the plugins Allan(overlapping=True) and Psd(nperseg=4096) in one
Sim.  Per run: the gyroscope's Allan deviation at tau = 1 s beside the white level of its power spectral density, both against
what the IMU model's angle random walk predicts (sigma(tau) = arw / sqrt(tau); a single-sided density of 2 arw^2), and the
frequency of the largest line of the accelerometer's spectrum -- the line an Allan curve cannot show.

    PYTHONPATH=gnss-ins-sim_amd python examples/demo_psd.py [runs]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'gnss-ins-sim_amd'))

from gnss_ins_sim.sim import imu_model, ins_sim                # noqa: E402
from demo_algorithms import allan_analysis, psd_analysis       # noqa: E402

MOTION = os.path.join(os.path.dirname(HERE), 'gnss-ins-sim_amd', 'motion_profiles', 'static_1800s.csv')
FS = 100.0
ENV = {'acc': '[0.02 0.0 0.0]g-25Hz-sinusoidal'}


def main(runs):
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=False)
    sim = ins_sim.Sim([FS, 0.0, 0.0], MOTION, ref_frame=1, imu=imu, mode=None, env=ENV,
                      algorithm=[allan_analysis.Allan(overlapping=True), psd_analysis.Psd(nperseg=4096)], seed=952)
    sim.run(runs)
    d = sim.dmgr
    arw = np.asarray(imu.gyro_err['arw']) * np.ones(3)
    print('gyro x: model arw %.3e rad/s/sqrt(Hz) -> Allan deviation at 1 s %.3e, PSD white level %.3e (rad/s)^2/Hz'
          % (arw[0], arw[0], 2 * arw[0] ** 2))
    print('%4s  %14s  %14s  %16s  %12s' % ('run', 'AD(1 s) gyro x', 'PSD gyro x', 'accel x line [Hz]', 'line height'))
    for r in range(runs):
        tau, ad = d.algo_time.data['algo0_%d' % r], d.ad_gyro.data['algo0_%d' % r]
        freq, pg, pa = (getattr(d, k).data['algo1_%d' % r] for k in ('psd_freq', 'psd_gyro', 'psd_accel'))
        at_1s = ad[np.argmin(np.abs(tau - 1.0)), 0]
        white = np.mean(pg[freq > 5.0, 0])                  # above the bias instability's corner
        line = np.argmax(pa[1:, 0]) + 1
        print('%4d  %14.3e  %14.3e  %16.3f  %12.3e' % (r, at_1s, white, freq[line], pa[line, 0]))


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 4)
