#!/usr/bin/env python3
"""Two-series questions on the device-resident sensor series of an MI355X: a few runs of static_1800s.csv with a sinusoidal
vibration of 25 Hz on the three accelerometer axes, analysed by the plugin Coherence() in one Sim.  Per run it prints the
magnitude-squared coherence and the phase of the three accelerometer pairs at the vibration line and the mean coherence away from
it -- the line is common to the axes, the noise is not -- and then the test of the Monte-Carlo engine's own assumption: the largest
coherence between axis x of run 0 and axis x of run 1 away from the line (both runs carry the same vibration), next to 1 / K, from
ginsim.welch_csd on the job's buffer.  It prints what it measures and asserts nothing.

    PYTHONPATH=gnss-ins-sim_amd python examples/demo_coherence.py [runs]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'gnss-ins-sim_amd'))

from gnss_ins_sim.sim import imu_model, ins_sim                # noqa: E402
from demo_algorithms import csd_analysis                       # noqa: E402

MOTION = os.path.join(os.path.dirname(HERE), 'gnss-ins-sim_amd', 'motion_profiles', 'static_1800s.csv')
FS = 100.0
LINE = 25.0
ENV = {'acc': '[0.02 0.01 0.015]g-25Hz-sinusoidal'}
NPERSEG = 1024


class CoherenceAndRuns(csd_analysis.Coherence):
    """Coherence() that also takes accelerometer x of run 0 against run 1 from the job's buffer while it is on the device."""
    between_runs = None

    def run_device(self, sensor_job, fs):
        import ginsim
        if sensor_job.runs > 1:
            ptr, nseries = sensor_job.series_buffer(('accel', 'gyro'))
            self.between_runs = ginsim.welch_csd(sensor_job.ctx, ptr, sensor_job.n, nseries, sensor_job.n, fs, [(0, 3)], self.nperseg,
                                                 self.step, self.window, self.detrend)
        return super().run_device(sensor_job, fs)


def main(runs):
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=False)
    plugin = CoherenceAndRuns(nperseg=NPERSEG)
    sim = ins_sim.Sim([FS, 0.0, 0.0], MOTION, ref_frame=1, imu=imu, mode=None, env=ENV, algorithm=plugin, seed=952)
    sim.run(runs)
    d = sim.dmgr
    pairs = csd_analysis.default_pairs()
    acc = [i for i, (a, b) in enumerate(pairs) if a[0] == b[0] == 'accel']
    print('%4s  %-16s  %18s  %14s  %22s' % ('run', 'pair', 'coherence at 25 Hz', 'phase [rad]', 'mean coherence elsewhere'))
    for r in range(runs):
        freq, coh, ph = (getattr(d, k).data['algo0_%d' % r] for k in ('csd_freq', 'coherence', 'csd_phase'))
        line = int(np.argmin(np.abs(freq - LINE)))
        away = np.abs(np.arange(freq.size) - line) > 4
        away[:2] = False
        for i in acc:
            (_, a), (_, b) = pairs[i]
            print('%4d  accel %s - accel %s  %18.6f  %14.4f  %22.4f' % (r, 'xyz'[a], 'xyz'[b], coh[line, i], ph[line, i], np.mean(coh[away, i])))
    if plugin.between_runs is not None:
        c = plugin.between_runs.coherence[0]
        freq = plugin.between_runs.freq
        line = int(np.argmin(np.abs(freq - LINE)))
        away = np.abs(np.arange(freq.size) - line) > 4
        away[:2] = False
        K = (d.accel.data[0].shape[0] - NPERSEG) // (NPERSEG // 2) + 1
        print('accel x of run 0 against accel x of run 1: coherence at 25 Hz %.6f; away from the line largest %.4f, mean %.4f; 1 / K = %.4f'
              % (c[line], np.max(c[away]), np.mean(c[away]), 1.0 / K))


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 2)
