#!/usr/bin/env python3
"""Is the covariance of the filter with EVERY aid honest along the run?  On an MI355X: the loosely coupled GPS/INS Kalman filter of
demo_algorithms.ins_loose_device on GPS alone and with the odometer, the non-holonomic constraints, the odometer's scale factor as a
16th state, the magnetometer and the standstill updates in one launch (combined=True), over the Monte-Carlo runs of a ground-vehicle
profile with two stops and a stretch without GPS -- and, every 5 s, what each filter PREDICTS of its own error (the 1 sigma of its
covariance, averaged over the runs) next to the error it actually makes (the RMS over the runs, in the filter's own error
coordinates), the normalised error of the position, velocity and attitude block (NEES: 3 for a consistent filter) and, for the
scale-factor state, its sigma and the RMS of k_est - k against the Sim's odometer scale.
The sums are taken inside the filter's launch (Sim.consistency_curve_any_family()): nothing is kept, so the Sim is
statistics-only.

    PYTHONPATH=gnss-ins-sim_amd python examples/demo_ins_loose_all_consistency.py [runs]

Printed per filter (runs: default 4096): horizontal position and velocity sigma and RMS, their largest ratio over the nine
navigation states, the three block NEES and, for the combined filter, the scale state.
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

MOTION = os.path.join(REPO, 'tests', 'golden', 'ins_loose', 'motion_def_stops.csv')
fs = 100.0          # IMU sample frequency
fs_gps = 10.0       # GPS sample frequency
GEO = [30.0, -3.0, 40.0]


def main(runs):
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=9, gps=True, odo=True)
    imu.odo_err = dict(imu.odo_err, scale=0.99)                 # the odometer reads 1 % low; the filter starts from 1.0
    every = InsLoose(odo=True, nhc=True, odo_scale_state=True, mag=True, zupt=True, zaru=True, combined=True)
    sim = ins_sim.Sim([fs, fs_gps, fs], MOTION, ref_frame=1, imu=imu, mode=None, env=None, algorithm=[InsLoose(), every], seed=2026,
                      keep_trajectories=False, geo_mag_n=GEO)
    sim.run(runs)
    t0 = time.perf_counter()
    curve = sim.consistency_curve_any_family(every=5.0)
    print('%d runs x %d samples, two filters, %d checkpoints each: %.1f ms' % (runs, len(sim.dmgr.time.data), len(curve['time']),
                                                                             (time.perf_counter() - t0) * 1e3))
    vis = np.asarray(sim.dmgr.gps_visibility.data)
    gt = np.asarray(sim.dmgr.gps_time.data)
    for name, label in zip(sim.mc.loose_names, ('InsLoose()', 'InsLoose(every aid, combined=True)')):
        c = curve[name]
        scale = c.get('scale')
        print('\n%s over %d runs (* = no GPS)' % (label, int(c['count'].min())))
        print('   t [s]   horizontal position [m]   horizontal velocity [m/s]   largest     NEES' + ('                         scale factor' if scale else ''))
        print('            sigma      RMS            sigma      RMS             RMS/sigma   position velocity attitude' +
              ('   sigma    RMS      RMS/sigma' if scale else ''))
        for k, t in enumerate(curve['time']):
            out = vis[np.argmin(np.abs(gt - t))] == 0
            hp = [float(np.hypot(*c[key][k, 0:2])) for key in ('sigma', 'rms')]
            hv = [float(np.hypot(*c[key][k, 3:5])) for key in ('sigma', 'rms')]
            with np.errstate(all='ignore'):
                worst = np.nanmax(c['ratio'][k]) if np.any(np.isfinite(c['ratio'][k])) else float('nan')
            line = '%s %6.1f   %8.3f  %8.3f         %8.4f  %8.4f         %6.2f      %6.2f   %6.2f   %6.2f' \
                % ('*' if out else ' ', t, hp[0], hp[1], hv[0], hv[1], worst, c['nees'][k, 0], c['nees'][k, 1], c['nees'][k, 2])
            if scale:
                line += '     %.5f  %.5f  %6.2f' % (scale['sigma'][k], scale['rms'][k], scale['ratio'][k])
            print(line)


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 4096)
