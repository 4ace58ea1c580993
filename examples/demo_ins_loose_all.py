#!/usr/bin/env python3
"""Every aid of the loosely coupled GPS/INS filter together, on an MI355X: the filter of demo_algorithms.ins_loose_device six times
over the same Monte-Carlo runs of a 55 s ground-vehicle profile with two stops, one of them inside an 18 s GPS outage.  The car has
a wheel-speed sensor that reads 0.99 of the truth (nobody knows its scale to 1 %), a magnetometer and a standstill signal:

    InsLoose()                                      GPS alone
    InsLoose(odo=True, nhc=True)                    odometer (the filter assumes a scale of 1.0) and non-holonomic constraints
    InsLoose(odo=True, nhc=True, odo_scale_state=True)   the same with the scale factor as a 16th state
    InsLoose(mag=True)                              magnetometer
    InsLoose(zupt=True, zaru=True)                  zero-velocity and zero-angular-rate updates at standstill
    InsLoose(odo=True, nhc=True, odo_scale_state=True, mag=True, zupt=True, zaru=True, combined=True)   all of them, one launch

All filters see the same sensor realisation per run; every run is a lane of one launch per filter that makes its own IMU samples,
fixes, odometer and magnetometer samples (DESIGN 4.11h for the last; 4.11b, d, e, g for the single aids).

    PYTHONPATH=gnss-ins-sim_amd python examples/demo_ins_loose_all.py [runs]

Printed per filter: the across-run 1 sigma of the horizontal position and of the yaw error at the end of the outage, and the mean
scale-factor estimate at the profile's end where the filter has one (runs: default 4096).
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
READS = 0.99        # what the odometer reads of the true speed


def main(runs):
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=9, gps=True, odo=True)
    imu.odo_err = dict(imu.odo_err, scale=READS)
    filters = [('GPS alone', InsLoose()),
               ('odometer (assumes 1.0) + constraints', InsLoose(odo=True, nhc=True, odo_scale=1.0)),
               ('odometer with the scale state + constraints', InsLoose(odo=True, nhc=True, odo_scale_state=True)),
               ('magnetometer', InsLoose(mag=True)),
               ('standstill (ZUPT + ZARU)', InsLoose(zupt=True, zaru=True)),
               ('all of them, combined=True', InsLoose(odo=True, nhc=True, odo_scale_state=True, mag=True, zupt=True, zaru=True, combined=True))]
    sim = ins_sim.Sim([fs, fs_gps, fs], MOTION, ref_frame=1, imu=imu, mode=None, env=None, algorithm=[a for _, a in filters], seed=2026,
                      keep_trajectories=True, geo_mag_n=[30.0, -3.0, 40.0])
    t0 = time.perf_counter()
    sim.run(runs)
    n = len(sim.dmgr.time.data)
    print('%d runs x %d samples, %d filters, everything kept: %.1f ms' % (runs, n, len(filters), (time.perf_counter() - t0) * 1e3))
    vis, gt = np.asarray(sim.dmgr.gps_visibility.data), np.asarray(sim.dmgr.gps_time.data)
    hidden = gt[vis == 0]
    last = int(round((hidden.max() + 1.0 / fs_gps) * fs)) - 1         # the sample before the first fix after the outage
    print('GPS outage: %.1f-%.1f s; the odometer reads %.2f of the true speed' % (hidden.min(), (last + 1) / fs, READS))
    curve = sim.error_curve(('att_euler', 'pos'), samples=np.array([last]))
    print('\n%-46s %-34s %12s %10s %10s' % ('filter', 'kernel', 'horizontal m', 'yaw deg', 'scale'))
    for (label, algo), name, (_, job, _) in zip(filters, sim.mc.nav_names, sim.loose_jobs):
        hor = float(np.hypot(*curve['pos']['std'][name][0, 0:2]))
        yaw = float(curve['att_euler']['std'][name][0, 0])
        scale = '%10.4f' % float(np.mean(job.final_scale()[0])) if algo.odo_scale_state else '%10s' % '-'
        kernel = job.kernel_name().replace('ginsim::', '').split('<')[0]
        print('%-46s %-34s %12.3f %10.4f %s' % (label, kernel, hor, yaw, scale))


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 4096)
