#!/usr/bin/env python3
"""The reference's inclinometer plugins on an MI355X: MahonyFilter and TiltAcc (demo_algorithms.inclinometer_device) over 65 536 runs
of motion_def.csv (542 s at 100 Hz), statistics only -- the runs of the MahonyFilter chained as the reference chains them (each starts
from the gyro_bias the previous run ended with), solved by whole-batch passes.

    PYTHONPATH=gnss-ins-sim_amd python examples/demo_inclinometer.py [runs]
"""
import contextlib
import io
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, 'gnss-ins-sim_amd'))

from gnss_ins_sim.sim import imu_model, ins_sim                        # noqa: E402
from demo_algorithms.inclinometer_device import MahonyFilter, TiltAcc  # noqa: E402

MOTION = os.path.join(REPO, 'tests', 'golden', 'inclinometer', 'motion_def.csv')


def main(runs):
    import ginsim
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=False)
    ctx = ginsim.default_context()
    for label in ('first Sim.run (library loads, arena, truth)', 'second Sim.run (the chain goes on)'):
        mah = MahonyFilter() if label.startswith('first') else mah
        sim = ins_sim.Sim([100.0, 0.0, 0.0], MOTION, ref_frame=1, imu=imu, algorithm=[mah, TiltAcc()], seed=2026,
                          keep_trajectories=False)
        ctx.sync()
        t0 = time.perf_counter()
        sim.run(runs)
        dt = time.perf_counter() - t0
        n = len(sim.dmgr.time.data)
        with contextlib.redirect_stdout(io.StringIO()):
            sim.results(err_stats_start=-1)
        st = sim.err_stats['att_euler']
        print('%s: %d runs x %d samples, %d passes, %.1f ms (%.1f ms per pass), %.3g sample*MC/s' % (
            label, runs, n, sim.passes[0], dt * 1e3, dt * 1e3 / sim.passes[0], n * runs / dt))
        print('    end-point att_euler error std [deg]: Mahony %s  tilt %s   gyro_bias after the last run %s' % (
            np.array2string(np.asarray(st['std']['algo0']), precision=4), np.array2string(np.asarray(st['std']['StaticTilt']), precision=4),
            np.array2string(mah.gyro_bias, precision=6)))


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 65536)
