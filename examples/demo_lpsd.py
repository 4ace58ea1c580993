#!/usr/bin/env python3
"""The drift corner of a gyroscope in its power spectral density, on an MI355X: a few runs of a static profile (the start of
static_1800s.csv held for 7200 s) at 100 Hz with the 'mid-accuracy' IMU, whose Gauss-Markov bias has a correlation time of 100 s
-- a corner at 1 / (2 pi Tc) = 1.6 mHz.  ``psd()`` with the longest segment there is, 8192 samples, resolves 12 mHz and its first
bins sit on the drift's slope; ``lpsd()`` runs the same estimate on the series halved again and again and reports each level's
best octave, down to 0.2 mHz here.  Both are printed per octave, averaged over runs and the octave's bins, next to the model's own
density (ginsim.model_psd): white, 2 sigma^2 / fs, plus the single-sided spectrum of the discrete first-order process that the
generator runs for the drift.  The plateau below the corner is in one curve and not in the other.

    PYTHONPATH=gnss-ins-sim_amd python examples/demo_lpsd.py [runs] [seconds]
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'gnss-ins-sim_amd'))

import ginsim                          # noqa: E402
from ginsim import workloads           # noqa: E402

FS, L = 100.0, 8192


def main(runs, seconds):
    n = int(seconds * FS)
    text = open(workloads.profile_path('static_1800s')).read().split('\n')
    ini, _ = workloads.parse_motion('\n'.join(text[:4]))
    raw = ginsim.pathgen(ini, np.array([[1.0, 0, 0, 0, 0, 0, 0, n / FS, 0.0]]), FS, 0.0, workloads.HIGH_MOBILITY, 1)
    truth = {'ref_accel': np.ascontiguousarray(raw['imu'][:, 1:4]), 'ref_gyro': np.ascontiguousarray(raw['imu'][:, 4:7]),
             'ref_pos': raw['nav'][:, 1:4], 'ref_vel': raw['nav'][:, 4:7], 'ref_att': raw['nav'][:, 7:10]}
    acc, gyr = workloads.imu_grade('mid-accuracy')
    ctx = ginsim.Context(0)
    job = ginsim.MonteCarloJob(ctx, FS, 1, truth, acc, gyr, None, runs=runs, algos=(), seed=952, keep_sensors=True).run()
    f1, p1 = job.psd(names=('gyro',), nperseg=L)
    f2, p2, lev = job.lpsd(names=('gyro',), nperseg=L, min_segments=2)
    job.release()
    ctx.close()
    tc = float((np.asarray(gyr['b_corr'], dtype=np.float64) * np.ones(3))[0])
    corner = 1.0 / (2 * math.pi * tc)
    print('gyro x, %d runs of %d s at %g Hz, nperseg %d: drift corner 1 / (2 pi %g s) = %.2e Hz' % (runs, seconds, FS, L, tc, corner))
    print('psd():  %d bins from %.2e Hz;   lpsd(): %d bins in %d levels from %.2e Hz' % (f1.size - 1, f1[1], f2.size - 1, lev.max() + 1, f2[1]))
    print('%-24s %12s %12s %12s' % ('octave [Hz]', 'model', 'lpsd()', 'psd()'))
    hi = FS / 2
    while hi > f2[1]:
        lo = hi / 2
        mid = math.sqrt(lo * hi)
        model = ginsim.model_psd(gyr, 'arw', FS, [mid])[0, 0]
        cols = []
        for f, p in ((f2, p2), (f1, p1)):
            sel = (f >= lo) & (f < hi) & (f > 0)
            cols.append('%12.3e' % p['gyro'][:, sel, 0].mean() if sel.any() else '%12s' % '-')
        print('%10.3e .. %-10.3e %12.3e %s %s%s' % (lo, hi, model, cols[0], cols[1], '   <- corner' if lo <= corner < hi else ''))
        hi = lo


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 4, float(sys.argv[2]) if len(sys.argv) > 2 else 7200.0)
