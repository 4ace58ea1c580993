"""Shared inputs of the InsLoose tests (tests/test_ins_loose_oracle.py on the CPU, tests/test_gpu_ins_loose.py on the device): the
outage profile's truth, the error models, sampled sensors, and the constants one file measures and the other holds the device to."""
import functools
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTAGE_CSV = os.path.join(REPO, 'tests', 'golden', 'ins_loose', 'motion_def_outage.csv')
# 41 S, 150 W, 300 m; yaw 165 deg through +-180 deg twice, pitch 20 -> -20 -> 20 deg, roll -15 -> 15 -> -15 deg, climbing and descending,
# vb = (vx, 0, 0) throughout; 40 s with a 10 s GPS outage (tests/test_ins_loose_attitude_oracle.py, tests/test_gpu_ins_loose_attitude.py)
TILTED_CSV = os.path.join(REPO, 'tests', 'golden', 'ins_loose', 'motion_def_tilted.csv')
GPS_ERR = {'stdp': np.array([5.0, 5.0, 7.0]), 'stdv': np.array([0.05, 0.05, 0.05])}       # imu_model.py's gps_low_accuracy

# Consistency of the restatement, measured by tests/test_ins_loose_oracle.py::test_restatement_consistency (1024 runs sampled from the
# filter's own model with np.random.default_rng(20260117), the outage profile at 20 Hz with 2 Hz GPS, 'mid-accuracy' IMU, ref_frame 1):
# RMS end error over sqrt(mean pdiag_end) for the 15 states.  A consistent filter has 1; the band the issue allows is [0.7, 1.4].
# This table is for ref_frame 1 on the LEVEL outage profile only; the tilted profile's and what ref_frame 0 carries instead
# (a deterministic offset) are in ins_loose_mag_cases.CONSISTENCY_BY_PROFILE and E0_OVER_SIGMA.
CONSISTENCY_FS, CONSISTENCY_FS_GPS, CONSISTENCY_RUNS, CONSISTENCY_SEED = 20.0, 2.0, 1024, 20260117
CONSISTENCY_RATIOS = (0.988, 0.982, 0.942, 1.022, 0.963, 0.950, 0.941, 0.960, 1.015, 1.010, 1.013, 0.996, 0.999, 0.972, 0.980)


@functools.lru_cache(maxsize=None)
def outage_truth(fs, ref_frame, fs_gps, n=None, profile=OUTAGE_CSV):
    """(ini_pva, truth dict, gps stamps int64) of a motion profile (default: the outage profile), cut to the first n samples (and
    the fixes inside them)."""
    import ginsim
    from ginsim import workloads
    ini, seg = workloads.parse_motion(profile)
    raw = ginsim.pathgen(ini, seg, fs, fs_gps, workloads.HIGH_MOBILITY, ref_frame, gps=True)
    n = raw['imu'].shape[0] if n is None else int(n)
    stamps = np.rint(raw['gps'][:, 0]).astype(np.int64)
    m = int(np.count_nonzero(stamps < n))
    truth = {'ref_accel': np.ascontiguousarray(raw['imu'][:n, 1:4]), 'ref_gyro': np.ascontiguousarray(raw['imu'][:n, 4:7]),
             'ref_pos': np.ascontiguousarray(raw['nav'][:n, 1:4]), 'ref_vel': np.ascontiguousarray(raw['nav'][:n, 4:7]),
             'ref_att': np.ascontiguousarray(raw['nav'][:n, 7:10]), 'ref_gps': np.ascontiguousarray(raw['gps'][:m, 1:7]),
             'gps_time': raw['gps'][:m, 0] / fs, 'gps_visibility': raw['gps'][:m, 7].copy()}
    for v in truth.values():
        v.setflags(write=False)
    return ini, truth, stamps[:m]


def imu_errors(name='mid-accuracy', gyro_b=None, accel_b=None):
    """(accel_err, gyro_err) of a built-in grade as plain dicts, with optional constant biases."""
    from ginsim import workloads
    acc, gyr = workloads.imu_grade(name)
    acc = {k: np.array(v, dtype=np.float64) for k, v in acc.items()}
    gyr = {k: np.array(v, dtype=np.float64) for k, v in gyr.items()}
    if gyro_b is not None:
        gyr['b'] = np.array(gyro_b, dtype=np.float64)
    if accel_b is not None:
        acc['b'] = np.array(accel_b, dtype=np.float64)
    return acc, gyr


def sample_gps(rng, truth, ref_frame, runs, gps_err=GPS_ERR):
    """(R, m, 6) fixes drawn from pathgen.gps_gen's model (oracle/ins_np.gps_errors)."""
    from oracle import ins_np
    m = truth['ref_gps'].shape[0]
    return ins_np.gps_errors(truth['ref_gps'], gps_err, ref_frame, rng.standard_normal((runs, m, 3)), rng.standard_normal((runs, m, 3)))


PARITY_KEYS = ('att', 'pos', 'vel', 'wb', 'ab', 'pdiag_end')
PARITY_MARGIN = 16.0            # MagCal's margin for the freedom in the order of operations


def deviation(a, b):
    """The metrics of the parity bound, per quantity, of result dict a against b: attitude in rad modulo 2 pi, pos and vel
    relative to max(1, |x|), wb and ab relative to the series' maximum, pdiag_end relative."""
    out = {}
    for k in PARITY_KEYS:
        x, y = np.asarray(a[k], dtype=np.longdouble), np.asarray(b[k], dtype=np.longdouble)
        d = np.abs(x - y)
        if k == 'att':
            d, s = np.abs(np.mod(x - y + np.pi, 2 * np.pi) - np.pi), 1.0
        elif k in ('pos', 'vel'):
            s = np.maximum(1.0, np.abs(y))
        elif k == 'pdiag_end':
            s = np.abs(y)
        else:
            s = max(float(np.max(np.abs(y))), np.finfo(np.float64).tiny)
        out[k] = float(np.max(d / s))
    return out


def restatement_error(ref_frame, fs, gyro, accel, ini, model, gps, stamps, visible, max_runs=8, run=None, deviation=deviation, **blocks):
    """The float64 restatement against its np.longdouble evaluation on the first max_runs runs of a case: {quantity: deviation}.
    The device is allowed PARITY_MARGIN times this (parity_bound).  blocks: the optional blocks' keyword arguments of run
    (default ins_loose_ref.run): aid, still, flags, mag_model, scale as they are, the per-run series odo and mag cut to the same runs."""
    import ins_loose_ref as ref
    k = min(max_runs, gyro.shape[0])
    ini = np.asarray(ini)
    ini = ini[:, :k] if ini.ndim == 2 else ini
    args = (ref_frame, fs, gyro[:k], accel[:k], ini, model, None if gps is None else gps[:k], stamps, visible)
    kw = {key: v[:k] if key in ('odo', 'mag') and v is not None else v for key, v in blocks.items()}
    run = run or ref.run
    return deviation(run(*args, **kw), run(*args, dtype=np.longdouble, **kw))


def parity_bound(*args, **kw):
    """PARITY_MARGIN (16) x restatement_error: what the device may deviate from the restatement, per quantity."""
    return {k: PARITY_MARGIN * v for k, v in restatement_error(*args, **kw).items()}
