"""Shared inputs of the magnetometer-aided InsLoose tests (tests/test_ins_loose_mag_oracle.py on the CPU,
tests/test_gpu_ins_loose_mag.py on the device): the outage profile's truth with the magnetometer's, the magnetometer models, the
restatement's own rounding error as the parity bound, and the constants the CPU test measures and the device test is held to."""
import functools

import numpy as np

import ins_loose_aided_cases as ac
import ins_loose_cases as cs

GEO = (30.0, -3.0, 40.0)                               # geomagnetic field [uT] in NED at the profile's start
# imu_model.py's mid accuracy: no soft iron, no hard iron, 0.01 uT of noise
MAG_ERR = {'si': np.eye(3), 'hi': np.zeros(3), 'std': np.array([0.01, 0.01, 0.01])}
# a general calibration: with it a wrong transpose, a missed hard iron or a swapped noise axis shows
MAG_ERR_SKEW = {'si': np.array([[1.05, 0.02, 0.0], [0.01, 0.97, -0.03], [0.0, 0.02, 1.02]]), 'hi': np.array([3.0, -2.0, 1.0]),
                'std': np.array([0.01, 0.02, 0.015])}

# Measured by tests/test_ins_loose_mag_oracle.py::test_restatement_consistency_and_benefit: 1024 runs drawn from the filter's own model
# with np.random.default_rng(ins_loose_cases.CONSISTENCY_SEED) (accel, gyro, GPS and the odometer as the aided case draws them, then
# the magnetometer as ref_mag + 0.01 N), the outage profile at 20 Hz with 2 Hz GPS, 'mid-accuracy' IMU, MAG_ERR, GEO, a block at every
# sample, ref_frame 1.  RMS end error over sqrt(mean pdiag_end) for the 15 states, keyed by the aiding mask next to the magnetometer:
# 0 (the magnetometer alone) lies in [0.7, 1.4]; 7 is bounded above only (as mask 7 without the magnetometer).
CONSISTENCY_RATIOS = {
    0: (0.972, 0.992, 0.906, 0.985, 0.977, 0.927, 0.971, 1.000, 0.975, 1.022, 1.031, 1.022, 0.999, 0.974, 0.980),
    7: (0.732, 0.780, 0.460, 0.921, 0.764, 0.703, 0.909, 0.998, 0.922, 1.023, 1.030, 1.020, 0.997, 0.971, 0.973),
}
# Yaw 1 sigma [rad] and horizontal position 1 sigma [m] across those runs at the outage's first sample / its last sample / 5 s
# later / the profile's end: 'gps' the unaided filter, 'mag' with the magnetometer, 'mag7' with the magnetometer and mask 7.
YAW_TABLE = {
    'gps': (3.418e-4, 5.385e-4, 5.959e-4, 7.401e-4),
    'mag': (2.281e-4, 3.944e-4, 2.382e-4, 2.414e-4),
    'mag7': (1.605e-4, 1.346e-4, 1.538e-4, 1.815e-4),
}
HORIZONTAL_TABLE = {
    'gps': (0.164, 1.237, 0.536, 0.505),
    'mag': (0.110, 0.653, 0.346, 0.360),
    'mag7': (0.056, 0.104, 0.109, 0.112),
}


@functools.lru_cache(maxsize=None)
def outage_truth(fs, ref_frame, fs_gps, n=None):
    """ins_loose_aided_cases.outage_truth with 'ref_mag' (n, 3), the truth field in the body frame for GEO."""
    import ginsim
    from ginsim import workloads
    ini, truth, stamps = ac.outage_truth(fs, ref_frame, fs_gps, n)
    ini_m, seg = workloads.parse_motion(cs.OUTAGE_CSV)
    raw = ginsim.pathgen(ini_m, seg, fs, fs_gps, workloads.HIGH_MOBILITY, ref_frame, gps=True, geo_mag_n=GEO)
    truth = dict(truth, ref_mag=np.ascontiguousarray(raw['mag'][:truth['ref_accel'].shape[0], 1:4]))
    truth['ref_mag'].setflags(write=False)
    return ini, truth, stamps


def model(mag_err, ref_frame, every=1, **kw):
    """The block's numbers (ginsim.ins_loose.mag_model) for the filter that assumes mag_err's own calibration and GEO."""
    from ginsim.ins_loose import mag_model
    return mag_model(mag_err, GEO, ref_frame, dict({'every': every}, **kw))


def restatement_error(ref_frame, fs, gyro, accel, ini, model, gps, stamps, visible, odo, aid_numbers, mag, mag_numbers, max_runs=8):
    """The float64 restatement against its np.longdouble evaluation on the first max_runs runs of a case, in the metrics of
    ins_loose_cases.deviation."""
    import ins_loose_mag_ref as mref
    k = min(max_runs, gyro.shape[0])
    ini = np.asarray(ini)
    ini = ini[:, :k] if ini.ndim == 2 else ini
    args = (ref_frame, fs, gyro[:k], accel[:k], ini, model, None if gps is None else gps[:k], stamps, visible)
    kw = dict(odo=None if odo is None else odo[:k], aid=aid_numbers, mag=None if mag is None else mag[:k], mag_model=mag_numbers)
    return cs.deviation(mref.run(*args, **kw), mref.run(*args, dtype=np.longdouble, **kw))


def parity_bound(*args, **kw):
    """ins_loose_cases.PARITY_MARGIN (16) x restatement_error: what the device may deviate from the restatement, per quantity."""
    return {k: cs.PARITY_MARGIN * v for k, v in restatement_error(*args, **kw).items()}
