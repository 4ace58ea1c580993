"""Shared inputs of the magnetometer-aided InsLoose tests (tests/test_ins_loose_mag_oracle.py on the CPU,
tests/test_gpu_ins_loose_mag.py on the device): the outage profile's truth with the magnetometer's, the magnetometer models,
and the constants the CPU test measures and the device test is held to."""
import functools

import numpy as np

import ins_loose_aided_cases as ac
import ins_loose_cases as cs

GEO = (30.0, -3.0, 40.0)                               # geomagnetic field [uT] in NED at the profile's start
GEO_SOUTH = (20.0, 5.0, -45.0)                         # a southern field for the tilted profile: upward vertical component, opposite declination
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
# ref_frame 1, the LEVEL outage profile only; CONSISTENCY_BY_PROFILE below has the tilted profile, E0_OVER_SIGMA what ref_frame 0 carries.
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
def outage_truth(fs, ref_frame, fs_gps, n=None, profile=cs.OUTAGE_CSV, geo=GEO):
    """ins_loose_aided_cases.outage_truth with 'ref_mag' (n, 3), the truth field in the body frame for the field geo."""
    import ginsim
    from ginsim import workloads
    ini, truth, stamps = ac.outage_truth(fs, ref_frame, fs_gps, n, profile)
    ini_m, seg = workloads.parse_motion(profile)
    raw = ginsim.pathgen(ini_m, seg, fs, fs_gps, workloads.HIGH_MOBILITY, ref_frame, gps=True, geo_mag_n=geo)
    truth = dict(truth, ref_mag=np.ascontiguousarray(raw['mag'][:truth['ref_accel'].shape[0], 1:4]))
    truth['ref_mag'].setflags(write=False)
    return ini, truth, stamps


def model(mag_err, ref_frame, every=1, geo=GEO, **kw):
    """The block's numbers (ginsim.ins_loose.mag_model) for the filter that assumes mag_err's own calibration and the field geo."""
    from ginsim.ins_loose import mag_model
    return mag_model(mag_err, geo, ref_frame, dict({'every': every}, **kw))


def mag_kw(mag_err, geo=GEO, every=1, **kw):
    """The keywords of an InsLooseJob aided by the magnetometer mag_err in the field geo, under kw."""
    return dict(dict(mag_err=mag_err, geo_mag_n=geo, mag={'every': every}), **kw)


# ------------------------------------------------------------------------------------------------- consistency by profile and frame
# profile name -> (motion CSV, geomagnetic field, magnetometer model): the level outage profile as the tests above use it, and the
# tilted southern profile with a general calibration
PROFILES = {'level': (cs.OUTAGE_CSV, GEO, MAG_ERR), 'tilted': (cs.TILTED_CSV, GEO_SOUTH, MAG_ERR_SKEW)}
FILTERS = {'gps': (False, 0), 'odo1': (False, 1), 'mag': (True, 0), 'mag7': (True, 7)}         # name -> (magnetometer block, aiding mask)


# RMS end error over sqrt(mean pdiag_end) of the 15 states in ref_frame 1, by profile and filter; measured by
# tests/test_ins_loose_attitude_oracle.py::test_consistency_on_the_tilted_profile on consistency_draw(profile, 1, 20 Hz, 1024 runs).
# 'level' repeats the tables recorded above and in ins_loose_cases / ins_loose_aided_cases (ref_frame 1, the level outage profile, each
# from its own file's draw); 'tilted' is the tilted southern profile with MAG_ERR_SKEW and GEO_SOUTH.  'gps', 'odo1' and 'mag' lie in
# [0.7, 1.4]; 'mag7' is bounded above only.  The device is held to them within x/: 1.25 (tests/test_gpu_ins_loose_attitude.py).
CONSISTENCY_BY_PROFILE = {
    'level': {'gps': cs.CONSISTENCY_RATIOS, 'odo1': ac.CONSISTENCY_RATIOS[1], 'mag': CONSISTENCY_RATIOS[0], 'mag7': CONSISTENCY_RATIOS[7]},
    'tilted': {
        'gps': (1.018, 0.994, 0.909, 1.010, 0.998, 0.987, 0.965, 0.968, 1.017, 1.036, 1.040, 1.024, 0.966, 0.957, 0.953),
        'odo1': (1.042, 1.001, 0.908, 1.022, 1.001, 0.983, 0.961, 0.972, 1.017, 1.033, 1.040, 1.023, 0.966, 0.957, 0.954),
        'mag': (0.960, 0.991, 0.898, 0.997, 1.028, 0.996, 0.997, 0.974, 1.035, 1.032, 1.057, 1.013, 0.965, 0.957, 0.953),
        'mag7': (0.858, 0.585, 0.587, 0.918, 0.778, 0.795, 0.949, 0.973, 0.975, 1.035, 1.056, 1.008, 0.964, 0.957, 0.946),
    },
}
# ref_frame 0 only: the end error e0 of ONE run with error-free sensors, fixes and magnetometer over that run's sqrt(pdiag_end), for
# the 15 states, keyed (profile, filter, IMU rate in Hz); measured by tests/test_ins_loose_attitude_oracle.py::test_error_free_offset.
# The ref_frame 0 mechanisation and the path generator's truth differ by a discretisation term of first order in dt; the filter takes
# that drift for sensor error, so every run's estimate carries this same offset, which its covariance does not describe.  It SCALES
# WITH dt (compare 20 and 100 Hz).  In ref_frame 1 the same quantity is below 1e-6 in every state.  The across-run mean of the end
# error is this table within 4 sigma / sqrt(R) and the spread is the covariance's (test_ref_frame_0_spread_and_mean; on the device
# tests/test_gpu_ins_loose_attitude.py::test_consistency_in_ref_frame_0).
E0_OVER_SIGMA = {
    ('level', 'gps', 20): (0.109, 0.468, -0.232, -0.242, -0.803, 0.222, 1.142, -0.558, 0.366, -0.158, -0.128, 0.203, 0.019, 0.003, -0.007),
    ('level', 'mag', 20): (4.197, 1.111, -0.353, 3.310, -1.389, 0.299, 1.978, -0.645, 2.018, -0.018, -0.116, 0.186, 0.012, -0.203, -0.008),
    ('level', 'gps', 100): (0.020, 0.071, -0.053, -0.050, -0.161, 0.042, 0.224, -0.112, 0.071, -0.031, -0.022, 0.040, 0.004, 0.001, -0.002),
    ('level', 'mag', 100): (1.018, 0.215, -0.078, 0.788, -0.287, 0.059, 0.400, -0.179, 0.404, -0.004, -0.021, 0.032, 0.003, -0.043, -0.002),
    ('tilted', 'gps', 20): (-0.601, -0.011, -0.393, 0.406, 0.322, -0.092, -0.283, 1.162, 0.012, -0.027, -0.131, 0.023, 0.010, -0.000, -0.005),
    ('tilted', 'mag', 20): (-10.142, -1.730, -0.059, -13.574, -0.351, 0.131, -0.889, -0.476, 0.987, 0.261, 0.028, 0.312, 0.359, -0.093, -0.000),
    ('tilted', 'gps', 100): (-0.123, 0.000, -0.035, 0.088, 0.064, 0.025, -0.054, 0.233, 0.001, -0.006, -0.023, 0.004, 0.002, 0.000, -0.000),
    ('tilted', 'mag', 100): (-2.576, -0.426, 0.055, -3.506, -0.081, 0.092, -0.204, -0.139, 0.217, 0.055, 0.000, 0.069, 0.082, -0.021, 0.001),
}


def consistency_draw(profile, rf, fs, runs, error_free=False):
    """One draw for all four FILTERS: accel, gyro, fixes, odometer, magnetometer in that order from
    np.random.default_rng(ins_loose_cases.CONSISTENCY_SEED), 2 Hz GPS, 'mid-accuracy' IMU.  error_free: ONE run whose sensors, fixes,
    odometer and magnetometer are the truth's (the magnetometer's through its soft and hard iron, which the filter undoes)."""
    import ins_loose_ref as ref
    from ginsim.ins_loose import filter_model
    csv, geo, mag_err = PROFILES[profile]
    ini, truth, stamps = outage_truth(fs, rf, cs.CONSISTENCY_FS_GPS, None, csv, geo)
    acc_e, gyr_e = cs.imu_errors()
    c = {'profile': profile, 'rf': rf, 'fs': fs, 'ini': ini, 'truth': truth, 'stamps': stamps, 'geo': geo, 'mag_err': mag_err, 'acc_e': acc_e,
         'gyr_e': gyr_e, 'model': filter_model(fs, acc_e, gyr_e, cs.GPS_ERR)}
    if error_free:
        n = truth['ref_accel'].shape[0]
        c.update(runs=1, accel=truth['ref_accel'][None], gyro=truth['ref_gyro'][None], gps=truth['ref_gps'][None], tba=np.zeros((1, n, 3)),
                 tbg=np.zeros((1, n, 3)), odo=ac.ODO_ERR['scale'] * truth['ref_odo'][None],
                 mag=((truth['ref_mag'] + mag_err['hi']) @ np.asarray(mag_err['si']).reshape(3, 3).T)[None])
        return c
    rng = np.random.default_rng(cs.CONSISTENCY_SEED)
    c['accel'], c['gyro'], c['tba'], c['tbg'] = ref.sample_sensors(rng, fs, truth['ref_accel'], truth['ref_gyro'], acc_e, gyr_e, runs)
    c['gps'] = cs.sample_gps(rng, truth, rf, runs)
    c['odo'] = ref.sample_odo(rng, truth['ref_odo'], ac.ODO_ERR, runs)
    c['mag'] = ref.sample_mag(rng, truth['ref_mag'], mag_err, runs)
    c['runs'] = runs
    return c


def restate_filter(c, name):
    """The restatement's result of filter FILTERS[name] on a consistency_draw."""
    import ins_loose_ref as ref
    with_mag, mask = FILTERS[name]
    return ref.run(c['rf'], c['fs'], c['gyro'], c['accel'], c['ini'], c['model'], c['gps'], c['stamps'], c['truth']['gps_visibility'],
                    odo=c['odo'], aid=ac.aid(mask) if mask else None, mag=c['mag'] if with_mag else None,
                    mag_model=model(c['mag_err'], c['rf'], 1, c['geo']) if with_mag else None)


def end_error(c, att, pos, vel, wb, ab):
    """(R, 15) error state at the last sample of a consistency_draw, from the (R, 3) end states."""
    import ins_loose_ref as ref
    t = c['truth']
    return ref.error_state(c['rf'], att, pos, vel, wb, ab, t['ref_att'][-1], t['ref_pos'][-1], t['ref_vel'][-1], c['tbg'][:, -1], c['tba'][:, -1])


def end_statistics(e, pdiag_end):
    """{'ratio' RMS / sigma, 'spread' across-run std / sigma, 'mean' across-run mean / sigma, 'sigma'} per state; sigma = sqrt(mean P_kk)."""
    sigma = np.sqrt(np.mean(pdiag_end, axis=0))
    return {'ratio': np.sqrt(np.mean(e * e, axis=0)) / sigma, 'spread': np.std(e, axis=0) / sigma, 'mean': np.mean(e, axis=0) / sigma, 'sigma': sigma}
