"""Shared inputs of the standstill-aided InsLoose tests (tests/test_ins_loose_still_oracle.py on the CPU,
tests/test_gpu_ins_loose_still.py and tests/test_gpu_ins_loose_tilted_aids.py on the device): the stops profiles' truth and its standstill windows, the block's numbers,
and the constants the CPU test measures and the device test is held to."""
import functools
import os

import numpy as np

import ins_loose_aided_cases as ac
import ins_loose_cases as cs

# cruise at 5 m/s, brake to a stop (GPS visible), drive on, turn, an 18 s GPS outage (27-45 s) with a second stop inside it, turn back
STOPS_CSV = os.path.join(cs.REPO, 'tests', 'golden', 'ins_loose', 'motion_def_stops.csv')
# 41 S 150 W, 300 m: the same shape on a slope.  Yaw 170, pitch 12, roll -10 deg, braking from 6 m/s to a stop of 8 s (GPS visible), a
# turn of 30 deg through +-180 deg that also takes the pitch to -8 and the roll to 5 deg, a second stop inside a 16 s GPS outage (24-40 s),
# the turn back: 48 s.  vb = (vx, 0, 0) throughout, so the vehicle climbs and descends while it moves
TILTED_STOPS_CSV = os.path.join(cs.REPO, 'tests', 'golden', 'ins_loose', 'motion_def_tilted_stops.csv')

FILTERS = {'gps': 0, 'zupt': 1, 'zaru': 2, 'still': 3}                      # name -> still_mask

# Measured by tests/test_ins_loose_still_oracle.py::test_restatement_consistency: 1024 runs drawn from the filter's own model with
# np.random.default_rng(ins_loose_cases.CONSISTENCY_SEED) (accel, gyro, GPS as the unaided case draws them), the stops profile at
# 20 Hz with 2 Hz GPS, 'mid-accuracy' IMU, ref_frame 1, the default block (speed 0.01 m/s, rate 2e-4 rad/s, zupt_std 0.02 m/s,
# zaru_std sqrt(q_psi) fs, every sample).  RMS error over sqrt(mean pdiag) of the 15 states at the LAST SAMPLE OF THE FIRST STOP
# ('stop': the profile truncated there) and at the profile's end ('end'), for the unaided filter and the filter with both rows.
# The band: BAND, what the project holds the unaided and the magnetometer-aided filter to; see the test for the one state the
# standstill filter's own approximation moves.
BAND = (0.7, 1.4)
CONSISTENCY_RATIOS = {
    'gps': {'stop': (1.010, 0.995, 0.786, 1.009, 0.989, 0.915, 0.985, 1.014, 1.034, 1.004, 0.986, 0.977, 0.979, 0.935, 0.950),
            'end': (1.011, 1.006, 0.911, 0.929, 1.006, 0.965, 1.001, 0.966, 1.015, 0.985, 1.000, 0.992, 1.012, 0.957, 1.023)},
    'still': {'stop': (0.769, 0.734, 0.512, 0.498, 0.497, 0.692, 0.794, 0.812, 0.991, 1.008, 0.998, 0.976, 0.979, 0.935, 0.951),
              'end': (0.884, 0.912, 0.535, 0.927, 0.997, 0.873, 1.012, 0.972, 0.913, 1.056, 1.061, 1.008, 1.012, 0.957, 1.017)},
}
# CONSISTENCY_RATIOS is the LEVEL stops profile's.  By profile: 'tilted' is tests/golden/ins_loose/motion_def_tilted_stops.csv, the filter
# with both rows on consistency_draw(1, 20 Hz, 1024 runs, profile=TILTED_STOPS_CSV), at the last sample of its first stop (sample 301)
# and at its end; measured by tests/test_ins_loose_still_oracle.py::test_restatement_consistency_on_the_tilted_stops_profile, which
# asserts of them what the level test asserts of the filter with both rows.  tests/test_gpu_ins_loose_tilted_aids.py holds the device
# to them within x/: 1.25.
CONSISTENCY_BY_PROFILE = {
    'level': CONSISTENCY_RATIOS,
    'tilted': {'still': {'stop': (0.788, 0.625, 0.493, 0.504, 0.499, 0.686, 0.812, 0.828, 1.004, 1.050, 0.993, 0.972, 0.973, 0.943, 0.925),
                         'end': (0.890, 0.872, 0.517, 0.913, 0.918, 0.858, 0.939, 0.969, 0.925, 1.028, 1.071, 0.972, 0.999, 0.965, 0.966)}},
}


@functools.lru_cache(maxsize=None)
def stops_truth(fs, ref_frame, fs_gps, n=None, profile=STOPS_CSV):
    """(ini_pva, truth with 'ref_odo', gps stamps) of the stops profile, cut to the first n samples."""
    return ac.outage_truth(fs, ref_frame, fs_gps, n, profile)


def flags_of(truth, speed=0.01, rate=2e-4):
    from ginsim.ins_loose import standstill_flags
    return standstill_flags(truth, speed, rate)


def windows(flags):
    """[(first, last)] sample indices of the runs of non-zero flags."""
    f = np.concatenate([[0], (np.asarray(flags) != 0).astype(np.int8), [0]])
    d = np.diff(f)
    return list(zip(np.nonzero(d == 1)[0].tolist(), (np.nonzero(d == -1)[0] - 1).tolist()))


def options(mask, every=1, **kw):
    """The `still` dict InsLooseJob takes for a row mask: 1 ZUPT, 2 ZARU, 3 both."""
    assert mask in (1, 2, 3)
    return dict({'zupt': bool(mask & 1), 'zaru': bool(mask & 2), 'every': every}, **kw)


def model(filter_numbers, fs, mask, every=1, **kw):
    """The block's numbers (ginsim.ins_loose.still_model) for the filter with filter_model's numbers."""
    from ginsim.ins_loose import still_model
    return still_model(filter_numbers, fs, options(mask, every, **kw))


def consistency_draw(rf, fs, runs, n=None, profile=STOPS_CSV):
    """One draw for all FILTERS: accel, gyro, fixes in that order from np.random.default_rng(ins_loose_cases.CONSISTENCY_SEED), 2 Hz
    GPS, 'mid-accuracy' IMU, the stops profile (or `profile`) cut to its first n samples."""
    import ins_loose_ref as ref
    from ginsim.ins_loose import filter_model
    ini, truth, stamps = stops_truth(fs, rf, cs.CONSISTENCY_FS_GPS, n, profile)
    acc_e, gyr_e = cs.imu_errors()
    c = {'rf': rf, 'fs': fs, 'ini': ini, 'truth': truth, 'stamps': stamps, 'acc_e': acc_e, 'gyr_e': gyr_e, 'runs': runs,
         'model': filter_model(fs, acc_e, gyr_e, cs.GPS_ERR)}
    rng = np.random.default_rng(cs.CONSISTENCY_SEED)
    c['accel'], c['gyro'], c['tba'], c['tbg'] = ref.sample_sensors(rng, fs, truth['ref_accel'], truth['ref_gyro'], acc_e, gyr_e, runs)
    c['gps'] = cs.sample_gps(rng, truth, rf, runs)
    c['flags'] = flags_of(truth)
    return c


def restate_filter(c, name, keep_pdiag=False):
    """The restatement's result of filter FILTERS[name] on a consistency_draw."""
    import ins_loose_ref as ref
    mask = FILTERS[name]
    return ref.run(c['rf'], c['fs'], c['gyro'], c['accel'], c['ini'], c['model'], c['gps'], c['stamps'], c['truth']['gps_visibility'],
                    still=model(c['model'], c['fs'], mask) if mask else None, flags=c['flags'], keep_pdiag=keep_pdiag)


def error_at(c, o, j):
    """(R, 15) error state of a restatement's (or the device's) series at sample j of a consistency_draw."""
    import ins_loose_ref as ref
    t = c['truth']
    return ref.error_state(c['rf'], o['att'][:, j], o['pos'][:, j], o['vel'][:, j], o['wb'][:, j], o['ab'][:, j], t['ref_att'][j],
                           t['ref_pos'][j], t['ref_vel'][j], c['tbg'][:, j], c['tba'][:, j])


def ratios(e, pdiag):
    """RMS error over sqrt(mean P_kk), per state."""
    return np.sqrt(np.mean(e * e, axis=0)) / np.sqrt(np.mean(pdiag, axis=0))
