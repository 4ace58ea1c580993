"""Shared inputs of the tests of InsLoose's scale-factor state (tests/test_ins_loose_scale_oracle.py on the CPU,
tests/test_gpu_ins_loose_scale.py and tests/test_gpu_ins_loose_tilted_aids.py on the device): the options, the draws, the metrics of the parity bound (deviation),
and every number the CPU test measures and records."""
import numpy as np

import ins_loose_aided_cases as ac
import ins_loose_cases as cs

SCALE0, P0_SCALE = 1.0, 0.02                   # the defaults of ginsim.ins_loose.scale_model
ODO_STDV = ac.ODO_ERR['stdv']
READS = 0.99                                    # the odometer of the payoff table and of the defect (ins_loose_aided_cases.ODO_ERR)

# Measured by tests/test_ins_loose_scale_oracle.py::test_restatement_consistency: 1024 runs drawn from the filter's own model with
# np.random.default_rng(ins_loose_cases.CONSISTENCY_SEED) (accel, gyro, GPS as the unaided case draws them, then the true scales
# ~ N(1, 0.02^2), then the odometer's noise), the outage profile at 20 Hz with 2 Hz GPS, 'mid-accuracy' IMU, stdv 0.1, the odometer
# row alone (mask 1: the constraint rows are pessimistic by construction on this profile, ins_loose_aided_cases), a block at every
# sample, ref_frame 1, scale0 = 1, p0 = 0.02, q = 0.  RMS end error over sqrt(mean P_kk) for the 16 states; the 16th is k_est - k.
CONSISTENCY_BAND = (0.8, 1.25)
CONSISTENCY_RATIOS = (1.001, 0.982, 0.925, 1.059, 0.974, 0.939, 0.950, 0.974, 1.007, 1.014, 1.015, 0.998, 0.999, 0.972, 0.980, 0.999)
# at the end of those runs: RMS of k_est - k 0.00040, sqrt(mean P[15][15]) 0.00040 (from the initial 0.02)
# CONSISTENCY_RATIOS is the LEVEL outage profile's.  By profile: 'tilted' is the same draw (draws(1024, CONSISTENCY_SEED, profile=
# ins_loose_cases.TILTED_CSV)) and the same filter on tests/golden/ins_loose/motion_def_tilted.csv; measured by
# tests/test_ins_loose_scale_oracle.py::test_restatement_consistency_on_the_tilted_profile, inside the same band.
# tests/test_gpu_ins_loose_tilted_aids.py holds the device to them within x/: 1.25.
CONSISTENCY_BY_PROFILE = {
    'level': CONSISTENCY_RATIOS,
    'tilted': (0.999, 1.015, 0.915, 1.014, 0.989, 0.990, 0.955, 0.982, 1.023, 1.030, 1.043, 1.023, 0.966, 0.957, 0.954, 1.008),
    # at the end of those runs: RMS of k_est - k 0.00048, sqrt(mean P[15][15]) 0.00047
}
# The defect the state removes: on the same runs (the same noise, every odometer reading 0.99) the 15-state filter that assumes 1.0.
# The largest of its position and velocity ratios (it must exceed 3) and the state it belongs to.
# All 15: 4.089, 28.037, 5.093, 7.317, 1.371, 5.607, 2.961, 1.317, 1.015, 1.012, 2.299, 1.003, 0.999, 0.973, 1.041.
WRONG_SCALE_RATIO = (28.037, 1)

# Measured by tests/test_ins_loose_scale_oracle.py::test_payoff_table: 257 runs (np.random.default_rng(PAYOFF_SEED); accel, gyro, GPS,
# then the odometer's noise), the same profile and rates, an odometer that reads 0.99, odometer and constraints (mask 7) at every
# sample.  At the outage's last sample: (sqrt(mean(P_00 + P_11)) [m], RMS horizontal position error across the runs [m]) of the filter
# that assumes 1.0, of the filter told 0.99 and of the filter with the state (scale0 1, p0 0.02); for the last also the mean k_est
# and the mean 1 sigma of the scale factor at the profile's end.
PAYOFF_RUNS, PAYOFF_SEED = 257, 20260118
PAYOFF_TABLE = {'wrong': (0.197, 3.575), 'told': (0.198, 0.196), 'state': (0.266, 0.252)}
PAYOFF_SCALE = (0.9900, 0.0004)
# the RMS of the filter with the state over that of the filter told the truth: measured, recorded, asserted with this head-room
PAYOFF_FACTOR = 1.282
PAYOFF_HEADROOM = 1.1

# Measured by tests/test_ins_loose_scale_oracle.py::test_float64_error_of_the_restatement: the float64 restatement against its
# np.longdouble evaluation (deviation's metrics) on 5 runs of the outage profile at 20 Hz (draws(5, 3, ref_frame)), the defaults of
# the state, per (ref_frame, mask).  wb and ab are relative to series of 1e-5 and smaller, hence their size.
RESTATEMENT_ERROR = {
    (0, 1): dict(att=8.12e-13, pos=1.04e-11, vel=9.92e-12, wb=7.06e-10, ab=4.10e-10, pdiag_end=7.95e-13, k_est=6.47e-12, scale_end=6.46e-12,
                 pcross_end=2.19e-12),
    (0, 7): dict(att=9.29e-13, pos=1.90e-11, vel=1.32e-11, wb=1.05e-09, ab=6.23e-09, pdiag_end=3.12e-12, k_est=6.09e-12, scale_end=6.09e-12,
                 pcross_end=2.24e-12),
    (1, 1): dict(att=3.32e-13, pos=4.82e-15, vel=9.02e-12, wb=4.27e-10, ab=6.15e-10, pdiag_end=3.12e-13, k_est=1.74e-12, scale_end=1.74e-12,
                 pcross_end=5.81e-13),
    (1, 7): dict(att=1.09e-12, pos=6.18e-15, vel=5.03e-12, wb=3.34e-10, ab=2.03e-09, pdiag_end=7.89e-13, k_est=1.47e-12, scale_end=1.47e-12,
                 pcross_end=6.86e-13),
}

PARITY_KEYS = cs.PARITY_KEYS + ('k_est', 'scale_end', 'pcross_end')


def scale(scale0=SCALE0, p0=P0_SCALE, q=0.0, fs=None):
    """The numbers of the state (ginsim.ins_loose.scale_model)."""
    from ginsim.ins_loose import scale_model
    return scale_model(None, {'scale0': scale0, 'p0': p0, 'q': q}, fs)


def aid(mask, every=1, scale0=SCALE0):
    """The aiding numbers of the filter with the state: ins_loose_aided_cases.aid with r_odo = (stdv / scale0)^2, as InsLooseJob
    makes them (odo_scale_f is not read)."""
    return ac.aid(mask, every, odo_err={'scale': scale0, 'stdv': ODO_STDV})


def deviation(a, b):
    """ins_loose_cases.deviation and, for the outputs of the state: k_est (the series) and scale_end (k_est, P[15][15]) relative,
    pcross_end relative to sqrt(P_kk P[15][15]) of b (a zero reference: absolute).  The family's parity bound is
    ins_loose_cases.parity_bound(..., run=ins_loose_scale_ref.run, deviation=deviation, odo=, aid=, scale=)."""
    out = cs.deviation(a, b)
    lo = np.longdouble
    for k in ('k_est', 'scale_end'):
        x, y = np.asarray(a[k], dtype=lo), np.asarray(b[k], dtype=lo)
        out[k] = float(np.max(np.abs(x - y) / np.where(y == 0, 1.0, np.abs(y))))
    x, y = np.asarray(a['pcross_end'], dtype=lo), np.asarray(b['pcross_end'], dtype=lo)
    s = np.sqrt(np.asarray(b['pdiag_end'], dtype=lo) * np.asarray(b['scale_end'], dtype=lo)[:, 1:2])
    out['pcross_end'] = float(np.max(np.abs(x - y) / np.where(s == 0, 1.0, s)))
    return out


def draws(runs, seed, ref_frame=1, fs=cs.CONSISTENCY_FS, fs_gps=cs.CONSISTENCY_FS_GPS, scales=None, profile=cs.OUTAGE_CSV):
    """One set of runs drawn from the filter's own model on the outage profile (or `profile`): accel, gyro and GPS as
    tests/test_ins_loose_aided_oracle.py draws them, then the true scale of every run (scales None: ~ N(1, P0_SCALE^2); a number:
    that scale in every run, nothing drawn) and the odometer's noise.  Returns a dict: ini, truth, stamps, acc_e, gyr_e, accel, gyro,
    tba, tbg, gps, scales (R,), noise (R, n) [the odometer's, stdv z] and model."""
    import ins_loose_ref as ref
    from ginsim.ins_loose import filter_model
    ini, truth, stamps = ac.outage_truth(fs, ref_frame, fs_gps, None, profile)
    acc_e, gyr_e = cs.imu_errors()
    rng = np.random.default_rng(seed)
    accel, gyro, tba, tbg = ref.sample_sensors(rng, fs, truth['ref_accel'], truth['ref_gyro'], acc_e, gyr_e, runs)
    gps = cs.sample_gps(rng, truth, ref_frame, runs)
    k = 1.0 + P0_SCALE * rng.standard_normal(runs) if scales is None else np.full(runs, float(scales))
    noise = ODO_STDV * rng.standard_normal((runs, truth['ref_odo'].shape[0]))
    return dict(ini=ini, truth=truth, stamps=stamps, acc_e=acc_e, gyr_e=gyr_e, accel=accel, gyro=gyro, tba=tba, tbg=tbg, gps=gps, scales=k,
                noise=noise, model=filter_model(fs, acc_e, gyr_e, cs.GPS_ERR), fs=fs, fs_gps=fs_gps, rf=ref_frame)


def odometer(d, scales=None):
    """(R, n): scales[r] ref_odo + the drawn noise (scales None: the drawn ones; a number: every run reads that)."""
    k = d['scales'] if scales is None else np.full(d['noise'].shape[0], float(scales))
    return k[:, None] * np.asarray(d['truth']['ref_odo'])[None] + d['noise']


def ratios16(d, o, k_true):
    """RMS end error over sqrt(mean P_kk) of the 16 states of a result of ins_loose_scale_ref.run (15 of one of ins_loose_ref.run)."""
    import ins_loose_ref as ref
    t = d['truth']
    e = ref.error_state(d['rf'], o['att'][:, -1], o['pos'][:, -1], o['vel'][:, -1], o['wb'][:, -1], o['ab'][:, -1], t['ref_att'][-1],
                        t['ref_pos'][-1], t['ref_vel'][-1], d['tbg'][:, -1], d['tba'][:, -1])
    p = np.asarray(o['pdiag_end'], dtype=np.float64)
    if 'scale_end' in o:
        se = np.asarray(o['scale_end'], dtype=np.float64)
        e = np.concatenate([e, (se[:, 0] - k_true)[:, None]], axis=1)
        p = np.concatenate([p, se[:, 1:2]], axis=1)
    return np.sqrt(np.mean(e * e, axis=0)) / np.sqrt(np.mean(p, axis=0))
