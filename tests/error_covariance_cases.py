"""Shared inputs of the error-covariance tests (tests/test_error_covariance_oracle.py on the CPU, tests/test_gpu_error_covariance.py
on the device; no test in it): the short cut of the turn profile, the motivation's three filters on the outage profile, and the
numbers the CPU test measured."""
import functools

import numpy as np

import ins_loose_cases as cs
import ins_loose_aided_cases as ac

FS = 100.0
CUT = 64                        # samples of the turn profile the device tests keep (the first 0.64 s)

# The motivation, measured by tests/test_error_covariance_oracle.py::test_the_odometer_leaves_a_strip_across_the_track: the NumPy
# restatement tests/ins_loose_ref.py on the outage profile, ref_frame 1, 20 Hz, 2 Hz GPS, 'mid-accuracy' IMU, ODO_ERR and NHC_STD of
# tests/ins_loose_aided_cases.py, 256 runs drawn with np.random.default_rng(1) (accel, gyro, GPS, odometer, in that order), the
# position error at the last sample of the 20 s outage (truth heading 120 degrees).  Per aiding mask (0: GPS only, 1: + odometer,
# 7: + odometer + constraints): sigma x, sigma y, rho xy, along-track sigma, cross-track sigma, ellipse semi-major, semi-minor [m],
# azimuth of the major axis from the x axis [deg].  Only the qualitative claim is asserted (along < 0.25 cross for mask 1).
MOTIVATION_FS, MOTIVATION_FS_GPS, MOTIVATION_RUNS, MOTIVATION_SEED = 20.0, 2.0, 256, 1
MOTIVATION_TABLE = {
    0: (0.958, 0.892, -0.009, 0.913, 0.939, 0.958, 0.892, -3.5),
    1: (0.772, 0.445, 0.944, 0.129, 0.882, 0.882, 0.129, 29.2),
    7: (0.153, 0.100, 0.149, 0.107, 0.148, 0.154, 0.098, 9.5),
}

# The first 0.64 s of the 90-degree turn as a motion definition of its own (64 samples at 100 Hz): what the Sims of the device
# tests run, so that 4096 kept runs are 19 MB
SHORT_TURN = """ini lat (deg),ini lon (deg),ini alt (m),ini vx_body (m/s),ini vy_body (m/s),ini vz_body (m/s),ini yaw (deg),ini pitch (deg),ini roll (deg)
31.9965,120.004,0,10,0,0,315,0,0
command type,yaw (deg),pitch (deg),roll (deg),vx_body (m/s),vy_body (m/s),vz_body (m/s),command duration (s),GPS visibility
1,0,0,0,0,0,0,0.2,0
1,15,0,0,0,0,0,0.44,0
"""


def short_sim(pkg, runs, rf=1, seed=99, **kw):
    """A Sim of FreeIntegration over SHORT_TURN, run."""
    import sys
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    from gnss_ins_sim.sim import imu_model, ins_sim
    from demo_algorithms import free_integration
    from ginsim import workloads
    ini = workloads.parse_motion(SHORT_TURN)[0]
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=False)
    sim = ins_sim.Sim([FS, 0.0, 0.0], SHORT_TURN, ref_frame=rf, imu=imu, algorithm=free_integration.FreeIntegration(ini), seed=seed, **kw)
    sim.run(runs)
    return sim


@functools.lru_cache(maxsize=None)
def turn_truth(rf, n=CUT):
    """(ini, truth dict, ref_nav (n, 9)) of the first n samples of the 90-degree turn at 100 Hz."""
    from ginsim import workloads
    ini, truth, _ = workloads.truth_from_profile('turn_90deg', FS, rf)
    truth = {k: np.ascontiguousarray(v[:n]) for k, v in truth.items()}
    ref_nav = np.ascontiguousarray(np.concatenate([truth['ref_att'], truth['ref_pos'], truth['ref_vel']], axis=1))
    for v in list(truth.values()) + [ref_nav]:
        v.setflags(write=False)
    return ini, truth, ref_nav


def motivation_errors(mask):
    """(position errors (runs, 3) at the outage's last sample, the truth's yaw there) of the restatement with aiding mask 0, 1 or 7."""
    import ins_loose_ref as ref
    from ginsim.ins_loose import filter_model
    fs, fs_gps, R = MOTIVATION_FS, MOTIVATION_FS_GPS, MOTIVATION_RUNS
    ini, truth, stamps = ac.outage_truth(fs, 1, fs_gps)
    acc_e, gyr_e = cs.imu_errors()
    rng = np.random.default_rng(MOTIVATION_SEED)
    accel, gyro, _, _ = ref.sample_sensors(rng, fs, truth['ref_accel'], truth['ref_gyro'], acc_e, gyr_e, R)
    gps = cs.sample_gps(rng, truth, 1, R)
    odo = ref.sample_odo(rng, truth['ref_odo'], ac.ODO_ERR, R)
    model = filter_model(fs, acc_e, gyr_e, cs.GPS_ERR)
    j = ac.outage_samples(truth, stamps, fs, fs_gps)[1]
    o = ref.run(1, fs, gyro[:, :j + 1], accel[:, :j + 1], ini, model, gps, [s for s in stamps if s <= j], truth['gps_visibility'],
                odo=odo, aid=ac.aid(mask) if mask else None)
    return o['pos'][:, j] - truth['ref_pos'][j], float(truth['ref_att'][j, 0])
