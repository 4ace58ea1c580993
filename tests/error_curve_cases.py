"""The golden cases of the error-growth curve (test infrastructure shared by tests/golden/make_golden_error_curve.py and the
tests; no test in it): 16 runs, the demo IMU of make_golden.py, an odometer of scale 0.999 / stdv 0.1.

    turn_rf1       the 90-degree turn, ref_frame 1, odometer + free integration (algo0 = odo, algo1 = free)
    turn_rf0_ned   the 90-degree turn, ref_frame 0, extra_opt='ned', free integration
    wrap_rf1       a turn whose yaw passes 180 degrees at sample 400 (150 deg + 10 deg/s from t = 1 s): truth and estimates
                   sit on both sides of +-pi there, so that array_error's angle_range_pi is live
"""
import numpy as np

RUNS = 16
FS = 100.0
ODO = {'scale': 0.999, 'stdv': 0.1}
DEMO_IMU = {'gyro_b': np.array([0.0, 0.0, 0.0]),
            'gyro_arw': np.array([0.25, 0.25, 0.25]),
            'gyro_b_stability': np.array([3.5, 3.5, 3.5]),
            'gyro_b_corr': np.array([100.0, 100.0, 100.0]),
            'accel_b': np.array([0.0, 0.0, 0.0]),
            'accel_vrw': np.array([0.03119, 0.03009, 0.04779]),
            'accel_b_stability': np.array([4.29e-5, 5.72e-5, 8.02e-5]),
            'accel_b_corr': np.array([200.0, 200.0, 200.0])}
WRAP = """ini lat (deg),ini lon (deg),ini alt (m),ini vx_body (m/s),ini vy_body (m/s),ini vz_body (m/s),ini yaw (deg),ini pitch (deg),ini roll (deg)
31.9965,120.004,0,10,0,0,150,0,0
command type,yaw (deg),pitch (deg),roll (deg),vx_body (m/s),vy_body (m/s),vz_body (m/s),command duration (s),GPS visibility
1,0,0,0,0,0,0,1,0
1,10,0,0,0,0,0,6,0
1,0,0,0,0,0,0,3,0
"""
# case -> (motion: None = the 90-degree turn, ref_frame, extra_opt, plugins in algorithm order)
CASES = {'turn_rf1': (None, 1, '', ('odo', 'free')),
         'turn_rf0_ned': (None, 0, 'ned', ('free',)),
         'wrap_rf1': (WRAP, 1, '', ('free',))}
ALGOS = {k: v[3] for k, v in CASES.items()}


def dropin_sim(g, pkg):
    """The drop-in Sim of a golden case: same motion, IMU, plugins and seed (the counter RNG serves the normals the reference was
    given)."""
    import os
    import sys
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    from gnss_ins_sim.sim import imu_model, ins_sim
    from demo_algorithms import free_integration, free_integration_odo
    motion, rf, _, algos = CASES[str(g['case'])]
    csv = os.path.join(pkg, 'motion_profiles', 'turn_90deg.csv') if motion is None else motion
    imu = imu_model.IMU(accuracy={k: v.copy() for k, v in DEMO_IMU.items()}, axis=6, gps=False, odo=True, odo_opt=dict(ODO))
    objs = [(free_integration_odo if a == 'odo' else free_integration).FreeIntegration(np.array(g['ini'])) for a in algos]
    return ins_sim.Sim([FS, 0.0, 0.0], csv, ref_frame=rf, imu=imu, algorithm=objs, seed=int(g['seed']), keep_trajectories=True)
