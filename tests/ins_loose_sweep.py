"""The table of 130 initial states of the InsLoose GPU tests and every run's own truth and noise on the host (test infrastructure; no
test in it): tests/test_gpu_ins_loose_attitude.py runs loose_kernel and loose_mag_kernel on it, tests/test_gpu_ins_loose_tilted_aids.py
loose_scale_kernel and, with the speed column zero, loose_still_kernel.

    sweep_table()                 -> (10, 130): yaw at 0, +-90, +-179.999 and 180 deg, pitch to +-85 deg, roll over +-180 deg, latitude
                                     -80 to 80 deg, longitude to +-179.9 deg, altitude -100 m to 10 km, 3-15 m/s forward
    make_sweep(rf, table, seg)    -> every run's truth (ginsim.pathgen of the segment `seg` from its row) plus noise drawn with NumPy
    sweep                         -> the module-scoped fixture, per frame: make_sweep of 10 s straight ahead
"""
import numpy as np
import pytest

import ins_loose_cases as cs
import ins_loose_mag_cases as mc
import ins_loose_ref as ref

FS, FS_GPS = 20.0, 2.0
SWEEP_RUNS, SWEEP_N = 130, 200
STRAIGHT = ((1.0, 0, 0, 0, 0, 0, 0, SWEEP_N / FS, 1.0),)              # 10 s straight ahead, GPS visible


def sweep_table():
    """(10, 130): lat, lon, alt, vb3, yaw, pitch, roll, g of every run."""
    from oracle import ins_np
    rng = np.random.default_rng(20260118)
    R = SWEEP_RUNS
    yaw = np.deg2rad(rng.uniform(-180, 180, R))
    yaw[:7] = np.deg2rad([0.0, 90.0, -90.0, 179.999, -179.999, 180.0, 179.999])
    pitch = np.deg2rad(rng.uniform(-85, 85, R))
    pitch[[3, 4, 64, 65, 129]] = np.deg2rad([85.0, -85.0, 85.0, -85.0, 84.0])
    roll = np.deg2rad(rng.uniform(-180, 180, R))
    roll[[5, 6, 63, 66]] = np.deg2rad([180.0, -180.0, 90.0, -90.0])
    lat = np.deg2rad(rng.permutation(np.linspace(-80, 80, R)))
    lon = np.deg2rad(rng.uniform(-179.9, 179.9, R))
    lon[[0, 1]] = np.deg2rad([179.9, -179.9])
    alt = rng.uniform(-100, 10000, R)
    alt[[2, 3]] = [-100.0, 10000.0]
    t = np.zeros((10, R))
    t[0], t[1], t[2], t[3], t[6], t[7], t[8] = lat, lon, alt, rng.uniform(3, 15, R), yaw, pitch, roll
    t[9] = ins_np.geo_param(lat, alt)[2]
    return t


def make_sweep(rf, table, seg=STRAIGHT):
    """Every run's own truth (ginsim.pathgen on the host: the segment `seg` from its row of the table) plus noise drawn with NumPy
    (np.random.default_rng(5); per run accel and gyro, the fixes, the magnetometer): accel, gyro, mag (R, n, 3), gps (R, m, 6), ref_odo
    (R, n) the truth forward speed and ref_vel, ref_gyro (R, n, 3), the first run's truth dict and the stamps all runs share."""
    import ginsim
    from ginsim import workloads
    acc_e, gyr_e = cs.imu_errors()
    rng = np.random.default_rng(5)
    seg = np.array(seg, dtype=np.float64)
    out = {k: [] for k in ('accel', 'gyro', 'gps', 'mag', 'ref_odo', 'ref_vel', 'ref_gyro')}
    for r in range(SWEEP_RUNS):
        raw = ginsim.pathgen(table[:9, r], seg, FS, FS_GPS, workloads.HIGH_MOBILITY, rf, gps=True, geo_mag_n=mc.GEO_SOUTH)
        assert raw['imu'].shape[0] == SWEEP_N
        truth = {'ref_gps': raw['gps'][:, 1:7]}
        a, g, _, _ = ref.sample_sensors(rng, FS, raw['imu'][:, 1:4], raw['imu'][:, 4:7], acc_e, gyr_e, 1)
        out['accel'].append(a[0])
        out['gyro'].append(g[0])
        out['gps'].append(cs.sample_gps(rng, truth, rf, 1)[0])
        out['mag'].append(ref.sample_mag(rng, raw['mag'][:, 1:4], mc.MAG_ERR_SKEW, 1)[0])
        out['ref_odo'].append(raw['odo'][:, 2])
        out['ref_vel'].append(raw['nav'][:, 4:7])
        out['ref_gyro'].append(raw['imu'][:, 4:7])
        if r == 0:
            first = {'ref_accel': raw['imu'][:, 1:4], 'ref_gyro': raw['imu'][:, 4:7], 'ref_pos': raw['nav'][:, 1:4], 'ref_vel': raw['nav'][:, 4:7],
                     'ref_att': raw['nav'][:, 7:10], 'ref_gps': raw['gps'][:, 1:7], 'gps_time': raw['gps'][:, 0] / FS, 'gps_visibility': raw['gps'][:, 7]}
            stamps = np.rint(raw['gps'][:, 0]).astype(np.int64)
    out = {k: np.stack(v) for k, v in out.items()}
    return dict(out, rf=rf, table=table, truth=first, stamps=stamps, acc_e=acc_e, gyr_e=gyr_e, model=ginsim.filter_model(FS, acc_e, gyr_e, cs.GPS_ERR))


@pytest.fixture(scope='module', params=[0, 1], ids=['rf0', 'rf1'])
def sweep(request):
    """Every run's own truth (ginsim.pathgen on the host: 10 s straight ahead from its row of the table) plus noise drawn with NumPy."""
    return make_sweep(request.param, sweep_table())
