"""CPU: the NumPy restatement of MahonyFilter / TiltAcc (tests/inclinometer_ref.py) against the goldens of the unmodified
reference (tests/golden/make_golden_inclinometer.py), the chain of a MahonyFilter's runs included; the new C-ABI symbols."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, REPO
import inclinometer_ref as iref


def load_golden(name):
    import os
    return dict(np.load(os.path.join(GOLDEN, 'inclinometer', name + '.npz'), allow_pickle=False))

CASES = ['incl_mahony_tilt_rf1', 'incl_mag9_gps_rf0', 'incl_chain_rf1']


def golden_inputs(g):
    """Truth and the engine's sensors of the golden's runs (the goldens were made with the same Philox normals)."""
    import ginsim
    from ginsim import workloads
    from gnss_ins_sim.sim import imu_model
    ini, seg = workloads.parse_motion(str(g['profile']))
    fs = float(g['fs'])
    raw = ginsim.pathgen(ini, seg, fs, float(g['fs_gps']), (1.0, 0.5, 2.0), int(g['ref_frame']), gps=float(g['fs_gps']) > 0,
                         geo_mag_n=g['geo_mag_n'] if 'geo_mag_n' in g else None)
    imu = imu_model.IMU(accuracy='mid-accuracy' if int(g['axis']) == 6 else 'low-accuracy', axis=int(g['axis']),
                        gps=float(g['fs_gps']) > 0)
    from oracle import ins_np
    accel, gyro = ins_np.mc_sensors(int(g['seed']), np.arange(int(g['R'])), fs, np.ascontiguousarray(raw['imu'][:, 1:4]),
                                    np.ascontiguousarray(raw['imu'][:, 4:7]), imu.accel_err, imu.gyro_err)
    return raw, accel, gyro


def quat_close(a, b, tol):
    """att_quat up to sign (quat_normalize flips it near q0 = 0)."""
    d = np.minimum(np.max(np.abs(a - b), axis=-1), np.max(np.abs(a + b), axis=-1))
    assert np.max(d) < tol, np.max(d)


@pytest.mark.parametrize('name', CASES)
def test_restatement_reproduces_reference(name):
    g = load_golden(name)
    raw, accel, gyro = golden_inputs(g)
    fs, R = float(g['fs']), int(g['R'])
    k = g['c0_rows']
    assert np.allclose(accel[:, k], g['c0_accel'], rtol=0, atol=1e-12) and np.allclose(gyro[:, k], g['c0_gyro'], rtol=0, atol=1e-12)
    bias = np.zeros(3)
    for call in range(int(g['calls'])):
        p = 'c%d_' % call
        assert np.max(np.abs(g[p + 'bias_before'] - bias)) < 1e-12      # the chain goes on across Sim.run calls
        bias = g[p + 'bias_before']
        q, wb, ab, starts, last = iref.chain(gyro, accel, 1.0 / fs, bias)
        assert np.max(np.abs(wb[:, k] - g[p + 'wb'])) < 1e-10
        assert np.max(np.abs(ab[:, k] - g[p + 'ab'])) < 1e-10
        quat_close(q[:, k], g[p + 'algo0_att_quat'], 1e-10)
        e = iref.quat2euler(q)
        d = np.mod(e[:, k] - g[p + 'algo0_att_euler'] + np.pi, 2 * np.pi) - np.pi
        assert np.max(np.abs(d)) < 1e-10
        assert np.max(np.abs(last - g[p + 'bias_after'])) < 1e-12
        # the chain is real: a run started from zero ends elsewhere
        if R > 1:
            assert not np.array_equal(starts[1], np.zeros(3))
        if 'StaticTilt_att_quat' in [kk[len(p):] for kk in g if kk.startswith(p)]:
            tq = iref.tilt(accel)
            quat_close(tq[:, k], g[p + 'StaticTilt_att_quat'], 1e-12)
        # process statistics from t = 2 s, internal units
        ref_att = raw['nav'][:, 7:10]
        _, proc = iref.stats(e, ref_att, int(np.where(raw['nav'][:, 0] / fs >= 2.0)[0][0]))
        for row, s in enumerate(('max', 'avg', 'std')):
            assert np.allclose(proc[:, row], g[p + 'proc_' + s][:R], rtol=1e-8, atol=1e-10)
        bias = last


def test_restatement_rare_branches():
    """acc along +x / -y takes the pseudo-magnetometer branches; zero rate with level gravity gives theta == 0."""
    n = 5
    acc = np.zeros((3, n, 3))
    acc[0, :, 2] = -9.8                      # level: zero rate -> theta == 0 (bias stays zero: no innovation)
    acc[1, :, 0] = 9.8                       # +x
    acc[2, :, 1] = -9.8                      # -y
    q, wb, ab, b = iref.mahony(np.zeros((3, n, 3)), acc, 0.01, np.zeros((3, 3)))
    assert np.all(np.isfinite(q))
    assert np.array_equal(q[0, -1], [1.0, 0.0, 0.0, 0.0]) and np.array_equal(wb[0], np.zeros((n, 3)))


def test_new_symbols_declared_exported_bound():
    import ctypes
    import ginsim
    hdr = open(os.path.join(REPO, 'include', 'ginsim.h')).read()
    new = {'ginsim_incl_run', 'ginsim_incl_variant', 'ginsim_incl_kernel_name'}
    declared = set(re.findall(r'\b(ginsim_[a-z0-9_]+)\s*\(', hdr))
    assert new <= declared
    raw = ctypes.CDLL(ginsim.LIB_PATH)
    assert all(hasattr(raw, s) for s in new)
    assert new <= set(ginsim.EXPORTS)
    assert ginsim.lib.ginsim_abi_version() == 9


def test_kernel_name_and_variant_without_a_gpu():
    import ginsim
    from ginsim import workloads
    ini, truth, _ = workloads.truth_from_profile('turn_90deg', 100.0, 1)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    from ginsim.inclinometer import InclinometerJob
    job = InclinometerJob.__new__(InclinometerJob)       # the name query allocates nothing: a job shell without a context
    job.runs = 8
    import ginsim._lib as L
    job.mc = L.McParams()
    job.mc.n, job.mc.runs, job.mc.fs = truth['ref_accel'].shape[0], 8, 100.0
    job.mc.ref_accel = job.mc.ref_gyro = 8       # any non-NULL: not dereferenced by the query
    job.mc.accel = ginsim.sensor_model(acc, 'vrw', 100.0)
    job.mc.gyro = ginsim.sensor_model(gyr, 'arw', 100.0)
    job.params = L.InclParams()
    job.params.algo_mask, job.params.dt, job.params.bias_in = 3, 0.01, 8
    assert job.kernel_name() == 'ginsim::incl_kernel<3, false, false>'
    assert job.variant() == 0
    job.params.algo_mask = 0
    with pytest.raises(ValueError, match='algo_mask'):
        job.kernel_name()
