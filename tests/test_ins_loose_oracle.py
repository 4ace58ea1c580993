"""CPU: the loosely coupled GPS/INS filter's specification (tests/ins_loose_ref.py) and everything about InsLoose that needs no device.

Recorded here (measured by test_restatement_consistency, 1024 runs drawn from the filter's own model, outage profile at 20 Hz with
2 Hz GPS, 'mid-accuracy' IMU, ref_frame 1): RMS end error / sqrt(mean pdiag_end) per state =
    dr 0.988 0.982 0.942   dv 1.022 0.963 0.950   psi 0.941 0.960 1.015   dbg 1.010 1.013 0.996   dba 0.999 0.972 0.980
(ins_loose_cases.CONSISTENCY_RATIOS; the device is held to them within x/: 1.25 by tests/test_gpu_ins_loose.py).  In ref_frame 0 the
same case gives a spread / sigma of 0.93-1.02 for every state but a MEAN of up to 1.2 sigma (psi_N): the 20 Hz mechanisation's own
discretisation error against the truth, common to all runs, which no covariance describes; at 100 Hz the ratios are 0.92-1.06."""
import ctypes
import os
import re

import numpy as np
import pytest

import ins_loose_cases as cs
import ins_loose_ref as ref
from conftest import REPO

NEW = {'ginsim_loose_run', 'ginsim_loose_variant', 'ginsim_loose_kernel_name'}


def test_loose_entry_points_are_declared_exported_and_bound_at_abi_9():
    import ginsim
    hdr = open(os.path.join(REPO, 'include', 'ginsim.h')).read()
    declared = set(re.findall(r'\b(ginsim_[a-z0-9_]+)\s*\(', hdr))
    assert NEW <= declared
    assert re.search(r'\}\s*ginsim_loose_params\s*;', hdr)
    so = ctypes.CDLL(ginsim.LIB_PATH)
    assert all(hasattr(so, f) for f in NEW)
    assert NEW <= set(ginsim.EXPORTS)
    assert set(ginsim.EXPORTS) == declared, set(ginsim.EXPORTS) ^ declared
    assert ginsim.lib.ginsim_abi_version() == 9
    assert hasattr(ginsim, 'InsLooseJob')
    readme = open(os.path.join(REPO, 'README.md')).read()
    assert '%d entry points' % len(declared) in readme


def test_struct_layout_matches_the_header():
    """The ctypes mirror has one field per member of the C struct, in order (a drifted mirror would shift every pointer)."""
    from ginsim import _lib
    hdr = open(os.path.join(REPO, 'include', 'ginsim.h')).read()
    body = re.search(r'typedef struct \{((?:(?!typedef struct).)*?)\}\s*ginsim_loose_params\s*;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            names += [re.sub(r'\[.*', '', x).strip(' *') for x in re.sub(r'^(const\s+)?\w+\s*\*?', '', decl, count=1).split(',')]
    assert names == [f[0] for f in _lib.LooseParams._fields_]


def test_bad_arguments_are_refused_without_a_device():
    from ginsim import _lib as L
    m, p = L.McParams(), L.LooseParams()
    buf = ctypes.create_string_buffer(256)
    ini = np.zeros(10)
    stamps = np.array([0, 10, 20], dtype=np.int64)
    dummy = np.zeros(64)
    m.n, m.runs, m.fs, m.ref_frame, m.n_ini, m.ini = 30, 4, 100.0, 1, 1, ini.ctypes.data
    m.given_sensors, m.in_accel, m.in_gyro = 1, dummy.ctypes.data, dummy.ctypes.data
    p.m, p.gps_stamp, p.in_gps, p.n_list = 3, stamps.ctypes.data, dummy.ctypes.data, 4
    p.r_diag[:], p.p0[:] = [1.0] * 6, [1.0] * 5
    p.decay_g[:], p.decay_a[:] = [1.0] * 3, [1.0] * 3

    def name():
        return L.lib.ginsim_loose_kernel_name(ctypes.byref(m), ctypes.byref(p), buf, 256)
    assert name() == L.OK and buf.value == b'ginsim::loose_kernel<1, true, false, false>'
    for bad in ([0, 10, 30], [-1, 10, 20], [0, 10, 10], [0, 20, 10]):          # outside [0, n), not strictly increasing
        stamps[:] = bad
        assert name() == L.ERR_ARG, bad
    stamps[:] = [0, 10, 29]
    assert name() == L.OK
    m.precision = 1
    assert name() == L.ERR_ARG                                                 # fp32
    m.precision = 0
    p.p0[2] = 0.0
    assert name() == L.ERR_ARG
    p.p0[2] = 1.0
    m.given_sensors = 0
    assert name() == L.ERR_ARG                                                 # generated form without truth
    m.given_sensors = 1
    m.vib_accel.type = 1
    assert name() == L.ERR_ARG                                                 # vibration on given sensors
    m.vib_accel.type = 3
    assert name() == L.ERR_ARG                                                 # 'psd'
    m.vib_accel.type = 0
    v = ctypes.c_int32(-1)
    assert L.lib.ginsim_loose_variant(ctypes.byref(m), ctypes.byref(p), ctypes.byref(v)) == L.OK and v.value == 1


def test_plugin_surface():
    from demo_algorithms.ins_loose_device import InsLoose
    a = InsLoose()
    assert a.input == ['fs', 'gyro', 'accel', 'time', 'gps_time', 'gps']
    assert a.output == ['pos', 'vel', 'att_euler', 'wb', 'ab']
    assert (a.batch, a.mc_algo, a.get_results()) == (True, 'loose', None)
    a.reset()
    with pytest.raises(ValueError, match='logged series'):
        a.run([100.0, np.zeros((10, 3)), np.zeros((10, 3)), np.arange(10) / 100.0, np.zeros(1), np.zeros((1, 6))])
    for bad in ((1, 2, 3), (1, 1, 1, 1, 0.0), (1, 1, 1, 1, -1)):
        with pytest.raises(ValueError):
            InsLoose(p0=bad)
    with pytest.raises(ValueError):
        InsLoose(q_scale=0.0)


def test_sim_refuses_an_insloose_it_cannot_run():
    """No device is needed for the refusals: they are the plan's."""
    from gnss_ins_sim.sim import imu_model, ins_sim
    from demo_algorithms.ins_loose_device import InsLoose

    def roles(gps=True, **kw):
        sim = ins_sim.Sim([100.0, 10.0, 0.0], cs.OUTAGE_CSV, ref_frame=1, imu=imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=gps),
                          algorithm=InsLoose(), **kw)
        return sim, ins_sim._plugin_roles(sim, ['loose'])
    with pytest.raises(ValueError, match='GPS'):
        roles(gps=False)
    with pytest.raises(NotImplementedError, match='fp64'):
        roles(precision='f32')
    with pytest.raises(NotImplementedError, match='psd'):
        roles(env={'acc': np.array([[0.0, 1e-4, 1e-4, 1e-4], [50.0, 1e-4, 1e-4, 1e-4]])})
    sim, r = roles()
    assert tuple(r) == ([], [], []) and r.loose == [0] and r.magcal == []
    sim.sim_count = 8
    plan = lambda in_group, ndev: ins_sim.plan_monte_carlo(sim, sim.amgr.algo, r, np.arange(1000) / 100.0, 100, 0, 2 if in_group else 1,
                                                           in_group, lambda work, dist: (ndev > 1, ndev))
    with pytest.raises(ValueError, match='process group'):
        plan(True, 1)
    with pytest.raises(ValueError, match='several GPUs'):
        plan(False, 2)                                                          # devices=
    p = plan(False, 1)
    assert (p.loose, p.fused, p.incl, p.hosted, p.magcal) == ([0], [], [], [], [])


def _case(rf, n, runs, seed, fs=100.0, fs_gps=10.0, **bias):
    ini, truth, stamps = cs.outage_truth(fs, rf, fs_gps, n)
    acc_e, gyr_e = cs.imu_errors(**bias)
    rng = np.random.default_rng(seed)
    accel, gyro, tba, tbg = ref.sample_sensors(rng, fs, truth['ref_accel'], truth['ref_gyro'], acc_e, gyr_e, runs)
    from ginsim.ins_loose import filter_model
    return ini, truth, stamps, accel, gyro, cs.sample_gps(rng, truth, rf, runs), filter_model(fs, acc_e, gyr_e, cs.GPS_ERR), tba, tbg


@pytest.mark.parametrize('rf', [0, 1])
def test_without_a_usable_fix_the_restatement_is_free_integration(rf):
    from oracle import ins_np
    ini, truth, stamps, accel, gyro, gps, model, _, _ = _case(rf, 700, 7, 11)
    att, pos, vel = ins_np.free_integration(rf, 100.0, gyro, accel, ini)
    for vis, st, g in ((np.zeros(stamps.size), stamps, gps), (None, (), None)):           # every fix invisible; no fix at all
        o = ref.run(rf, 100.0, gyro, accel, ini, model, g, st, vis)
        np.testing.assert_allclose(o['att'], att, rtol=1e-10, atol=0)
        np.testing.assert_allclose(o['pos'], pos, rtol=1e-10, atol=0)
        np.testing.assert_allclose(o['vel'], vel, rtol=1e-10, atol=1e-300)
        assert not o['wb'].any() and not o['ab'].any()


@pytest.mark.parametrize('rf', [0, 1])
def test_covariance_stays_symmetric_with_a_positive_diagonal(rf):
    ini, truth, stamps, accel, gyro, gps, model, _, _ = _case(rf, 2600, 5, 12)            # into the outage
    f = ref.LooseFilter(rf, 100.0, ini, 5, model)
    kf = 0
    for j in range(2599):
        if kf < stamps.size and stamps[kf] == j:
            if truth['gps_visibility'][kf]:
                f.correct(gps[:, kf])
            kf += 1
        f.propagate(gyro[:, j], accel[:, j])
        if j % 97 == 0 or j == 2598:
            d = f.P[:, np.arange(15), np.arange(15)]
            assert np.all(d > 0.0)
            assert np.max(np.abs(f.P - np.swapaxes(f.P, 1, 2)) / np.sqrt(d[:, :, None] * d[:, None, :])) < 1e-12
            assert np.all(np.linalg.eigvalsh(f.P / np.sqrt(d[:, :, None] * d[:, None, :])) > -1e-9)


def test_a_fix_pulls_the_state_towards_it_and_shrinks_p():
    ini, truth, stamps, accel, gyro, gps, model, _, _ = _case(1, 300, 9, 13)
    f = ref.LooseFilter(1, 100.0, ini, 9, model)
    for j in range(200):
        f.propagate(gyro[:, j], accel[:, j])
    before, d0 = f.pos.copy(), f.P[:, np.arange(15), np.arange(15)].copy()
    fix = np.concatenate([f.pos + np.array([3.0, -2.0, 1.0]), f.vel], axis=1)
    f.correct(fix)
    moved = f.pos - before
    assert np.all(moved * np.array([3.0, -2.0, 1.0]) > 0.0) and np.all(np.abs(moved) < np.array([3.0, 2.0, 1.0]))
    assert np.all(f.P[:, np.arange(15), np.arange(15)] <= d0 * (1 + 1e-12))


def test_restatement_consistency():
    """1024 runs drawn from the filter's own model: for every state the RMS end error over sqrt(mean pdiag_end) lies in [0.7, 1.4]
    (a consistent filter has 1) and equals the ratios recorded in ins_loose_cases, which the device is held to."""
    fs, R = cs.CONSISTENCY_FS, cs.CONSISTENCY_RUNS
    ini, truth, stamps, accel, gyro, gps, model, tba, tbg = _case(1, None, R, cs.CONSISTENCY_SEED, fs, cs.CONSISTENCY_FS_GPS)
    o = ref.run(1, fs, gyro, accel, ini, model, gps, stamps, truth['gps_visibility'])
    e = ref.error_state(1, o['att'][:, -1], o['pos'][:, -1], o['vel'][:, -1], o['wb'][:, -1], o['ab'][:, -1], truth['ref_att'][-1],
                        truth['ref_pos'][-1], truth['ref_vel'][-1], tbg[:, -1], tba[:, -1])
    ratio = np.sqrt(np.mean(e * e, axis=0)) / np.sqrt(np.mean(o['pdiag_end'], axis=0))
    print('consistency ratios:', np.array2string(ratio, precision=3))
    assert np.all(ratio >= 0.7) and np.all(ratio <= 1.4), ratio
    np.testing.assert_allclose(ratio, cs.CONSISTENCY_RATIOS, rtol=0, atol=2e-3)


def test_filter_model_follows_the_error_dicts():
    from ginsim.ins_loose import filter_model
    acc_e, gyr_e = cs.imu_errors(gyro_b=[1e-4, -2e-4, 0.0])
    m = filter_model(100.0, acc_e, gyr_e, cs.GPS_ERR, q_scale=2.0)
    dt = 0.01
    np.testing.assert_allclose(m['q_v'], 2.0 * acc_e['vrw'] ** 2 * dt * np.ones(3))
    np.testing.assert_allclose(m['q_bg'], 2.0 * 2.0 * gyr_e['b_drift'] ** 2 / gyr_e['b_corr'] * dt * np.ones(3))
    np.testing.assert_allclose(m['decay_a'], 1.0 - dt / (acc_e['b_corr'] * np.ones(3)))
    np.testing.assert_allclose(m['r_diag'], [25.0, 25.0, 49.0, 0.0025, 0.0025, 0.0025])
    assert m['p0'][3] == 2e-4 and m['p0'][4] == 1e-5
    inf = dict(gyr_e, b_corr=np.array([np.inf, 100.0, 100.0]))
    mi = filter_model(100.0, acc_e, inf, cs.GPS_ERR)
    assert mi['decay_g'][0] == 1.0 and mi['q_bg'][0] == 0.0 and mi['q_psi'][0] > mi['q_psi'][1]


@pytest.mark.parametrize('rf', [0, 1])
def test_restatement_in_long_double_gives_the_parity_bound(rf):
    """The bound of tests/test_gpu_ins_loose.py is 16 x the float64 restatement's deviation from its np.longdouble evaluation, measured
    on each GPU case's own inputs (ins_loose_cases.restatement_error).  Here on the parity cases' shape with sensors drawn on the CPU:
    long double must really propagate (a restatement that fell back to float64 somewhere would measure 0 and the bound would be 0),
    and the measurement stays of the size recorded for the MI355X cases: att 2.6e-13, pos 3.1e-12, vel 5.1e-12, wb 8.4e-10,
    ab 3.8e-10, pdiag_end 1.9e-13 -- within a factor 30 either way (it is a maximum of rounding errors over another draw)."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip('np.longdouble is float64 on this platform')
    ini, truth, stamps, accel, gyro, gps, model, _, _ = _case(rf, 2300, 8, 5)
    o = ref.run(rf, 100.0, gyro, accel, ini, model, gps, stamps, truth['gps_visibility'], dtype=np.longdouble)
    assert all(o[k].dtype == np.longdouble for k in cs.PARITY_KEYS)
    err = cs.restatement_error(rf, 100.0, gyro, accel, ini, model, gps, stamps, truth['gps_visibility'])
    print('float64 against long double, rf%d:' % rf, {k: '%.1e' % v for k, v in err.items()})
    recorded = {'att': 2.6e-13, 'pos': 3.1e-12, 'vel': 5.1e-12, 'wb': 8.4e-10, 'ab': 3.8e-10, 'pdiag_end': 1.9e-13}
    for k, v in err.items():                # (the position of ref_frame 1, ECEF metres, is relatively far below ref_frame 0's record)
        assert 0.0 < v < recorded[k] * 30.0 and (k == 'pos' or v > recorded[k] / 30.0), (k, v)
    assert cs.parity_bound(rf, 100.0, gyro, accel, ini, model, gps, stamps, truth['gps_visibility'])['vel'] == cs.PARITY_MARGIN * err['vel']


def test_build_reports_no_scratch_for_any_instantiation_of_the_kernel():
    """P lives in LDS so that no lane spills: the compiler's resource report (build/ins_loose.resources.txt, written
    by build.py) shows 0 bytes of scratch and no dynamic stack for all 12 instantiations <RF, GIVEN, VIB, PS>, at one wavefront per
    SIMD.  A header or compiler change that brings scratch back fails here, not silently on the GPU."""
    from conftest import PKG
    path = os.path.join(PKG, 'build', 'ins_loose.resources.txt')
    assert os.path.exists(path), 'run gnss-ins-sim_amd/build.py (it writes %s)' % path
    kernels, cur = {}, None
    for line in open(path):
        k, _, v = line.strip().partition(':')
        if k == 'Function Name':
            cur = kernels.setdefault(v.strip(), {})
        elif cur is not None and v.strip():
            cur[k.split('[')[0].strip()] = v.strip()
    loose = {n: r for n, r in kernels.items() if '12loose_kernelI' in n}
    seen = set(re.search(r'loose_kernelILi(\d)ELb(\d)ELb(\d)ELb(\d)E', n).groups() for n in loose)
    want = set((rf, g, v, ps) for rf in '01' for g in '01' for v in '01' for ps in '01' if not (g == '1' and v == '1'))
    assert seen == want, seen ^ want
    for n, r in loose.items():
        assert int(r['ScratchSize']) == 0, '%s: %s bytes of scratch per lane' % (n, r['ScratchSize'])
        assert int(r['Occupancy']) >= 1 and int(r['VGPRs']) <= 256, (n, r)
        assert int(r['LDS Size']) <= 8192 + 4 * 4, (n, r['LDS Size'])         # static LDS: the normal tables; P is dynamic LDS
