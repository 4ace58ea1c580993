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


# ------------------------------------------------------------------- the attitudes, rates and gains the vehicle never has
def sphere_golden():
    return load_golden('incl_sphere')


def quat_diff(a, b):
    """max over components of the difference up to sign, per quaternion; NaN where either side is NaN."""
    with np.errstate(invalid='ignore'):
        return np.minimum(np.max(np.abs(a - b), axis=-1), np.max(np.abs(a + b), axis=-1))


def asin_raises(q):
    """Where attitude.quat2euler raises (math.asin outside [-1, 1]); a NaN argument does not raise."""
    with np.errstate(invalid='ignore'):
        return np.abs(-2.0 * (q[..., 1] * q[..., 3] - q[..., 0] * q[..., 2])) > 1.0


# measured worst difference of the restatement from the golden in the ill-conditioned groups (directions within 1e-6 / 1e-9 rad
# of +-x): quaternions, wb, ab, final bias -- all 0.0: every operation before the first sin / cos is a correctly rounded one
ILL_MEASURED = {'near_x_1e-06': 0.0, 'near_x_1e-09': 0.0}


def test_restatement_reproduces_the_sphere_golden():
    """iref.mahony / tilt / quat2euler against the unmodified reference's objects on the records of inclinometer_records.py:
    quaternions to 1e-12 up to sign, wb / ab / final bias to 1e-14, NaN patterns and the asin mask equal.  The groups
    near_x_1e-06 and near_x_1e-09 are ill-conditioned by construction (1 - ax^2 cancels): their bound is 4 x the measured worst
    difference of THIS pair (reference vs restatement, not the kernel), which is 0.0 for every output in both groups
    (the margins file of _record, entry incl_sphere_restatement_vs_golden) -- they must be bit-identical."""
    import inclinometer_records as rec
    from test_gpu_full_size import _record
    g = sphere_golden()
    worst = {}
    for b in rec.sphere_batches():
        p, R = b['name'] + '_', b['accel'].shape[0]
        k = g[p + 'rows']
        assert np.array_equal(b['accel'][:, 0], g[p + 'accel0']) and np.array_equal(b['gyro'][:, 0], g[p + 'gyro0'])   # the same records
        q, wb, ab, fin = iref.mahony(b['gyro'], b['accel'], 1.0 / b['fs'], np.zeros((R, 3)), b['gains'])
        tq = iref.tilt(b['accel'])
        got = {'mahony_quat': q[:, k], 'tilt_quat': tq[:, k], 'wb': wb[:, k], 'ab': ab[:, k], 'bias_after': fin}
        for nm, x in got.items():
            assert np.array_equal(np.isnan(x), np.isnan(g[p + nm])), (b['name'], nm)
        for gn, ids in b['groups'].items():
            assert np.array_equal(ids, g[p + 'group_' + gn])
            for nm, x in got.items():
                d = quat_diff(x[ids], g[p + nm][ids]) if nm.endswith('quat') else np.abs(x[ids] - g[p + nm][ids])
                d = float(np.nanmax(d)) if np.isfinite(d).any() else 0.0
                worst[gn + '_' + nm] = d
                tol = 4.0 * ILL_MEASURED[gn] if gn in rec.ILL_GROUPS else (1e-12 if nm.endswith('quat') else 1e-14)
                assert d <= tol, (gn, nm, d)
        for a in ('mahony', 'tilt'):
            gq = g[p + a + '_quat']
            assert np.array_equal(asin_raises(gq), g[p + a + '_asin_raises'])
            assert np.array_equal(asin_raises(got[a + '_quat']), g[p + a + '_asin_raises'])
            e = np.where(asin_raises(gq)[..., None], np.nan, iref.quat2euler(gq))      # the Euler function on the golden's own quaternions
            assert np.array_equal(np.isnan(e), np.isnan(g[p + a + '_euler']))
            d = np.abs(e - g[p + a + '_euler'])
            assert not np.isfinite(d).any() or np.nanmax(d) < 1e-13
    print(worst)
    _record('incl_sphere_restatement_vs_golden', **worst)


def test_sphere_groups_reach_what_they_are_named_for():
    """Census from the inputs with the restatement alone."""
    import inclinometer_records as rec
    B = {b['name']: b for b in rec.sphere_batches()}
    tr = {}
    for name, b in B.items():
        tr[name] = {}
        iref.mahony(b['gyro'], b['accel'], 1.0 / b['fs'], np.zeros((b['accel'].shape[0], 3)), b['gains'], trace=tr[name])
        tr[name]['tilt_branch'] = iref.tilt(b['accel'], True)[1]
    s, ids = tr['sphere'], B['sphere']['groups']['sphere']
    for br in (0, 3):       # both reachable dcm2quat branches through both callers, >= 30 records each
        assert np.sum(s['ini_branch'][ids] == br) >= 30 and np.sum(s['tilt_branch'][ids, 0] == br) >= 30
    # the two middle branches are not reachable through the callers (see iref.acc_mag_quat): never taken by any finite record
    for name in B:
        assert not np.isin(tr[name]['ini_branch'], (1, 2)).any()
    fin = ~np.isnan(iref.tilt(B['sphere']['accel'])).any(axis=(1, 2))
    assert not np.isin(s['tilt_branch'][fin], (1, 2)).any()
    for d in ('0.001', '1e-06', '1e-09'):           # both sides of tr == 0, both callers
        i = B['sphere']['groups']['tr0_' + d]
        assert set(s['ini_branch'][i]) == {0, 3} and set(s['tilt_branch'][i, 0]) == {0, 3}
        assert len(B['sphere']['groups']['near_x_' + d]) == 8
    f = tr['flip']
    i = B['flip']['groups']['cneg']
    assert f['cneg'][i].sum() > 0 and (~f['cneg'][i]).sum() > 0 and np.all(f['cneg'][i].any(axis=1)[1:])
    assert f['theta0'][B['flip']['groups']['theta0']].all() and not f['theta0'][i].any()
    z, zg = tr['zero_acc'], B['zero_acc']['groups']
    assert np.all(z['postponed'][zg['zero_1']].sum(axis=1) == 1) and np.all(z['postponed'][zg['zero_2']].sum(axis=1) == 2)
    assert z['postponed'][zg['zero_all']].all() and np.all(z['ini_branch'][zg['zero_all']] == -1)
    w = tr['gains']
    assert w['limited'].sum() > 0 and (~w['limited']).sum() > 0 and w['low'].sum() > 0 and (~w['low']).sum() > 0
    assert np.all(w['limited'].any(axis=1) & (~w['limited']).any(axis=1) & w['low'].any(axis=1) & (~w['low']).any(axis=1))
    assert s['low'].sum() > 0 and (~s['low']).sum() > 0          # the default gains switch too
    assert B['gains']['fs'] != 100.0 and B['gains']['gains'] is not None


def test_angle_err_wraps_as_the_reference_does():
    """iref.angle_err is attitude.angle_range_pi of the difference: bit for bit on the golden's values (+pi for -pi, +pi, +-3 pi)."""
    g = sphere_golden()
    x, y = g['wrap_x'], g['wrap_y']
    assert np.array_equal(y[:4], [np.pi] * 4)
    assert np.array_equal(iref.angle_range_pi(x), y)
    assert np.array_equal(iref.angle_err(x, np.zeros_like(x)), y)
    assert np.array_equal(iref.angle_err(np.zeros_like(x), -x), y)
    e = np.zeros((x.size, 2, 3))
    e[:, :, 0] = x[:, None]
    end, proc = iref.stats(e, np.zeros((2, 3)))
    assert np.array_equal(end[:, 0], y) and np.array_equal(proc[:, 1, 0], y) and np.array_equal(proc[:, 0, 0], np.abs(y))


# ------------------------------------------------------------------- the C ABI's refusals
def _valid_incl_block():
    import ginsim
    import ginsim._lib as L
    from ginsim import workloads
    acc, gyr = workloads.imu_grade('mid-accuracy')
    m, p = L.McParams(), L.InclParams()
    m.n, m.runs, m.fs = 100, 8, 100.0
    m.ref_accel = m.ref_gyro = 8                 # any non-NULL: the query dereferences nothing
    m.accel, m.gyro = ginsim.sensor_model(acc, 'vrw', 100.0), ginsim.sensor_model(gyr, 'arw', 100.0)
    p.algo_mask, p.dt, p.bias_in, p.n_list = 3, 0.01, 8, 8
    return m, p


def _set(path, value):
    def f(m, p):
        obj = {'m': m, 'p': p}[path[0]]
        for a in path[1:-1]:
            obj = getattr(obj, a)
        if isinstance(path[-1], int):
            obj[path[-1]] = value
        else:
            setattr(obj, path[-1], value)
    return f


def _both(*fs):
    def f(m, p):
        for g in fs:
            g(m, p)
    return f


_REFUSALS = [
    ('n_0', _set(('m', 'n'), 0), 'n=0'),
    ('runs_0', _set(('m', 'runs'), 0), 'runs=0'),
    ('n_past_32_bits', _set(('m', 'n'), 2 ** 32), '32-bit sample counter'),
    ('too_many_runs', _both(_set(('m', 'runs'), 0x7FFFFFFF * 64 + 1), _set(('p', 'n_list'), 1)), 'too many runs'),
    ('algo_mask_0', _set(('p', 'algo_mask'), 0), 'algo_mask'),
    ('algo_mask_4', _set(('p', 'algo_mask'), 4), 'algo_mask'),
    ('n_list_past_runs', _set(('p', 'n_list'), 9), 'n_list'),
    ('n_list_negative', _set(('p', 'n_list'), -1), 'n_list'),
    ('mahony_without_bias_in', _set(('p', 'bias_in'), None), 'bias_in'),
    ('dt_0', _set(('p', 'dt'), 0.0), 'dt must be positive'),
    ('dt_nan', _set(('p', 'dt'), float('nan')), 'dt must be positive'),
    ('dt_inf', _set(('p', 'dt'), float('inf')), 'dt must be positive'),
    ('block_threads_32', _set(('m', 'block_threads'), 32), 'block_threads'),
    ('block_threads_512', _set(('m', 'block_threads'), 512), 'block_threads'),
    ('precision_1', _set(('m', 'precision'), 1), 'fp64 only'),
    ('given_without_pointer', _both(_set(('m', 'given_sensors'), 1), _set(('m', 'in_accel'), 8)), 'in_accel and in_gyro'),
    ('no_truth', _set(('m', 'ref_gyro'), None), 'ref_accel/ref_gyro missing'),
    ('non_finite_model', _set(('m', 'gyro', 'white', 1), float('inf')), 'gyro model has a non-finite coefficient'),
    ('psd_vibration', _set(('m', 'vib_accel', 'type'), 3), "'random' and 'sinusoidal' vibration only"),
    ('vibration_on_given', _both(_set(('m', 'given_sensors'), 1), _set(('m', 'in_accel'), 8), _set(('m', 'in_gyro'), 8),
                                 _set(('m', 'vib_gyro', 'type'), 1)), 'cannot be added to given sensors'),
    ('non_finite_amplitude', _both(_set(('m', 'vib_accel', 'type'), 2), _set(('m', 'vib_accel', 'amp', 2), float('nan'))), 'must be finite'),
    ('non_finite_frequency', _both(_set(('m', 'vib_gyro', 'type'), 2), _set(('m', 'vib_gyro', 'omega_dt'), float('inf'))), 'must be finite'),
    ('statistics_without_ref_nav', _set(('p', 'out_end', 1), 8), 'statistics need ref_nav'),
    ('negative_proc_first', _both(_set(('p', 'out_proc', 0), 8), _set(('m', 'ref_nav'), 8), _set(('m', 'proc_first'), -1)), 'proc_first must be >= 0'),
    ('mahony_output_without_its_bit', _both(_set(('p', 'algo_mask'), 2), _set(('p', 'out_wb'), 8)), 'Mahony outputs without the Mahony bit'),
    ('tilt_output_without_its_bit', _both(_set(('p', 'algo_mask'), 1), _set(('p', 'out_quat', 1), 8)), 'tilt outputs without the tilt bit'),
]


@pytest.mark.parametrize('case', _REFUSALS, ids=[c[0] for c in _REFUSALS])
def test_incl_parameter_refusals_without_a_gpu(case):
    """Each REQUIRE of check_incl_params from an otherwise valid block: GINSIM_ERR_ARG and its message."""
    import ctypes
    import ginsim._lib as L
    m, p = _valid_incl_block()
    buf = ctypes.create_string_buffer(256)
    assert L.lib.ginsim_incl_kernel_name(ctypes.byref(m), ctypes.byref(p), buf, 256) == L.OK     # the block is valid as it is
    assert buf.value.decode() == 'ginsim::incl_kernel<3, false, false>'
    case[1](m, p)
    assert L.lib.ginsim_incl_kernel_name(ctypes.byref(m), ctypes.byref(p), buf, 256) == L.ERR_ARG
    assert case[2] in L.lib.ginsim_last_error().decode()
    v = ctypes.c_int32(0)
    assert L.lib.ginsim_incl_variant(ctypes.byref(m), ctypes.byref(p), ctypes.byref(v)) == L.ERR_ARG
