"""CPU: InsLoose's magnetometer aiding: the C ABI's new block, entry points and refusals, the build's resource report of
loose_mag_kernel, the restatement (tests/ins_loose_ref.py) against the first-order model, against the statistics of its own
covariance and the benefit it measures for the heading and through the GPS outage, mag_model, the plugin's surface and the Sim's
refusal.

Recorded in ins_loose_mag_cases (measured by test_restatement_consistency_and_benefit; 1024 runs drawn from the filter's own model,
outage profile at 20 Hz with 2 Hz GPS, 'mid-accuracy' IMU, magnetometer noise 0.01 uT, field (30, -3, 40) uT, a block at every
sample, ref_frame 1): CONSISTENCY_RATIOS for the magnetometer alone and with mask 7, and YAW_TABLE / HORIZONTAL_TABLE, the yaw and the
horizontal position 1 sigma at the outage's start / its end / 5 s later / the profile's end."""
import ctypes
import os
import re

import numpy as np
import pytest

import ins_loose_aided_cases as ac
import ins_loose_cases as cs
import ins_loose_mag_cases as mc
import ins_loose_ref as ref
from conftest import REPO

NEW = {'ginsim_loose_mag_run', 'ginsim_loose_mag_kernel_name'}
FIELDS = [('mag_every', ctypes.c_int64), ('ref_mag', ctypes.c_void_p), ('mag_si', ctypes.c_double * 9), ('mag_hi', ctypes.c_double * 3),
          ('mag_std', ctypes.c_double * 3), ('in_mag', ctypes.c_void_p), ('mag_n', ctypes.c_double * 3), ('cal_si', ctypes.c_double * 9),
          ('cal_hi', ctypes.c_double * 3), ('r_mag', ctypes.c_double * 3)]


# ------------------------------------------------------------------------------------------------- C ABI
def test_the_magnetometer_block_is_declared_exported_bound_and_mirrored():
    import ginsim
    from ginsim import _lib
    hdr = open(os.path.join(REPO, 'include', 'ginsim.h')).read()
    declared = set(re.findall(r'\b(ginsim_[a-z0-9_]+)\s*\(', hdr))
    so = ctypes.CDLL(ginsim.LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(so, name) and name in ginsim.EXPORTS
    assert ginsim.lib.ginsim_abi_version() == 9
    body = re.search(r'typedef struct \{((?:(?!typedef struct).)*?)\}\s*ginsim_loose_mag_params\s*;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    members = []                                                                # (name, C type, array length or None)
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        ctype = re.match(r'^(?:const\s+)?(\w+)\s*(\*?)', decl)
        rest = re.sub(r'^(?:const\s+)?\w+\s*\*?', '', decl, count=1)
        for x in rest.split(','):
            dim = re.search(r'\[(\d+)\]', x)
            members.append((re.sub(r'\[.*', '', x).strip(' *'), ctype.group(1) + ctype.group(2), int(dim.group(1)) if dim else None))
    assert [m[0] for m in members] == [f[0] for f in _lib.LooseMagParams._fields_] == [f[0] for f in FIELDS]
    for (name, ctype, dim), (_, want) in zip(members, _lib.LooseMagParams._fields_):
        if ctype == 'int64_t':
            assert want is ctypes.c_int64 and dim is None, name
        elif ctype == 'double*':
            assert want is ctypes.c_void_p, name
        else:
            assert ctype == 'double' and want._type_ is ctypes.c_double and want._length_ == dim, name
    assert [(n, t) for n, t in _lib.LooseMagParams._fields_ if not hasattr(t, '_length_')] == [f for f in FIELDS if not hasattr(f[1], '_length_')]
    assert hasattr(ginsim, 'mag_model')


def blocks():
    """(m, p, g, keep-alive arrays): a given-form launch of 4 runs x 30 samples that every check passes."""
    from ginsim import _lib as L
    m, p, g = L.McParams(), L.LooseParams(), L.LooseMagParams()
    ini, dummy = np.zeros(10), np.zeros(64)
    stamps = np.array([0, 10, 20], dtype=np.int64)
    m.n, m.runs, m.fs, m.ref_frame, m.n_ini, m.ini = 30, 4, 100.0, 1, 1, ini.ctypes.data
    m.given_sensors, m.in_accel, m.in_gyro, m.in_odo = 1, dummy.ctypes.data, dummy.ctypes.data, dummy.ctypes.data
    p.m, p.gps_stamp, p.in_gps, p.n_list = 3, stamps.ctypes.data, dummy.ctypes.data, 4
    p.r_diag[:], p.p0[:] = [1.0] * 6, [1.0] * 5
    p.decay_g[:], p.decay_a[:] = [1.0] * 3, [1.0] * 3
    return m, p, g, (ini, dummy, stamps)


def test_magnetometer_arguments_are_refused_without_a_device():
    from ginsim import _lib as L
    m, p, g, (ini, dummy, stamps) = blocks()
    buf = ctypes.create_string_buffer(256)

    def name():
        return L.lib.ginsim_loose_mag_kernel_name(ctypes.byref(m), ctypes.byref(p), ctypes.byref(g), buf, 256)

    def refused(wording='loose_mag_run: '):
        rc = name()
        return rc == L.ERR_ARG and L.lib.ginsim_last_error().decode().startswith(wording)

    # mag_every = 0 is the launch ginsim_loose_run makes, whatever the rest of the block says
    assert name() == L.OK and buf.value == b'ginsim::loose_kernel<1, true, false, false>'
    g.r_mag[:], g.mag_n[:], g.cal_si[0] = [-1.0, float('nan'), 0.0], [0.0] * 3, float('inf')
    assert name() == L.OK and buf.value == b'ginsim::loose_kernel<1, true, false, false>'
    p.aid_mask, p.aid_every, p.odo_scale_f, p.r_odo, p.r_nhc = 7, 1, 0.99, 0.01, 0.0025
    assert name() == L.OK and buf.value == b'ginsim::loose_aided_kernel<1, true, false, false>'
    p.aid_mask = 0
    assert L.lib.ginsim_loose_mag_kernel_name(ctypes.byref(m), ctypes.byref(p), None, buf, 256) == L.ERR_ARG
    g.mag_every = -1
    assert refused()
    # a good block, given form
    g.mag_every, g.in_mag = 1, dummy.ctypes.data
    g.mag_n[:], g.cal_hi[:], g.r_mag[:] = [30.0, 0.0, 40.0], [0.0] * 3, [1e-4] * 3
    g.cal_si[:] = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
    assert name() == L.OK and buf.value == b'ginsim::loose_mag_kernel<1, true, false, false>'
    g.mag_every = 2 ** 40                                                      # never fires: legal
    assert name() == L.OK
    g.mag_every = 1
    g.in_mag = None
    assert refused()
    g.in_mag = dummy.ctypes.data
    # the generation numbers are not read in the given form
    g.mag_si[0], g.mag_hi[1], g.mag_std[2] = float('nan'), float('inf'), float('nan')
    assert name() == L.OK
    for field in ('mag_n', 'cal_si', 'cal_hi'):
        for bad in (float('nan'), float('inf'), -float('inf')):
            good = getattr(g, field)[1]
            getattr(g, field)[1] = bad
            assert refused(), (field, bad)
            getattr(g, field)[1] = good
    for k in range(3):
        for bad in (0.0, -1.0, float('nan'), float('inf')):
            g.r_mag[k] = bad
            assert refused(), (k, bad)
            g.r_mag[k] = 1e-4
    g.mag_n[:] = [0.0, 0.0, 0.0]
    assert refused()
    g.mag_n[:] = [0.0, 0.0, -40.0]
    assert name() == L.OK
    # what ginsim_loose_run refuses stays refused, in its own wording
    p.aid_mask = 8
    assert refused('loose_run: aid_mask=8 must lie in 0 .. 7')
    p.aid_mask = 0
    m.precision = 1
    assert refused('loose_run: ')
    m.precision = 0
    # generated form: ref_mag and finite generation numbers
    m.given_sensors = 0
    m.ref_accel, m.ref_gyro, p.ref_gps = dummy.ctypes.data, dummy.ctypes.data, dummy.ctypes.data
    assert refused()                                                           # no ref_mag
    g.ref_mag = dummy.ctypes.data
    assert refused()                                                           # the non-finite generation numbers
    g.mag_si[0], g.mag_hi[1], g.mag_std[2] = 1.0, 0.0, 0.01
    m.ref_frame, m.vib_accel.type = 0, 1
    assert name() == L.OK and buf.value == b'ginsim::loose_mag_kernel<0, false, true, false>'
    for field in ('mag_si', 'mag_hi', 'mag_std'):
        getattr(g, field)[2] = float('nan')
        assert refused(), field
        getattr(g, field)[2] = 0.0
    m.vib_accel.type = 0
    m.ref_nav, p.out_proc = dummy.ctypes.data, dummy.ctypes.data
    assert name() == L.OK and buf.value == b'ginsim::loose_mag_kernel<0, false, false, true>'
    # with the odometer / non-holonomic block next to it: the same kernel
    p.aid_mask, m.ref_odo = 7, dummy.ctypes.data
    assert name() == L.OK and buf.value == b'ginsim::loose_mag_kernel<0, false, false, true>'
    # the run entry point makes the same checks before it touches a device
    g.mag_every = -1
    assert L.lib.ginsim_loose_mag_run(None, ctypes.byref(m), ctypes.byref(p), ctypes.byref(g)) == L.ERR_ARG


def test_build_reports_no_scratch_for_any_instantiation_of_the_magnetometer_kernel():
    """build/ins_loose_mag.resources.txt (written by build.py): the 12 instantiations <RF, GIVEN, VIB, PS> of loose_mag_kernel, each
    with 0 bytes of scratch, at most 256 VGPRs and the static LDS bound the sibling kernels are held to (nothing new in LDS)."""
    from conftest import PKG
    path = os.path.join(PKG, 'build', 'ins_loose_mag.resources.txt')
    assert os.path.exists(path), 'run gnss-ins-sim_amd/build.py (it writes %s)' % path
    kernels, cur = {}, None
    for line in open(path):
        k, _, v = line.strip().partition(':')
        if k == 'Function Name':
            cur = kernels.setdefault(v.strip(), {})
        elif cur is not None and v.strip():
            cur[k.split('[')[0].strip()] = v.strip()
    mag = {n: r for n, r in kernels.items() if '16loose_mag_kernelI' in n}
    seen = set(re.search(r'loose_mag_kernelILi(\d)ELb(\d)ELb(\d)ELb(\d)E', n).groups() for n in mag)
    want = set((rf, g, v, ps) for rf in '01' for g in '01' for v in '01' for ps in '01' if not (g == '1' and v == '1'))
    assert seen == want and len(mag) == 12, seen ^ want
    for n, r in mag.items():
        print(n, {k: r[k] for k in ('VGPRs', 'AGPRs', 'ScratchSize', 'Occupancy', 'LDS Size') if k in r})
        assert int(r['ScratchSize']) == 0, '%s: %s bytes of scratch per lane' % (n, r['ScratchSize'])
        assert int(r['Occupancy']) >= 1 and int(r['VGPRs']) <= 256, (n, r)
        assert int(r['LDS Size']) <= 8192 + 4 * 4, (n, r['LDS Size'])


# ------------------------------------------------------------------------------------------------- the restatement
def test_rows_follow_the_first_order_model():
    """h_i is the derivative of D_est m_n with respect to psi: a filter whose attitude is perturbed by a small psi sees the field in
    the body frame change by h . psi, to 1e-8 of |m_n|."""
    att = np.array([[0.7, -0.3, 0.4]])                                          # yaw, pitch, roll: a general attitude
    Dr = ref.dcm_zyx(att)
    D = Dr[0]
    assert np.min(np.abs(D)) > 0.01                                             # no axis of the body lies along an axis of the frame
    m_n = np.array([31.0, -4.0, 39.0])
    psi = np.array([1e-5, 2e-5, -3e-5])
    skew = lambda a: np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0.0]])
    C_est = (np.eye(3) - skew(psi)) @ D.T
    H = ref.mag_rows(Dr, m_n)[0]
    np.testing.assert_allclose(H, -D @ skew(m_n), rtol=0, atol=1e-12)
    np.testing.assert_allclose(C_est.T @ m_n - D @ m_n, H @ psi, rtol=0, atol=1e-8 * np.linalg.norm(m_n))
    assert np.linalg.norm(H @ psi) > 1e-4                                       # and the change is far above that


@pytest.mark.parametrize('mask', [0, 7])
def test_a_block_that_never_fires_is_the_aided_restatement_and_a_block_shrinks_p(mask):
    fs, n, R = 100.0, 400, 5
    ini, truth, stamps = mc.outage_truth(fs, 1, 10.0, n)
    acc_e, gyr_e = cs.imu_errors()
    rng = np.random.default_rng(3)
    accel, gyro, _, _ = ref.sample_sensors(rng, fs, truth['ref_accel'], truth['ref_gyro'], acc_e, gyr_e, R)
    gps = cs.sample_gps(rng, truth, 1, R)
    odo = ref.sample_odo(rng, truth['ref_odo'], ac.ODO_ERR, R)
    mag = ref.sample_mag(rng, truth['ref_mag'], mc.MAG_ERR_SKEW, R)
    from ginsim.ins_loose import filter_model
    model = filter_model(fs, acc_e, gyr_e, cs.GPS_ERR)
    args = (1, fs, gyro, accel, ini, model, gps, stamps, truth['gps_visibility'])
    aid = ac.aid(mask) if mask else None
    a = ref.run(*args, odo=odo, aid=aid)
    for every in (n, n + 1, 2 ** 40):
        never = ref.run(*args, odo=odo, aid=aid, mag=mag, mag_model=mc.model(mc.MAG_ERR_SKEW, 1, every))
        for k in cs.PARITY_KEYS + ('P_end',):
            assert np.array_equal(a[k], never[k]), (k, every)
    none = ref.run(*args, odo=odo, aid=aid)                                     # and so is no block at all
    for k in cs.PARITY_KEYS:
        assert np.array_equal(a[k], none[k]), k
    c = ref.run(*args, odo=odo, aid=aid, mag=mag, mag_model=mc.model(mc.MAG_ERR_SKEW, 1))
    assert not np.array_equal(a['att'], c['att'])
    assert np.all(c['pdiag_end'][:, 6:9] < a['pdiag_end'][:, 6:9])              # psi is what the rows see
    d = c['P_end']
    dd = np.sqrt(c['pdiag_end'])
    assert np.max(np.abs(d - np.swapaxes(d, 1, 2)) / (dd[:, :, None] * dd[:, None, :])) < 1e-12
    assert np.all(np.linalg.eigvalsh(d / (dd[:, :, None] * dd[:, None, :])) > -1e-9)
    # the wrong calibration shows: a filter that forgets the hard iron is dragged off by it
    wrong = ref.run(*args, odo=odo, aid=aid, mag=mag, mag_model=mc.model(mc.MAG_ERR_SKEW, 1, hi=np.zeros(3)))
    yaw = lambda o: np.abs(np.mod(o['att'][:, -1, 0] - truth['ref_att'][-1, 0] + np.pi, 2 * np.pi) - np.pi)
    assert np.all(yaw(wrong) > 10.0 * yaw(c) + 1e-3)


def yaw_sigma(att, truth_att):
    return float(np.std(np.mod(att[:, 0] - truth_att[0] + np.pi, 2 * np.pi) - np.pi))


@pytest.fixture(scope='module')
def consistency():
    """The 1024-run case once: accel, gyro, GPS and the odometer as tests/test_ins_loose_aided_oracle.py draws them (so 'gps' IS the
    unaided filter of that file), then the magnetometer; the restatement for GPS only, the magnetometer alone and with mask 7."""
    from ginsim.ins_loose import filter_model
    fs, fs_gps, R = cs.CONSISTENCY_FS, cs.CONSISTENCY_FS_GPS, cs.CONSISTENCY_RUNS
    ini, truth, stamps = mc.outage_truth(fs, 1, fs_gps)
    acc_e, gyr_e = cs.imu_errors()
    rng = np.random.default_rng(cs.CONSISTENCY_SEED)
    accel, gyro, tba, tbg = ref.sample_sensors(rng, fs, truth['ref_accel'], truth['ref_gyro'], acc_e, gyr_e, R)
    gps = cs.sample_gps(rng, truth, 1, R)
    odo = ref.sample_odo(rng, truth['ref_odo'], ac.ODO_ERR, R)
    mag = ref.sample_mag(rng, truth['ref_mag'], mc.MAG_ERR, R)
    model = filter_model(fs, acc_e, gyr_e, cs.GPS_ERR)
    samples = ac.outage_samples(truth, stamps, fs, fs_gps)
    out = {}
    for key, mask, use_mag in (('gps', 0, False), ('mag', 0, True), ('mag7', 7, True)):
        o = ref.run(1, fs, gyro, accel, ini, model, gps, stamps, truth['gps_visibility'], odo=odo, aid=ac.aid(mask) if mask else None,
                     mag=mag, mag_model=mc.model(mc.MAG_ERR, 1) if use_mag else None)
        e = ref.error_state(1, o['att'][:, -1], o['pos'][:, -1], o['vel'][:, -1], o['wb'][:, -1], o['ab'][:, -1], truth['ref_att'][-1],
                            truth['ref_pos'][-1], truth['ref_vel'][-1], tbg[:, -1], tba[:, -1])
        ratio = np.sqrt(np.mean(e * e, axis=0)) / np.sqrt(np.mean(o['pdiag_end'], axis=0))
        h = [float(np.linalg.norm(np.std(o['pos'][:, j, 0:2] - truth['ref_pos'][j, 0:2], axis=0))) for j in samples]
        y = [yaw_sigma(o['att'][:, j], truth['ref_att'][j]) for j in samples]
        out[key] = (ratio, np.array(y), np.array(h))
    return out


def test_restatement_consistency_and_benefit(consistency):
    """RMS end error over sqrt(mean pdiag_end) per state.  The magnetometer alone: inside the band the project uses for the unaided
    filter, [0.7, 1.4].  With mask 7: every ratio <= 1.4, as mask 7 is held without the magnetometer.  The yaw 1 sigma at the
    profile's end with the magnetometer is below half the GPS-only filter's, the horizontal position 1 sigma at the outage's last
    sample below the GPS-only filter's; ratios and both four-instant tables are the ones recorded."""
    for key in ('gps', 'mag', 'mag7'):
        r, y, h = consistency[key]
        print('%s consistency ratios:' % key, np.array2string(r, precision=3, separator=', '))
        print('%s yaw 1 sigma [rad] at outage start / end / +5 s / profile end:' % key, ', '.join('%.4e' % v for v in y))
        print('%s horizontal 1 sigma [m] at outage start / end / +5 s / profile end:' % key, np.array2string(h, precision=3, separator=', '))
    np.testing.assert_allclose(consistency['gps'][0], cs.CONSISTENCY_RATIOS, rtol=0, atol=2e-3)   # the unaided case of the other files
    np.testing.assert_allclose(consistency['gps'][2], ac.OUTAGE_TABLE[0], rtol=0, atol=2e-3)
    rm, r7 = consistency['mag'][0], consistency['mag7'][0]
    assert np.all(rm >= 0.7) and np.all(rm <= 1.4), rm
    assert np.all(r7 <= 1.4), r7
    assert consistency['mag'][1][3] < 0.5 * consistency['gps'][1][3], (consistency['mag'][1][3], consistency['gps'][1][3])
    assert consistency['mag'][2][1] < consistency['gps'][2][1], (consistency['mag'][2][1], consistency['gps'][2][1])
    np.testing.assert_allclose(rm, mc.CONSISTENCY_RATIOS[0], rtol=0, atol=2e-3)
    np.testing.assert_allclose(r7, mc.CONSISTENCY_RATIOS[7], rtol=0, atol=2e-3)
    for key in ('gps', 'mag', 'mag7'):
        np.testing.assert_allclose(consistency[key][1], mc.YAW_TABLE[key], rtol=2e-3, atol=0)
        np.testing.assert_allclose(consistency[key][2], mc.HORIZONTAL_TABLE[key], rtol=0, atol=2e-3)


# ------------------------------------------------------------------------------------------------- Python surface
def test_mag_model_defaults_and_refusals():
    from ginsim.ins_loose import mag_model
    a = mag_model(mc.MAG_ERR, mc.GEO, 0, {})
    assert sorted(a) == ['cal_hi', 'cal_si', 'mag_every', 'mag_n', 'r_mag']
    assert a['mag_every'] == 1 and np.array_equal(a['mag_n'], mc.GEO)
    assert np.array_equal(a['cal_si'], np.eye(3)) and np.array_equal(a['cal_hi'], np.zeros(3))
    np.testing.assert_allclose(a['r_mag'], [1e-4] * 3, rtol=1e-15)
    assert mag_model(mc.MAG_ERR, mc.GEO, 0, None)['mag_every'] == 1
    # ref_frame 1: x along the horizontal field
    b = mag_model(mc.MAG_ERR, mc.GEO, 1, {'every': 4})
    assert b['mag_every'] == 4 and np.array_equal(b['mag_n'], [np.hypot(30.0, -3.0), 0.0, 40.0])
    # the field the profile's truth carries at its level start is the frame's form
    _, truth, _ = mc.outage_truth(20.0, 1, 2.0, 10)
    _, truth0, _ = mc.outage_truth(20.0, 0, 2.0, 10)
    for rf, t in ((1, truth), (0, truth0)):
        from ginsim.ins_loose import mag_field
        att = t['ref_att'][0]
        D = ref.dcm_zyx(att[None])[0]
        np.testing.assert_allclose(t['ref_mag'][0], D @ mag_field(mc.GEO, rf), rtol=0, atol=1e-9)
    # a general calibration
    s = mag_model(mc.MAG_ERR_SKEW, mc.GEO, 0, {})
    inv = np.linalg.inv(mc.MAG_ERR_SKEW['si'])
    np.testing.assert_allclose(s['cal_si'], inv, rtol=1e-15)
    assert np.array_equal(s['cal_hi'], mc.MAG_ERR_SKEW['hi'])
    full = inv @ np.diag(mc.MAG_ERR_SKEW['std'] ** 2) @ inv.T
    np.testing.assert_allclose(s['r_mag'], np.diag(full), rtol=1e-14)
    assert len(set(np.round(s['r_mag'], 12))) == 3
    # what the filter assumes can differ from what generates: options override mag_err, and mag_err may be absent
    o = mag_model(None, None, 0, {'std': 0.1, 'si': np.diag([2.0, 1.0, 1.0]), 'hi': [1.0, 2.0, 3.0], 'field': [20.0, 0.0, 45.0]})
    np.testing.assert_allclose(o['r_mag'], [0.0025, 0.01, 0.01], rtol=1e-15)
    assert np.array_equal(o['cal_hi'], [1.0, 2.0, 3.0]) and np.array_equal(o['mag_n'], [20.0, 0.0, 45.0])
    for bad in ({'evry': 1}, {'si': np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]])}, {'si': np.zeros((3, 3))}, {'every': 0},
                {'every': 1.5}, {'std': 0.0}, {'std': [0.01, -0.01, 0.01]}, {'std': float('nan')}, {'field': [0.0, 0.0, 0.0]},
                {'field': [1.0, float('inf'), 0.0]}, {'hi': [1.0, 2.0]}):
        with pytest.raises(ValueError):
            mag_model(mc.MAG_ERR, mc.GEO, 0, bad)
    with pytest.raises(ValueError, match='unknown keys'):
        mag_model(mc.MAG_ERR, mc.GEO, 0, {'evry': 1})
    with pytest.raises(ValueError, match='singular'):
        mag_model(mc.MAG_ERR, mc.GEO, 0, {'si': np.zeros((3, 3))})
    with pytest.raises(ValueError, match='mag_err'):
        mag_model(None, mc.GEO, 0, {})
    with pytest.raises(ValueError, match='geomagnetic'):
        mag_model(mc.MAG_ERR, None, 0, {})


def test_plugin_surface():
    from demo_algorithms.ins_loose_device import InsLoose
    plain = InsLoose()
    assert plain.input == ['fs', 'gyro', 'accel', 'time', 'gps_time', 'gps'] and plain.mag_options() is None and plain.aid() is None
    a = InsLoose(mag=True)
    assert a.input == plain.input + ['mag'] and a.aid() is None
    assert a.mag_options() == {'every': 1, 'std': None, 'si': None, 'hi': None}
    assert a.output == ['pos', 'vel', 'att_euler', 'wb', 'ab'] and (a.batch, a.mc_algo) == (True, 'loose')
    b = InsLoose(odo=True, nhc=True, mag=True, mag_every=4, mag_std=0.1, mag_si=mc.MAG_ERR_SKEW['si'], mag_hi=mc.MAG_ERR_SKEW['hi'],
                 geo_mag_n=mc.GEO)
    assert b.input == plain.input + ['odo', 'mag'] and b.aid()['odo']
    opt = b.mag_options()
    assert opt['every'] == 4 and np.array_equal(opt['std'], [0.1] * 3) and np.array_equal(opt['si'], mc.MAG_ERR_SKEW['si'])
    assert np.array_equal(opt['hi'], mc.MAG_ERR_SKEW['hi']) and np.array_equal(b.geo_mag_n, mc.GEO)
    assert InsLoose(mag_every=4, mag_std=0.1).mag_options() is None            # the numbers alone switch nothing on
    for bad in (dict(mag_every=0), dict(mag_every=2.5), dict(mag_std=0.0), dict(mag_std=float('inf')), dict(mag_std=[0.1, 0.1]),
                dict(mag_si=np.eye(2)), dict(mag_si=np.full((3, 3), np.nan)), dict(mag_hi=[1.0]), dict(geo_mag_n=[1.0, 2.0])):
        with pytest.raises((ValueError, TypeError)):
            InsLoose(mag=True, **bad)
    series = [100.0, np.zeros((10, 3)), np.zeros((10, 3)), np.arange(10) / 100.0, np.zeros(1), np.zeros((1, 6))]
    with pytest.raises(ValueError, match='logged series'):
        a.run(series + [np.zeros((10, 3))])
    from gnss_ins_sim.sim import imu_model
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=9, gps=True)
    ini = np.zeros(9)
    with pytest.raises(ValueError, match="'mag'"):                              # the series is missing
        InsLoose(ini_pos_vel_att=ini, ref_frame=1, imu=imu, mag=True, geo_mag_n=mc.GEO).run(series)
    with pytest.raises(ValueError, match='geo_mag_n'):                          # no Sim to take the field from
        InsLoose(ini_pos_vel_att=ini, ref_frame=1, imu=imu, mag=True).run(series + [np.zeros((10, 3))])
    with pytest.raises(ValueError, match=r'\(n, 3\)'):
        InsLoose(ini_pos_vel_att=ini, ref_frame=1, imu=imu, mag=True, geo_mag_n=mc.GEO).run(series + [np.zeros(10)])


def test_sim_refuses_a_magnetometer_aided_insloose_without_a_magnetometer():
    from gnss_ins_sim.sim import imu_model, ins_sim
    from demo_algorithms.ins_loose_device import InsLoose

    def roles(algo, axis):
        sim = ins_sim.Sim([100.0, 10.0, 0.0], cs.OUTAGE_CSV, ref_frame=1, geo_mag_n=mc.GEO,
                          imu=imu_model.IMU(accuracy='mid-accuracy', axis=axis, gps=True), algorithm=algo)
        return ins_sim._plugin_roles(sim, [getattr(a, 'mc_algo', None) for a in sim.amgr.algo])
    with pytest.raises(ValueError, match=r"algorithm 0 needs 'mag' but the IMU model has no magnetometer \(IMU\(axis=9\)\)"):
        roles(InsLoose(mag=True), 6)
    with pytest.raises(ValueError, match="algorithm 1 needs 'mag' but the IMU model has no magnetometer"):
        roles([InsLoose(), InsLoose(mag=True)], 6)
    assert roles([InsLoose(), InsLoose(mag=True)], 9).loose == [0, 1]
    assert roles(InsLoose(), 6).loose == [0]
