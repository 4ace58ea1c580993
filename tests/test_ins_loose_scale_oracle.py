"""CPU: the odometer's scale factor as a 16th state of InsLoose: the C ABI's block and refusals, the build's resource
report of loose_scale_kernel, the restatement (tests/ins_loose_scale_ref.py) against the 15-state restatement in the degenerate
case, against its own np.longdouble evaluation, against the statistics of its own covariance and in the payoff it measures through
the GPS outage, and the Python surface.  Every recorded number is in tests/ins_loose_scale_cases.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import ins_loose_aided_cases as ac
import ins_loose_cases as cs
import ins_loose_ref as ref
import ins_loose_scale_cases as sc
import ins_loose_scale_ref as sref
from conftest import REPO

NEW = {'ginsim_loose_scale_run', 'ginsim_loose_scale_kernel_name'}


# ------------------------------------------------------------------------------------------------- 1. C ABI
def test_scale_entry_points_are_declared_exported_and_bound_at_abi_9():
    import ginsim
    hdr = open(os.path.join(REPO, 'include', 'ginsim.h')).read()
    declared = set(re.findall(r'\b(ginsim_[a-z0-9_]+)\s*\(', hdr))
    assert NEW <= declared
    so = ctypes.CDLL(ginsim.LIB_PATH)
    assert all(hasattr(so, f) for f in NEW)
    assert NEW <= set(ginsim.EXPORTS)
    assert ginsim.lib.ginsim_abi_version() == 9
    assert hasattr(ginsim, 'scale_model')
    assert re.search(r'#define GINSIM_ABI_VERSION 9\b', hdr)


def test_struct_mirror_matches_the_header_field_by_field():
    from ginsim import _lib
    hdr = open(os.path.join(REPO, 'include', 'ginsim.h')).read()
    body = re.search(r'typedef struct \{((?:(?!typedef struct).)*?)\}\s*ginsim_loose_scale_params\s*;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            t, name = re.match(r'^(double\s*\*|double)\s*(\w+)$', decl).groups()
            fields.append((name, ctypes.c_void_p if '*' in t else ctypes.c_double))
    assert fields == list(_lib.LooseScaleParams._fields_)
    assert [f[0] for f in fields] == ['scale0', 'p0_scale', 'q_k', 'out_scale', 'out_scale_end', 'out_pcross_end']
    assert ctypes.sizeof(_lib.LooseScaleParams) == 48
    # the blocks beside it are what they were
    assert [f[0] for f in _lib.LooseParams._fields_][-5:] == ['aid_mask', 'aid_every', 'odo_scale_f', 'r_odo', 'r_nhc']
    assert re.search(r'double\*\s+out_pdiag_end;\s*/\* \[15\]\[runs\]', hdr)


def _blocks():
    from ginsim import _lib as L
    m, p, g = L.McParams(), L.LooseParams(), L.LooseScaleParams()
    keep = [np.zeros(10), np.zeros(64), np.array([0, 10, 20], dtype=np.int64)]
    ini, dummy, stamps = keep
    m.n, m.runs, m.fs, m.ref_frame, m.n_ini, m.ini = 30, 4, 100.0, 1, 1, ini.ctypes.data
    m.given_sensors, m.in_accel, m.in_gyro, m.in_odo = 1, dummy.ctypes.data, dummy.ctypes.data, dummy.ctypes.data
    p.m, p.gps_stamp, p.in_gps, p.n_list = 3, stamps.ctypes.data, dummy.ctypes.data, 4
    p.r_diag[:], p.p0[:] = [1.0] * 6, [1.0] * 5
    p.decay_g[:], p.decay_a[:] = [1.0] * 3, [1.0] * 3
    p.aid_mask, p.aid_every, p.odo_scale_f, p.r_odo, p.r_nhc = 7, 1, 1.0, 0.01, 0.0025
    g.scale0, g.p0_scale, g.q_k = 1.0, 0.02, 0.0
    return L, m, p, g, keep


def test_scale_arguments_are_refused_without_a_device():
    L, m, p, g, keep = _blocks()
    dummy = keep[1]
    buf = ctypes.create_string_buffer(256)

    def name():
        return L.lib.ginsim_loose_scale_kernel_name(ctypes.byref(m), ctypes.byref(p), ctypes.byref(g), buf, 256)

    assert name() == L.OK and buf.value == b'ginsim::loose_scale_kernel<1, true, false, false>'
    for field, bad in (('p0_scale', (-1e-9, float('nan'), float('inf'))), ('scale0', (0.0, -1.0, float('nan'), float('inf'))),
                       ('q_k', (-1e-12, float('nan'), float('inf')))):
        good = getattr(g, field)
        for v in bad:
            setattr(g, field, v)
            assert name() == L.ERR_ARG, (field, v)
        setattr(g, field, good)
    g.p0_scale, g.q_k = 0.0, 0.0                                                # the degenerate case is legal
    assert name() == L.OK
    g.p0_scale, g.q_k = 0.02, 1e-9
    assert name() == L.OK
    for mask in (0, 2, 4, 6):                                                   # a scale state without the odometer
        p.aid_mask = mask
        assert name() == L.ERR_ARG, mask
    for mask in (1, 3, 5, 7):
        p.aid_mask = mask
        assert name() == L.OK, mask
    m.precision = 1                                                             # fp32
    assert name() == L.ERR_ARG
    m.precision = 0
    # everything ginsim_loose_run refuses: a few of its checks through this entry point
    for change, restore in ((lambda: setattr(p, 'aid_every', 0), lambda: setattr(p, 'aid_every', 1)),
                            (lambda: setattr(p, 'r_odo', 0.0), lambda: setattr(p, 'r_odo', 0.01)),
                            (lambda: setattr(m, 'in_odo', None), lambda: setattr(m, 'in_odo', dummy.ctypes.data)),
                            (lambda: setattr(m, 'ref_frame', 2), lambda: setattr(m, 'ref_frame', 1)),
                            (lambda: setattr(p, 'n_list', 5), lambda: setattr(p, 'n_list', 4))):
        change()
        assert name() == L.ERR_ARG
        assert L.lib.ginsim_loose_kernel_name(ctypes.byref(m), ctypes.byref(p), buf, 256) == L.ERR_ARG
        restore()
        assert name() == L.OK
    assert L.lib.ginsim_loose_scale_kernel_name(ctypes.byref(m), ctypes.byref(p), None, buf, 256) == L.ERR_ARG
    assert L.lib.ginsim_loose_scale_run(None, ctypes.byref(m), ctypes.byref(p), ctypes.byref(g)) == L.ERR_ARG


def test_the_printed_kernel_name_follows_rf_given_vib_and_ps():
    L, m, p, g, keep = _blocks()
    dummy = keep[1]
    buf = ctypes.create_string_buffer(256)

    def name():
        assert L.lib.ginsim_loose_scale_kernel_name(ctypes.byref(m), ctypes.byref(p), ctypes.byref(g), buf, 256) == L.OK
        return buf.value.decode()

    for rf in (0, 1):
        m.ref_frame = rf
        m.given_sensors = 1
        assert name() == 'ginsim::loose_scale_kernel<%d, true, false, false>' % rf
        m.ref_nav, m.proc_first, p.out_proc = dummy.ctypes.data, 0, dummy.ctypes.data
        assert name() == 'ginsim::loose_scale_kernel<%d, true, false, true>' % rf
        m.given_sensors = 0
        m.ref_accel, m.ref_gyro, p.ref_gps, m.ref_odo, m.odo_scale = (dummy.ctypes.data,) * 4 + (0.99,)
        assert name() == 'ginsim::loose_scale_kernel<%d, false, false, true>' % rf
        m.vib_accel.type = 1
        assert name() == 'ginsim::loose_scale_kernel<%d, false, true, true>' % rf
        p.out_proc = None
        assert name() == 'ginsim::loose_scale_kernel<%d, false, true, false>' % rf
        m.vib_accel.type = 0
        assert name() == 'ginsim::loose_scale_kernel<%d, false, false, false>' % rf


# ------------------------------------------------------------------------------------------------- 2. the resource report
def test_build_reports_no_scratch_and_the_stated_lds_for_the_12_instantiations():
    """build/ins_loose_scale.resources.txt (written by build.py): the 12 instantiations <RF, GIVEN, VIB, PS> of loose_scale_kernel,
    each with 0 bytes of scratch and at most 256 VGPRs.  LDS as DESIGN 4.11e states it: the report counts the static part only, the
    8192 B of normal tables of the generating forms (16 B of the given form); the covariance is 136 x 64 doubles = 69 632 B of
    dynamic LDS, and two workgroups (2 x (69 632 + 8192) = 155 648 B) fit the CU's 160 KiB."""
    from conftest import PKG
    path = os.path.join(PKG, 'build', 'ins_loose_scale.resources.txt')
    assert os.path.exists(path), 'run gnss-ins-sim_amd/build.py (it writes %s)' % path
    kernels, cur = {}, None
    for line in open(path):
        k, _, v = line.strip().partition(':')
        if k == 'Function Name':
            cur = kernels.setdefault(v.strip(), {})
        elif cur is not None and v.strip():
            cur[k.split('[')[0].strip()] = v.strip()
    mine = {n: r for n, r in kernels.items() if '18loose_scale_kernelI' in n}
    seen = set(re.search(r'loose_scale_kernelILi(\d)ELb(\d)ELb(\d)ELb(\d)E', n).groups() for n in mine)
    want = set((rf, g, v, ps) for rf in '01' for g in '01' for v in '01' for ps in '01' if not (g == '1' and v == '1'))
    assert seen == want and len(mine) == 12, seen ^ want
    dynamic = 8 * (16 * 17 // 2) * 64
    assert dynamic == 69632
    for n, r in mine.items():
        print(n, {k: r[k] for k in ('VGPRs', 'AGPRs', 'ScratchSize', 'Occupancy', 'LDS Size') if k in r})
        assert int(r['ScratchSize']) == 0, '%s: %s bytes of scratch per lane' % (n, r['ScratchSize'])
        assert int(r['Occupancy']) >= 1 and int(r['VGPRs']) <= 256, (n, r)
        given = re.search(r'loose_scale_kernelILi\dELb(\d)', n).group(1) == '1'
        assert int(r['LDS Size']) == (0 if given else 8192), (n, r['LDS Size'])     # the given form's 16 B table is never read
        assert 2 * (dynamic + int(r['LDS Size'])) <= 160 * 1024
    hpp = open(os.path.join(PKG, 'csrc', 'ins_loose.hpp')).read()
    assert 'loose_cov_lds(int ns)' in hpp and 'kLooseScaleStates = kLooseStates + 1' in hpp


# ------------------------------------------------------------------------------------------------- 3. the degenerate case
@pytest.fixture(scope='module')
def small():
    """5 runs on the outage profile at 20 Hz (1200 samples), per frame: every test of the arithmetic shares them."""
    out = {}
    for rf in (0, 1):
        d = sc.draws(5, 3, ref_frame=rf)
        d['odo'] = sc.odometer(d)
        out[rf] = d
    return out


def _args(d):
    return (d['rf'], d['fs'], d['gyro'], d['accel'], d['ini'], d['model'], d['gps'], d['stamps'], d['truth']['gps_visibility'])


@pytest.mark.parametrize('mask', [1, 7])
@pytest.mark.parametrize('rf', [0, 1])
def test_p0_zero_is_the_15_state_restatement_exactly(small, rf, mask):
    d, s = small[rf], 0.99
    assert d['gyro'].shape[1] == 1200 and np.any(d['truth']['gps_visibility'] == 0)
    a = ref.run(*_args(d), odo=d['odo'], aid=ac.aid(mask, odo_err={'scale': s, 'stdv': sc.ODO_STDV}))
    b = sref.run(*_args(d), odo=d['odo'], aid=sc.aid(mask, scale0=s), scale=sc.scale(s, 0.0, 0.0))
    for k in cs.PARITY_KEYS:
        assert np.array_equal(a[k], b[k]), k                                    # adding 0 * h changes nothing
    assert np.array_equal(a['P_end'], b['P_end'][:, :15, :15])
    assert np.all(b['k_est'] == s) and np.all(b['scale_end'] == [s, 0.0]) and not b['pcross_end'].any()
    c = sref.run(*_args(d), odo=d['odo'], aid=sc.aid(mask, scale0=s), scale=sc.scale(s, 0.02, 0.0))
    assert not np.array_equal(a['vel'], c['vel']) and np.all(c['k_est'][:, -1] != s)     # and the state does something
    assert np.all(c['scale_end'][:, 1] < 0.02 ** 2) and np.all(c['scale_end'][:, 1] > 0)
    P = c['P_end']
    dd = np.sqrt(P[:, np.arange(16), np.arange(16)])
    assert np.all(np.linalg.eigvalsh(P / (dd[:, :, None] * dd[:, None, :])) > -1e-9)


def test_the_random_walk_only_adds_to_the_last_diagonal_element(small):
    d = small[1]
    never = sc.aid(1, every=10 ** 6)
    args = (d['rf'], d['fs'], d['gyro'][:, :200], d['accel'][:, :200], d['ini'], d['model'])
    a = sref.run(*args, odo=d['odo'], aid=never, scale=sc.scale(1.0, 0.02, 0.0))
    b = sref.run(*args, odo=d['odo'], aid=never, scale=sc.scale(1.0, 0.02, 0.003, fs=d['fs']))
    for k in cs.PARITY_KEYS + ('k_est', 'pcross_end'):
        assert np.array_equal(a[k], b[k]), k
    np.testing.assert_allclose(b['scale_end'][:, 1] - a['scale_end'][:, 1], 199 * 0.003 ** 2 / d['fs'], rtol=1e-9)


# ------------------------------------------------------------------------------------------------- 4. float64 error
@pytest.mark.parametrize('mask', [1, 7])
@pytest.mark.parametrize('rf', [0, 1])
def test_float64_error_of_the_restatement(small, rf, mask):
    """The float64 restatement against its np.longdouble evaluation, per output (ins_loose_scale_cases.deviation), measured on
    the case: this, times ins_loose_cases.PARITY_MARGIN, is what the device test allows, measured anew on each of its cases (as
    ins_loose_cases.parity_bound does).  Here every figure is printed and held to 4 x the one recorded in
    ins_loose_scale_cases.RESTATEMENT_ERROR, the freedom another NumPy build's order of operations may take."""
    d = small[rf]
    err = cs.restatement_error(*_args(d), run=sref.run, deviation=sc.deviation, odo=d['odo'], aid=sc.aid(mask), scale=sc.scale())
    print('rf%d mask %d float64 error: ' % (rf, mask) + ', '.join('%s %.2e' % kv for kv in err.items()))
    assert set(err) == set(sc.PARITY_KEYS)
    for k, v in err.items():
        assert 0.0 < v <= 4.0 * sc.RESTATEMENT_ERROR[(rf, mask)][k], (k, v)


# ------------------------------------------------------------------------------------------------- 5. consistency
@pytest.fixture(scope='module')
def consistency():
    d = sc.draws(cs.CONSISTENCY_RUNS, cs.CONSISTENCY_SEED)
    o16 = sref.run(*_args(d), odo=sc.odometer(d), aid=sc.aid(1), scale=sc.scale())
    # the defect: the same runs and noise, an odometer that reads 0.99, the 15-state filter that assumes 1.0
    o15 = ref.run(*_args(d), odo=sc.odometer(d, sc.READS), aid=sc.aid(1))
    return d, sc.ratios16(d, o16, d['scales']), sc.ratios16(d, o15, None), o16


def test_restatement_consistency(consistency):
    """RMS end error over sqrt(mean P_kk) for all 16 states, every run with a true scale of its own ~ N(1, 0.02^2) that the filter
    does not know (scale0 = 1, p0 = 0.02): inside [0.8, 1.25] and as recorded."""
    d, r16, _, o16 = consistency
    print('consistency ratios, 16 states:', np.array2string(r16, precision=3, separator=', '))
    print('k_est - k at the end: rms %.5f, mean sigma %.5f' % (np.sqrt(np.mean((o16['scale_end'][:, 0] - d['scales']) ** 2)),
                                                                np.sqrt(np.mean(o16['scale_end'][:, 1]))))
    lo, hi = sc.CONSISTENCY_BAND
    assert r16.shape == (16,) and np.all(r16 >= lo) and np.all(r16 <= hi), r16
    np.testing.assert_allclose(r16, sc.CONSISTENCY_RATIOS, rtol=0, atol=2e-3)
    assert np.sqrt(np.mean(o16['scale_end'][:, 1])) < 0.25 * sc.P0_SCALE        # the state was learnt, not only carried


def test_restatement_consistency_on_the_tilted_profile():
    """The same filter and draw on tests/golden/ins_loose/motion_def_tilted.csv (41 S, yaw through +-180 deg twice, pitch and roll away
    from level, climbing and descending): all 16 ratios inside the same band and as recorded in
    ins_loose_scale_cases.CONSISTENCY_BY_PROFILE['tilted'], which tests/test_gpu_ins_loose_tilted_aids.py holds the device to."""
    d = sc.draws(cs.CONSISTENCY_RUNS, cs.CONSISTENCY_SEED, profile=cs.TILTED_CSV)
    assert d['gyro'].shape[1] == 800
    o16 = sref.run(*_args(d), odo=sc.odometer(d), aid=sc.aid(1), scale=sc.scale())
    r16 = sc.ratios16(d, o16, d['scales'])
    print('tilted profile, consistency ratios, 16 states:', np.array2string(r16, precision=3, separator=', '))
    print('k_est - k at the end: rms %.5f, mean sigma %.5f' % (np.sqrt(np.mean((o16['scale_end'][:, 0] - d['scales']) ** 2)),
                                                                np.sqrt(np.mean(o16['scale_end'][:, 1]))))
    lo, hi = sc.CONSISTENCY_BAND
    assert r16.shape == (16,) and np.all(r16 >= lo) and np.all(r16 <= hi), r16
    np.testing.assert_allclose(r16, sc.CONSISTENCY_BY_PROFILE['tilted'], rtol=0, atol=2e-3)
    assert np.sqrt(np.mean(o16['scale_end'][:, 1])) < 0.25 * sc.P0_SCALE        # the state was learnt, not only carried


def test_the_wrong_scale_is_the_defect_the_state_removes(consistency):
    """The same 15-state filter assuming 1.0 for an odometer that reads 0.99, on the same runs: a position or velocity ratio above 3."""
    _, _, r15, _ = consistency
    print('consistency ratios of the 15-state filter assuming 1.0 of an odometer that reads 0.99:',
          np.array2string(r15, precision=3, separator=', '))
    worst = int(np.argmax(r15[0:6]))
    assert r15[worst] > 3.0, r15
    assert worst == sc.WRONG_SCALE_RATIO[1]
    np.testing.assert_allclose(r15[worst], sc.WRONG_SCALE_RATIO[0], rtol=0, atol=5e-3)


# ------------------------------------------------------------------------------------------------- 6. the payoff
def test_payoff_table():
    """The three filters of examples/demo_ins_loose_odo_scale.py on 257 runs of an odometer that reads 0.99 (odometer and
    constraints at every sample), at the outage's last sample: the filter with the state is better than the filter that assumes
    1.0 and within PAYOFF_FACTOR x PAYOFF_HEADROOM of the filter that is told 0.99."""
    d = sc.draws(sc.PAYOFF_RUNS, sc.PAYOFF_SEED, scales=sc.READS)
    odo = sc.odometer(d)
    j = ac.outage_samples(d['truth'], d['stamps'], d['fs'], d['fs_gps'])[1]
    told_aid = ac.aid(7, odo_err={'scale': sc.READS, 'stdv': sc.ODO_STDV})
    wrong_aid = dict(told_aid, odo_scale_f=1.0)                                 # the same r_odo: only the assumed scale differs
    res = {'wrong': ref.run(*_args(d), odo=odo, aid=wrong_aid, keep_pdiag=True),
           'told': ref.run(*_args(d), odo=odo, aid=told_aid, keep_pdiag=True),
           'state': sref.run(*_args(d), odo=odo, aid=sc.aid(7), scale=sc.scale(), keep_pdiag=True)}
    table = {}
    for k, o in res.items():
        e = o['pos'][:, j, 0:2] - d['truth']['ref_pos'][j, 0:2]
        table[k] = (float(np.sqrt(np.mean(o['pdiag'][:, j, 0] + o['pdiag'][:, j, 1]))), float(np.sqrt(np.mean(np.sum(e * e, axis=1)))))
        print('%-5s horizontal 1 sigma %.3f m, RMS %.3f m at the outage\'s end' % (k, table[k][0], table[k][1]))
    se = res['state']['scale_end']
    k_end = (float(np.mean(se[:, 0])), float(np.sqrt(np.mean(se[:, 1]))))
    print('k_est %.4f +- %.4f at the profile\'s end' % k_end)
    factor = table['state'][1] / table['told'][1]
    print('RMS of the filter with the state over that of the filter told the truth: %.3f' % factor)
    assert table['state'][1] < table['wrong'][1]
    assert table['state'][1] <= sc.PAYOFF_FACTOR * sc.PAYOFF_HEADROOM * table['told'][1]
    for k in table:
        np.testing.assert_allclose(table[k], sc.PAYOFF_TABLE[k], rtol=0, atol=2e-3)
    np.testing.assert_allclose(k_end, sc.PAYOFF_SCALE, rtol=0, atol=2e-4)
    np.testing.assert_allclose(factor, sc.PAYOFF_FACTOR, rtol=0, atol=5e-3)
    assert abs(k_end[0] - sc.READS) < 3 * k_end[1]


# ------------------------------------------------------------------------------------------------- 7. Python surface
def test_scale_model_defaults_and_errors():
    from ginsim.ins_loose import scale_model
    assert scale_model(ac.ODO_ERR, None) is None and scale_model(None, False) is None
    assert scale_model(ac.ODO_ERR, {}) == {'scale0': 1.0, 'p0_scale': 0.02, 'q_k': 0.0} == scale_model(None, True)
    got = scale_model(None, {'scale0': 0.98, 'p0': 0.0, 'q': 0.01}, fs=100.0)
    assert got == {'scale0': 0.98, 'p0_scale': 0.0, 'q_k': 0.01 ** 2 / 100.0}
    for bad in ({'scale0': 0.0}, {'scale0': -1.0}, {'scale0': float('nan')}, {'p0': -0.01}, {'p0': float('inf')}, {'q': -1.0},
                {'q': float('nan')}, {'sigma': 0.02}):
        with pytest.raises(ValueError):
            scale_model(None, bad, fs=100.0)
    with pytest.raises(ValueError, match='fs'):
        scale_model(None, {'q': 0.01})


def test_plugin_surface():
    from demo_algorithms.ins_loose_device import InsLoose
    plain = InsLoose(odo=True, nhc=True)
    assert plain.output == ['pos', 'vel', 'att_euler', 'wb', 'ab'] and plain.scale_options() is None
    a = InsLoose(odo=True, nhc=True, odo_scale_state=True)
    assert a.input == ['fs', 'gyro', 'accel', 'time', 'gps_time', 'gps', 'odo']
    assert a.output == ['pos', 'vel', 'att_euler', 'wb', 'ab', 'odo_scale'] and (a.batch, a.mc_algo) == (True, 'loose')
    assert a.scale_options() == {'scale0': 1.0, 'p0': 0.02, 'q': 0.0} and a.aid()['scale'] is None
    b = InsLoose(odo=True, odo_scale_state=True, odo_scale0=0.98, odo_scale_p0=0.05, odo_scale_q=1e-3)
    assert b.scale_options() == {'scale0': 0.98, 'p0': 0.05, 'q': 1e-3}
    with pytest.raises(ValueError, match='odo_scale0'):
        InsLoose(odo=True, odo_scale_state=True, odo_scale=0.99)
    with pytest.raises(ValueError, match='odo=True'):
        InsLoose(odo_scale_state=True)
    with pytest.raises(ValueError, match='odo=True'):
        InsLoose(nhc=True, odo_scale_state=True)
    with pytest.raises(ValueError, match='mag=True'):
        InsLoose(odo=True, mag=True, odo_scale_state=True)
    for bad in (dict(odo_scale0=0.0), dict(odo_scale_p0=-1.0), dict(odo_scale_q=float('nan'))):
        with pytest.raises(ValueError):
            InsLoose(odo=True, odo_scale_state=True, **bad)
    with pytest.raises(ValueError, match='logged series'):
        a.run([100.0, np.zeros((10, 3)), np.zeros((10, 3)), np.arange(10) / 100.0, np.zeros(1), np.zeros((1, 6)), np.zeros(10)])
    a.finish(1, 2, 3, 4, 5, 6)
    assert a.get_results() == [1, 2, 3, 4, 5, 6]
    plain.finish(1, 2, 3, 4, 5)
    assert plain.get_results() == [1, 2, 3, 4, 5]


def test_sim_takes_the_plugin_refuses_it_without_an_odometer_and_refuses_its_consistency_curve():
    from gnss_ins_sim.sim import imu_model, ins_sim
    from demo_algorithms.ins_loose_device import InsLoose

    def make(algo, odo):
        return ins_sim.Sim([100.0, 10.0, 0.0], cs.OUTAGE_CSV, ref_frame=1,
                           imu=imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=True, odo=odo), algorithm=algo)

    def roles(sim):
        return ins_sim._plugin_roles(sim, [getattr(a, 'mc_algo', None) for a in sim.amgr.algo])
    with pytest.raises(ValueError, match="algorithm 1 needs 'odo' but the IMU model has no odometer"):
        roles(make([InsLoose(), InsLoose(odo=True, odo_scale_state=True)], False))
    sim = make([InsLoose(odo=True, nhc=True), InsLoose(odo=True, nhc=True, odo_scale_state=True)], True)
    assert roles(sim).loose == [0, 1]
    assert sim.dmgr.is_supported('odo_scale')

    # consistency_curve: the refusal is decided on the job of the last run; no device is needed to see it
    class Job(object):
        mag, scale = None, {'scale0': 1.0, 'p0_scale': 0.02, 'q_k': 0.0}

    class Mc(object):
        loose_names = ('InsLoose_1',)
    sim.sim_complete, sim.mc, sim.loose_jobs = True, Mc(), [(1, Job(), None)]
    sim.dmgr.time.data = np.arange(10) / 100.0
    with pytest.raises(NotImplementedError, match='odo_scale_state'):
        sim.consistency_curve(every=0.05)


def test_the_job_refuses_what_is_not_built():
    """The refusals InsLooseJob makes before it touches a device (ctx is not used before them)."""
    import ginsim
    ini, truth, _ = ac.outage_truth(20.0, 1, 2.0, 100)
    acc_e, gyr_e = cs.imu_errors()
    base = dict(odo_err=ac.ODO_ERR, odo_scale_state={})

    def job(**kw):
        return ginsim.InsLooseJob(None, 20.0, 1, truth, acc_e, gyr_e, cs.GPS_ERR, ini, 4, **dict(base, **kw))
    with pytest.raises(ValueError, match='without the odometer'):
        job(aid={'nhc': True})
    with pytest.raises(ValueError, match='without the odometer'):
        job(aid=None)
    with pytest.raises(ValueError, match='magnetometer'):
        job(aid={'odo': True}, mag={})
    with pytest.raises(ValueError, match='cons_samples'):
        job(aid={'odo': True}, cons_samples=[10])
    with pytest.raises(ValueError, match='keep_scale'):
        job(aid={'odo': True}, odo_scale_state=None, keep_scale=True)
