"""CPU: InsLoose's consistency checkpoints: the C ABI's checkpoint block and its refusals, the build's resource report
of loose_cons_kernel, the restatement (tests/ins_loose_cons_ref.py) on the consistency case, its long-double evaluation, and the
Python surface that needs no device.

Recorded here (measured by test_consistency_bands: 1024 runs drawn from the filter's own model with
np.random.default_rng(ins_loose_cases.CONSISTENCY_SEED), the outage profile at 20 Hz with 2 Hz GPS, 'mid-accuracy' IMU, ref_frame 1,
GPS only; a checkpoint every 5 s and at the last sample; all 1024 runs included at every checkpoint).
RMS error / sqrt(mean P_kk) of dr, dv, psi and the mean block NEES of position, velocity, attitude:
    t [s]    dr                   dv                   psi                  NEES
     0.00    0.000 0.000 0.000    0.020 0.020 0.019    0.000 0.000 0.000    0.000 0.001 0.000    (the runs start ON the truth)
     5.00    0.877 0.874 0.575    0.976 0.971 0.809    0.993 0.980 1.010    1.848 2.510 2.967
    10.00    0.968 0.985 0.728    0.986 1.004 0.893    1.021 1.013 0.961    2.387 2.701 2.990
    15.00    1.011 0.972 0.801    1.016 0.987 0.975    1.002 0.997 0.988    2.570 2.868 2.973
    20.00    0.970 0.998 0.862    0.968 1.013 0.967    1.008 1.024 1.000    2.654 2.843 3.068    (the outage: 20 s - 40 s)
    25.00    0.968 1.010 0.901    0.987 1.013 0.941    0.987 1.027 1.002    2.723 2.859 3.038
    30.00    0.979 1.013 0.917    1.005 1.008 0.940    0.983 1.014 0.997    2.766 2.918 2.991
    35.00    0.990 1.011 0.927    1.006 0.999 0.961    0.970 1.002 0.986    2.807 2.949 2.920
    40.00    1.001 1.036 0.922    1.023 1.016 0.956    0.960 0.974 0.982    2.908 3.011 2.837
    45.00    0.990 1.001 0.930    0.993 0.995 0.978    1.017 0.955 0.999    2.840 2.918 2.941
    50.00    0.982 0.984 0.949    1.020 0.996 0.992    1.023 0.981 1.005    2.826 2.964 3.009
    55.00    0.990 0.977 0.956    0.986 1.025 0.984    1.000 0.993 1.010    2.846 2.956 3.007
    59.95    0.988 0.982 0.942    1.022 0.963 0.950    0.941 0.960 1.015    2.828 2.877 2.844    (= CONSISTENCY_RATIOS[:9])
From 15 s on: ratios 0.80-1.04, NEES 2.57-3.07.  Before that the filter is pessimistic (the vertical channel longest): P0 and R
describe more error than runs that start on the truth have."""
import ctypes
import os
import re

import numpy as np
import pytest

import ins_loose_aided_cases as ac
import ins_loose_cases as cs
import ins_loose_cons_ref as cref
import ins_loose_ref as ref
from conftest import REPO
from ins_loose_cons_cases import SETTLED, in_bands

NEW = {'ginsim_loose_cons_run', 'ginsim_loose_cons_kernel_name'}


# ------------------------------------------------------------------------------------------------- C ABI
def test_the_checkpoint_block_is_declared_exported_bound_and_mirrored():
    import ginsim
    from ginsim import _lib
    hdr = open(os.path.join(REPO, 'include', 'ginsim.h')).read()
    declared = set(re.findall(r'\b(ginsim_[a-z0-9_]+)\s*\(', hdr))
    so = ctypes.CDLL(ginsim.LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(so, name) and name in ginsim.EXPORTS
    assert re.search(r'#define\s+GINSIM_CONS_RECORD\s+43\b', hdr) and _lib.CONS_RECORD == 43 == cref.RECORD
    assert ginsim.lib.ginsim_abi_version() == 9
    body = re.search(r'typedef struct \{((?:(?!typedef struct).)*?)\}\s*ginsim_loose_cons_params\s*;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [re.sub(r'^(const\s+)?\w+\s*\*?', '', d.strip(), count=1).strip(' *') for d in body.split(';') if d.strip()]
    assert names == [f[0] for f in _lib.LooseConsParams._fields_] == ['cons_sample', 'cons_m', 'out_cons', 'cons_work']
    types = dict(_lib.LooseConsParams._fields_)
    assert types['cons_m'] is ctypes.c_int64 and all(types[k] is ctypes.c_void_p for k in ('cons_sample', 'out_cons', 'cons_work'))
    assert hasattr(ginsim, 'ConsistencyResult') and ginsim.ConsistencyResult.WIDTH == 43


def test_checkpoint_arguments_are_refused_without_a_device():
    from ginsim import _lib as L
    m, p, q = L.McParams(), L.LooseParams(), L.LooseConsParams()
    buf = ctypes.create_string_buffer(256)
    ini, dummy = np.zeros(10), np.zeros(64)
    stamps = np.array([0, 10, 20], dtype=np.int64)
    cons = np.array([0, 10, 29], dtype=np.int64)
    m.n, m.runs, m.fs, m.ref_frame, m.n_ini, m.ini = 30, 4, 100.0, 1, 1, ini.ctypes.data
    m.given_sensors, m.in_accel, m.in_gyro, m.in_odo = 1, dummy.ctypes.data, dummy.ctypes.data, dummy.ctypes.data
    p.m, p.gps_stamp, p.in_gps, p.n_list = 3, stamps.ctypes.data, dummy.ctypes.data, 4
    p.r_diag[:], p.p0[:] = [1.0] * 6, [1.0] * 5
    p.decay_g[:], p.decay_a[:] = [1.0] * 3, [1.0] * 3

    def name():
        return L.lib.ginsim_loose_cons_kernel_name(ctypes.byref(m), ctypes.byref(p), ctypes.byref(q), buf, 256)

    # a zeroed block is the launch ginsim_loose_run makes, whatever the pointers say
    assert name() == L.OK and buf.value == b'ginsim::loose_kernel<1, true, false, false>'
    assert L.lib.ginsim_loose_cons_kernel_name(ctypes.byref(m), ctypes.byref(p), None, buf, 256) == L.ERR_ARG
    q.cons_m = -1
    assert name() == L.ERR_ARG
    q.cons_m = 3
    assert name() == L.ERR_ARG                                                  # no pointers at all
    q.cons_sample, q.out_cons, q.cons_work, m.ref_nav = cons.ctypes.data, dummy.ctypes.data, dummy.ctypes.data, dummy.ctypes.data
    assert name() == L.OK and buf.value == b'ginsim::loose_cons_kernel<1, true, false, false>'
    for field, owner in (('cons_sample', q), ('out_cons', q), ('cons_work', q), ('ref_nav', m)):
        good = getattr(owner, field)
        setattr(owner, field, None)
        assert name() == L.ERR_ARG, field
        setattr(owner, field, good)
    assert name() == L.OK
    for bad in ([0, 10, 30], [-1, 10, 20], [0, 10, 10], [0, 20, 10]):          # outside [0, n), not strictly increasing
        cons[:] = bad
        assert name() == L.ERR_ARG, bad
    cons[:] = [0, 1, 29]
    assert name() == L.OK
    p.out_proc = dummy.ctypes.data                                             # online process statistics and checkpoints
    assert name() == L.ERR_ARG
    p.out_proc = None
    m.precision = 1                                                            # what ginsim_loose_run refuses is refused here too
    assert name() == L.ERR_ARG
    m.precision = 0
    # every instantiation has its name: <RF, GIVEN, VIB, AID>
    p.aid_mask, p.aid_every, p.odo_scale_f, p.r_odo, p.r_nhc = 7, 1, 0.99, 0.01, 0.0025
    assert name() == L.OK and buf.value == b'ginsim::loose_cons_kernel<1, true, false, true>'
    m.given_sensors = 0
    m.ref_accel, m.ref_gyro, m.ref_odo, p.ref_gps = dummy.ctypes.data, dummy.ctypes.data, dummy.ctypes.data, dummy.ctypes.data
    m.ref_frame = 0
    assert name() == L.OK and buf.value == b'ginsim::loose_cons_kernel<0, false, false, true>'
    m.vib_accel.type = 1
    p.aid_mask = 0
    assert name() == L.OK and buf.value == b'ginsim::loose_cons_kernel<0, false, true, false>'
    # the run entry point makes the same checks before it touches a device
    q.cons_m = -1
    assert L.lib.ginsim_loose_cons_run(None, ctypes.byref(m), ctypes.byref(p), ctypes.byref(q)) == L.ERR_ARG


def test_build_reports_no_scratch_for_any_instantiation_of_the_checkpoint_kernel():
    """build/ins_loose_cons.resources.txt (written by build.py): the 12 instantiations <RF, GIVEN, VIB, AID> of loose_cons_kernel,
    each with 0 bytes of scratch, at most 256 VGPRs, one wavefront per SIMD or more and the static LDS bound the two existing filter
    kernels are held to."""
    from conftest import PKG
    path = os.path.join(PKG, 'build', 'ins_loose_cons.resources.txt')
    assert os.path.exists(path), 'run gnss-ins-sim_amd/build.py (it writes %s)' % path
    kernels, cur = {}, None
    for line in open(path):
        k, _, v = line.strip().partition(':')
        if k == 'Function Name':
            cur = kernels.setdefault(v.strip(), {})
        elif cur is not None and v.strip():
            cur[k.split('[')[0].strip()] = v.strip()
    cons = {n: r for n, r in kernels.items() if '17loose_cons_kernelI' in n}
    seen = set(re.search(r'loose_cons_kernelILi(\d)ELb(\d)ELb(\d)ELb(\d)E', n).groups() for n in cons)
    want = set((rf, g, v, aid) for rf in '01' for g in '01' for v in '01' for aid in '01' if not (g == '1' and v == '1'))
    assert seen == want, seen ^ want
    for n, r in cons.items():
        print(n, {k: r[k] for k in ('VGPRs', 'AGPRs', 'ScratchSize', 'Occupancy', 'LDS Size') if k in r})
        assert int(r['ScratchSize']) == 0, '%s: %s bytes of scratch per lane' % (n, r['ScratchSize'])
        assert int(r['Occupancy']) >= 1 and int(r['VGPRs']) <= 256, (n, r)
        assert int(r['LDS Size']) <= 8192 + 4 * 4, (n, r['LDS Size'])
    assert any('cons_final_kernel' in n for n in kernels)


# ------------------------------------------------------------------------------------------------- the restatement
def consistency_case(runs=cs.CONSISTENCY_RUNS):
    """The consistency case of tests/test_ins_loose_oracle.py (the same draws): (args of cref.run up to cons_samples, kwargs)."""
    from ginsim.ins_loose import filter_model
    fs = cs.CONSISTENCY_FS
    ini, truth, stamps = cs.outage_truth(fs, 1, cs.CONSISTENCY_FS_GPS)
    acc_e, gyr_e = cs.imu_errors()
    rng = np.random.default_rng(cs.CONSISTENCY_SEED)
    accel, gyro, _, _ = ref.sample_sensors(rng, fs, truth['ref_accel'], truth['ref_gyro'], acc_e, gyr_e, cs.CONSISTENCY_RUNS)
    gps = cs.sample_gps(rng, truth, 1, cs.CONSISTENCY_RUNS)
    nav = np.concatenate([truth['ref_att'], truth['ref_pos'], truth['ref_vel']], axis=1)
    model = filter_model(fs, acc_e, gyr_e, cs.GPS_ERR)
    return (1, fs, gyro[:runs], accel[:runs], ini, model, nav), dict(gps=gps[:runs], stamps=stamps, visible=truth['gps_visibility'])


def test_consistency_bands():
    """The curve of this file's header.  From 15 s on every navigation-state ratio lies in [0.7, 1.4] and every block NEES in
    [1.47, 5.88]; before, the upper ends; the last checkpoint is the end-point figure tests/test_ins_loose_oracle.py records."""
    args, kw = consistency_case()
    fs, n = args[1], args[2].shape[1]
    samples = list(range(0, n, int(round(5 * fs)))) + [n - 1]
    rec = cref.run(*args, samples, **kw)
    m = cref.means(rec)
    t = np.array(samples) / fs
    for row in zip(t, m['ratio'], m['nees']):
        print('%6.2f  ' % row[0] + '  '.join(' '.join('%.3f' % x for x in v) for v in (row[1][0:3], row[1][3:6], row[1][6:9], row[2])))
    assert np.all(m['count'] == cs.CONSISTENCY_RUNS) and not rec[:, 37:].any()
    in_bands(t, m['ratio'], m['nees'])
    late = t >= SETTLED
    print('from %g s on: ratios %.2f-%.2f, NEES %.2f-%.2f' % (SETTLED, m['ratio'][late].min(), m['ratio'][late].max(),
                                                               m['nees'][late].min(), m['nees'][late].max()))
    np.testing.assert_allclose(m['ratio'][-1], cs.CONSISTENCY_RATIOS[:9], rtol=0, atol=2e-3)


def test_the_long_double_evaluation_really_propagates():
    """Every field of the long-double record has dtype longdouble, and the float64 record deviates from it by more than 0 (a
    restatement that fell back to float64 inside would agree exactly)."""
    args, kw = consistency_case(runs=8)
    n = 200
    args = args[:2] + (args[2][:, :n], args[3][:, :n]) + args[4:]
    samples = [0, 1, 57, 199, 57]                                            # any order, a repeat
    lo = cref.run(*args, samples, **kw)
    hi = cref.run(*args, samples, dtype=np.longdouble, **kw)
    assert lo.dtype == np.float64 and hi.dtype == np.longdouble and hi.shape == (5, cref.RECORD)
    assert np.array_equal(lo[2], lo[4]) and np.array_equal(hi[2], hi[4])
    mh = cref.means(hi)
    assert all(v.dtype == np.longdouble for v in mh.values())
    dev = cref.deviation(lo, hi)
    assert dev[0] == 0.0                                                     # the count
    assert np.all(dev[1:] > 0.0) and np.all(dev[1:] < 1e-6), dev
    # the aided filter goes through the same record
    ini, truth, stamps = ac.outage_truth(args[1], 1, cs.CONSISTENCY_FS_GPS)
    odo = np.tile(truth['ref_odo'][None, :n] * ac.ODO_ERR['scale'], (8, 1))
    a7 = cref.run(*args, samples, odo=odo, aid=ac.aid(7), **kw)
    assert np.all(a7[3, 4:10] < lo[3, 4:10])                                 # the rows shrink P on dv and psi


def test_a_run_that_is_not_finite_or_not_positive_definite_is_left_out():
    args, kw = consistency_case(runs=8)
    n = 120
    gyro, accel = args[2][:, :n].copy(), args[3][:, :n].copy()
    accel[5, 60:, 1] = np.nan
    bad = cref.run(*(args[:2] + (gyro, accel) + args[4:]), [10, 60, 61, 119], **kw)
    keep = np.setdiff1d(np.arange(8), [5])
    rest = cref.run(*(args[:2] + (gyro[keep], accel[keep]) + (args[4], args[5], args[6])), [10, 60, 61, 119],
                    gps=kw['gps'][keep], stamps=kw['stamps'], visible=kw['visible'])
    assert list(bad[:, 0]) == [8, 8, 7, 7] and np.all(np.isfinite(bad))
    np.testing.assert_allclose(bad[2:], rest[2:], rtol=1e-12)
    # the block rule alone
    B = np.array([[[2.0, 0, 0], [0, 1, 0], [0, 0, 1]], [[1.0, 2, 0], [2, 1, 0], [0, 0, 1]], [[-1.0, 0, 0], [0, 1, 0], [0, 0, 1]]])
    e = np.ones((3, 3))
    v = cref.block_nees(B, e)
    assert v[0] == 2.5 and np.isnan(v[1]) and np.isnan(v[2])
    np.testing.assert_allclose(cref.block_nees(B[:1] + 0.3, e[:1]), e[0] @ np.linalg.solve(B[0] + 0.3, e[0]), rtol=1e-14)


# ------------------------------------------------------------------------------------------------- Python surface
def test_consistency_result_means_properties_and_merge():
    from ginsim import ConsistencyResult
    rng = np.random.default_rng(5)
    a, b = rng.uniform(1.0, 2.0, (4, 43)), rng.uniform(1.0, 2.0, (4, 43))
    a[:, 0], b[:, 0] = 10, 6
    ra = ConsistencyResult(a)
    assert ra.m == 4 and ra.pbar.shape == (4, 15) and ra.e2.shape == (4, 9) and ra.nes.shape == (4, 9) and ra.nees.shape == (4, 3)
    np.testing.assert_array_equal(ra.count, 10)
    np.testing.assert_array_equal(ra.pbar, a[:, 1:16] / 10)
    np.testing.assert_array_equal(ra.nees, a[:, 34:37] / 10)
    np.testing.assert_array_equal(ra.sigma, np.sqrt(ra.pbar))
    np.testing.assert_array_equal(ra.rms, np.sqrt(ra.e2))
    np.testing.assert_array_equal(ra.ratio, ra.rms / ra.sigma[:, :9])
    np.testing.assert_array_equal(ConsistencyResult.unpack(ra.pack()).pack(), a)
    both = ConsistencyResult.merge([ra.pack(), ConsistencyResult(b).pack(), ConsistencyResult.zero(4).pack()])
    np.testing.assert_array_equal(both.count, 16)
    np.testing.assert_array_equal(both.pack(), a + b)
    np.testing.assert_array_equal(both.e2, (a + b)[:, 16:25] / 16)


def test_sim_without_an_insloose_has_no_consistency_curve():
    from gnss_ins_sim.sim import ins_sim
    assert hasattr(ins_sim.Sim, 'consistency_curve')
    import inspect
    sig = inspect.signature(ins_sim.Sim.consistency_curve)
    assert [p.kind for p in sig.parameters.values()][1:] == [inspect.Parameter.KEYWORD_ONLY] * 2
    assert list(sig.parameters)[1:] == ['every', 'samples']
    doc = ins_sim.Sim.consistency_curve.__doc__
    assert all(u in doc for u in ('m/s', 'rad', 'rad/s', 'm/s^2'))
