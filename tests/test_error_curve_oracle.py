"""Error-growth curves without a device: the NumPy restatement (tests/error_curve_ref.py) on the C oracle's series against the
executed reference (tests/golden/error_curve/*.npz, made by tests/golden/make_golden_error_curve.py), the C ABI's three new entry
points, and ginsim_curve_merge (host only) against NumPy."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import load_golden, REPO, PKG
from oracle import c_oracle
import error_curve_cases
import error_curve_ref

R2D = 180.0 / np.pi
NEW = ('ginsim_error_curve', 'ginsim_error_curve_f32', 'ginsim_curve_merge')


def _errs(g):
    acc = {k[6:]: g[k] for k in g if k.startswith('accel_') and k != 'accel'}
    gyr = {k[5:]: g[k] for k in g if k.startswith('gyro_') and k != 'gyro'}
    return acc, gyr


def _oracle_series(g, algo, odo_err):
    truth = {k: g[k] for k in ('ref_accel', 'ref_gyro', 'ref_att', 'ref_pos', 'ref_vel')}
    if 'ref_odo' in g:
        truth['ref_odo'] = g['ref_odo']
    acc, gyr = _errs(g)
    R = int(g['R'])
    _, traj, _ = c_oracle.mc_run(int(g['seed']), 0, R, float(g['fs']), int(g['ref_frame']), truth, acc, gyr, g['ini'], algo=algo,
                                 odo_err=odo_err, keep=R)
    return traj, np.concatenate([g['ref_att'], g['ref_pos'], g['ref_vel']], axis=1)


@pytest.mark.parametrize('case', sorted(error_curve_cases.CASES))
def test_restatement_on_the_oracle_series_equals_the_reference_curve(case):
    """Every record of every sample, within the golden's own bound (16 x max(long-double distance, spread over eight permutations
    of the run order, eps |q|), measured on the reference's series when the golden was made): attitude and position, NED included,
    are held to that bound alone.  The velocity is not: the C oracle's velocity series is not bit-identical to the reference's
    (one unit in the last place of the 10 m/s speed, which the rotation into the navigation frame spreads over the three
    components), and a bound that goes down to 1e-17 m/s cannot absorb a difference of the INPUT.  Its records get, added to the
    golden's bound, 4 units in the last place of the largest speed of any run at that sample (4 eps max |v| = 8.9e-15 m/s):
    max |e|, the mean and the std over the runs move by no more than the largest change of one error.  Measured when the file
    was written: velocity at most 1.78e-15 m/s from the golden (1.75e-15 beyond its bound), everything else inside the bound."""
    g = load_golden(os.path.join('error_curve', case))
    assert str(g['case']) == case and int(g['R']) == 16 and int(g['n']) == 1000
    assert np.array_equal(g['rows'], np.arange(1000))
    if case.startswith('wrap'):
        assert int(g['wraps']) > 0
    ned = str(g['extra_opt']) == 'ned'
    for a, algo in enumerate(error_curve_cases.ALGOS[case]):
        traj, ref_nav = _oracle_series(g, algo, error_curve_cases.ODO)
        c = error_curve_ref.curve(traj, ref_nav, None, ned)
        speed = np.max(np.linalg.norm(traj[:, :, 6:9], axis=2), axis=0)[:, None]             # (n, 1)
        slack = {'att_euler': 0.0, 'pos': 0.0, 'vel': 4.0 * np.finfo(np.float64).eps * speed}
        for k, name in enumerate(('att_euler', 'pos', 'vel')):
            scale = R2D if name == 'att_euler' else 1.0
            for s in ('max', 'avg', 'std'):
                got, want = c[s][:, 3 * k:3 * k + 3] * scale, g['%s_%s_algo%d' % (name, s, a)]
                bound = g['%s_tol_%s_algo%d' % (name, s, a)]
                d = np.abs(got - want)
                print('%s %s %s %s: max |d| = %.3g, largest |d| - golden bound = %.3g' % (case, algo, name, s, d.max(), (d - bound).max()))
                assert np.all(d <= bound + slack[name]), (case, algo, name, s, float((d - bound - slack[name]).max()))


@pytest.mark.parametrize('name,algos', [('t3_demo_rf1', ('odo', 'free')), ('t3_mid_rf0', ('free',)), ('t3_high_odo_rf0', ('odo', 'free'))])
def test_last_row_equals_the_end_point_statistics_of_the_t3_goldens(name, algos):
    """stat_* of the T3 goldens is get_error_stats(err_stats_start=-1, use_output_units=True) of the executed reference: the last
    row of the curve.  Tolerance of tests/test_oracle_golden.py for the same numbers (rtol 1e-7, atol 1e-12)."""
    g = load_golden(name)
    rf = int(g['ref_frame'])
    odo_err = {'scale': float(g['odo_scale']), 'stdv': float(g['odo_stdv'])} if 'odo' in g else None
    scale = np.concatenate([np.full(3, R2D), np.array([R2D, R2D, 1.0]) if rf == 0 else np.ones(3), np.ones(3)])
    for a, algo in enumerate(algos):
        traj, ref_nav = _oracle_series(g, algo, odo_err)
        n = traj.shape[1]
        c = error_curve_ref.curve(traj, ref_nav, [0, n // 2, n - 1], False)
        for s in ('max', 'avg', 'std'):
            want = np.concatenate([g['stat_%s_%s_algo%d' % (dn, s, a)] for dn in ('att_euler', 'pos', 'vel')])
            np.testing.assert_allclose(c[s][-1] * scale, want, rtol=1e-7, atol=1e-12)
        if rf == 0:
            ned = error_curve_ref.curve(traj, ref_nav, [n - 1], True)
            for s in ('max', 'avg', 'std'):
                np.testing.assert_allclose(ned[s][0, 3:6], g['ned_end_%s_algo%d' % (s, a)], rtol=1e-6, atol=1e-8)


def test_header_declares_and_library_exports_the_new_entry_points():
    import ginsim
    hdr = open(os.path.join(REPO, 'include', 'ginsim.h')).read()
    declared = set(re.findall(r'\b(ginsim_[a-z0-9_]+)\s*\(', hdr))
    raw = C.CDLL(ginsim.LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(raw, name) and name in ginsim.EXPORTS
    assert ginsim.lib.ginsim_abi_version() == 9
    assert 'GINSIM_CURVE_RECORD 4' in hdr
    readme = open(os.path.join(REPO, 'README.md')).read()
    assert '%d entry points' % len(declared) in readme


def _records(e):
    """(m, 9, 4) records of errors (runs, m, 9), as a device would hand them over."""
    if e.shape[0] == 0:
        return np.zeros(e.shape[1:] + (4,))
    with np.errstate(invalid='ignore', over='ignore'):
        fin = np.isfinite(e).all(axis=0)
        mean = np.where(fin, np.mean(np.where(np.isfinite(e), e, 0.0), axis=0), np.sum(e, axis=0))     # +-inf, or NaN for both signs / NaN
        m2 = np.where(fin, np.sum((e - mean) ** 2, axis=0), np.nan)
        mx = np.max(np.abs(e), axis=0)
    return np.stack([np.full(mean.shape, float(e.shape[0])), mean, m2, mx], axis=-1)


@pytest.mark.parametrize('nparts', range(1, 9))
def test_curve_merge_on_random_partitions_follows_numpy(nparts):
    """ginsim_curve_merge (host only, no device) on partitions of unequal counts with an empty part, a part with a NaN and parts
    with +inf and -inf: values against NumPy on the whole, masks equal."""
    import ginsim
    rng = np.random.RandomState(100 + nparts)
    runs, m = 211, 7
    e = rng.standard_normal((runs, m, 9)) * np.array([1e-3] * 3 + [5.0] * 3 + [0.1] * 3) + np.array([0.0] * 3 + [1e6, -2e6, 4e6] + [0.0] * 3)
    e[3, 1, 0] = np.nan
    e[50, 2, 4] = np.inf
    e[60, 3, 5], e[200, 3, 5] = np.inf, -np.inf          # both signs: the mean is NaN
    e[61, 4, 6], e[201, 4, 6] = -np.inf, -np.inf
    cuts = np.sort(rng.choice(np.arange(1, runs), size=nparts - 1, replace=False)) if nparts > 1 else np.array([], dtype=int)
    pieces = np.split(e, cuts)
    if nparts > 2:
        pieces.insert(int(rng.randint(0, nparts)), e[:0])        # an empty part
    got = ginsim.CurveResult.merge([_records(p) for p in pieces])
    with np.errstate(invalid='ignore', over='ignore'):
        want = error_curve_ref.array_stats(e)
        assert np.all(got.count == runs)
        for dev, ref, rtol in ((got.maxabs, want['max'], 0.0), (got.mean, want['avg'], 1e-12), (got.std, want['std'], 1e-9)):
            np.testing.assert_array_equal(np.isnan(dev), np.isnan(ref))
            np.testing.assert_array_equal(np.isposinf(dev), np.isposinf(ref))
            np.testing.assert_array_equal(np.isneginf(dev), np.isneginf(ref))
            fin = np.isfinite(ref)
            np.testing.assert_allclose(dev[fin], ref[fin], rtol=rtol, atol=1e-9 if rtol else 0.0)
    assert np.isnan(want['avg']).sum() == 2 and np.isinf(want['avg']).sum() == 2 and np.isnan(want['std']).sum() == 4
    # records that hold no non-finite value do not see the others: their bits are those of the merge of the clean parts
    clean = np.where(np.isfinite(e), e, 0.0)
    ref = ginsim.CurveResult.merge([_records(p) for p in np.split(clean, cuts)])
    ok = np.isfinite(want['avg'])
    assert np.array_equal(got.mean[ok], ref.mean[ok]) and np.array_equal(got.m2[ok], ref.m2[ok])


def test_curve_merge_of_empty_parts_and_bad_arguments():
    import ginsim
    from ginsim import _lib
    z = ginsim.CurveResult.merge([np.zeros((3, 9, 4)), np.zeros((3, 9, 4))])
    assert np.all(z.pack() == 0.0) and z.m == 3
    one = _records(np.random.RandomState(0).standard_normal((5, 3, 9)))
    same = ginsim.CurveResult.merge([np.zeros((3, 9, 4)), one, np.zeros((3, 9, 4))])
    assert np.array_equal(same.pack(), one)
    assert np.array_equal(ginsim.CurveResult.unpack(same.pack()).pack(), one)
    out = np.empty((3, 9, 4))
    assert _lib.lib.ginsim_curve_merge(_lib.dptr(one), 0, 3, _lib.dptr(out)) == _lib.ERR_ARG
    assert _lib.lib.ginsim_curve_merge(_lib.dptr(one), 1, 0, _lib.dptr(out)) == _lib.ERR_ARG
    assert _lib.lib.ginsim_curve_merge(None, 1, 3, _lib.dptr(out)) == _lib.ERR_ARG
    # the device entry points refuse a NULL context before anything is launched
    buf = np.zeros(8)
    assert _lib.lib.ginsim_error_curve(None, buf.ctypes.data, buf.ctypes.data, 1, 1, None, 1, 0, _lib.dptr(out)) == _lib.ERR_ARG
    assert _lib.lib.ginsim_error_curve_f32(None, buf.ctypes.data, buf.ctypes.data, 1, 1, None, 1, 0, buf.ctypes.data, 1, 0,
                                           _lib.dptr(out)) == _lib.ERR_ARG


def test_the_restatement_is_imported_by_tests_only():
    """`import ginsim` on the product path pulls in nothing from oracle or from the tests' restatement."""
    for root, _, files in os.walk(PKG):
        for f in files:
            if f.endswith(('.py', '.hip', '.hpp', '.cpp', '.h')):
                src = open(os.path.join(root, f)).read()
                assert 'error_curve_ref' not in src and 'error_curve_cases' not in src, f
    for f in ('bench.py', '__graft_entry__.py', os.path.join('examples', 'demo_error_growth.py')):
        assert 'error_curve_ref' not in open(os.path.join(REPO, f)).read(), f
    import subprocess
    import sys
    code = ("import sys; sys.path[:0] = [%r]; import ginsim; bad = [m for m in sys.modules if m.split('.')[0] in ('oracle', "
            "'error_curve_ref', 'error_curve_cases')]; assert not bad, bad" % PKG)
    subprocess.run([sys.executable, '-c', code], check=True, timeout=120)
