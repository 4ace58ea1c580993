"""Error covariance across runs without a device: the C ABI's three new entry points and their refusals through the built library,
the NumPy restatement (tests/error_covariance_ref.py) against np.cov / np.mean and against the executed reference's numbers
(tests/golden/error_curve/*.npz), ginsim_cov_merge (host only) against the restatement, the two host helpers, the CPU measurement
that motivates the feature, and the build's resource report of csrc/error_cov.hip."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import load_golden, REPO, PKG
import error_curve_cases
import error_covariance_cases as cc
import error_covariance_ref as ref
from test_error_curve_oracle import _oracle_series

NEW = ('ginsim_error_cov', 'ginsim_error_cov_f32', 'ginsim_cov_merge')
EPS = np.finfo(np.float64).eps


def test_header_declares_and_library_exports_and_binds_the_new_entry_points():
    import ginsim
    hdr = open(os.path.join(REPO, 'include', 'ginsim.h')).read()
    declared = set(re.findall(r'\b(ginsim_[a-z0-9_]+)\s*\(', hdr))
    raw = C.CDLL(ginsim.LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(raw, name) and name in ginsim.EXPORTS
        assert getattr(ginsim.lib, name).argtypes is not None
    assert ginsim.lib.ginsim_abi_version() == 9
    assert 'GINSIM_COV_RECORD 10' in hdr
    assert len(declared) == 86
    readme = open(os.path.join(REPO, 'README.md')).read()
    assert '86 entry points' in readme
    assert callable(ginsim.track_frame) and callable(ginsim.error_ellipse)
    for f in ('pack', 'unpack', 'merge', 'zero', 'cov'):
        assert hasattr(ginsim.CovResult, f)
    from ginsim import multi, distributed
    for cls in (ginsim.MonteCarloJob, ginsim.InsLooseJob, multi.JobSet):
        assert callable(cls.error_cov)
    assert callable(distributed.allgather_cov)


def _refused(rc, prefix):
    from ginsim import _lib
    msg = _lib.lib.ginsim_last_error().decode()
    return rc == _lib.ERR_ARG and msg.startswith(prefix + ':'), (rc, msg)


def test_error_cov_refusals_come_before_a_device_is_needed():
    """Every refusal on a NULL context or, where the context must not be NULL for the check to be reached, on a pointer that is
    never followed: nothing is launched, no device is asked for."""
    from ginsim import _lib
    L = _lib.lib
    buf, out = np.zeros(16), np.zeros(40)
    p = buf.ctypes.data                                 # stands for a context, a trajectory and the truth
    ids = lambda *v: np.array(v, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))          # noqa: E731
    n, runs = 4, 2
    good = dict(c=p, traj=p, ref=p, n=n, runs=runs, samples=ids(0, 3), m=2, which=0, ned=0, out=_lib.dptr(out))
    cases = [dict(c=None), dict(traj=None), dict(ref=None), dict(out=None),
             dict(n=0), dict(runs=0), dict(runs=-5), dict(m=0), dict(m=-1), dict(samples=None, m=2),
             dict(samples=ids(0, 4)), dict(samples=ids(-1, 0)),
             dict(which=2), dict(which=-1)]
    for change in cases:
        a = dict(good, **change)
        rc = L.ginsim_error_cov(a['c'], a['traj'], a['ref'], a['n'], a['runs'], a['samples'], a['m'], a['which'], a['ned'], a['out'])
        ok, seen = _refused(rc, 'error_cov')
        assert ok, (change, seen)
        rc = L.ginsim_error_cov_f32(a['c'], a['traj'], a['ref'], a['n'], a['runs'], a['samples'], a['m'], a['which'], a['ned'], p, 1, 0,
                                    a['out'])
        ok, seen = _refused(rc, 'error_cov_f32')
        assert ok, (change, seen)
    for origin, n_ini in ((None, 1), (p, 0)):           # the fp32 form without its origin table
        rc = L.ginsim_error_cov_f32(p, p, p, n, runs, ids(0, 3), 2, 0, 0, origin, n_ini, 0, _lib.dptr(out))
        ok, seen = _refused(rc, 'error_cov_f32')
        assert ok, seen
    part = np.zeros((2, 3, 10))
    for a in (dict(parts=None), dict(out=None), dict(nparts=0), dict(nparts=-1), dict(m=0), dict(m=-2)):
        a = dict(dict(parts=_lib.dptr(part), nparts=2, m=3, out=_lib.dptr(out)), **a)
        ok, seen = _refused(L.ginsim_cov_merge(a['parts'], a['nparts'], a['m'], a['out']), 'cov_merge')
        assert ok, (a, seen)
    assert np.all(out == 0.0)


# ------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('seed', range(4))
def test_restatement_is_numpys_cov_and_mean(seed):
    rng = np.random.RandomState(seed)
    runs, m = int(rng.choice([2, 3, 65, 257])), 5
    A = rng.standard_normal((m, 3, 3))
    e = np.einsum('mab,rmb->rma', A, rng.standard_normal((runs, m, 3))) + rng.standard_normal((m, 3)) * 10.0
    for dtype in (np.float64, np.longdouble):
        rec = ref.record(e, dtype)
        assert rec.dtype == dtype and rec.shape == (m, 10) and np.all(rec[:, 0] == runs)
        cov = ref.cov_of(rec)
        for k in range(m):
            np.testing.assert_allclose(cov[k].astype(np.float64), np.cov(e[:, k].T, bias=True), rtol=1e-12, atol=1e-14)
            np.testing.assert_allclose(rec[k, 1:4].astype(np.float64), np.mean(e[:, k], axis=0), rtol=1e-13, atol=1e-15)
    # the non-finite rule: a run with ANY component not finite at a sample is left out of that sample, and of no other
    bad = e.copy()
    bad[1, 2, 0], bad[0, 2, 2], bad[1, 4, 1] = np.nan, np.inf, -np.inf
    rec, clean = ref.record(bad), ref.record(e)
    assert rec[:, 0].tolist() == [runs, runs, runs - 2, runs, runs - 1]
    assert rec[[0, 1, 3]].tobytes() == clean[[0, 1, 3]].tobytes()
    if runs > 3:
        np.testing.assert_allclose(ref.cov_of(rec)[2], np.cov(e[2:, 2].T, bias=True), rtol=1e-12, atol=1e-14)
    none = ref.record(np.full((3, 2, 3), np.nan))
    assert none[:, 0].tolist() == [0.0, 0.0] and np.isnan(none[:, 1:]).all()
    one = ref.record(e[:1])
    assert np.all(one[:, 0] == 1) and np.array_equal(one[:, 1:4], e[0]) and np.all(one[:, 4:] == 0.0)


@pytest.mark.parametrize('case', ['turn_rf1', 'turn_rf0_ned', 'wrap_rf1'])
def test_restatement_on_the_oracle_series_equals_the_reference_curve(case):
    """mean and sqrt(diag(cov)) of the restatement on the C oracle's series (made as tests/test_error_curve_oracle.py makes them)
    against the executed reference's avg and std of the first algorithm, every sample, within the golden's own bounds.  The
    velocity carries what that file documents and adds for it: the C oracle's velocity series is not bit-identical to the
    reference's (one unit in the last place of the 10 m/s speed), a difference of the INPUT of 4 eps max |v| that a bound going
    down to 1e-17 m/s cannot absorb."""
    g = load_golden(os.path.join('error_curve', case))
    ned = str(g['extra_opt']) == 'ned'
    traj, ref_nav = _oracle_series(g, error_curve_cases.ALGOS[case][0], error_curve_cases.ODO)
    speed = np.max(np.linalg.norm(traj[:, :, 6:9], axis=2), axis=0)[:, None]
    for which, name in enumerate(('pos', 'vel')):
        rec = ref.record(ref.errors3(traj, ref_nav, None, which, ned))
        assert np.all(rec[:, 0] == int(g['R']))
        std = np.sqrt(np.einsum('kaa->ka', ref.cov_of(rec)))
        slack = 4.0 * EPS * speed if which else 0.0
        for got, s in ((rec[:, 1:4], 'avg'), (std, 'std')):
            want, bound = g['%s_%s_algo0' % (name, s)], g['%s_tol_%s_algo0' % (name, s)]
            d = np.abs(got - want)
            print('%s %s %s: max |d| = %.3g, largest |d| - golden bound = %.3g' % (case, name, s, d.max(), (d - bound).max()))
            assert np.all(d <= bound + slack), (case, name, s, float((d - bound - slack).max()))


# ------------------------------------------------------------------------------------------ the host merge
@pytest.mark.parametrize('nparts', range(1, 8))
def test_cov_merge_on_partitions_follows_the_restatement(nparts):
    """ginsim_cov_merge (host only) on partitions of unequal counts with an empty part, a one-run part and a part whose runs are
    all left out: merged equals whole within the record's own bound, and equals the restated merge of the same parts."""
    import ginsim
    rng = np.random.RandomState(200 + nparts)
    runs, m = 211, 6
    A = rng.standard_normal((m, 3, 3)) * np.array([5.0, 0.1, 1e-3])[None, :, None]
    e = np.einsum('mab,rmb->rma', A, rng.standard_normal((runs, m, 3))) + np.array([10.0, -2.0, 0.0])
    e[5, 1, 0], e[9, 1, 2] = np.nan, np.inf                 # left out of sample 1
    e[100:104] = np.nan                                     # four runs left out of every sample
    cuts = sorted(set([100, 104][:max(0, nparts - 1)] + list(rng.choice(np.arange(1, runs), size=max(0, nparts - 3), replace=False))))
    pieces = np.split(e, cuts)
    if nparts > 1:
        pieces.insert(int(rng.randint(0, len(pieces))), e[:0])          # an empty part
        pieces = [pieces[0][:1], pieces[0][1:]] + pieces[1:]            # a one-run part
    packed = [ref.record(p) if p.shape[0] else np.zeros((m, 10)) for p in pieces]
    if nparts > 2:
        assert any(np.all(p[:, 0] == 0) and np.isnan(p[:, 1:]).all() for p in packed)          # the part of left-out runs only
    got = ginsim.CovResult.merge(packed)
    b = ref.bounded(e)
    assert b['rec'][:, 0].tolist() == [207.0, 205.0] + [207.0] * 4
    ref.assert_record(got.pack(), b, 'merge of %d parts' % len(pieces))
    again = ref.merge(packed)
    np.testing.assert_allclose(got.pack(), again, rtol=64 * EPS, atol=0.0)
    np.testing.assert_array_equal(got.cov, ref.cov_of(got.pack()))
    assert np.array_equal(ginsim.CovResult.unpack(got.pack()).pack(), got.pack())


def test_cov_merge_of_empty_and_single_parts():
    import ginsim
    z = ginsim.CovResult.merge([np.zeros((3, 10)), ginsim.CovResult.zero(3).pack()])
    assert np.all(z.count == 0) and np.isnan(z.mean).all() and np.isnan(z.comoment).all() and np.isnan(z.cov).all() and z.m == 3
    one = ref.record(np.random.RandomState(0).standard_normal((5, 3, 3)))
    same = ginsim.CovResult.merge([np.zeros((3, 10)), one, z.pack()])
    assert np.array_equal(same.pack(), one)                 # empty parts, all-zero or NaN with count 0, change no bit
    single = ref.record(np.random.RandomState(1).standard_normal((1, 3, 3)))
    assert np.all(single[:, 4:] == 0.0)
    assert np.array_equal(ginsim.CovResult.merge([single, np.zeros((3, 10))]).pack(), single)


# ------------------------------------------------------------------------------------------ the host helpers
@pytest.mark.parametrize('impl', ['ginsim', 'restatement'])
def test_track_frame(impl):
    import ginsim
    fn = ginsim.track_frame if impl == 'ginsim' else ref.track_frame
    rng = np.random.RandomState(4)
    A = rng.standard_normal((7, 3, 3))
    cov = np.einsum('kab,kcb->kac', A, A)
    mean = rng.standard_normal((7, 3))
    m0, c0 = fn(mean, cov, np.zeros(7))
    assert np.array_equal(m0, mean) and np.array_equal(c0, cov)                    # yaw 0 is the identity
    m9, c9 = fn(mean, cov, np.full(7, np.pi / 2))                                    # along = e1, cross = -e0
    np.testing.assert_allclose(m9, np.stack([mean[:, 1], -mean[:, 0], mean[:, 2]], axis=1), atol=1e-15)
    np.testing.assert_allclose(c9[:, 0, 0], cov[:, 1, 1], rtol=1e-14)
    np.testing.assert_allclose(c9[:, 1, 1], cov[:, 0, 0], rtol=1e-14)
    np.testing.assert_allclose(c9[:, 0, 1], -cov[:, 0, 1], rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(c9[:, 0, 2], cov[:, 1, 2], atol=1e-15)               # the vertical row rotates with it
    np.testing.assert_allclose(c9[:, 1, 2], -cov[:, 0, 2], atol=1e-15)
    yaw = rng.uniform(-np.pi, np.pi, size=7)
    m, c = fn(mean, cov, yaw)
    np.testing.assert_allclose(c[:, 0, 0] + c[:, 1, 1], cov[:, 0, 0] + cov[:, 1, 1], rtol=1e-13)
    np.testing.assert_allclose(np.linalg.det(c[:, :2, :2]), np.linalg.det(cov[:, :2, :2]), rtol=1e-11)
    np.testing.assert_allclose(c[:, 2, 2], cov[:, 2, 2], rtol=1e-15)
    np.testing.assert_allclose(c, np.swapaxes(c, 1, 2), atol=1e-15)
    np.testing.assert_allclose(m[:, 0], np.cos(yaw) * mean[:, 0] + np.sin(yaw) * mean[:, 1], atol=1e-15)
    np.testing.assert_allclose(m[:, 1], -np.sin(yaw) * mean[:, 0] + np.cos(yaw) * mean[:, 1], atol=1e-15)
    other = (ref.track_frame if impl == 'ginsim' else ginsim.track_frame)(mean, cov, yaw)
    np.testing.assert_allclose(m, other[0], atol=1e-14)
    np.testing.assert_allclose(c, other[1], atol=1e-13)


@pytest.mark.parametrize('impl', ['ginsim', 'restatement'])
def test_error_ellipse(impl):
    import ginsim
    if impl == 'ginsim':
        fn = lambda c: tuple(float(v) for v in ginsim.error_ellipse(np.asarray(c, dtype=np.float64)))       # noqa: E731
    else:
        fn = ref.error_ellipse
    assert fn([[9.0, 0.0], [0.0, 4.0]]) == (3.0, 2.0, 0.0)                          # a diagonal block
    assert fn([[4.0, 0.0], [0.0, 9.0]]) == (3.0, 2.0, 90.0)
    for deg in (30.0, -60.0, 90.0, 0.0, 135.0):                                     # rank 1: u u^T, |u| = 2
        u = 2.0 * np.array([np.cos(np.radians(deg)), np.sin(np.radians(deg))])
        a, b, az = fn(np.outer(u, u))
        assert abs(a - 2.0) < 1e-14 and b < 1e-7
        want = np.degrees(np.arctan2(u[1], u[0]))
        assert -90.0 < az <= 90.0 and abs((az - want + 90.0) % 180.0 - 90.0) < 1e-12, (deg, az)
    assert fn([[1.0, 2.0], [2.0, 4.0]])[1] == 0.0                                   # exactly singular: the smaller root is exactly 0
    assert fn([[2.5, 0.0], [0.0, 2.5]]) == (np.sqrt(2.5), np.sqrt(2.5), 0.0)        # the circle
    a, b, az = fn([[1.0, 1.0 + 1e-15], [1.0 + 1e-15, 1.0]])                         # a smaller root that is (slightly) negative
    assert b == 0.0 and not np.isnan(a) and az == 45.0
    if impl == 'ginsim':
        many = ginsim.error_ellipse(np.array([[[9.0, 0.0], [0.0, 4.0]], [[1.0, 2.0], [2.0, 4.0]]]))
        assert many[0].tolist() == [3.0, np.sqrt(5.0)] and many[1].tolist() == [2.0, 0.0]
        assert abs(many[2][1] - np.degrees(np.arctan2(2.0, 1.0))) < 1e-12
        assert '39.3' in ginsim.error_ellipse.__doc__ and 'sqrt(-2 ln(1 - p))' in ginsim.error_ellipse.__doc__


# ------------------------------------------------------------------------------------------ the motivation
def test_the_odometer_leaves_a_strip_across_the_track():
    """The issue's table, recomputed by the restatement (tests/error_covariance_cases.py has the set-up and the numbers measured
    here).  Asserted: with the odometer alone the along-track sigma at the outage's end is below a quarter of the cross-track
    sigma -- while the two per-axis sigmas show nothing of it."""
    rows = {}
    for mask in (0, 1, 7):
        e, yaw = cc.motivation_errors(mask)
        rec = ref.record(e[:, None, :])
        cov = ref.cov_of(rec)
        _, tc = ref.track_frame(rec[:, 1:4], cov, [yaw])
        sx, sy = np.sqrt(cov[0, 0, 0]), np.sqrt(cov[0, 1, 1])
        rows[mask] = (sx, sy, cov[0, 0, 1] / (sx * sy), np.sqrt(tc[0, 0, 0]), np.sqrt(tc[0, 1, 1])) + ref.error_ellipse(cov[0, :2, :2])
        print('mask %d (yaw %.1f deg): sx %.3f sy %.3f rho %.3f along %.3f cross %.3f ellipse %.3f x %.3f at %.1f deg' % ((mask, np.degrees(yaw)) + rows[mask]))
    along, cross = rows[1][3], rows[1][4]
    assert along < 0.25 * cross, (along, cross)


# ------------------------------------------------------------------------------------------ the build's report
def test_no_kernel_of_the_file_uses_scratch_or_spills():
    """The build's resource report of csrc/error_cov.hip: the four instantiations of cov_partial_kernel and cov_final_kernel, none
    with scratch, spills, AGPRs or LDS."""
    path = os.path.join(PKG, 'build', 'error_cov.resources.txt')
    assert os.path.exists(path), 'run gnss-ins-sim_amd/build.py (it writes %s)' % path
    kernels, cur = {}, None
    for line in open(path):
        k, _, v = line.strip().partition(':')
        if k == 'Function Name':
            cur = kernels.setdefault(v.strip(), {})
        elif cur is not None and v.strip():
            cur[k.split('[')[0].strip()] = v.strip()
    assert sum('cov_partial_kernel' in k for k in kernels) == 4 and sum('cov_final_kernel' in k for k in kernels) == 1
    for name, r in kernels.items():
        assert int(r['ScratchSize']) == 0 and int(r['AGPRs']) == 0 and int(r['VGPRs Spill']) == 0 and int(r['SGPRs Spill']) == 0, (name, r)
        assert int(r['LDS Size']) == 0 and r['Dynamic Stack'] == 'False', (name, r)


def test_the_restatement_is_imported_by_tests_only():
    for root, _, files in os.walk(PKG):
        for f in files:
            if f.endswith(('.py', '.hip', '.hpp', '.cpp', '.h')):
                src = open(os.path.join(root, f)).read()
                assert 'error_covariance_ref' not in src and 'error_covariance_cases' not in src, f
    for f in ('bench.py', '__graft_entry__.py', os.path.join('examples', 'demo_error_ellipse.py'),
              os.path.join('tools', 'bench_error_covariance.py')):
        assert 'error_covariance_ref' not in open(os.path.join(REPO, f)).read(), f
