"""Error quantiles across runs without a device: the C ABI's three new entry points and their refusals through the built library,
the NumPy restatement (tests/error_quantiles_ref.py) against np.quantile(method='inverted_cdf') and against ranks worked out by
hand, and the build's resource report of csrc/error_quantile.hip."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO, PKG
import error_quantiles_ref as ref

NEW = ('ginsim_radial_keys', 'ginsim_radial_keys_f32', 'ginsim_quantile_rows')


def test_header_declares_and_library_exports_the_new_entry_points():
    import ginsim
    hdr = open(os.path.join(REPO, 'include', 'ginsim.h')).read()
    declared = set(re.findall(r'\b(ginsim_[a-z0-9_]+)\s*\(', hdr))
    raw = C.CDLL(ginsim.LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(raw, name) and name in ginsim.EXPORTS
        assert getattr(ginsim.lib, name).argtypes is not None
    assert ginsim.lib.ginsim_abi_version() == 9
    assert 'GINSIM_QUANTILE_MAX_PROBS 8' in hdr
    readme = open(os.path.join(REPO, 'README.md')).read()
    assert '%d entry points' % len(declared) in readme
    assert callable(ginsim.quantile_rows) and ginsim.QuantileResult._fields == ('values', 'count')
    for cls in (ginsim.MonteCarloJob, ginsim.InsLooseJob):
        assert callable(cls.radial_keys) and callable(cls.error_quantiles)


def _refused(rc, prefix):
    from ginsim import _lib
    msg = _lib.lib.ginsim_last_error().decode()
    return rc == _lib.ERR_ARG and msg.startswith(prefix + ':'), (rc, msg)


def test_radial_keys_refusals_come_before_a_device_is_needed():
    """Every refusal on a NULL context or, where the context must not be NULL for the check to be reached, on a pointer that is
    never followed: nothing is launched, no device is asked for."""
    from ginsim import _lib
    L = _lib.lib
    buf = np.zeros(16)
    p = buf.ctypes.data                                 # stands for a context, a trajectory, the truth and the keys
    ids = lambda *v: np.array(v, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))          # noqa: E731
    n, runs = 4, 2
    good = dict(c=p, traj=p, ref=p, n=n, runs=runs, samples=ids(0, 3), m=2, which=0, ned=0, keys=p, stride=runs, col0=0)
    cases = [dict(c=None), dict(traj=None), dict(ref=None), dict(keys=None),
             dict(m=0), dict(m=-1), dict(samples=None, m=2),
             dict(samples=ids(0, 4)), dict(samples=ids(-1, 0)),
             dict(which=2), dict(which=-1),
             dict(stride=runs - 1), dict(col0=1, stride=runs), dict(col0=-1, stride=runs + 1)]
    for change in cases:
        a = dict(good, **change)
        rc = L.ginsim_radial_keys(a['c'], a['traj'], a['ref'], a['n'], a['runs'], a['samples'], a['m'], a['which'], a['ned'], a['keys'],
                                  a['stride'], a['col0'])
        ok, seen = _refused(rc, 'radial_keys')
        assert ok, (change, seen)
        rc = L.ginsim_radial_keys_f32(a['c'], a['traj'], a['ref'], a['n'], a['runs'], a['samples'], a['m'], a['which'], a['ned'], p, 1, 0,
                                      a['keys'], a['stride'], a['col0'])
        ok, seen = _refused(rc, 'radial_keys_f32')
        assert ok, (change, seen)
    for origin, n_ini in ((None, 1), (p, 0)):           # the fp32 form without its origin table
        rc = L.ginsim_radial_keys_f32(p, p, p, n, runs, ids(0, 3), 2, 0, 0, origin, n_ini, 0, p, runs, 0)
        ok, seen = _refused(rc, 'radial_keys_f32')
        assert ok, seen


def test_quantile_rows_refusals_come_before_a_device_is_needed():
    from ginsim import _lib
    L = _lib.lib
    buf, out, cnt = np.zeros(16), np.zeros(16), np.zeros(4)
    p = buf.ctypes.data
    pr = lambda *v: _lib.dptr(np.array(v, dtype=np.float64))                                    # noqa: E731
    good = dict(c=p, keys=p, rows=2, len=4, stride=4, probs=pr(0.5, 0.95), q=2, out=_lib.dptr(out), cnt=_lib.dptr(cnt))
    cases = [dict(c=None), dict(keys=None), dict(probs=None), dict(out=None), dict(cnt=None),
             dict(rows=0), dict(rows=-3), dict(len=0), dict(stride=3),
             dict(q=0), dict(q=9, probs=pr(*([0.5] * 9))), dict(q=-1),
             dict(probs=pr(0.0, 0.5)), dict(probs=pr(0.5, -0.1)), dict(probs=pr(1.5, 0.5)), dict(probs=pr(0.5, 1.0000000000000002)),
             dict(probs=pr(np.nan, 0.5)), dict(probs=pr(0.5, np.inf))]
    for change in cases:
        a = dict(good, **change)
        rc = L.ginsim_quantile_rows(a['c'], a['keys'], a['rows'], a['len'], a['stride'], a['probs'], a['q'], a['out'], a['cnt'])
        ok, seen = _refused(rc, 'quantile_rows')
        assert ok, (change, seen)
    assert np.all(out == 0.0) and np.all(cnt == 0.0)


@pytest.mark.parametrize('seed', range(6))
def test_nearest_rank_of_the_restatement_is_numpys_inverted_cdf(seed):
    rng = np.random.RandomState(seed)
    for _ in range(40):
        N = int(rng.choice([1, 2, 3, 7, 64, 65, 100, 257, 1000, 4097]))
        row = np.exp(rng.standard_normal(N) * 2.0)
        if rng.rand() < 0.3:
            row[rng.randint(0, N, size=N // 3)] = row[0]                # ties
        probs = np.concatenate([rng.uniform(1e-6, 1.0, size=5), [1.0, 0.5, 0.95]])
        got, count = ref.nearest_rank(row, probs)
        want = np.quantile(row, probs, method='inverted_cdf')
        assert count == N
        assert got.tobytes() == want.tobytes(), (N, probs, got, want)


def test_nearest_rank_pinned_by_hand():
    row = np.random.RandomState(1).permutation(64).astype(np.float64) + 1.0             # the values 1 .. 64: the k-th smallest is k
    N = row.size
    got, count = ref.nearest_rank(row, [0.5, 1.0 / N, 1.0, 1e-300, 33.0 / 64.0, 0.5 + 2.0 ** -40])
    # p N = 32 exactly -> the 32nd; 1 -> the 1st; 64 -> the 64th; ceil(tiny) = 1 -> the 1st; 33 -> the 33rd; just above 32 -> the 33rd
    assert count == 64 and got.tolist() == [32.0, 1.0, 64.0, 1.0, 33.0, 33.0]
    # keys that are not finite are left out: N drops and the ranks are those of the rest
    poisoned = np.concatenate([row, [np.nan, np.inf, np.nan]])
    got, count = ref.nearest_rank(poisoned, [0.5, 1.0])
    assert count == 64 and got.tolist() == [32.0, 64.0]
    got, count = ref.nearest_rank([np.nan, np.inf], [0.5])
    assert count == 0 and np.isnan(got).all()
    values, counts = ref.quantile_rows(np.stack([row, row[::-1] * 2.0]), [0.5, 1.0])
    assert values.tolist() == [[32.0, 64.0], [64.0, 128.0]] and counts.tolist() == [64.0, 64.0]


def test_keys_of_the_restatement_pinned_by_hand():
    """Errors (3, 4, 12) in position and (-0.3, 0.4, -1.2) in velocity at every sample of two runs: 5 / 12 / 13 and 0.5 / 1.2 / 1.3."""
    n, runs = 5, 2
    rng = np.random.RandomState(3)
    ref_nav = rng.standard_normal((n, 9)) * 100.0
    traj = np.broadcast_to(ref_nav, (runs, n, 9)).copy()
    traj[:, :, 3:6] += [3.0, 4.0, 12.0]
    traj[1, :, 3:6] -= [6.0, 8.0, 24.0]                      # the second run: the same radius on the other side
    traj[:, :, 6:9] += [-0.3, 0.4, -1.2]
    k = ref.keys(traj, ref_nav, [4, 0, 0], 0, False)
    assert k.shape == (3, 3, runs)
    np.testing.assert_allclose(k, np.array([5.0, 12.0, 13.0]).reshape(3, 1, 1) * np.ones((3, 3, runs)), rtol=1e-12)
    k = ref.keys(traj, ref_nav, None, 1, True)              # ned says nothing about the velocity
    np.testing.assert_allclose(k, np.array([0.5, 1.2, 1.3]).reshape(3, 1, 1) * np.ones((3, n, runs)), rtol=1e-12)
    tol = ref.key_tolerance(k, 1, True)
    assert tol.shape == k.shape and np.all(tol[1] < 1.1e-9) and np.all(tol[2] > np.sqrt(3.0) * 1e-9)
    assert np.all(ref.key_tolerance(ref.keys(traj, ref_nav, None, 0, False), 0, True)[0] > np.sqrt(2.0) * 2e-8)


def test_no_kernel_of_the_file_uses_scratch():
    """The build's resource report of csrc/error_quantile.hip: the select and the four instantiations of the key kernel, none with
    scratch, spills or AGPRs; the select's LDS is the staged row, eight histograms and the per-probability state."""
    path = os.path.join(PKG, 'build', 'error_quantile.resources.txt')
    assert os.path.exists(path), 'run gnss-ins-sim_amd/build.py (it writes %s)' % path
    kernels, cur = {}, None
    for line in open(path):
        k, _, v = line.strip().partition(':')
        if k == 'Function Name':
            cur = kernels.setdefault(v.strip(), {})
        elif cur is not None and v.strip():
            cur[k.split('[')[0].strip()] = v.strip()
    assert sum('radial_keys_kernel' in k for k in kernels) == 4 and sum('quantile_rows_kernel' in k for k in kernels) == 1
    src = open(os.path.join(PKG, 'csrc', 'error_quantile.hip')).read()
    stage = int(re.search(r'kSelStage = (\d+);', src).group(1))
    for name, r in kernels.items():
        assert int(r['ScratchSize']) == 0 and int(r['AGPRs']) == 0 and int(r['VGPRs Spill']) == 0 and int(r['SGPRs Spill']) == 0, (name, r)
        if 'quantile_rows_kernel' in name:
            assert 8 * stage + 8 * 256 * 4 <= int(r['LDS Size']) <= 8 * stage + 8 * 256 * 4 + 256, r
        else:
            assert int(r['LDS Size']) == 0, (name, r)


def test_the_restatement_is_imported_by_tests_only():
    for root, _, files in os.walk(PKG):
        for f in files:
            if f.endswith(('.py', '.hip', '.hpp', '.cpp', '.h')):
                assert 'error_quantiles_ref' not in open(os.path.join(root, f)).read(), f
    for f in ('bench.py', '__graft_entry__.py', os.path.join('examples', 'demo_cep.py'), os.path.join('tools', 'bench_error_quantiles.py')):
        assert 'error_quantiles_ref' not in open(os.path.join(REPO, f)).read(), f
