"""Error quantiles across runs on the device (csrc/error_quantile.hip, ginsim_radial_keys*, ginsim_quantile_rows,
BatchJob.radial_keys / error_quantiles, Sim.error_quantiles) against the NumPy restatement tests/error_quantiles_ref.py.

The select is exact: every value is compared bit for bit.  The keys carry the component tolerance of tests/test_gpu_error_curve.py
(1e-9, 2e-8 for NED metres) propagated to the key -- sqrt(2) of it for the horizontal key, 1 for the vertical, sqrt(3) for the 3-D
key -- plus 4 units in the last place of the key (error_quantiles_ref.key_tolerance).  Measured on the MI355X (each comparison
prints its figure): NED position keys at most 0.151 of that tolerance (3.0e-9 m: the geodetic conversion), every other key within
5.6e-17 of the restatement."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, PKG
import error_quantiles_ref as ref

pytestmark = pytest.mark.gpu

FS = 100.0
STAGE = int(re.search(r'kSelStage = (\d+);', open(os.path.join(PKG, 'csrc', 'error_quantile.hip')).read()).group(1))
PROBS8 = (0.5, 0.95, 1.0, 1e-9, 0.25, 0.999, 0.05, 0.75)


@pytest.fixture(scope='module')
def ctx():
    import ginsim
    c = ginsim.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------ 1. the select alone
def _rows(length, seed):
    """Seven rows of `length` keys: log-normal; all equal; two distinct values; keys that differ in the lowest mantissa bit only;
    keys that differ in the top exponent bits only; 0.0 and denormals among normals; log-normal with NaN and +inf sprinkled in."""
    rng = np.random.RandomState(seed)
    logn = np.exp(rng.standard_normal(length) * 1.5 + 2.0)
    equal = np.full(length, 3.25)
    two = np.where(rng.rand(length) < 0.3, 7.0, 7.000000000000001)
    low = (np.full(length, 1.7).view(np.uint64) + rng.randint(0, 2, size=length).astype(np.uint64)).view(np.float64)
    top = 1.5 * 2.0 ** rng.choice([-600.0, -88.0, 0.0, 424.0, 936.0], size=length)
    small = np.where(rng.rand(length) < 0.5, rng.choice([0.0, 5e-324, 2.5e-310, 2.2250738585072014e-308], size=length), logn * 1e-3)
    dirty = logn[::-1].copy()
    k = max(1, length // 9) if length > 1 else 0
    bad = rng.choice(length, size=k, replace=False)
    dirty[bad[::2]] = np.nan
    dirty[bad[1::2]] = np.inf
    return np.stack([logn, equal, two, low, top, small, dirty]), k


def _padded(rows, stride, seed):
    """The rows `stride` apart, the gap filled with finite keys that would move every quantile if they were read."""
    out = np.empty((rows.shape[0], stride))
    out[:, :rows.shape[1]] = rows
    out[:, rows.shape[1]:] = np.random.RandomState(seed).choice([1e-300, 1e300, 0.0], size=(rows.shape[0], stride - rows.shape[1]))
    return out


@pytest.mark.parametrize('length', [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, STAGE - 1, STAGE, STAGE + 1, 65537])
def test_select_is_the_restatement_bit_for_bit(ctx, length):
    """Seven rows and eight probabilities, and the first row alone with one probability, with row_stride > len and with
    row_stride = len; the lengths lie on both sides of a wavefront, of the workgroup (1024) and of the LDS-staging limit, 65 537 is
    one past the C2 row.  Two calls give the same bytes."""
    import ginsim
    rows, n_bad = _rows(length, length)
    probs = PROBS8[:3] + (1.0 / length,) + PROBS8[4:]
    want, want_n = ref.quantile_rows(rows, probs)
    assert want_n.tolist() == [length] * 6 + [length - n_bad]
    for stride in (length + 5, length):
        buf = ctx.upload(_padded(rows, stride, 1))
        got = ginsim.quantile_rows(ctx, buf, 7, length, stride, probs)
        assert got.values.shape == (7, 8) and got.count.shape == (7,)
        np.testing.assert_array_equal(got.count, want_n)
        np.testing.assert_array_equal(_bits(got.values), _bits(want), err_msg='len %d stride %d' % (length, stride))
        again = ginsim.quantile_rows(ctx, buf, 7, length, stride, probs)
        assert again.values.tobytes() == got.values.tobytes() and again.count.tobytes() == got.count.tobytes()
        one = ginsim.quantile_rows(ctx, buf, 1, length, stride, [0.95])
        assert one.values.shape == (1, 1) and _bits(one.values)[0, 0] == _bits(want)[0, 1] and one.count[0] == length
        # a row that starts inside the buffer: a device pointer, the last row alone
        last = ginsim.quantile_rows(ctx, buf.ptr + 6 * stride * 8, 1, length, stride, probs)
        np.testing.assert_array_equal(_bits(last.values)[0], _bits(want)[6])
        buf.free()


@pytest.mark.parametrize('length', [65, STAGE + 1])
def test_keys_that_are_not_finite_lower_the_count_of_their_row_only(ctx, length):
    """NaN and +inf in one row: its count drops by exactly their number, every other row keeps its bytes; a row without a finite
    key has count 0 and NaN values."""
    import ginsim
    rows, _ = _rows(length, 5)
    clean = rows[:6]
    pois = clean.copy()
    pois[2, [0, length // 2, length - 1]] = [np.nan, np.inf, np.nan]
    pois[4, :] = np.nan
    pois[4, 1::2] = np.inf
    a, b = ctx.upload(clean), ctx.upload(pois)
    ga = ginsim.quantile_rows(ctx, a, 6, length, length, PROBS8)
    gb = ginsim.quantile_rows(ctx, b, 6, length, length, PROBS8)
    want, want_n = ref.quantile_rows(pois, PROBS8)
    assert gb.count.tolist() == [length, length, length - 3, length, 0, length] == want_n.tolist()
    keep = [0, 1, 3, 5]
    assert ga.values[keep].tobytes() == gb.values[keep].tobytes()
    assert np.isnan(gb.values[4]).all()
    np.testing.assert_array_equal(_bits(gb.values)[[0, 1, 2, 3, 5]], _bits(want)[[0, 1, 2, 3, 5]])
    a.free()
    b.free()


# ------------------------------------------------------------------------------------------ 2. the keys
def _job(ctx, rf, runs, precision='f64', seed=20261019, **kw):
    import ginsim
    from ginsim import workloads
    ini, truth, _ = workloads.truth_from_profile('turn_90deg', FS, rf)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    return ginsim.MonteCarloJob(ctx, FS, rf, truth, acc, gyr, ini, runs=runs, seed=seed, keep_traj=True, precision=precision, **kw).run()


def _series(job, algo):
    att, pos, vel = job.trajectories(algo, np.arange(job.runs))
    return np.concatenate([att, pos, vel], axis=2)


def _keys(job, algo, samples, which, **kw):
    buf = job.radial_keys(algo, samples, which, **kw)
    m = job.n if samples is None else len(samples)
    out = job.ctx.download(buf, (3, m, buf.nbytes // (24 * m)))
    buf.free()
    return out


def _assert_keys(got, want, which, ned, what):
    assert got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(np.isfinite(got), np.isfinite(want), err_msg=what)
    fin = np.isfinite(want)
    tol = ref.key_tolerance(want, which, ned)
    d = np.where(fin, np.abs(np.where(fin, got, 0.0) - np.where(fin, want, 0.0)), 0.0)
    print('%s: largest |d| / tol = %.3g (|d| %.3g)' % (what, np.max(d / np.where(fin, tol, 1.0)), d.max()))
    assert np.all(got[fin] >= 0.0)
    worst = np.unravel_index(np.argmax(d - np.where(fin, tol, 0.0)), d.shape)
    assert d[worst] <= tol[worst], '%s: key %s is %.3e from the restatement, tolerance %.3e' % (what, worst, d[worst], tol[worst])


def _sample_sets(n, seed):
    shuffled = np.random.RandomState(seed).randint(0, n, size=37)
    shuffled[5], shuffled[20] = shuffled[4], shuffled[0]                   # repeats
    return (('all', None), ('stride', np.arange(3, n, 7)), ('shuffled', shuffled), ('last', np.array([n - 1])))


@pytest.mark.parametrize('rf', [1, 0])
@pytest.mark.parametrize('precision', ['f64', 'f32'])
@pytest.mark.parametrize('runs', [1, 63, 64, 65, 1000])
def test_keys_against_the_restatement_on_the_downloaded_trajectories(ctx, runs, precision, rf):
    job = _job(ctx, rf, runs, precision)
    assert job.n == 1000
    series, ned = _series(job, 'free'), rf == 0
    for which in (0, 1):
        want = ref.keys(series, job._ref_nav, None, which, ned)
        for name, rows in _sample_sets(job.n, runs):
            got = _keys(job, 'free', rows, which)
            _assert_keys(got, want if rows is None else want[:, rows], which, ned, 'rf%d %s %d which %d %s' % (rf, precision, runs, which, name))
    job.release()


@pytest.mark.parametrize('precision,rf', [('f64', 1), ('f32', 0)])
def test_two_jobs_fill_one_row_through_col0(ctx, precision, rf):
    """The runs 0..99 and 100..256 of a 257-run batch as jobs of their own (the counter RNG reproduces them) write their columns of
    one buffer: bit for bit the keys of the whole batch; the gap of a wider row_stride is left alone."""
    whole = _job(ctx, rf, 257, precision)
    a = _job(ctx, rf, 100, precision)
    b = _job(ctx, rf, 157, precision, run_offset=100, ini_first=100)
    rows = np.arange(0, whole.n, 50)
    m, stride = rows.size, 257 + 3
    for which in (0, 1):
        want = _keys(whole, 'free', rows, which)
        out = ctx.upload(np.full((3, m, stride), -7.0))
        assert a.radial_keys('free', rows, which, out=out, col0=0) is out
        b.radial_keys('free', rows, which, out=out, col0=100)
        got = ctx.download(out, (3, m, stride))
        assert got[:, :, :257].tobytes() == want.tobytes()
        assert np.all(got[:, :, 257:] == -7.0)
        with pytest.raises(ValueError, match='radial_keys'):
            b.radial_keys('free', rows, which, out=out, col0=104)             # 104 + 157 > 260
        out.free()
    q = whole.error_quantiles('free', rows, 0, (0.5, 0.95))
    want, count = ref.quantile_rows(_keys(whole, 'free', rows, 0).reshape(3 * m, 257), (0.5, 0.95))
    assert q.values.shape == (3, m, 2) and q.count.shape == (3, m) and np.all(q.count == 257)
    np.testing.assert_array_equal(_bits(q.values).reshape(3 * m, 2), _bits(want))
    for j in (whole, a, b):
        j.release()


def test_bad_arguments_are_refused(ctx):
    import ginsim
    from ginsim import workloads
    job = _job(ctx, 1, 8)
    for bad in ([], [-1], [job.n], [0, 5, job.n]):
        with pytest.raises(ValueError, match='radial_keys'):
            job.radial_keys('free', bad)
    with pytest.raises(ValueError, match='which=2'):
        job.radial_keys('free', [0], 2)
    with pytest.raises(ValueError, match='col0'):
        job.radial_keys('free', [0], 0, col0=-1)
    with pytest.raises(ValueError, match='probability'):
        job.error_quantiles('free', [0], 0, (0.5, 0.0))
    with pytest.raises(ValueError, match='q=9'):
        job.error_quantiles('free', [0], 0, [0.5] * 9)
    job.release()
    ini, truth, _ = workloads.truth_from_profile('turn_90deg', FS, 1)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    nokeep = ginsim.MonteCarloJob(ctx, FS, 1, truth, acc, gyr, ini, runs=8).run()
    with pytest.raises(ValueError, match='keep_traj=True'):
        nokeep.radial_keys('free')
    with pytest.raises(ValueError, match='keep_traj=True'):
        nokeep.error_quantiles('free')
    nokeep.release()


@pytest.mark.parametrize('rf', [1, 0])
def test_keys_of_an_ins_loose_job(ctx, rf):
    """InsLooseJob(keep_traj=True), 65 runs: the keys of 'traj_loose' are the restatement's on the job's own trajectories()."""
    import ginsim
    import ins_loose_cases as cs
    ini, truth, _ = cs.outage_truth(FS, rf, 10.0, 1500)
    acc_e, gyr_e = cs.imu_errors()
    job = ginsim.InsLooseJob(ctx, FS, rf, truth, acc_e, gyr_e, cs.GPS_ERR, ini, 65, seed=11, keep_traj=True).run()
    series = _series(job, 'loose')
    rows = np.arange(0, job.n, 25)
    for which in (0, 1):
        want = ref.keys(series, job._ref_nav, rows, which, rf == 0)
        _assert_keys(_keys(job, 'loose', rows, which), want, which, rf == 0, 'InsLoose rf%d which %d' % (rf, which))
    q = job.error_quantiles(None, rows, 0, (0.5,))
    assert q.values.shape == (3, rows.size, 1) and np.all(q.count == 65)
    job.release()


# ------------------------------------------------------------------------------------------ 3. through Sim
def _loose_sim(runs, keep, rf, **kw):
    sys.path[:0] = [PKG] if PKG not in sys.path else []
    import ins_loose_cases as cs
    from gnss_ins_sim.sim import imu_model, ins_sim
    from demo_algorithms import free_integration
    from demo_algorithms.ins_loose_device import InsLoose
    from ginsim import workloads
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=True)
    ini = workloads.parse_motion(cs.OUTAGE_CSV)[0]
    sim = ins_sim.Sim([FS, 10.0, 0.0], cs.OUTAGE_CSV, ref_frame=rf, imu=imu, algorithm=[free_integration.FreeIntegration(ini), InsLoose()],
                      seed=1234, keep_trajectories=keep, **kw)
    sim.run(runs)
    return sim


def _free_sim(runs, rf=1, seed=99, **kw):
    sys.path[:0] = [PKG] if PKG not in sys.path else []
    from gnss_ins_sim.sim import imu_model, ins_sim
    from demo_algorithms import free_integration
    csv = os.path.join(PKG, 'motion_profiles', 'turn_90deg.csv')
    ini = np.genfromtxt(csv, delimiter=',', skip_header=1, max_rows=1)
    ini[0:2] *= np.pi / 180
    ini[6:9] *= np.pi / 180
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=False)
    sim = ins_sim.Sim([FS, 0.0, 0.0], csv, ref_frame=rf, imu=imu, algorithm=free_integration.FreeIntegration(ini), seed=seed, **kw)
    sim.run(runs)
    return sim


PARTS = ('horizontal', 'vertical', '3d')


@pytest.mark.parametrize('rf', [0, 1])
def test_sim_error_quantiles_of_free_integration_and_ins_loose(rf):
    """257 kept runs of the outage profile: shapes, units, probs and time; every value within the key tolerance of the restatement
    on the Sim's kept series and bit-equal to one key of job.radial_keys; cached, and a copy is handed out."""
    sim = _loose_sim(257, True, rf)
    assert sim.error_quantiles.__kwdefaults__ == {'every': None, 'samples': None}
    t = np.asarray(sim.dmgr.time.data)
    n = t.shape[0]
    rows = np.arange(0, n, 100)
    probs = (0.5, 0.95, 1.0)
    res = sim.error_quantiles(('pos', 'vel'), probs, every=1.0)
    assert sorted(res) == ['pos', 'vel']
    names = sim.mc.nav_names
    assert len(names) == 2
    for which, nm in enumerate(('pos', 'vel')):
        r = res[nm]
        assert sorted(r) == ['3d', 'count', 'horizontal', 'probs', 'time', 'units', 'vertical']
        assert r['units'] == (['m'] if nm == 'pos' else ['m/s'])
        np.testing.assert_array_equal(r['probs'], probs)
        np.testing.assert_array_equal(r['time'], t[rows])
        for a in names:
            job, kind = sim.mc.job_of(a), sim.mc.kinds[sim.mc.algo_names.index(a)]
            assert r['count'][a].shape == (rows.size,) and np.all(r['count'][a] == 257)
            want_keys = ref.keys(_series(job, kind), job._ref_nav, rows, which, rf == 0)
            dev_keys = _keys(job, kind, rows, which)
            want, _ = ref.quantile_rows(want_keys.reshape(-1, 257), probs)
            tol = ref.key_tolerance(want.reshape(3, rows.size, 3), which, rf == 0)
            for k, part in enumerate(PARTS):
                got = r[part][a]
                assert got.shape == (rows.size, 3)
                assert np.all(np.abs(got - want.reshape(3, rows.size, 3)[k]) <= tol[k]), (nm, a, part)
                for s in range(rows.size):
                    assert np.isin(_bits(got[s]), _bits(dev_keys[k, s])).all(), (nm, a, part, s)
                assert np.all(np.diff(got, axis=1) >= 0.0)                      # a larger share of the runs, a larger radius
            assert np.all(r['3d'][a] >= r['horizontal'][a]) and np.all(r['3d'][a] >= r['vertical'][a])
    again = sim.error_quantiles('pos', probs, samples=rows)['pos']
    assert again['horizontal'][names[1]] is not res['pos']['horizontal'][names[1]]
    np.testing.assert_array_equal(again['horizontal'][names[1]], res['pos']['horizontal'][names[1]])
    every = sim.error_quantiles('vel', (0.5,))['vel']                             # every sample
    assert every['time'].shape == (n,) and every['3d'][names[0]].shape == (n, 1)
    np.testing.assert_array_equal(every['3d'][names[0]][rows, 0], res['vel']['3d'][names[0]][:, 0])
    # what is refused
    with pytest.raises(ValueError, match="'att_euler' has no error quantiles"):
        sim.error_quantiles(('att_euler',))
    with pytest.raises(ValueError, match='not both'):
        sim.error_quantiles(every=1.0, samples=[0])
    with pytest.raises(ValueError, match='samples must be indices'):
        sim.error_quantiles(samples=[n])
    with pytest.raises(ValueError, match='shorter than one sample'):
        sim.error_quantiles(every=1e-4)
    with pytest.raises(ValueError, match='probability'):
        sim.error_quantiles(probs=(0.5, 1.5))
    for _, job, _ in sim.loose_jobs:
        job.release()


def test_statistics_only_ins_loose_and_sims_without_a_navigation_plugin_are_refused(capsys):
    sim = _loose_sim(64, False, 1)
    with pytest.raises(ValueError, match=r'\(InsLoose\) kept statistics only'):
        sim.error_quantiles()
    sys.path[:0] = [PKG] if PKG not in sys.path else []
    from gnss_ins_sim.sim import imu_model, ins_sim
    from demo_algorithms import inclinometer_device
    csv = os.path.join(PKG, 'motion_profiles', 'turn_90deg.csv')
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=False)
    sim = ins_sim.Sim([FS, 0.0, 0.0], csv, ref_frame=1, imu=imu, algorithm=inclinometer_device.TiltAcc(), seed=1)
    assert sim.error_quantiles() is None and 'Call Sim.run()' in capsys.readouterr().out
    sim.run(8)
    with pytest.raises(ValueError, match='inclinometer'):
        sim.error_quantiles()


BLOCK_BYTES = 1024 * 9 * 8 * 1000           # max_device_bytes that makes _blocks re-integrate 1024 runs of 1000 samples at a time


@pytest.mark.parametrize('rf', [1, 0])
def test_blocked_and_spread_statistics_only_sims_equal_the_kept_sim_bit_for_bit(rf):
    """4096 runs: kept; statistics only, integrated again in four blocks of 1024 that write their column ranges; and the same over
    four contexts on one device, whose columns come through the host.  The counter RNG reproduces the runs and the select does not
    depend on an order: the same bytes.  The keys of every sample (98 MB) are more than this budget: refused with the numbers."""
    kept = _free_sim(4096, rf=rf, keep_trajectories=True)
    whole = kept.error_quantiles(('pos', 'vel'), (0.5, 0.95, 0.999), every=0.1)
    name = kept.mc.nav_names[0]
    blocked = _free_sim(4096, rf=rf, keep_trajectories=False, max_device_bytes=BLOCK_BYTES)
    assert blocked.mc.jobs[0].keep_traj is False and blocked.mc._block_runs == 1024
    spread = _free_sim(4096, rf=rf, keep_trajectories=False, max_device_bytes=BLOCK_BYTES, devices=[0, 0, 0, 0])
    assert spread.mc.devices == [0, 0, 0, 0] and spread.mc.jobs[0].keep_traj is False
    kept_spread = _free_sim(4096, rf=rf, keep_trajectories=True, devices=[0, 0, 0, 0])
    for what, sim in (('blocked', blocked), ('spread', spread), ('kept, spread', kept_spread)):
        got = sim.error_quantiles(('pos', 'vel'), (0.5, 0.95, 0.999), every=0.1)
        for nm in ('pos', 'vel'):
            assert np.all(got[nm]['count'][name] == 4096) and got[nm]['count'][name].shape == (100,)
            for part in PARTS:
                assert got[nm][part][name].tobytes() == whole[nm][part][name].tobytes(), (what, nm, part)
    with pytest.raises(ValueError, match=r'1000 samples x 4096 runs are 98304000 bytes .* max_device_bytes = %d' % BLOCK_BYTES):
        blocked.error_quantiles()
    kept.mc.jobs[0].release()
    kept_spread.mc.jobs[0].release()


def test_a_poisoned_run_lowers_the_count_at_its_sample_only():
    """The three position planes of run 77 are NaN at sample 400 of a kept Sim: count is 256 there and 257 at every other sample,
    the position quantiles there are those of the other 256 runs, the velocity's are untouched."""
    import ginsim
    from ginsim import _lib
    sim = _free_sim(257, keep_trajectories=True)
    job = sim.mc.jobs[0]
    n, runs, j, r = job.n, job.runs, 400, 77
    clean = _keys(job, 'free', [j], 0)
    nan = np.array([np.nan])
    for c in (3, 4, 5):
        _lib.check(_lib.lib.ginsim_memcpy_h2d(job.ctx.handle, job.buffer('traj_free').ptr + ((c * n + j) * runs + r) * 8, nan.ctypes.data, 8))
    rows = np.array([0, 399, 400, 401, n - 1])
    res = sim.error_quantiles(('pos', 'vel'), (0.5, 0.95), samples=rows)
    name = sim.mc.nav_names[0]
    assert res['pos']['count'][name].tolist() == [257, 257, 256, 257, 257]
    assert res['vel']['count'][name].tolist() == [257] * 5
    want, count = ref.quantile_rows(np.delete(clean[:, 0], r, axis=1), (0.5, 0.95))
    assert count.tolist() == [256.0] * 3
    for k, part in enumerate(PARTS):
        np.testing.assert_array_equal(_bits(res['pos'][part][name][2]), _bits(want[k]))
    q = job.error_quantiles('free', rows, 0, (0.5, 0.95))
    assert q.count.tolist() == [[257, 257, 256, 257, 257]] * 3
    job.release()


def _port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


_WORKER = r'''
import os, sys
sys.path[:0] = [%(pkg)r, %(repo)r]
import numpy as np, torch.distributed as dist
dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%(port)d', rank=int(sys.argv[1]), world_size=2)
os.environ['LOCAL_RANK'] = '0'
from gnss_ins_sim.sim import imu_model, ins_sim
from demo_algorithms import free_integration
csv = os.path.join(%(pkg)r, 'motion_profiles', 'turn_90deg.csv')
ini = np.genfromtxt(csv, delimiter=',', skip_header=1, max_rows=1)
ini[0:2] *= np.pi / 180; ini[6:9] *= np.pi / 180
imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=False)
sim = ins_sim.Sim([100.0, 0.0, 0.0], csv, ref_frame=1, imu=imu, algorithm=free_integration.FreeIntegration(ini), seed=99, keep_trajectories=False)
sim.run(%(runs)d)
try:
    sim.error_quantiles(every=1.0)
    print('NOT REFUSED')
except NotImplementedError as e:
    print('REFUSED: %%s' %% e)
dist.barrier(); dist.destroy_process_group()
'''


def test_every_rank_of_a_process_group_is_refused(tmp_path):
    """Two gloo ranks sharing the device, one run in all so that rank 1 holds none: both raise NotImplementedError, before any
    collective (a collective entered by one rank only would hang the barrier that follows)."""
    script = tmp_path / 'w.py'
    script.write_text(_WORKER % {'pkg': PKG, 'repo': REPO, 'port': _port(), 'runs': 1})
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env) for r in range(2)]
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
        assert 'REFUSED: error_quantiles: quantiles are not mergeable records' in o and 'not gathered yet' in o, o[-3000:]
