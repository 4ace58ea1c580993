"""The per-step inputs of the wave-specialised fp64 kernel: in the two-producer instantiations the consumer of mc_kernel_split takes
the truth rows of a step from LDS, where the producers staged them tile by tile, and the coefficients of the sensor models in one
batch of scalar loads; the one-producer instantiations (vibration, two algorithms, ref_frame 0) read them as the plain kernel does.

Every case runs the wave-specialised kernel and the plain one (block_threads = 256) on the same parameters and holds every kept
plane and the end-point records equal BIT FOR BIT, and the wave-specialised result to the C oracle at the tolerances of
tests/test_gpu_parity.py.  The truth rows are seeded random numbers on top of the turn, so a row taken one step early or late is
off by ~1e-1, and the eighteen coefficients of the two sensor models are pairwise different, so a swapped one shows.

Shapes: n below, at and above one and two tiles of 6 steps, across the attitude resync at 32 and 64, eleven tiles (both stages
wrap); runs from one lane over partial wavefronts and workgroups with whole inactive wavefronts to three workgroups; run ids
beyond 32 bits; everything / trajectories only / nothing kept.  n x runs is the full 8 x 8 square, the other factors are dealt
over it so that every pair of values of two factors occurs.  The oracle runs once per (n, offset, model, ...) for the largest
batch and is shared: run r of a launch is global run offset + r whatever the batch.
"""
import functools

import numpy as np
import pytest

from conftest import assert_traj_close

pytestmark = pytest.mark.gpu

FS = 100.0
NS = (2, 3, 6, 7, 12, 13, 33, 65)
RUNS = (1, 63, 64, 65, 255, 256, 257, 513)
OFFSETS = (0, 2 ** 32 + 5)
KEEPS = ('all', 'traj', 'none')
ODO_ERR = {'scale': 0.99, 'stdv': 0.1}


@pytest.fixture(scope='module')
def ctx():
    import ginsim
    c = ginsim.Context(0)
    yield c
    c.close()


def _models(wd):
    """18 pairwise different coefficients (gm_a, gm_b, white of three axes of two sensors); wd: a constant bias on every axis and one
    axis of the accelerometer with an infinite correlation time -> the general sensor model (WD = true)"""
    acc = {'b': np.zeros(3), 'b_drift': np.array([5e-3, 7e-3, 9e-3]), 'b_corr': np.array([100.0, 150.0, 250.0]),
           'vrw': np.array([0.03, 0.04, 0.05])}
    gyr = {'b': np.zeros(3), 'b_drift': np.array([1e-4, 2e-4, 3e-4]), 'b_corr': np.array([80.0, 120.0, 300.0]),
           'arw': np.array([1e-3, 1.5e-3, 2e-3])}
    if wd:
        acc['b'] = np.array([0.01, -0.02, 0.03])
        gyr['b'] = np.array([1e-3, -2e-3, 3e-3])
        acc['b_corr'] = np.array([100.0, np.inf, 250.0])
    return acc, gyr


@functools.lru_cache(maxsize=None)
def _truth(rf, n):
    """the first n samples of the turn with seeded random rows added to the specific force and the angular rate"""
    from ginsim import workloads
    ini, truth, _ = workloads.truth_from_profile('turn_90deg', FS, rf)
    t = {k: (v[:n].copy() if hasattr(v, 'shape') and v.shape and v.shape[0] >= n else v) for k, v in truth.items()}
    rng = np.random.default_rng(1000 * rf + n)
    t['ref_accel'] = t['ref_accel'] + rng.normal(0.0, 0.3, (n, 3))
    t['ref_gyro'] = t['ref_gyro'] + rng.normal(0.0, 0.05, (n, 3))
    t['ref_odo'] = t['ref_odo'] + rng.normal(0.0, 0.5, n)
    d = np.abs(np.diff(np.hstack([t['ref_accel'], t['ref_gyro']]), axis=0))
    assert n < 3 or np.median(d) > 1e-3
    return ini, t


def _vib(kind):
    if kind is None:
        return None, None
    if kind == 'random':
        return {'type': 'random', 'x': 0.11, 'y': 0.13, 'z': 0.17}, {'type': 'random', 'x': 0.011, 'y': 0.013, 'z': 0.017}
    return ({'type': 'sinusoidal', 'x': 0.11, 'y': 0.13, 'z': 0.17, 'freq': 7.0},
            {'type': 'sinusoidal', 'x': 0.011, 'y': 0.013, 'z': 0.017, 'freq': 11.0})


ORACLE_RUNS = max(RUNS)


@functools.lru_cache(maxsize=None)
def _oracle(rf, n, off, wd, algo, vib, seed):
    from oracle import c_oracle
    ini, t = _truth(rf, n)
    acc, gyr = _models(wd)
    va, vg = _vib(vib)
    end, traj, sens = c_oracle.mc_run(seed, off, ORACLE_RUNS, FS, rf, t, acc, gyr, ini, algo=algo, odo_err=ODO_ERR, keep=ORACLE_RUNS,
                                      vib_accel=va, vib_gyro=vg)
    for x in (end, traj, sens):
        x.setflags(write=False)
    return end, traj, sens


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def _job(ctx, rf, n, runs, off, wd, keep, algos, vib, seed, plain):
    import ginsim
    ini, t = _truth(rf, n)
    acc, gyr = _models(wd)
    va, vg = _vib(vib)
    job = ginsim.MonteCarloJob(ctx, FS, rf, t, acc, gyr, ini, runs=runs, algos=algos, odo_err=ODO_ERR if 'odo' in algos else None,
                               seed=seed, run_offset=off, keep_sensors=keep == 'all', keep_traj=keep in ('all', 'traj'),
                               vib_accel=va, vib_gyro=vg)
    if plain:
        job.params.block_threads = 256
    return job


def _check(ctx, rf, n, runs, off, wd, keep, algos=('free',), vib=None, seed=77, want=None):
    split = _job(ctx, rf, n, runs, off, wd, keep, algos, vib, seed, False)
    plain = _job(ctx, rf, n, runs, off, wd, keep, algos, vib, seed, True)
    assert 'split' in split.kernel_name() and 'split' not in plain.kernel_name(), (split.kernel_name(), plain.kernel_name())
    if want is not None:
        assert split.kernel_name() == want, split.kernel_name()
    assert split.params.block_threads == 0
    split.run()
    plain.run()
    ids = np.arange(runs)
    what = 'rf %d n %d runs %d off %d wd %d keep %s %s %s' % (rf, n, runs, off, wd, keep, algos, vib)
    for a in algos:
        e_s, e_p = split.end_errors(a), plain.end_errors(a)
        assert np.array_equal(_bits(e_s), _bits(e_p)), what + ': end-point record, ' + a
        end, traj, sens = _oracle(rf, n, off, wd, a, vib, seed)
        d_end = np.abs(np.mod(e_s[:, :3] - end[:runs, :3] + np.pi, 2 * np.pi) - np.pi).max()
        assert d_end <= 1e-9, what
        np.testing.assert_allclose(e_s[:, 3:6], end[:runs, 3:6], rtol=1e-12 if rf == 0 else 0, atol=2e-8, err_msg=what)
        np.testing.assert_allclose(e_s[:, 6:9], end[:runs, 6:9], rtol=0, atol=1e-9, err_msg=what)
        if keep in ('all', 'traj'):
            ts, tp = split.trajectories(a, ids), plain.trajectories(a, ids)
            for k in range(3):
                assert np.array_equal(_bits(ts[k]), _bits(tp[k])), what + ': trajectory plane group %d, %s' % (k, a)
            assert_traj_close(ts[0], ts[1], ts[2], traj[:runs, :, 0:3], traj[:runs, :, 3:6], traj[:runs, :, 6:9], rtol=1e-9, what=what)
    if keep == 'all':
        names = ('accel', 'gyro') + (('odo',) if 'odo' in algos else ())
        for name in names:
            assert np.array_equal(_bits(split.sensors(name, ids)), _bits(plain.sensors(name, ids))), what + ': ' + name
        _, _, sens = _oracle(rf, n, off, wd, algos[0], vib, seed)
        np.testing.assert_allclose(split.sensors('accel', ids), sens[:runs, :, 0:3], rtol=0, atol=1e-12, err_msg=what)
        np.testing.assert_allclose(split.sensors('gyro', ids), sens[:runs, :, 3:6], rtol=0, atol=1e-14, err_msg=what)
    split.release()
    plain.release()


def _square():
    """n x runs in full; offset, kept set and sensor model dealt by i + j so that every pair of values of two factors occurs"""
    cases = []
    for i, n in enumerate(NS):
        for j, runs in enumerate(RUNS):
            s = i + j
            cases.append(pytest.param(n, runs, OFFSETS[s % 2], KEEPS[s % 3], bool((s // 2) % 2),
                                      id='n%d-r%d-o%d-%s-wd%d' % (n, runs, s % 2, KEEPS[s % 3], (s // 2) % 2)))
    return cases


def test_the_square_covers_every_pair():
    """the selection itself: every pair of values of any two of the five factors occurs"""
    rows = [p.values for p in _square()]
    sets = (NS, RUNS, OFFSETS, KEEPS, (False, True))
    for a in range(5):
        for b in range(a + 1, 5):
            assert {(r[a], r[b]) for r in rows} == {(x, y) for x in sets[a] for y in sets[b]}, (a, b)


@pytest.mark.parametrize('n, runs, off, keep, wd', _square())
def test_split_consumer_inputs_match_the_plain_kernel_and_the_oracle(ctx, n, runs, off, keep, wd):
    """ref_frame 1, one free integration: two producer groups (the headline kernel), tiles of 6 steps"""
    want = 'ginsim::mc_kernel_split<1, 1, %s, 2, true, false>' % ('true' if wd else 'false')
    _check(ctx, 1, n, runs, off, wd, keep, want=want)


@pytest.mark.parametrize('n, runs, off, keep, kind', [
    (4, 65, 0, 'all', 'random'), (5, 257, 2 ** 32 + 5, 'traj', 'random'), (8, 1, 2 ** 32 + 5, 'all', 'random'), (9, 513, 0, 'none', 'random'),
    (4, 256, 2 ** 32 + 5, 'none', 'sinusoidal'), (5, 63, 0, 'all', 'sinusoidal'), (8, 255, 0, 'traj', 'sinusoidal'),
    (9, 64, 2 ** 32 + 5, 'all', 'sinusoidal')])
def test_split_consumer_inputs_with_vibration(ctx, n, runs, off, keep, kind):
    """the vibration variant: tiles of 4 steps, eighteen normals per step in the ring, one producer group, general model"""
    _check(ctx, 1, n, runs, off, True, keep, vib=kind, want='ginsim::mc_kernel_split<1, 1, true, 1, true, true>')


@pytest.mark.parametrize('rf, n, runs, off, keep, wd', [
    (1, 13, 65, 0, 'all', False), (1, 7, 257, 2 ** 32 + 5, 'traj', True), (0, 12, 64, 2 ** 32 + 5, 'all', False), (0, 33, 255, 0, 'none', True)])
def test_split_consumer_inputs_with_both_algorithms(ctx, rf, n, runs, off, keep, wd):
    """('free', 'odo') on a small batch: one producer group, the odometer's truth and coefficients among the step's inputs"""
    _check(ctx, rf, n, runs, off, wd, keep, algos=('free', 'odo'),
           want='ginsim::mc_kernel_split<%d, 3, %s, 1, true, false>' % (rf, 'true' if (wd or rf == 0) else 'false'))


@pytest.mark.parametrize('n, runs, off, keep, wd', [
    (2, 513, 0, 'none', False), (6, 1, 2 ** 32 + 5, 'none', True), (13, 257, 2 ** 32 + 5, 'none', False), (65, 63, 0, 'none', True),
    (7, 256, 0, 'all', False), (33, 65, 2 ** 32 + 5, 'traj', True)])
def test_split_consumer_inputs_in_ref_frame_0(ctx, n, runs, off, keep, wd):
    """ref_frame 0 at no more than 1024 wavefronts, statistics only and with series kept: one producer group by default (the
    KEEP = false instantiation with two is chosen only under $GINSIM_SPLIT_PROD, which is read once per process), so the name is
    whatever the dispatch reports, as long as it is a wave-specialised one"""
    _check(ctx, 0, n, runs, off, wd, keep)
