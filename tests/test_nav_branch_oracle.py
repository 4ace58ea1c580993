"""The cases of tests/nav_branch_cases.py on the CPU alone: each shows the branch events it is there for, the two oracles agree on it
through the folds, and the runs that the device tests compare are those the C oracle alone shows to be well conditioned and clear
of every fold and wrap threshold.  Plus the two oracles on the odometer plugin's tumble fixture (what the unmodified reference's
free_integration_odo returned on rates that fold the pitch and wrap yaw and roll)."""
import numpy as np
import pytest

from conftest import load_golden, assert_traj_close
import nav_branch_cases as nb


def _split(traj):
    return traj[..., 0:3], traj[..., 3:6], traj[..., 6:9]


@pytest.mark.parametrize('algo', nb.ALGOS)
@pytest.mark.parametrize('name', nb.NAMES)
def test_case_shows_its_branch_events(name, algo):
    """counted over the compared runs only, from the C oracle's trajectory; the recomputed step must land on the oracle's own next
    sample (otherwise the count describes some other trajectory)"""
    c = nb.cases()[name]
    ok = nb.compared(name, algo)
    gyro, _ = nb.sensors(name)
    base = nb.oracle_given(name, algo)
    s = nb.steps(c, base, gyro)
    d = np.abs(np.mod(s['next'][ok] - base[ok][:, 1:, 0:3] + np.pi, 2 * np.pi) - np.pi)
    assert d.max() <= 1e-14, 'the recomputed steps miss the oracle by %.3e' % d.max()
    ev = nb.events(c, s, ok)
    print('%s %s: %s' % (name, algo, {k: v for k, v in ev.items() if v}))
    for key, least in c.want.items():
        only, _, key = key.rpartition(':')
        if only and only != algo:
            continue
        assert ev[key] >= least, '%s %s: %d x %s, at least %d wanted' % (name, algo, ev[key], key, least)


@pytest.mark.parametrize('algo', nb.ALGOS)
@pytest.mark.parametrize('name', nb.NAMES)
def test_numpy_and_c_oracle_agree_through_the_folds(name, algo):
    """every sample of every compared run within a tenth of the device tolerance; a generate-mode case gives the given-data
    oracle's bits (a zero-error IMU reproduces the rates; with noise the series are the oracle's own)"""
    c = nb.cases()[name]
    ok = nb.compared(name, algo)
    base = nb.oracle_given(name, algo)
    r = nb.ratio(nb.oracle_numpy(name, algo)[ok], base[ok], c.n)
    print('%s %s: NumPy against C, error / tolerance %.3g' % (name, algo, r.max()))
    assert r.max() <= 0.1
    if c.generate:
        end, traj = nb.oracle_mc(name, algo)
        assert np.array_equal(traj, base, equal_nan=True)
    # the bad runs of (f): both oracles are non-finite at the same samples and planes
    for run in c.bad:
        assert np.array_equal(np.isfinite(nb.oracle_numpy(name, algo)[run]), np.isfinite(base[run]))


@pytest.mark.parametrize('algo', nb.ALGOS)
@pytest.mark.parametrize('name', nb.NAMES)
def test_compared_runs_are_well_conditioned_and_clear_of_the_thresholds(name, algo):
    c = nb.cases()[name]
    moved, held, margin = nb.conditioning(name, algo)
    ok = nb.compared(name, algo)
    good = np.ones(c.runs, dtype=bool)
    good[list(c.bad)] = False
    left_out = int(np.sum(good & ~ok))
    print('%s %s: %d of %d runs left out; compared runs move by %.3g of the tolerance, margin %.3g' % (
        name, algo, left_out, c.runs, moved[ok].max(), margin[ok].min()))
    assert ok.any()
    assert moved[ok].max() <= 0.1 and held[ok].all() and margin[ok].min() >= nb.MARGIN
    assert 8 * left_out <= c.runs, '%d of %d runs left out' % (left_out, c.runs)
    if c.strict:
        assert left_out == 0
    # a bad run is bad from the sample the case names, and only there
    base = nb.oracle_given(name, algo)
    for run, first in c.bad.items():
        fin = np.isfinite(base[run, :, 0:3]).all(axis=1)
        assert fin[:first].all() and not fin[first:].any(), (run, first)
        assert np.isnan(base[run, first + 2:]).all(), 'all nine planes are NaN two samples on'
    assert np.isfinite(base[good]).all()


def test_threshold_rows_of_the_pitch_case_are_exact():
    """case (a): the four threshold steps are there to the bit, in both directions, and nothing but the pitch moves"""
    c = nb.cases()['a_pitch_thresholds']
    s = nb.steps(c, nb.oracle_given(c.name, 'free'), nb.sensors(c.name)[0])
    dp = s['dp'][0]
    for v in (nb.SMALL, nb.UP(nb.SMALL, 1.0), nb.BIG, nb.UP(nb.BIG, 1.0)):
        assert (dp == v).any() and (dp == -v).any(), v
    assert np.array_equal(np.abs(dp), s['big'][0])
    assert np.abs(s['dy']).max() < 1e-12 and np.abs(s['dr']).max() < 1e-12        # sin(pi) = 1.2e-16 over cos(pitch) >= 7e-4


@pytest.mark.parametrize('tag, rf, use_g, erot', [('extg', 0, True, False), ('wgs', 0, False, True), ('rf1', 1, False, True)])
def test_oracles_on_the_odometer_tumble_fixture(tag, rf, use_g, erot):
    from oracle import c_oracle, ins_np
    g = load_golden('t1_fixture_tumble_odo')
    ini = g['ini'] if use_g else g['ini'][:9]
    fs = float(g['fs'])
    att, pos, vel = c_oracle.free_integration(rf, fs, g['gyro'], None, ini, earth_rot=erot, odo=g['odo'])
    assert_traj_close(att, pos, vel, g['att_' + tag], g['pos_' + tag], g['vel_' + tag], rtol=1e-10, what='C ' + tag)
    att, pos, vel = ins_np.free_integration(rf, fs, g['gyro'][None], None, ini, earth_rot=erot, odo=g['odo'][None])
    assert_traj_close(att[0], pos[0], vel[0], g['att_' + tag], g['pos_' + tag], g['vel_' + tag], rtol=1e-10, what='NumPy ' + tag)
