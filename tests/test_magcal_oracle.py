"""CPU tests of the magnetometer calibration: the NumPy restatement (tests/magcal_ref.py) against the reference's own libmagcal.so
(tests/golden/magcal/*.npz, made by tests/golden/make_golden_magcal.py), the C ABI's new entry point, the ranges found in the
truth, and the plugin's surface.  The device kernel is held to the restatement by tests/test_gpu_magcal.py."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden, REPO

import magcal_ref

FINITE_CASES = ['full', 'arc', 'unequal']
SI_TOL, HI_TOL = 1e-13, 1e-11           # soft_iron; hard_iron and mag_cal [uT]


def _case(name):
    return load_golden(os.path.join('magcal', name))


@pytest.mark.parametrize('name', FINITE_CASES)
def test_restatement_equals_the_reference_library(name):
    g = _case(name)
    si, hi, cal = magcal_ref.calibrate(g['rows_x'], g['rows_y'], g['rows_z'])
    d = [np.max(np.abs(si - g['soft_iron'])), np.max(np.abs(hi - g['hard_iron'][:, 0])), np.max(np.abs(cal - g['mag_cal']))]
    print('%s: max |restatement - libmagcal.so|  soft_iron %.3g  hard_iron %.3g  mag_cal %.3g' % ((name,) + tuple(d)))
    assert bool(g['finite'])
    assert np.isfinite(si).all() and np.isfinite(hi).all() and np.isfinite(cal).all()
    assert d[0] <= SI_TOL and d[1] <= HI_TOL and d[2] <= HI_TOL
    # what the maker measured (the same comparison, on the machine that made the file) is a quarter of the tolerance at most
    assert np.all(g['lib_vs_restatement'] <= np.array([SI_TOL, HI_TOL, HI_TOL]) / 4)


def test_restatement_over_a_range_without_rotation_has_the_librarys_non_finite_mask():
    """The z range lies in a stretch without rotation.  The sensor noise keeps the normal equations invertible, so the reference's
    library returns finite (ill-conditioned: the maker's reorder_spread is 1e-7 .. 7e-6) values; the comparison is by mask."""
    g = _case('norot')
    si, hi, cal = magcal_ref.calibrate(g['rows_x'], g['rows_y'], g['rows_z'])
    assert np.array_equal(np.isfinite(si), np.isfinite(g['soft_iron']))
    assert np.array_equal(np.isfinite(hi), np.isfinite(g['hard_iron'][:, 0]))
    assert np.array_equal(np.isfinite(cal), np.isfinite(g['mag_cal']))
    assert bool(g['mask_same'])


def test_restatement_divides_by_zero_as_the_c_code_does():
    """Rows that are all the same vector of small integers: M^T M is singular in exact arithmetic and the elimination meets 0 / 0.
    No exception, NaN in everything that depends on that range (every output: the sensitivities couple the rows)."""
    rng = np.random.RandomState(5)
    mx = np.tile(np.array([1.0, 2.0, 2.0]), (1, 40, 1))
    my, mz = rng.randn(1, 50, 3) * 30.0, rng.randn(1, 60, 3) * 30.0
    si, hi, cal = magcal_ref.calibrate(mx, my, mz)
    assert np.isnan(si).all() and np.isnan(hi).all() and np.isnan(cal).all()


def test_solve_is_a_solver():
    rng = np.random.RandomState(3)
    for n in (3, 4):
        a = rng.randn(7, n, n)
        a = np.einsum('rik,rjk->rij', a, a) + np.eye(n)
        b = rng.randn(7, n)
        assert np.allclose(magcal_ref.solve(a, b), np.linalg.solve(a, b[..., None])[..., 0], rtol=1e-12, atol=1e-12)


def test_magcal_entry_point_is_declared_exported_and_bound_at_abi_9():
    import ctypes
    import ginsim
    hdr = open(os.path.join(REPO, 'include', 'ginsim.h')).read()
    declared = set(re.findall(r'\b(ginsim_[a-z0-9_]+)\s*\(', hdr))
    assert 'ginsim_magcal_run' in declared
    assert re.search(r'\}\s*ginsim_magcal_params\s*;', hdr)
    assert hasattr(ctypes.CDLL(ginsim.LIB_PATH), 'ginsim_magcal_run')
    assert 'ginsim_magcal_run' in ginsim.EXPORTS
    assert ginsim.lib.ginsim_abi_version() == 9
    assert hasattr(ginsim, 'MagCalJob')


def test_segments_from_truth_finds_the_three_rotations():
    from demo_algorithms.mag_calibrate_device import segments_from_truth
    t = _case('truth')
    seg = segments_from_truth(t['ref_gyro'])
    for (a, b), (lo, hi) in zip(seg, ((2000, 3010), (7000, 8010), (12000, 13010))):
        assert lo <= a < b <= hi and b - a >= 900, seg
    with pytest.raises(ValueError):
        segments_from_truth(np.zeros((100, 3)))                             # no rotation at all
    with pytest.raises(ValueError):
        segments_from_truth(np.zeros((100, 2)))


def test_magcal_plugin_surface():
    from demo_algorithms.mag_calibrate_device import MagCal
    m = MagCal()
    assert (m.input, m.output, m.batch, m.mc_algo) == (['mag'], ['soft_iron', 'hard_iron', 'mag_cal'], True, 'magcal')
    assert m.segments is None and m.get_results() is None
    m.reset()
    assert MagCal(segments=((1, 5), (7, 9), (10, 20))).segments == ((1, 5), (7, 9), (10, 20))
    assert MagCal(segments=[[1, 5], [7, 9], [10, 20]]).segments == ((1, 5), (7, 9), (10, 20))
    for bad in (((1, 5), (7, 9)), ((1, 5), (9, 9), (10, 20)), ((5, 1), (7, 9), (10, 20)), ((-1, 5), (7, 9), (10, 20)), (1, 2, 3), 'xyz'):
        with pytest.raises(ValueError):
            MagCal(segments=bad)
    with pytest.raises(ValueError, match='segments'):                       # called directly, the ranges cannot come from a truth
        MagCal().run([np.zeros((100, 3))])
    with pytest.raises(ValueError, match='outside'):                        # checked against the series before anything is launched
        MagCal(segments=((0, 50), (50, 100), (100, 101))).run([np.zeros((100, 3))])


def test_sim_refuses_a_magcal_it_cannot_run():
    """No device is needed for the refusals: they are the plan's."""
    from gnss_ins_sim.sim import imu_model, ins_sim
    from demo_algorithms.mag_calibrate_device import MagCal
    csv = os.path.join(REPO, 'tests', 'golden', 'magcal', 'motion_def_mag_cal.csv')
    seg = ((2007, 3007), (7007, 8007), (12007, 13007))

    def roles(axis, **kw):
        sim = ins_sim.Sim([100.0, 0.0, 100.0], csv, ref_frame=1, imu=imu_model.IMU(accuracy='mid-accuracy', axis=axis, gps=False),
                          algorithm=MagCal(segments=seg), geo_mag_n=[30.0, -3.0, 40.0], **kw)
        return sim, ins_sim._plugin_roles(sim, ['magcal'])
    with pytest.raises(ValueError, match='magnetometer'):
        roles(6)
    with pytest.raises(NotImplementedError, match='fp64'):
        roles(9, precision='f32')
    sim, r = roles(9)
    assert tuple(r) == ([], [], []) and r.magcal == [0]
    sim.sim_count = 8
    plan = lambda in_group, ndev: ins_sim.plan_monte_carlo(sim, sim.amgr.algo, r, np.arange(1000) / 100.0, 0, 0, 2 if in_group else 1, in_group,
                                                           lambda work, dist: (ndev > 1, ndev))
    with pytest.raises(ValueError, match='process group'):
        plan(True, 1)
    with pytest.raises(ValueError, match='several GPUs'):
        plan(False, 2)
    p = plan(False, 1)
    assert (p.magcal, p.fused, p.incl, p.hosted) == ([0], [], [], [])
