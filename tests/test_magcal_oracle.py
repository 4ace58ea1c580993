"""CPU tests of the magnetometer calibration: the NumPy restatement (tests/magcal_ref.py) against the reference's own libmagcal.so
(tests/golden/magcal/*.npz, made by tests/golden/make_golden_magcal.py), the C ABI's new entry point, the ranges found in the
truth, and the plugin's surface; the records of tests/magcal_records.py -- their reference-side bounds, the branches they take, and
the restatement's sign / vecMax logic against the library on them (signs.npz).  The device kernel is held to the restatement by
tests/test_gpu_magcal.py and tests/test_gpu_magcal_edges.py."""
import functools
import os
import re

import numpy as np
import pytest

from conftest import load_golden, REPO

import magcal_ref
import magcal_records as rec

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


# ------------------------------------------------------------------------------------------------- the records of magcal_records.py
@functools.lru_cache(maxsize=None)
def _value_batches():
    return [(b, rec.bounds(b['mag'], b['segments']), rec.choices(b['mag'], b['segments'])) for b in rec.value_batches()]


def test_record_bounds_are_tight_where_the_calibration_is_determined():
    """The tolerance of a record is 16 x max(E, S, eps |q|), measured on the reference side (magcal_records.bounds); a loose one
    could hide a wrong kernel.  Every record of `octants`, `axes`, `levels` is finite and held to 1e-5 (2e-7 of the 50 uT radius) or
    better in all three outputs, on every range set; every `short` record to 1e-3 of the quantity.  Measured: worst tolerance
    2.5e-10 / 8.2e-7 / 8.1e-7 (soft_iron / hard_iron / mag_cal; the noise-free record at |hi| = 500, E 2.5e-8, S 5.1e-8), with
    noise 1.7e-7; overlapping ranges 7.7e-6; short ranges at most 7.4e-5 of the quantity.  The two records of `overlap_ill`
    (magcal_records.OVERLAP_ILL) are finite; their bound is what it is (4.4e-3 and 0.84 on a fitted radius of 179 and 2899)."""
    seen = set()
    for b, bd, _ in _value_batches():
        assert all(np.isfinite(w).all() for w in bd['want']), b['name']
        assert np.isfinite(bd['tol']).all() and np.all(bd['tol'] > 0.0), b['name']
        for g, ix in b['groups'].items():
            seen.add(g)
            worst = bd['tol'][ix].max(axis=0)
            print('%-10s %-12s %3d records  tol %.3g %.3g %.3g   E %.3g %.3g %.3g   S %.3g %.3g %.3g' % (
                (b['name'], g, len(ix)) + tuple(worst) + tuple(bd['E'][ix].max(axis=0)) + tuple(bd['S'][ix].max(axis=0))))
            if g in rec.VALUE_GROUPS:
                assert np.all(bd['tol'][ix] <= 1e-5), (b['name'], g, worst)
            elif g == 'short':
                assert np.all(bd['tol'][ix] <= 1e-3 * bd['size'][ix]), (b['name'], (bd['tol'][ix] / bd['size'][ix]).max(axis=0))
            else:
                assert g == 'overlap_ill' and len(ix) == 2
    assert seen == set(rec.VALUE_GROUPS) | {'short', 'overlap_ill'}
    # no record of the three groups is outside the value comparison: every configuration is a run of `full` and of `unequal`
    cfgs = rec.configs()
    for b, _, _ in _value_batches()[:2]:
        assert b['names'] == list(cfgs) and sorted(np.concatenate([b['groups'][g] for g in rec.VALUE_GROUPS])) == list(range(len(cfgs)))


def test_records_take_every_branch_of_the_sign_and_of_vecmax():
    """Over the `octants` + `axes` records the flip pattern of the three normals takes all eight values; for each range each
    component index is the one vecMax selects in some record (the cyclic permutations of si move it off the diagonal, the 44 / 46
    degree rotations make the two largest differ by a few percent, each winning once); and in some record per range the two
    rotated columns of that range's ratio keep one sign (max / min that started from 0 would be wrong there).  The goldens and
    the series of truth.npz take pattern (no, no, no), the diagonal component, and straddle zero."""
    patterns, picked, one = set(), [set(), set(), set()], np.zeros(3, dtype=bool)
    for b, _, ch in _value_batches()[:5]:
        ix = np.concatenate([b['groups'][g] for g in ('octants', 'axes') if g in b['groups']])
        patterns |= set(map(tuple, ch['flip'][ix].tolist()))
        for a in range(3):
            picked[a] |= set(ch['idx'][ix, a].tolist())
        one |= ch['one_signed'][ix].any(axis=0)
    assert len(patterns) == 8 and picked == [{0, 1, 2}] * 3 and one.all(), (patterns, picked, one)
    g = _case('full')
    ch = rec.choices(np.concatenate([g['rows_x'], g['rows_y'], g['rows_z']], axis=1), ((0, 1000), (1000, 2000), (2000, 3000)))
    assert not ch['flip'].any() and np.array_equal(ch['idx'], np.tile([0, 1, 2], (3, 1))) and not ch['one_signed'].any()
    full = _value_batches()[0]
    near = [full[0]['names'].index(k) for k in ('rotz44+-+', 'rotz46+-+')]
    assert full[2]['idx'][near, 0].tolist() == [0, 1]                       # the x normal's two largest components: each wins once


def test_record_builder_is_deterministic():
    a, b = rec.value_batches(), rec.value_batches()
    assert [x['name'] for x in a] == [x['name'] for x in b]
    for x, y in zip(a, b):
        assert x['mag'].tobytes() == y['mag'].tobytes() and x['segments'] == y['segments'] and x['names'] == y['names']
    (p, pc), (q, qc) = rec.nonfinite_batch(), rec.nonfinite_batch()
    assert p['mag'].tobytes() == q['mag'].tobytes() and pc.tobytes() == qc.tobytes() and p['poisoned'].keys() == q['poisoned'].keys()
    assert sorted(p['poisoned']) == sorted(rec.NONFINITE_LANES) and p['mag'].shape[0] == 130
    assert np.array_equal(np.flatnonzero(~np.isfinite(p['mag']).all(axis=(1, 2))), np.array(sorted(rec.NONFINITE_LANES)))
    for (x, xc), (y, yc) in zip(rec.undetermined_batches(), rec.undetermined_batches()):
        assert x['mag'].tobytes() == y['mag'].tobytes() and x['segments'] == y['segments']
    k, cfg = rec.octants500_configs()[3]
    t = rec.truth()
    assert np.array_equal(a[0]['mag'][a[0]['names'].index(k)], rec.series(cfg, t['ref_mag']))
    assert rec.bounds(a[2]['mag'][:2], a[2]['segments'])['tol'].tobytes() == rec.bounds(b[2]['mag'][:2], b[2]['segments'])['tol'].tobytes()


@pytest.mark.parametrize('name', FINITE_CASES)
def test_extended_precision_restatement_is_the_same_calculation(name):
    """dtype=np.longdouble evaluates the same steps in the 80-bit format: on the goldens it differs from the float64 restatement by
    no more than the record's own bound allows for (E <= tol / 16 by construction) and by no more than 16 x what reordering the
    float64 sums moves (the maker's reorder_spread: an independent measure of the float64 rounding), and the float64 results are
    what they were -- within lib_vs_restatement of the library."""
    g = _case(name)
    rows = (g['rows_x'], g['rows_y'], g['rows_z'])
    f64 = magcal_ref.calibrate(*rows)
    ext = magcal_ref.calibrate(*rows, dtype=np.longdouble)
    assert all(x.dtype == np.longdouble for x in ext) and all(x.dtype == np.float64 for x in f64)
    assert all(np.array_equal(a, b) for a, b in zip(f64, magcal_ref.calibrate(*rows, dtype=np.float64)))
    mag = np.concatenate(rows, axis=1)
    seg = tuple((int(a), int(b)) for a, b in zip(np.cumsum([0] + [r.shape[1] for r in rows[:-1]]), np.cumsum([r.shape[1] for r in rows])))
    bd = rec.bounds(mag, seg)
    d = np.array([float(np.max(np.abs(a - b))) for a, b in zip(ext, f64)])
    print('%s: max |float64 - longdouble|  %.3g %.3g %.3g   reorder_spread %s' % ((name,) + tuple(d) + (g['reorder_spread'],)))
    assert np.all(d <= bd['E'].max(axis=0)) and np.all(d > 0.0)
    assert np.all(d <= 16.0 * g['reorder_spread'])
    # the library is as close to the 80-bit evaluation as the float64 restatement is, within what separates those two
    lib = (g['soft_iron'], g['hard_iron'][:, 0], g['mag_cal'])
    for a, b, e, l in zip(ext, lib, d, g['lib_vs_restatement']):
        assert float(np.max(np.abs(a - b))) <= e + l * (1 + 1e-9)


def test_restatement_equals_the_reference_library_on_flipped_and_permuted_records():
    """signs.npz: libmagcal.so on the `octants` (|hi| = 500) and `axes` records, both range sets -- all eight flip patterns, every
    component selected by vecMax.  Masks equal, values within the file's lib_vs_restatement (measured when it was made: soft_iron
    2.2e-13, hard_iron 5.7e-9, mag_cal 5.7e-9; |hi| = 500 makes the sums 100 x those of the goldens), which itself is held under
    1e-12 / 1e-7, a tenth of the 1e-5 the device's bound may reach on these records at most."""
    g = _case('signs')
    recs = rec.signs_records()
    assert [r[0] for r in recs] == [str(x) for x in g['names']] and bool(g['mask_same'])
    assert len(recs) == 2 * (8 + 12)
    worst = np.zeros(2)
    for k, (name, mag, seg) in enumerate(recs):
        si, hi, _ = magcal_ref.calibrate_series(mag, seg)
        assert np.isfinite(si).all() and np.isfinite(hi).all() and np.isfinite(g['soft_iron'][k]).all() and np.isfinite(g['hard_iron'][k]).all()
        d = np.array([np.max(np.abs(si - g['soft_iron'][k])), np.max(np.abs(hi - g['hard_iron'][k]))])
        worst = np.maximum(worst, d)
        assert np.all(d <= g['lib_vs_restatement'][k, :2] * (1 + 1e-9) + 1e-300), (name, d, g['lib_vs_restatement'][k])
    print('max |restatement - libmagcal.so| over %d records: soft_iron %.3g  hard_iron %.3g' % ((len(recs),) + tuple(worst)))
    assert np.all(g['lib_vs_restatement'].max(axis=0) <= np.array([1e-12, 1e-7, 1e-7]))
