"""The reference of the PSD vibration tests (tests/vib_psd_exact.py) held together without a device: the recorded deviation of
its float64 restatement from its long-double sum, the restatement against oracle.ins_np.psd_series (which the three T3_PSD goldens
hold to the reference), closed forms of the smallest periods, the coverage of the case table, and that every fault the GPU tests
rely on seeing moves the reference by more than 1e3 of the device's bounds."""
import numpy as np
import pytest

import vib_psd_exact as vx

LD = vx.LD
ALL = vx.CASES + vx.EXTRA


@pytest.mark.parametrize('cid', [c.id for c in ALL])
def test_recorded_deviation_of_the_float64_restatement(cid):
    """DEV[id] reproduces: the restatement is within its record of the long-double sum at every checked (axis, sample, run), and
    the record is no more than twice what is measured (a figure that has gone stale fails here too)."""
    case = vx.BY_ID[cid]
    ref = vx.reference(case)
    assert ref['exact'].dtype == LD and np.finfo(LD).nmant >= 63
    assert ref['exact'].shape == (3, ref['js'].size, ref['rr'].size) and ref['f64'].shape == (3, case.N, ref['runs'].size)
    d = vx.deviation(ref['f64'], ref)
    print('%s: float64 restatement %.3g units of A 2^-53 (recorded %.3g), device bound %.3g units' % (cid, d, vx.DEV[cid], vx.allowed(case)))
    assert d <= vx.DEV[cid]
    assert vx.DEV[cid] <= 2.0 * d + 1e-3
    if case.table == 'zero':
        assert vx.DEV[cid] == 0.0 and not ref['f64'].any() and not ref['exact'].any()
    assert vx.allowed(case) * vx.UNIT < vx.CEILING            # the margin-based bound is the tighter one everywhere


def test_positions_and_runs_of_the_long_double_sum():
    for N in vx.PERIODS:
        js = vx.positions(N)
        if N <= 2048:
            assert np.array_equal(js, np.arange(N))
        else:
            assert js.size == 256 and np.unique(js).size == 256 and js.min() == 0 and js.max() == N - 1
            assert set((0, 1, 63, 64, 65, N // 2 - 1, N // 2, N // 2 + 1, N - 2, N - 1)) <= set(js.tolist())
            assert np.array_equal(js, vx.positions(N))
    assert vx.ref_runs(1).tolist() == [0] and vx.ref_runs(64).tolist() == [0, 1, 62, 63]
    assert vx.ref_runs(129).tolist() == [0, 1, 62, 63, 64, 65, 127, 128]


@pytest.mark.parametrize('cid', vx.IDS + [c.id for c in vx.HALVING])
def test_float64_restatement_is_psd_series(cid):
    """The case as a vib_def given on the period's grid (the halved cases, calls_before = the global run id) or interpolated (the
    others) goes through oracle.ins_np.psd_series -- ifft of the Hermitian extension after sqrt(sxx N fs) -- and comes out the
    float64 restatement to 4 units: the amplitude's round trip through a PSD is three roundings, the two transforms differ."""
    from oracle import ins_np
    case = vx.BY_ID[cid]
    ref = vx.reference(case)
    vd = vx.as_vib_def(case)
    assert (vd['freq'].size == case.N // 2 + 1) == bool(case.halve)
    worst = 0.0
    for i, r in zip(ref['at'], ref['rr']):
        got = ins_np.psd_series(vd, vx.FS, case.N, vx.normals(case, int(r)), calls_before=case.off + int(r) if case.halve else 0).T
        worst = max(worst, vx._ratio(np.abs(got - ref['f64'][:, :, i]), ref['A'][:, None, i]))
    print('%s: psd_series against the restatement %.3g units' % (cid, worst))
    assert worst <= 4.0


def test_the_cases_cover_every_pair_of_run_count_and_period_class():
    """the selection itself: every (period class, run count) occurs, every one of the sixteen periods, both sensors with every
    offset, every table, and no seed fits 32 bits"""
    assert len(vx.PERIODS) == 16 and {c.N for c in vx.CASES} == set(vx.PERIODS)
    assert {(vx.period_class(c.N), c.runs) for c in vx.CASES} == {(k, r) for k in vx.CLASSES for r in vx.RUNS}
    assert len(vx.CASES) == sum(max(5, len(v)) for v in vx.CLASSES.values())            # as few as that takes
    assert {(c.sensor, c.off) for c in vx.CASES} == {(s, o) for s in ('acc', 'gyr') for o in vx.OFFSETS}
    assert {c.table for c in vx.CASES} == set(vx.TABLES)
    assert {vx.period_class(c.N) for c in vx.CASES if c.halve} >= {'tiny', 'tile', 'block', 'composite'}
    assert all(c.seed >= 2 ** 32 for c in vx.CASES + vx.EXTRA)
    assert len(set(vx.BY_ID)) == len(vx.CASES) + len(vx.EXTRA) and set(vx.DEV) == set(vx.BY_ID)
    a = vx.case_amplitudes(vx.CASES[0])
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[1], a[2])
    d12 = vx.case_amplitudes(vx.BY_ID['N512_R65_acc_off37_decades12'])
    assert d12.max() / d12.min() > 1e12


def test_closed_forms_of_the_smallest_periods_and_of_the_edge_bins():
    """N = 2: (a0 c0 +- a1 c1) / 2.  N = 4: (a0 c0 +- a2 c2 + 2 a1 cos(pi j / 2 + pi z1)) / 4.  A table with bins 0 and N/2 alone:
    (a0 c0 + (-1)^j aL cL) / N at any N -- no sine of z[0] or z[L-1] anywhere."""
    pi = vx.PI
    for case in (vx.BY_ID['N2_R1_gyr_off37_rand'], vx.BY_ID['N4_R63_acc_off0_rand_halved'], vx.BY_ID['N4_R65_gyr_off37_edges'],
                 vx.BY_ID['N130_R65_gyr_off37_edges']):
        ref = vx.reference(case)
        N, L = case.N, case.N // 2 + 1
        for i, r in enumerate(ref['rr']):
            a = vx.run_amplitudes(ref['a'], case.off + int(r), case.halve)
            z = vx.normals(case, int(r)).astype(LD)
            for c in range(3):
                e0, eL = a[c, 0] * np.cos(pi * z[0, c]), a[c, L - 1] * np.cos(pi * z[L - 1, c])
                for j in (0, 1, 2, 3, N - 1):
                    if j >= N:
                        continue
                    want = e0 + (-1) ** j * eL
                    if N == 4:
                        want = want + 2 * a[c, 1] * np.cos(pi * j / 2 + pi * z[1, c])
                    elif case.table != 'edges':
                        assert N == 2
                    want = want / N
                    assert abs(ref['exact'][c, j, i] - want) <= 4 * np.finfo(LD).eps * float(ref['A'][c, ref['at'][i]])


def test_halving_factor():
    """sqrt(0.5^(g + 1)), 0.5^(g + 1) first: in float64 it is zero from g = 1074 on, which is what the reference computes"""
    assert vx.halving(0, np.float64) == np.sqrt(0.5) and vx.halving(1, np.float64) == 0.5 and vx.halving(9, np.float64) == 2.0 ** -5
    assert vx.halving(1000, np.float64) == np.sqrt(2.0 ** -1001) > 0 and vx.halving(2300, np.float64) == 0.0
    assert float(vx.halving(2300)) == 0.0 and vx.halving(2 ** 32 + 5) == 0
    a = np.ones((3, 5))
    assert np.array_equal(vx.run_amplitudes(a, 1, 1, np.float64), np.array([[1, .5, .5, .5, 1]] * 3))
    assert np.array_equal(vx.run_amplitudes(a, 1, 0, np.float64), a)
    assert np.array_equal(vx.run_amplitudes(np.ones((3, 2)), 1, 1, np.float64), np.ones((3, 2)))           # N = 2: nothing to halve


FAULT_CASES = [(c.id, f) for c in vx.CASES if c.table == 'rand' and c.N > 2 for f in ('swap_axes', 'no_alternation')] \
    + [(c.id, 'local_run') for c in vx.CASES if c.off and c.table != 'zero'] \
    + [(c.id, 'block_local_run') for c in vx.BLOCKS] \
    + [(c.id, f) for c in vx.HALVING for f in ('halve_bin0', 'halve_last', 'skip_bin1', 'skip_last_interior')]


@pytest.mark.parametrize('cid,fault', FAULT_CASES)
def test_every_fault_moves_the_reference_by_more_than_1e3_bounds(cid, fault):
    """What the GPU tests assert before they ask the device, here for every case at once: the axes of the normals swapped, the
    (-1)^j of bin N/2 dropped, the run id taken without its offset (or within its block of 32768), the halving applied to bin 0 or
    N/2 or left off bin 1 or L-2."""
    m = vx.moved(vx.BY_ID[cid], fault)
    print('%s %s: moves a sample by %.3g bounds' % (cid, fault, m))
    assert m > 1e3


def test_sensors_and_swapped_rows_differ_by_more_than_1e3_bounds():
    for case in vx.OTHER_SENSOR + vx.RESEEDED + vx.SWAPPED:
        base, ref, other = vx.BY_ID[case.base], vx.reference(vx.BY_ID[case.base]), vx.reference(case)
        d = vx._ratio(np.abs(other['exact'] - ref['exact']).astype(np.float64), ref['A'][:, None, ref['at']]) / vx.allowed(base)
        print('%s: %.3g bounds from %s' % (case.id, d, case.base))
        assert d > 1e3
        if case.perm:                                           # the row that stayed gives the same series
            same = [c for c in range(3) if case.perm[c] == c]
            assert len(same) == 1 and np.array_equal(other['f64'][same[0]], ref['f64'][same[0]])
