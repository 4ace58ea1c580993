"""The edge shapes and constructed inputs of tests/csd_edge_cases.py without a device: on every one of them the float64
restatement csd_exact.packed stays within csd_exact.tol of csd_exact.exact (error / tol <= 1, printed), and the facts that
tests/test_gpu_csd_edges.py rests on hold for the definition itself: the quadrature pair on one bin has a negative imaginary
cross-spectrum and no real one, a power of two on both series scales the restatement bit for bit, and the exact values of the
scaled series are finite.

Measured here (CPU, long double of 64 mantissa bits; every test prints its figure): 0.26 at worst on the 40 shapes of one and two
segments (L = 4096, K = 1, Hann, white noise against the tone), 1.1e-4 and 1.2e-5 on D = 1 at L = 8 and 64, 0.024 and 0.027 on
L = 512 / 256 and L = 2048 / 2047; 0.047 at each of the four sampling rates; 0.050 on the 64 base pairs of the grid test; 0.047 /
0.23 / 0.41 / 0.80 on the single-bin pairs at L = 8 / 128 / 1024 / 4096 (the last: cos at bin 255 against 1e-6 sin at bin 256,
boxcar, where the tolerance on pyy at bin 255 is the term e alone -- about one and a half roundings of the large bin)."""
import numpy as np
import pytest

import csd_edge_cases as ce
import csd_exact as cx

FS = 100.0


def three(x, y, fs, L, D, win, det, form=cx.packed):
    exx, eyy, exy, _ = cx.exact(x, y, fs, L, D, win, det)
    return cx.ratios(form(x, y, fs, L, D, win, det), (exx, eyy, exy), cx.tol(x, y, fs, L, D, win, det, exx, eyy))


@pytest.mark.parametrize('case', ce.CASES, ids=ce.IDS)
def test_restatement_on_every_edge_shape(case):
    name, L, D, K, tail, kinds, pad, win, det, where = case
    n, S, stride = ce.shape(case)
    assert cx.segments(n, L, D) == K and tail == 0 and n == (K - 1) * D + L
    spp = 2 * max(8192 // D, 2 * L // D, 1)
    assert K == where[0] * spp + where[1] and 0 <= where[1] < spp
    a = ce.rows(case)
    worst = max(max(three(a[i, :n], a[j, :n], FS, L, D, win, det)) for i, j in ce.pairs_of(case))
    print('csd packed restatement on %s (n %d, K %d): error / tol %.3g' % (name, n, K, worst))
    assert worst <= 1.0


def test_the_named_shapes_are_what_their_names_say():
    by = {c[0]: c for c in ce.CASES}
    assert by['L8_D1_3_parts_plus_1'][3] == 3 * 16384 + 1 and ce.shape(by['L8_D1_3_parts_plus_1'])[0] == 49160
    assert by['L64_D1_part_plus_1'][3] == 16385 and ce.shape(by['L64_D1_part_plus_1'])[0] == 16448
    assert by['L512_half_overlap_3_parts_plus_1'][2:4] == (256, 193)
    assert by['L2048_step_L_minus_1'][2:4] == (2047, 17)
    few = [c for c in ce.CASES if c[3] <= 2]
    assert {(c[1], c[7]) for c in few if c[3] == 1} == {(L, w) for L in ce.FEW_L for w in cx.WINDOWS}
    assert {(c[1], c[2], c[7]) for c in few if c[3] == 2} == {(L, D, w) for L in ce.FEW_L for D in (L, 1) for w in cx.WINDOWS}
    for L in ce.FEW_L:
        assert {c[5] for c in few if c[1] == L and c[3] == 1} == set(ce.KIND_PAIRS)
    assert {c[8] for c in few} == {True, False}


@pytest.mark.parametrize('L', ce.BIN_L)
def test_restatement_on_the_single_bin_pairs(L):
    a, n, pairs, what = ce.single_bins(L)
    ks = ce.bins_of(L)
    assert {0, 1, 2, 3, L // 4 - 1, L // 4, L // 4 + 1, L // 2 - 2, L // 2 - 1, L // 2} <= set(ks) and ks[-1] == L // 2
    assert all(p in ks and p + 1 in ks and p - 1 in ks for p in (1 << k for k in range(1, 12)) if p < L // 2)
    assert cx.segments(n, L, L) == ce.BIN_K and len(pairs) == 4 * len(ks)
    worst = (0.0, None)
    for win, det in ce.BIN_OPTIONS:
        for (i, j), w in zip(pairs, what):
            r = max(three(a[i], a[j], FS, L, L, win, det))
            worst = max(worst, (r, (win, det) + w))
            if (win, det) == ('boxcar', False) and w[0] == 'same' and 0 < w[1] < L // 2:
                exy = cx.exact(a[i], a[j], FS, L, L, win, det)[2][w[1]]
                assert exy.imag < 0 and abs(exy.real) < 1e-9 * abs(exy.imag), w
    print('csd packed restatement on the single-bin pairs L %d (%d bins): error / tol %.3g at %s' % ((L, len(ks)) + worst))
    assert worst[0] <= 1.0


def test_the_other_series_bin_is_exactly_empty_where_it_can_be():
    """What makes the single-bin pairs sharp: at the bin of x, the exact pyy is below 1e-25 of pxx there under the boxcar, so
    the tolerance on pyy at that bin is e and nothing else."""
    for L in (128, 4096):
        a, n, pairs, what = ce.single_bins(L)
        for (i, j), w in zip(pairs, what):
            if w[0] == 'next' and w[3] == 1.0 and 0 < w[1] < L // 2 and abs(w[1] - w[2]) > 1:
                exx, eyy, exy, _ = cx.exact(a[i], a[j], FS, L, L, 'boxcar', False)
                txx, tyy, txy = cx.tol(a[i], a[j], FS, L, L, 'boxcar', False, exx, eyy)
                assert eyy[w[1]] < 1e-25 * exx[w[1]] and tyy[w[1]] < 1e-25 * exx[w[1]], (L, w)


@pytest.mark.parametrize('fs', ce.RATES)
def test_restatement_at_every_sampling_rate(fs):
    import csd_cases as cc
    case = cc.CASES[cc.IDS.index(ce.RATE_SHAPE)]
    _, L, D, K, tail, kinds, pad, win, det, _ = case
    n = cc.shape(case)[0]
    a = cc.rows(case)
    worst = max(max(three(a[i, :n], a[j, :n], fs, L, D, win, det)) for i, j in cc.pairs_of(case))
    print('csd packed restatement at fs %g: error / tol %.3g' % (fs, worst))
    assert worst <= 1.0


def test_restatement_on_the_grid_inputs():
    a, base = ce.grid_inputs()
    assert cx.segments(ce.GRID_N, ce.GRID_L, ce.GRID_D) == 4 and 3 * ce.GRID_D + ce.GRID_L == ce.GRID_N
    assert any(i == j for i, j in base) and any((j, i) in base for i, j in base if i != j)
    worst = max(max(three(a[i], a[j], FS, ce.GRID_L, ce.GRID_D, 'hann', True)) for i, j in base)
    print('csd packed restatement on the 64 base pairs of the grid test: error / tol %.3g' % worst)
    assert worst <= 1.0


@pytest.mark.parametrize('name', ce.SCALED_SHAPES)
def test_a_power_of_two_scales_the_restatement_bit_for_bit(name):
    case, a, n = ce.scaled_rows(name)
    _, L, D, K, tail, kinds, pad, win, det, _ = case
    big, tiny = np.ldexp(a, ce.UP), np.ldexp(a, ce.DOWN)
    assert np.isfinite(big).all() and np.all(tiny != 0)
    worst = 0.0
    for i, j in ce.SCALED_PAIRS:
        p = cx.packed(a[i], a[j], FS, L, D, win, det)
        q = cx.packed(big[i], big[j], FS, L, D, win, det)
        s = cx.packed(tiny[i], tiny[j], FS, L, D, win, det)
        for u, v, w in zip(p, q, s):
            assert np.isfinite(v.real).all() and np.isfinite(v.imag).all()
            for part in ('real', 'imag'):
                up, vp, wp = getattr(u, part), getattr(v, part), getattr(w, part)
                np.testing.assert_array_equal(vp, np.ldexp(up, 2 * ce.UP))
                if np.all((up == 0) | (np.abs(up) > 2.0 ** -400)):          # the device test asserts this guard on its own values
                    np.testing.assert_array_equal(wp, np.ldexp(up, 2 * ce.DOWN))
        exx, eyy, exy, _ = cx.exact(big[i], big[j], FS, L, D, win, det)
        assert np.isfinite(exx).all() and np.isfinite(eyy).all() and np.isfinite(exy.real).all() and np.isfinite(exy.imag).all()
        assert max(exx.max(), eyy.max()) > 2.0 ** 900
        worst = max(worst, max(three(a[i], a[j], FS, L, D, win, det)))
    print('csd packed restatement scaled by 2^%d and 2^%d on %s: error / bound 0 (bitwise); unscaled error / tol %.3g'
          % (ce.UP, ce.DOWN, name, worst))
    assert worst <= 1.0


def test_the_placement_batches_hold_what_they_say():
    for L, a_, b_ in ce.PLACE_SHAPES:
        spp = 2 * max(8192 // L, 2, 1)
        K = a_ * spp + b_
        clean, marked, table, hit, what, inf_pair = ce.placements(L, K, spp)
        S = clean.shape[0]
        assert clean.shape == marked.shape == (S, K * L) and np.isfinite(clean).all()
        odd = list(range(1, S, 2))
        assert sorted(what) == odd
        bad = ~np.isfinite(marked)
        assert not bad[0::2].any()
        count = bad.sum(axis=1)
        assert np.all(count[odd[:-4]] == 1) and count[odd[-4]] == 2 and count[odd[-3]] == count[odd[-2]] == 1 and count[odd[-1]] == 0
        segs = sorted({int(np.flatnonzero(bad[m])[0]) // L for m in odd[:-4]})
        assert segs == sorted(s for s in {0, 1, spp // 2, spp - 1, spp, 2 * spp - 1, 2 * spp} if s < K)
        assert {int(np.flatnonzero(bad[m])[0]) % L for m in odd[:-4]} == {0, L // 2, L - 1}
        assert len(table) == 4 * len(odd) + 1 and table[-1] == inf_pair
        assert marked[inf_pair[0]][bad[inf_pair[0]]][0] == np.inf and marked[inf_pair[1]][bad[inf_pair[1]]][0] == -np.inf
        assert np.array_equal(np.flatnonzero(bad[inf_pair[0]]), np.flatnonzero(bad[inf_pair[1]]))
        marked_rows = set(odd)
        assert sorted(hit) == [p for p, (i, j) in enumerate(table) if i in marked_rows or j in marked_rows]
        assert len(hit) == 3 * len(odd) + 1
