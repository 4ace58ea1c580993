"""The Welch cross-spectral kernel (csrc/csd.hip through ginsim_csd_welch) at its edges: one and two segments, a step of one
sample, part boundaries at lengths that had none, every place a non-finite sample can sit in a part and on either side of a pair,
magnitude alone, calls in sequence on one context, single bins that show the separation of X and Y and the bin each butterfly
owns, as many pairs as the grid takes, a capacity above the number of bins, the sampling rate and unusual tables.  The shapes and
the constructed inputs are those of tests/csd_edge_cases.py (tests/test_csd_edges_oracle.py holds them together without a
device); a result is held to csd_exact.exact within csd_exact.tol (error / tol <= 1) or to another launch bit for bit.  Every
test prints its error over its bound.

Measured on one MI355X, the largest error / tol of each group (DESIGN 4.3e has the same figures):
  a. parity on the 44 edge shapes: 0.518 for pxx and pyy (L4096_K1_n_equals_L_hann_offset_small) and 0.143 for pxy
     (L4096_K1_n_equals_L_hann_white_tone); the two D = 1 shapes stay at 0.001 and 9e-5;
  c. the two unscaled inputs of the scaling test: 0.067 (L4096_no_overlap_2_parts_plus_1);
  e. single bins, 4 lengths x 2 options, 5 / 65 / 27 / 33 bins: 0.595 (pyy of the quadrature pair) and 0.577 (pxy of the
     next-bin pair), both at L = 4096, boxcar, no detrend; 0.366 at L = 1024, 0.209 at L = 128, 0.048 at L = 8; the coherence of the
     quadrature pair is within 4.5e-16 of 1;
  f. the 64 base pairs of the grid test: 0.053 (the device took 65536 pairs);
  h. 0.041 at each of the four sampling rates;
  b, d, g, i and the rows of f: bit for bit."""
import ctypes as C
import re

import numpy as np
import pytest

import csd_cases as cc
import csd_edge_cases as ce
import csd_exact as cx
import psd_cases as pc
import psd_exact as px

pytestmark = pytest.mark.gpu

FS = 100.0


@pytest.fixture(scope='module')
def ctx():
    import ginsim
    c = ginsim.Context(0)
    yield c
    c.close()


def held_to_exact(r, a, n, pairs, L, D, win, det, fs=FS):
    """Largest error / tol of (pxx, pyy, pxy) over the pairs, and the properties every finite result has."""
    worst = np.zeros(3)
    for p, (i, j) in enumerate(pairs):
        x, y = a[i, :n], a[j, :n]
        exx, eyy, exy, _ = cx.exact(x, y, fs, L, D, win, det)
        t = cx.tol(x, y, fs, L, D, win, det, exx, eyy)
        worst = np.maximum(worst, cx.ratios((r.pxx[p], r.pyy[p], r.pxy[p]), (exx, eyy, exy), t))
    edge = r.pxy.imag[:, [0, -1]]
    assert np.all(edge == 0.0) and not np.signbit(edge).any()           # +0.0, sign bit included
    coh = r.coherence
    assert np.all(coh[np.isfinite(coh)] <= 1 + 1e-12)
    return worst


def same_bits(r, q, rows_r=slice(None), rows_q=slice(None)):
    for k in ('pxx', 'pyy', 'pxy'):
        np.testing.assert_array_equal(getattr(r, k)[rows_r], getattr(q, k)[rows_q])


def planes(r):
    return r.pxx, r.pyy, r.pxy.real, r.pxy.imag


def result_doubles(npairs, L):
    return 4 * npairs * (L // 2 + 1)


# ---- a. parity on every edge shape
@pytest.mark.parametrize('case', ce.CASES, ids=ce.IDS)
def test_parity_on_every_edge_shape(ctx, case):
    import ginsim
    name, L, D, K, tail, kinds, pad, win, det, where = case
    n, S, stride = ce.shape(case)
    pairs = ce.pairs_of(case)
    g = ginsim.csd_plan(n, S, stride, FS, len(pairs), L, D)
    assert g['segments'] == K and g['nparts'] == -(-K // g['segs_per_part']) and g['segs_per_part'] == pc.segs_per_part(L, D)
    assert K == where[0] * g['segs_per_part'] + where[1]
    a = ce.rows(case)
    r = ce.device_csd(ctx, a, n, pairs, L, D, win, det)
    assert r.pxx.shape == r.pyy.shape == r.pxy.shape == (len(pairs), L // 2 + 1) and r.pxy.dtype == np.complex128
    np.testing.assert_array_equal(r.freq, cx.freqs(FS, L))
    np.testing.assert_array_equal(r.pairs, pairs)
    worst = held_to_exact(r, a, n, pairs, L, D, win, det)
    print('csd edge %s (n %d, %d pairs, %d parts): error / tol pxx %.3g pyy %.3g pxy %.3g' % ((name, n, len(pairs), g['nparts']) + tuple(worst)))
    assert worst.max() <= 1.0


# ---- b. where a non-finite sample sits
@pytest.mark.parametrize('L,a_,b_', ce.PLACE_SHAPES, ids=['L128_three_parts_one_wavefront', 'L2048_two_parts_eight_wavefronts'])
def test_a_non_finite_sample_marks_its_pairs_wherever_it_sits(ctx, L, a_, b_):
    import ginsim
    D = L
    spp = pc.segs_per_part(L, D)
    K = a_ * spp + b_
    g = ginsim.csd_plan(K * L, 1, K * L, FS, 1, L, D)
    assert (g['segments'], g['nparts'], g['segs_per_part']) == (K, a_ + 1, spp) and g['threads'] == (64 if L == 128 else 512)
    assert px.window(L, 'hann', np.float64)[0] == 0.0               # sample 0 of a segment has no weight
    clean, marked, table, hit, what, inf_pair = ce.placements(L, K, spp)
    n, S = clean.shape[1], clean.shape[0]
    rest = [p for p in range(len(table)) if p not in set(hit)]
    assert len(rest) == (S - 1) // 2 and all(i % 2 == 0 and j % 2 == 0 for i, j in (table[p] for p in rest))
    for win, det in ce.PLACE_OPTIONS:
        ref = ce.device_csd(ctx, clean, n, table, L, D, win, det)
        assert all(np.isfinite(v).all() for v in planes(ref))
        got = ce.device_csd(ctx, marked, n, table, L, D, win, det)
        for p in hit:
            i, j = table[p]
            for v in planes(got):
                assert np.isnan(v[p]).all(), (win, det, table[p], what.get(i), what.get(j), int(np.isnan(v[p]).sum()))
        same_bits(got, ref, rest, rest)
    print('csd non-finite places L %d (%d marked of %d series, %d pairs of %d hold one, 3 options): error / bound 0 (bitwise)'
          % (L, len(what), S, len(hit), len(table)))


# ---- c. magnitude alone marks nothing
@pytest.mark.parametrize('name', ce.SCALED_SHAPES)
def test_magnitude_alone_marks_nothing(ctx, name):
    """A power of two on BOTH series scales every operation of the kernel exactly as long as nothing overflows or goes subnormal:
    2^460 on the series gives 2^920 on the four outputs, 2^-300 gives 2^-600, bit for bit.  (One series alone is not exact: the
    twiddle product mixes the two planes.)"""
    import ginsim
    case, a, n = ce.scaled_rows(name)
    _, L, D, K, tail, kinds, pad, win, det, where = case
    g = ginsim.csd_plan(n, 2, n, FS, len(ce.SCALED_PAIRS), L, D)
    assert (g['threads'] == 64 and g['nparts'] == 1) if L < 1024 else (L >= 1024 and g['nparts'] >= 2)
    big, tiny = np.ldexp(a, ce.UP), np.ldexp(a, ce.DOWN)
    assert np.isfinite(big).all() and np.all(tiny != 0)
    p = ce.device_csd(ctx, a, n, ce.SCALED_PAIRS, L, D, win, det)
    q = ce.device_csd(ctx, big, n, ce.SCALED_PAIRS, L, D, win, det)
    s = ce.device_csd(ctx, tiny, n, ce.SCALED_PAIRS, L, D, win, det)
    for u, v, w in zip(planes(p), planes(q), planes(s)):
        assert np.isfinite(v).all()
        np.testing.assert_array_equal(v, np.ldexp(u, 2 * ce.UP))
        assert np.all((u == 0.0) | (np.abs(u) > 2.0 ** -400))        # the guard: nothing compared goes subnormal at 2^-600
        np.testing.assert_array_equal(w, np.ldexp(u, 2 * ce.DOWN))
    worst = held_to_exact(p, a, n, ce.SCALED_PAIRS, L, D, win, det)
    print('csd scaled by 2^%d and 2^%d %s: error / bound 0 (bitwise); unscaled error / tol %.3g' % (ce.UP, ce.DOWN, name, worst.max()))
    assert worst.max() <= 1.0


# ---- d. calls in sequence on one context (before the large table of f: the pinned buffer grows inside this test)
WIDE = ('L4096_K1_128_pairs_over_16_series', 4096, 4096, 1, 0, ('white', 'tone', 'walk', 'small') * 4, 0, 'boxcar', True, (0, 1))
WIDE_PAIRS = [(i, (i + 1 + p // 16) % 16) for p in range(128) for i in [p % 16]]
SMALL = cc.CASES[cc.IDS.index('L64_K3_unaligned_hann_detrend')]
SMALL_PAIRS = [(1, 0), (2, 2), (0, 2)]        # as many pairs as the call before it has, and none of them the same


def test_calls_in_sequence_equal_first_calls_on_fresh_contexts(ctx):
    import ginsim
    large = ce.case_of('L8_D1_3_parts_plus_1')
    allan_series = np.stack([px.series(k, 4096, 7 + i) for i, k in enumerate(('white', 'walk', 'offset'))])
    psd_case = pc.CASES[pc.IDS.index('L64_D3_fewer_bins_than_lanes')]

    def csd_call(c, case):
        _, L, D, K, tail, kinds, pad, win, det, _ = case
        n, S, stride = cc.shape(case)
        pairs = WIDE_PAIRS if case is WIDE else SMALL_PAIRS if case is SMALL else cc.pairs_of(case)
        r = ce.device_csd(c, cc.rows(case), n, pairs, L, D, win, det)
        return np.stack(planes(r))

    def allan_call(c, _):
        return ginsim.allan_var_host(c, allan_series, FS)[0]

    def psd_call(c, case):
        _, L, D, K, tail, kinds, pad, win, det, _ = case
        n, S, stride = pc.shape(case)
        return pc.device_psd(c, pc.rows(case), n, L, D, win, det)[0]
    order = [(csd_call, large), (csd_call, SMALL), (allan_call, None), (psd_call, psd_case), (csd_call, WIDE), (csd_call, SMALL)]
    # more result doubles than any call of this file before it left room for (a grown buffer has 5/4 of its call plus 64):
    # the placement tables of b are the largest of them
    before = [result_doubles(len(cc.pairs_of(c)), c[1]) for c in ce.CASES]
    for L, a_, b_ in ce.PLACE_SHAPES:
        spp = pc.segs_per_part(L, L)
        before.append(result_doubles(ce.placement_pairs(a_ * spp + b_, spp), L))
    before.append(result_doubles(len(ce.SCALED_PAIRS), 4096))
    assert len(WIDE_PAIRS) == 128 and len(set(WIDE_PAIRS)) == 128 and len(WIDE[5]) == 16
    assert len(SMALL_PAIRS) == len(cc.pairs_of(large)) and not set(SMALL_PAIRS) & set(cc.pairs_of(large))
    assert result_doubles(128, 4096) > max(before) * 5 // 4 + 64
    got = [fn(ctx, case) for fn, case in order]
    for (fn, case), have in zip(order, got):
        fresh = ginsim.Context(0)
        try:
            first = fn(fresh, case)
        finally:
            fresh.close()
        assert np.isfinite(first).all()
        np.testing.assert_array_equal(have, first)
    np.testing.assert_array_equal(got[1], got[5])
    print('csd calls in sequence vs fresh contexts (6 calls, csd / csd / allan / psd / csd of %d results / csd): error / bound 0 (bitwise)'
          % result_doubles(128, 4096))


# ---- e. single bins: the separation of X and Y and the bin each butterfly owns
@pytest.mark.parametrize('win,det', ce.BIN_OPTIONS, ids=['%s_%s' % (w, 'detrend' if d else 'raw') for w, d in ce.BIN_OPTIONS])
@pytest.mark.parametrize('L', ce.BIN_L)
def test_single_bins_stay_in_their_series_and_their_bin(ctx, L, win, det):
    a, n, pairs, what = ce.single_bins(L)
    r = ce.device_csd(ctx, a, n, pairs, L, L, win, det)
    worst = {'next': np.zeros(3), 'same': np.zeros(3)}
    coh = r.coherence
    far = 0.0
    for p, ((i, j), (kind, k0, k1, amp)) in enumerate(zip(pairs, what)):
        exx, eyy, exy, _ = cx.exact(a[i], a[j], FS, L, L, win, det)
        t = cx.tol(a[i], a[j], FS, L, L, win, det, exx, eyy)
        got = cx.ratios((r.pxx[p], r.pyy[p], r.pxy[p]), (exx, eyy, exy), t)
        assert max(got) <= 1.0, (L, win, det, kind, k0, k1, amp, got)
        worst[kind] = np.maximum(worst[kind], got)
        if kind == 'same' and win == 'boxcar' and 0 < k0 < L // 2:
            assert r.pxy[p, k0].imag < 0 and abs(coh[p, k0] - 1.0) <= 1e-9, (L, k0, amp, r.pxy[p, k0], coh[p, k0])
            far = max(far, abs(coh[p, k0] - 1.0))
    edge = r.pxy.imag[:, [0, -1]]
    assert np.all(edge == 0.0) and not np.signbit(edge).any()
    assert np.all(coh[np.isfinite(coh)] <= 1 + 1e-12)
    print('csd single bins L %d %s %s (%d bins, %d pairs): error / tol next bin pxx %.3g pyy %.3g pxy %.3g, same bin %.3g %.3g %.3g; '
          '|coherence - 1| / 1e-9 %.3g' % ((L, win, 'detrend' if det else 'raw', len(ce.bins_of(L)), len(pairs)) + tuple(worst['next'])
                                          + tuple(worst['same']) + (far / 1e-9,)))


# ---- f. as many pairs as the grid takes
def grid_y_limit(ctx):
    """The device's maxGridSize[1], from the refusal's message (as test_gpu_csd.py::test_device_refusals_and_their_order)."""
    from ginsim import _lib
    freq, p, nf = np.empty(8), np.empty(8), C.c_int32(0)
    buf = ctx.upload(np.zeros(64))
    try:
        rc = _lib.lib.ginsim_psd_welch(ctx.handle, buf.ptr, 64, 2 ** 31 - 1, 64, 1.0, 64, 32, 1, 1, _lib.dptr(freq), _lib.dptr(p),
                                       C.byref(nf), 0)
    finally:
        buf.free()
    msg = _lib.lib.ginsim_last_error().decode()
    found = re.search(r'the device takes (\d+)', msg)
    assert rc == _lib.ERR_RANGE and found, msg
    return int(found.group(1))


def test_as_many_pairs_as_the_grid_takes(ctx):
    limit = grid_y_limit(ctx)
    P = min(limit, 70000)
    L, D, n = ce.GRID_L, ce.GRID_D, ce.GRID_N
    a, base = ce.grid_inputs()
    small = ce.device_csd(ctx, a, n, base, L, D, 'hann', True)
    worst = held_to_exact(small, a, n, base, L, D, 'hann', True)
    idx = np.arange(P) % 64
    big = ce.device_csd(ctx, a, n, [base[i] for i in idx], L, D, 'hann', True)
    assert big.pxx.shape == (P, 5)
    same_bits(big, small, slice(None), idx)
    print('csd %d pairs (the grid takes %d): rows vs a call of 64: error / bound 0 (bitwise); the 64 error / tol %.3g' % (P, limit, worst.max()))
    assert worst.max() <= 1.0


# ---- g. cap above nfreq through the C ABI
def test_capacity_above_the_number_of_bins(ctx):
    from ginsim import _lib
    case = cc.CASES[cc.IDS.index('L64_K3_unaligned_hann_detrend')]
    _, L, D, K, tail, kinds, pad, win, det, _ = case
    n, S, stride = cc.shape(case)
    a = cc.rows(case)
    pairs = cc.pairs_of(case) + [(2, 0), (1, 1)]
    want = ce.device_csd(ctx, a, n, pairs, L, D, win, det)
    nb, cap, mark = L // 2 + 1, L // 2 + 1 + 7, -7.5
    freq, out, nf = np.full(cap, mark), np.full((4, len(pairs), cap), mark), C.c_int32(-1)
    tab = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32))
    buf = ctx.upload(a)
    try:
        rc = _lib.lib.ginsim_csd_welch(ctx.handle, buf.ptr, n, S, stride, FS, tab.ctypes.data_as(C.POINTER(C.c_int32)), len(pairs), L, D,
                                       1, 1, _lib.dptr(freq), *[_lib.dptr(out[q]) for q in range(4)], C.byref(nf), cap)
    finally:
        buf.free()
    assert (win, det) == ('hann', True) and rc == _lib.OK and nf.value == nb and len(pairs) == 5
    np.testing.assert_array_equal(freq[:nb], want.freq)
    for q, v in enumerate(planes(want)):
        np.testing.assert_array_equal(out[q, :, :nb], v)               # rows at stride cap
    assert np.all(freq[nb:] == mark) and np.all(out[:, :, nb:] == mark)
    print('csd cap %d above %d bins, %d pairs: error / bound 0 (bitwise)' % (cap, nb, len(pairs)))


# ---- h. the sampling rate
@pytest.mark.parametrize('fs', ce.RATES)
def test_sampling_rate(ctx, fs):
    case = cc.CASES[cc.IDS.index(ce.RATE_SHAPE)]
    _, L, D, K, tail, kinds, pad, win, det, _ = case
    n, S, stride = cc.shape(case)
    a = cc.rows(case)
    pairs = cc.pairs_of(case)
    r = ce.device_csd(ctx, a, n, pairs, L, D, win, det, fs=fs)
    np.testing.assert_array_equal(r.freq, cx.freqs(fs, L))
    worst = held_to_exact(r, a, n, pairs, L, D, win, det, fs=fs)
    print('csd fs %g: error / tol pxx %.3g pyy %.3g pxy %.3g' % ((fs,) + tuple(worst)))
    assert worst.max() <= 1.0


# ---- i. a pair's bits in unusual tables
def test_a_pair_repeated_and_a_series_stored_twice(ctx):
    case = cc.CASES[cc.IDS.index('L512_K3_unaligned_hann_detrend')]
    _, L, D, K, tail, kinds, pad, win, det, _ = case
    n, S, stride = cc.shape(case)
    a = cc.rows(case)
    one = ce.device_csd(ctx, a, n, [(0, 1)], L, D, win, det)
    assert all(np.isfinite(v).all() for v in planes(one))
    many = ce.device_csd(ctx, a, n, [(0, 1)] * 300, L, D, win, det)
    assert many.pxx.shape == (300, L // 2 + 1)
    same_bits(many, one, slice(None), [0] * 300)
    twice = np.concatenate([a, a[[1, 0]]])                             # rows 3 and 4 are rows 1 and 0 again
    r = ce.device_csd(ctx, twice, n, [(0, 1), (4, 3), (0, 3), (4, 1), (2, 0), (2, 4)], L, D, win, det)
    same_bits(r, one, [0, 1, 2, 3], [0] * 4)
    same_bits(r, r, [4], [5])
    print('csd one pair 300 times, and two series stored twice: error / bound 0 (bitwise)')
