"""The Welch PSD kernel (csrc/psd.hip through ginsim_psd_welch) at its edges: every segment length under every option, every
place a non-finite sample can sit in a part, magnitude alone, the grid's y limit, calls in sequence on one context, a capacity
above the number of bins and the sampling rate.  The shapes, the exact values and the tolerance are those of tests/psd_cases.py
and tests/psd_exact.py; a result is held to `exact` within `tol` (error / tol <= 1) or to another launch bit for bit.  Every test
prints its error over its bound."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import psd_cases as pc
import psd_exact as px

pytestmark = pytest.mark.gpu

FS = 100.0
device_psd = pc.device_psd


@pytest.fixture(scope='module')
def ctx():
    import ginsim
    c = ginsim.Context(0)
    yield c
    c.close()


def case_of(name):
    return pc.CASES[pc.IDS.index(name)]


def worst_ratio(p, a, n, fs, L, D, win, det):
    """Largest error / tol of the device's rows p against the exact values of the series a[:, :n]."""
    worst = 0.0
    for s in range(a.shape[0]):
        e, _ = px.exact(a[s, :n], fs, L, D, win, det)
        worst = max(worst, px.ratio(p[s], e, px.tol(a[s, :n], fs, L, D, win, det, e)))
    return worst


# ---- a. every segment length under every option
LENGTHS = [1 << k for k in range(3, 14)]
OPTIONS = [(w, d) for w in px.WINDOWS for d in (True, False)]


def psd_threads(L):
    """csrc/psd.hpp restated."""
    return min(max(L // 4, 64), 512)


@functools.lru_cache(maxsize=None)
def odd_step_case(L):
    """K = 3 (the last segment pairs with zeros), D = L/2 + 1 (odd, above half a segment), one unread sample, a stride pad of 1."""
    case = ('L%d_K3_odd_step' % L, L, L // 2 + 1, 3, 1, ('white', 'tone', 'offset'), 1, None, None, None)
    a = pc.rows(case)
    a.setflags(write=False)
    return case, a


@pytest.mark.parametrize('win,det', OPTIONS, ids=['%s_%s' % (w, 'detrend' if d else 'raw') for w, d in OPTIONS])
@pytest.mark.parametrize('L', LENGTHS)
def test_every_length_under_every_option(ctx, L, win, det):
    import ginsim
    case, a = odd_step_case(L)
    D, K = case[2], case[3]
    n, S, stride = pc.shape(case)
    assert D % 2 == 1 and D > L // 2 and n == 2 * D + L + 1 and stride == n + 1 and px.segments(n, L, D) == K
    g = ginsim.welch_plan(n, S, stride, FS, L, D)
    assert g['threads'] == psd_threads(L) and (g['segments'], g['nparts']) == (K, 1)
    p, f = device_psd(ctx, a, n, L, D, win, det)
    assert p.shape == (S, L // 2 + 1)
    np.testing.assert_array_equal(f, px.freqs(FS, L))
    worst = worst_ratio(p, a, n, FS, L, D, win, det)
    print('psd length %d %s %s (%d threads): error / tol %.3g' % (L, win, 'detrend' if det else 'raw', g['threads'], worst))
    assert worst <= 1.0


# ---- b. where a non-finite sample sits
def marked_batch(L, K, spp):
    """No overlap (D = L): every sample belongs to exactly one segment.  Clean series at the even rows; every odd row has ONE
    non-finite value (or pair, or magnitude) of its own.  Returns (clean, marked, hit rows, what each hit row holds)."""
    assert K == spp + 1
    n = K * L
    segs = [0, 1, spp // 2, spp // 2 + 1, spp - 1, spp]     # first pair's planes, an even and an odd one inside, part 0's last, the lone one
    assert segs[2] % 2 == 0 and segs[3] % 2 == 1 and segs[2] > 1 and segs[3] < spp - 1
    places = [(s, k, v) for s in segs for k in (0, L // 2, L - 1) for v in (np.nan, np.inf, -np.inf)]
    S = 2 * (len(places) + 2) + 1
    kinds = ('white', 'tone', 'walk')
    clean = np.stack([px.series(kinds[r % 3], n, 100 + r) for r in range(S)])
    marked = clean.copy()
    what = {}
    for i, (s, k, v) in enumerate(places):
        marked[2 * i + 1, s * L + k] = v
        what[2 * i + 1] = 'segment %d sample %d value %r' % (s, k, v)
    r = 2 * len(places) + 1
    marked[r, (spp // 2) * L + 3] = np.inf
    marked[r, (spp // 2) * L + L - 5] = -np.inf
    what[r] = '+Inf and -Inf in segment %d' % (spp // 2)
    marked[r + 2, :] = 1.7e308
    what[r + 2] = '1.7e308 throughout: finite samples, the segment sum overflows'
    assert np.isfinite(marked[r + 2]).all() and sorted(what) == list(range(1, S, 2))
    return clean, marked, sorted(what), what


@pytest.mark.parametrize('L,K', [(128, 129), (2048, 9)], ids=['L128_one_wavefront', 'L2048_eight_wavefronts'])
def test_a_non_finite_sample_marks_its_series_wherever_it_sits(ctx, L, K):
    import ginsim
    D = L
    g = ginsim.welch_plan(K * L, 1, K * L, FS, L, D)
    spp = g['segs_per_part']
    assert (g['segments'], g['nparts']) == (K, 2) and K == spp + 1 and g['threads'] == psd_threads(L)
    assert px.window(L, 'hann', np.float64)[0] == 0.0               # sample 0 of a segment has no weight
    clean, marked, hit, what = marked_batch(L, K, spp)
    n, S = clean.shape[1], clean.shape[0]
    rest = [s for s in range(S) if s not in hit]
    for win, det in (('hann', True), ('hann', False), ('boxcar', False)):
        ref, _ = device_psd(ctx, clean, n, L, D, win, det)
        assert np.isfinite(ref).all()
        got, _ = device_psd(ctx, marked, n, L, D, win, det)
        for s in hit:
            assert np.isnan(got[s]).all(), (win, det, what[s], int(np.isnan(got[s]).sum()))
        np.testing.assert_array_equal(got[rest], ref[rest])
    print('psd non-finite places L %d (%d marked of %d series, 3 options): error / bound 0 (bitwise)' % (L, len(hit), S))


# ---- c. magnitude alone marks nothing
@pytest.mark.parametrize('name', ['L128_one_bin_more_than_lanes', 'L2048_half_overlap_part_plus_3'])
def test_magnitude_alone_marks_nothing(ctx, name):
    """A power of two scales every operation of the kernel exactly as long as nothing overflows or goes subnormal: the series
    times 2^460 gives 2^920 times the result, bit for bit."""
    case = case_of(name)
    _, L, D, K, tail, kinds, pad, win, det, _ = case
    n, S, stride = pc.shape(case)
    pick = [kinds.index('white'), kinds.index('tone')]              # not the offset of 1e6
    a = pc.rows(case)[pick][:, :n]
    big = np.ldexp(a, 460)
    assert np.isfinite(big).all()
    for s in range(2):
        e, _ = px.exact(big[s], FS, L, D, win, det)
        assert np.isfinite(e).all() and e.max() > 2.0 ** 900       # on the host: the exact values of the scaled series are finite
    p, _ = device_psd(ctx, a, n, L, D, win, det)
    q, _ = device_psd(ctx, big, n, L, D, win, det)
    assert np.isfinite(q).all()
    assert np.all((p == 0.0) | (p > 2.0 ** -500))                   # no subnormal on either side
    np.testing.assert_array_equal(q, np.ldexp(p, 920))
    worst = worst_ratio(p, a, n, FS, L, D, win, det)
    print('psd scaled by 2^460 %s: error / bound 0 (bitwise); unscaled error / tol %.3g' % (name, worst))
    assert worst <= 1.0


# ---- e. calls in sequence on one context (before the large call of d: the pinned buffer grows inside this test)
def test_calls_in_sequence_equal_first_calls_on_fresh_contexts(ctx):
    import ginsim
    large, small = case_of('L8_D1_two_parts_plus_1'), case_of('L64_D3_fewer_bins_than_lanes')
    wide = ('L8192_K1_S128', 8192, 8192, 1, 0, ('white', 'tone') * 64, 0, 'boxcar', True, None)    # 128 x 4097 results
    allan_series = np.stack([px.series(k, 4096, 7 + i) for i, k in enumerate(('white', 'walk', 'offset'))])

    def psd_call(c, case):
        _, L, D, K, tail, kinds, pad, win, det, _ = case
        n, S, stride = pc.shape(case)
        return device_psd(c, pc.rows(case), n, L, D, win, det)[0]

    def allan_call(c, _):
        return ginsim.allan_var_host(c, allan_series, FS)[0]
    order = [(psd_call, large), (psd_call, small), (allan_call, None), (psd_call, wide), (psd_call, small)]
    # more results than any call of this file before it, the 70 000 rows of 5 bins below included, whatever the order
    assert 128 * 4097 > (70000 * 5) * 5 // 4 + 64
    got = [fn(ctx, case) for fn, case in order]
    for (fn, case), have in zip(order, got):
        fresh = ginsim.Context(0)
        try:
            first = fn(fresh, case)
        finally:
            fresh.close()
        assert np.isfinite(first).all()
        np.testing.assert_array_equal(have, first)
    np.testing.assert_array_equal(got[1], got[4])
    print('psd calls in sequence vs fresh contexts: error / bound 0 (bitwise)')


# ---- d. the grid's y limit
def grid_y_limit(ctx):
    """The device's maxGridSize[1], from the refusal's message (as test_gpu_psd.py::test_device_refusals_and_their_order)."""
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


def test_as_many_series_as_the_grid_takes(ctx):
    limit = grid_y_limit(ctx)
    S = min(limit, 70000)
    L, D, n = 8, 3, 17
    assert px.segments(n, L, D) == 4 and 3 * D + L == n
    base = np.stack([px.series(px.KINDS[r % 5], n, 300 + r) for r in range(64)])
    small, _ = device_psd(ctx, base, n, L, D, 'hann', True)
    worst = worst_ratio(small, base, n, FS, L, D, 'hann', True)
    big, _ = device_psd(ctx, base[np.arange(S) % 64], n, L, D, 'hann', True)
    assert big.shape == (S, 5)
    np.testing.assert_array_equal(big, small[np.arange(S) % 64])
    print('psd %d series (the grid takes %d): rows vs a call of 64: error / bound 0 (bitwise); the 64 error / tol %.3g' % (S, limit, worst))
    assert worst <= 1.0


# ---- f. cap above nfreq through the C ABI
def test_capacity_above_the_number_of_bins(ctx):
    from ginsim import _lib
    case = case_of('L64_D3_fewer_bins_than_lanes')
    _, L, D, K, tail, kinds, pad, win, det, _ = case
    n, S, stride = pc.shape(case)
    a = pc.rows(case)
    want, wf = device_psd(ctx, a, n, L, D, win, det)
    nb, cap, mark = L // 2 + 1, L // 2 + 1 + 7, -7.5
    freq, p, nf = np.full(cap, mark), np.full((S, cap), mark), C.c_int32(-1)
    buf = ctx.upload(a)
    try:
        rc = _lib.lib.ginsim_psd_welch(ctx.handle, buf.ptr, n, S, stride, FS, L, D, 1, 1, _lib.dptr(freq), _lib.dptr(p), C.byref(nf), cap)
    finally:
        buf.free()
    assert (win, det) == ('hann', True) and rc == _lib.OK and nf.value == nb
    np.testing.assert_array_equal(freq[:nb], wf)
    np.testing.assert_array_equal(p[:, :nb], want)                  # rows at stride cap
    assert np.all(freq[nb:] == mark) and np.all(p[:, nb:] == mark)
    print('psd cap %d above %d bins: error / bound 0 (bitwise)' % (cap, nb))


# ---- g. the sampling rate
@pytest.mark.parametrize('fs', [1e-3, 1.0, 12345.678, 1e6])
def test_sampling_rate(ctx, fs):
    case = case_of('L256_step_half_plus_one')
    _, L, D, K, tail, kinds, pad, win, det, _ = case
    n, S, stride = pc.shape(case)
    a = pc.rows(case)
    p, f = device_psd(ctx, a, n, L, D, win, det, fs=fs)
    np.testing.assert_array_equal(f, px.freqs(fs, L))
    worst = worst_ratio(p, a, n, fs, L, D, win, det)
    print('psd fs %g: error / tol %.3g' % (fs, worst))
    assert worst <= 1.0
