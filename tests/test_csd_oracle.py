"""Welch's cross-spectral density without a device: the exact values and the tolerance of tests/csd_exact.py, the float64
restatement of the kernel's packed and separated form inside that tolerance and the recombined form outside it, properties of the
definition, the plan of ginsim_csd_plan through the built library, every refusal that needs no context, the fifth header, the
Python surface and the build's resource report.

Measured here (CPU, long double of 64 mantissa bits; every test prints its figures): the packed restatement reaches 0.52 of the
tolerance at worst (L = 8192; 0.39 up to 4096, the lengths the device takes) over L = 8 .. 8192, D = L/4, L/2, L, both windows,
detrend on and off and the seven pair kinds, and 0.25 on the 50 shapes of tests/csd_cases.py; the recombined form misses it by
factors of 3.6e4 to 1.5e5 in Pyy on the tone against 1e-6 of a tone (L = 64, 1024, 4096)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import csd_cases as cc
import csd_exact as cx
import psd_cases as pc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'gnss-ins-sim_amd')
FS = 100.0


def _three(x, y, L, D, win, det, form):
    exx, eyy, exy, _ = cx.exact(x, y, FS, L, D, win, det)
    t = cx.tol(x, y, FS, L, D, win, det, exx, eyy)
    return cx.ratios(form(x, y, FS, L, D, win, det), (exx, eyy, exy), t)


# ---- the definition and its tolerance
def test_exact_agrees_with_scipy():
    signal = pytest.importorskip('scipy.signal')
    worst = 0.0
    for L, n in ((64, 1000), (1024, 9000)):
        # no offset of 1e6 here: scipy's own float64 detrending leaves 5e-10 of the largest bin on it
        for kind in ('white/white', 'tone/white', 'small/large'):
            x, y = cx.pair(kind, n, 5)
            for win in cx.WINDOWS:
                for det in (True, False):
                    for D in (L // 2, L):
                        exx, eyy, exy, f = cx.exact(x, y, FS, L, D, win, det)
                        kw = dict(window=win, nperseg=L, noverlap=L - D, detrend='constant' if det else False, scaling='density')
                        fr, p = signal.csd(x, y, FS, **kw)
                        np.testing.assert_allclose(fr, f, rtol=1e-15, atol=0)
                        _, pw = signal.welch(x, FS, **kw)
                        _, pv = signal.welch(y, FS, **kw)
                        for got, want in ((p, exy), (pw, exx), (pv, eyy)):
                            r = np.max(np.abs(got - want)) / np.max(np.abs(want))
                            worst = max(worst, r)
                            assert r <= 1e-12, (L, kind, win, det, D)
    print('csd exact against scipy.signal.csd / welch: largest difference %.3g of the largest bin' % worst)


@pytest.mark.parametrize('L', cx.GRID_L)
def test_packed_restatement_stays_within_the_tolerance(L):
    worst = [(0.0, None)] * 3
    n = 3 * L + 5
    for D in (L // 4, L // 2, L):
        for kind in cx.PAIR_KINDS:
            x, y = cx.pair(kind, n, L + D)
            for win in cx.WINDOWS:
                for det in (True, False):
                    r = _three(x, y, L, D, win, det, cx.packed)
                    worst = [max(w, (ri, (D, kind, win, det))) for w, ri in zip(worst, r)]
    for name, w in zip(('pxx', 'pyy', 'pxy'), worst):
        print('csd packed restatement L %d %s: error / tol %.3g at %s' % (L, name, w[0], w[1]))
    assert max(w[0] for w in worst) <= 1.0


def test_recombined_form_is_outside_the_tolerance():
    """The tolerance can tell the separated sums from the recombined ones: Pyy = (sum AA + sum BB - 2 Re sum AB) / 4 cancels when
    y is 1e-6 of x."""
    for L in (64, 1024, 4096):
        x, y = cx.pair('tone/smalltone', 3 * L + 5, L)
        sep = _three(x, y, L, L // 2, 'hann', True, cx.packed)
        rec = _three(x, y, L, L // 2, 'hann', True, cx.recombined)
        print('csd L %d tone / 1e-6 tone: separated error / tol %.3g %.3g %.3g, recombined %.3g %.3g %.3g' % ((L,) + sep + rec))
        assert max(sep) <= 1.0 and rec[1] > 1e3
        # on a pair of equal scale the two forms are the same estimate
        x, y = cx.pair('white/white', 3 * L + 5, L)
        assert max(_three(x, y, L, L // 2, 'hann', True, cx.recombined)) <= 1.0


def test_restatement_on_every_gpu_shape():
    """The reference's own margin on the shapes the device is held to (tests/csd_cases.py)."""
    worst = (0.0, None)
    for case in cc.CASES:
        name, L, D, K, tail, kinds, pad, win, det, _ = case
        n, S, stride = cc.shape(case)
        a = cc.rows(case)
        for i, j in cc.pairs_of(case):
            r = max(_three(a[i, :n], a[j, :n], L, D, win, det, cx.packed))
            assert r <= 1.0, (name, i, j, r)
            worst = max(worst, (r, name))
    print('csd packed restatement on the %d device shapes: error / tol %.3g at %s' % (len(cc.CASES), worst[0], worst[1]))


def test_mirror_of_a_bit_reversed_position_is_an_xor():
    """The identity csd.hip reads its mirror bin by: bin k = rev(2j) of butterfly j >= 1 has its mirror L - k at position
    2 j' + 1 with j' = j ^ (2^floor(log2 j) - 1); 64 consecutive j >= 64 read 64 consecutive j' in descending order."""
    for lg in range(3, 13):
        L = 1 << lg
        rev = lambda v: int(format(v, '0%db' % lg)[::-1], 2)        # noqa: E731
        jm = [j ^ ((1 << (j.bit_length() - 1)) - 1) for j in range(1, L // 2)]
        for j, m in zip(range(1, L // 2), jm):
            k = rev(2 * j)
            assert 0 < k < L // 2 and rev(L - k) == 2 * m + 1
        assert sorted(jm) == list(range(1, L // 2)) and (rev(0), rev(1)) == (0, L // 2)
        for base in range(64, L // 2, 64):
            assert jm[base - 1:base + 63] == list(range(jm[base - 1], jm[base - 1] - 64, -1))


# ---- properties of the definition, on the restatement
def test_swapping_the_series_conjugates_and_a_series_with_itself_is_its_psd():
    """Exact identities of the definition; two float64 evaluations differ by what each may differ from the exact value."""
    x, y = cx.pair('tone/white', 2000, 3)
    L, D = 256, 128
    pxx, pyy, pxy = cx.packed(x, y, FS, L, D)
    qxx, qyy, qxy = cx.packed(y, x, FS, L, D)
    exx, eyy, exy, _ = cx.exact(x, y, FS, L, D)
    fxx, fyy, fxy, _ = cx.exact(y, x, FS, L, D)
    np.testing.assert_array_equal(fxy, np.conj(exy))
    np.testing.assert_array_equal(fxx, eyy)
    txx, tyy, txy = cx.tol(x, y, FS, L, D, 'hann', True, exx, eyy)
    assert np.all(np.abs(qxy - np.conj(pxy)) <= 2 * txy)
    assert np.all(np.abs(qxx - pyy) <= 2 * tyy) and np.all(np.abs(qyy - pxx) <= 2 * txx)
    sxx, syy, sxy = cx.packed(x, x, FS, L, D)
    gxx, gyy, gxy, _ = cx.exact(x, x, FS, L, D)
    np.testing.assert_array_equal(gxy.imag, 0.0)
    np.testing.assert_array_equal(gxy.real, gxx)
    uxx, _, uxy = cx.tol(x, x, FS, L, D, 'hann', True, gxx, gyy)
    assert np.all(np.abs(sxy.imag) <= uxy) and np.all(np.abs(sxy.real - sxx) <= uxy + uxx) and np.all(np.abs(sxx - syy) <= 2 * uxx)
    assert np.all(pxy.imag[[0, -1]] == 0.0)


def test_a_delay_is_a_linear_phase_at_full_coherence():
    n, L, D, lag = 8192, 256, 128, 3
    x = np.random.default_rng(1).standard_normal(n + lag)
    y, x = x[:n], x[lag:]                            # y[t] = x[t - 3]
    pxx, pyy, pxy = cx.packed(x, y, FS, L, D)
    k = np.arange(1, L // 2)
    coh = (np.abs(pxy) ** 2 / (pxx * pyy))[k]
    want = -2 * np.pi * lag * k / L
    dphi = np.angle(pxy[k] * np.exp(-1j * want))
    print('csd delay of 3 samples: smallest coherence %.4f, largest phase error %.4f rad' % (coh.min(), np.abs(dphi).max()))
    assert coh.min() > 0.98 and np.abs(dphi).max() < 0.03
    assert np.all(coh <= 1 + 1e-12)


def test_independent_white_series_have_coherence_one_over_k():
    n, L, D = 8192, 256, 128
    K = cx.segments(n, L, D)
    x, y = cx.pair('white/white', n, 2)
    pxx, pyy, pxy = cx.packed(x, y, FS, L, D)
    coh = np.abs(pxy) ** 2 / (pxx * pyy)
    print('csd independent white series: mean coherence %.4f at K = %d (1 / K = %.4f)' % (coh.mean(), K, 1.0 / K))
    assert K == 63 and 0.0125 / 2 <= coh.mean() <= 0.0125 * 2


# ---- the plan, through the built library
def _table_doubles(L):
    q = L // 4
    return (q + (q >> 5) + (q >> 10) + 2) & ~1


def _plan_restated(n, npairs, L, D):
    K = (n - L) // D + 1
    spp = pc.segs_per_part(L, D)
    nparts = -(-K // spp)
    T = min(max(L // 4, 64), 512)
    lds = 8 * (2 * L + _table_doubles(L) + (2 * (T // 64) if T > 64 else 0))
    pad = lambda b: (b + 255) // 256 * 256           # noqa: E731
    scratch = pad(8 * 4 * (L // 2 + 1) * npairs * nparts) + pad(8 * npairs)
    return dict(segments=K, scratch_bytes=scratch, segs_per_part=spp, nparts=nparts, lds_bytes=lds, threads=T)


def test_plan_follows_the_formulas():
    import ginsim
    for case in cc.CASES:
        _, L, D, K, tail, kinds, pad, _, _, where = case
        n, S, stride = cc.shape(case)
        npairs = len(cc.pairs_of(case))
        g = ginsim.csd_plan(n, S, stride, FS, npairs, L, D)
        assert g == _plan_restated(n, npairs, L, D), case[0]
        assert g['segments'] == K and g['lds_bytes'] <= 160 * 1024
        if where is not None:
            assert K == where[0] * g['segs_per_part'] + where[1], case[0]
        for np2, S2 in ((1, 1), (7, 3), (4096, 192)):          # the partition depends on (n, L, D) alone
            g2 = ginsim.csd_plan(n, S2, n, FS, np2, L, D)
            assert all(g2[k] == g[k] for k in ('segments', 'segs_per_part', 'nparts', 'threads', 'lds_bytes'))
        w = ginsim.welch_plan(n, S, stride, FS, L, D)          # and is the PSD's
        assert all(w[k] == g[k] for k in ('segments', 'segs_per_part', 'nparts', 'threads', 'lds_bytes'))
    g = ginsim.csd_plan(1440000, 192, 1440000, 400.0, 96, 1024)            # step defaults to half a segment
    assert (g['segments'], g['segs_per_part'], g['nparts']) == (2811, 32, 88)


def _err():
    from ginsim import _lib
    return _lib.lib.ginsim_last_error().decode()


BAD_SIZES = [dict(n=0), dict(S=0), dict(S=-1), dict(stride=99), dict(fs=0.0), dict(fs=-1.0), dict(fs=float('inf')),
             dict(fs=float('nan'))]
BAD_NPERSEG = [0, -8, 4, 7, 12, 1000, 16384, 4097]
MAX_PARTS = 2 ** 31 - 1
N_LAST = MAX_PARTS * 16384 + 7               # L = 8, D = 1: the longest series of 2^31 - 1 parts


def test_plan_refusals_and_their_order():
    from ginsim import _lib
    fields = [k for k, _ in _lib.CsdGeometry._fields_]
    g = _lib.CsdGeometry(-11, -12, -13, -14, -15, -16)
    before = [getattr(g, k) for k in fields]

    def call(n=100, S=1, stride=None, fs=1.0, P=1, L=64, D=32, gp=True):
        return _lib.lib.ginsim_csd_plan(n, S, n if stride is None else stride, fs, P, L, D, C.byref(g) if gp else None)
    assert call(n=0, P=0, L=7, D=0, gp=False) == _lib.ERR_ARG and _err() == 'csd_plan: NULL argument'
    for kw in BAD_SIZES:
        assert call(P=0, L=7, D=0, **kw) == _lib.ERR_ARG and _err() == 'csd_plan: bad sizes', kw           # before npairs
    for P in (0, -1):
        assert call(P=P, L=7, D=0) == _lib.ERR_ARG and _err().startswith('csd_plan: npairs %d' % P)        # before nperseg
    for L in BAD_NPERSEG:
        assert call(L=L, D=0) == _lib.ERR_ARG and _err() == 'csd_plan: nperseg %d is not a power of two in [8, 4096]' % L
    assert call(n=10, L=8192, D=0) == _lib.ERR_ARG                                                         # before step
    assert _err().startswith('csd_plan: nperseg 8192 is not taken') and 'registers' in _err() and '4096' in _err()
    for D in (0, -1, 65):
        assert call(n=10, D=D) == _lib.ERR_ARG and _err() == 'csd_plan: step %d outside [1, 64]' % D        # before the length
    assert call(n=63) == _lib.ERR_RANGE and _err() == 'csd_plan: a series of n = 63 samples is shorter than one segment of nperseg = 64'
    # parts, then bytes; n < nperseg before both
    assert call(n=N_LAST + 1, L=8, D=1) == _lib.ERR_RANGE and '%d parts' % 2 ** 31 in _err() and _err().startswith('csd_plan: ')
    assert call(n=N_LAST + 1, P=2 ** 31 - 1, L=8, D=1) == _lib.ERR_RANGE and '%d parts' % 2 ** 31 in _err()
    assert call(n=N_LAST, P=2 ** 31 - 1, L=8, D=1) == _lib.ERR_RANGE and '2^63 bytes' in _err() and '%d parts' % MAX_PARTS in _err()
    assert call(n=7, S=2 ** 31 - 1, stride=2 ** 62, P=2 ** 31 - 1, L=8, D=1) == _lib.ERR_RANGE and 'shorter than one segment' in _err()
    assert [getattr(g, k) for k in fields] == before             # a refused plan leaves *g as it was
    # the largest table of that length whose scratch stays below 2^63 bytes
    pad = lambda b: (b + 255) // 256 * 256           # noqa: E731
    fits = lambda P: 160 * MAX_PARTS * P + 255 + pad(8 * P) <= 2 ** 63 - 1       # noqa: E731
    P = (2 ** 63) // (160 * MAX_PARTS)
    while not fits(P):
        P -= 1
    assert fits(P) and not fits(P + 1) and call(n=N_LAST, P=P, L=8, D=1) == _lib.OK
    assert g.scratch_bytes == pad(160 * MAX_PARTS * P) + pad(8 * P) < 2 ** 63 and g.nparts == MAX_PARTS
    assert call(n=N_LAST, P=P + 1, L=8, D=1) == _lib.ERR_RANGE and '2^63 bytes' in _err()
    assert call(n=64) == _lib.OK and (g.segments, g.nparts) == (1, 1)
    for L in (8, 4096):
        assert call(n=4096, L=L, D=L) == _lib.OK
    hdr = open(os.path.join(REPO, 'include', 'ginsim_csd.h')).read()
    order = [hdr.index(w) for w in ('a NULL argument;', 'npairs < 1;', 'nperseg not a power', 'window or detrend',
                                    'index outside [0, nseries)', 'n < nperseg;', '2^31 - 1 parts', "device's maxGridSize[1]",
                                    'below *nfreq')]
    assert order == sorted(order)


def test_call_refusals_with_a_null_context():
    """NULL first, with everything else wrong too; nothing is written.  (The refusals behind it need a context:
    tests/test_gpu_csd.py.)"""
    from ginsim import _lib
    arr = [np.empty(4) for _ in range(5)]
    tab, nf = np.zeros(2, dtype=np.int32), C.c_int32(-7)
    fn = _lib.lib.ginsim_csd_welch
    ok = [1 << 30, tab.ctypes.data_as(C.POINTER(C.c_int32))] + [_lib.dptr(a) for a in arr] + [C.byref(nf)]
    for hole in range(len(ok)):
        x, t, f, a, b, c, d, q = [None if i == hole else v for i, v in enumerate(ok)]
        assert fn(None, x, 0, 0, 0, -1.0, t, 0, 7, 0, 5, 5, f, a, b, c, d, q, 0) == _lib.ERR_ARG
        assert _err() == 'csd: NULL argument' and nf.value == -7
    assert fn(None, ok[0], 100, 1, 100, 1.0, ok[1], 1, 64, 32, 1, 1, *ok[2:], 33) == _lib.ERR_ARG and _err() == 'csd: NULL argument'


def test_python_arguments():
    import ginsim
    with pytest.raises(ValueError, match='window'):
        ginsim.welch_csd(None, 0, 100, 1, 100, 1.0, [(0, 0)], 64, window='hamming')
    with pytest.raises(ValueError, match='pairs'):
        ginsim.welch_csd(None, 0, 100, 1, 100, 1.0, [0, 1], 64)
    with pytest.raises(ValueError, match='csd_plan: nperseg 100'):
        ginsim.csd_plan(1000, 1, 1000, 1.0, 1, 100)
    with pytest.raises(ValueError, match='csd_plan: nperseg 8192 is not taken'):
        ginsim.csd_plan(100000, 1, 100000, 1.0, 1, 8192)


# ---- the fifth header, the fifth table
def test_header_compiles_as_c99_and_its_names_are_exported_and_bound(tmp_path):
    import ginsim
    src = tmp_path / 'h.c'
    src.write_text('#include "ginsim_csd.h"\n'
                   'int main(void) { ginsim_csd_geometry g; g.segments = 1; g.nparts = 2;\n'
                   '  return (int)(g.segments + g.nparts) + (GINSIM_ABI_VERSION == 9 ? 0 : 1); }\n')
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I' + os.path.join(REPO, 'include'),
                    '-fsyntax-only', str(src)], check=True, timeout=120)
    hdr = open(os.path.join(REPO, 'include', 'ginsim_csd.h')).read()
    declared = set(re.findall(r'\b(ginsim_[a-z0-9_]+)\s*\(', hdr))
    assert declared == {'ginsim_csd_welch', 'ginsim_csd_plan'} == set(ginsim.CSD_EXPORTS)
    raw = C.CDLL(ginsim.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name) and getattr(ginsim.lib, name).argtypes is not None
    others = set(ginsim.EXPORTS) | set(ginsim.OALLAN_EXPORTS) | set(ginsim.PSD_EXPORTS) | set(ginsim.LPSD_EXPORTS)
    assert not declared & others and len(ginsim.EXPORTS) == 86
    from ginsim import _lib
    assert C.sizeof(_lib.CsdGeometry) == 32
    assert ginsim.lib.ginsim_abi_version() == 9
    readme = open(os.path.join(REPO, 'README.md')).read()
    assert '86 entry points' in readme and 'ginsim_csd.h' in readme


def test_python_surface():
    import ginsim
    from ginsim import multi
    for name in ('welch_csd', 'welch_csd_host', 'csd_plan', 'CsdResult'):
        assert callable(getattr(ginsim, name))
    for prop in ('coherence', 'phase', 'transfer', 'gain'):
        assert isinstance(getattr(ginsim.CsdResult, prop), property)
    assert callable(ginsim.MonteCarloJob.csd) and callable(multi.JobSet.csd)
    r = ginsim.CsdResult(np.arange(3.0), np.array([[0, 1]]), np.array([[4.0, 0.0, 1.0]]), np.array([[1.0, 2.0, 4.0]]),
                         np.array([[2.0 + 0j, 1j, -2j]]))
    np.testing.assert_array_equal(r.coherence, [[1.0, np.nan, 1.0]])
    np.testing.assert_array_equal(r.phase, np.angle(r.pxy))
    np.testing.assert_array_equal(r.transfer[0, [0, 2]], [0.5, -2j])
    np.testing.assert_array_equal(r.gain[0, [0, 2]], [0.5, 2.0])
    from demo_algorithms import csd_analysis
    from gnss_ins_sim.sim import ins_data_manager
    p = csd_analysis.Coherence()
    assert p.input == ['fs', 'accel', 'gyro'] and p.output == ['csd_freq', 'coherence', 'csd_phase']
    assert (p.pairs, p.nperseg, p.step, p.window, p.detrend) == (None, 1024, None, 'hann', True)
    assert all(callable(getattr(p, m)) for m in ('run', 'run_device', 'get_results', 'reset')) and p.get_results() is None
    d = ins_data_manager.InsDataMgr([100.0, None, None], 0)
    for name in p.output:
        assert d.is_supported(name)


def test_resource_report_has_every_segment_length_and_no_scratch():
    path = os.path.join(PKG, 'build', 'csd.resources.txt')
    assert os.path.exists(path), 'build.py writes it next to the object'
    blocks = open(path).read().split('Function Name: ')[1:]
    parts = {int(m.group(1)): b for b in blocks for m in [re.search(r'csd_part_kernelILi(\d+)E', b)] if m}
    assert sorted(parts) == [1 << k for k in range(3, 13)]
    assert any('csd_finish_kernel' in b for b in blocks)
    for b in blocks:
        assert re.search(r'ScratchSize \[bytes/lane\]: (\d+)', b).group(1) == '0', b.splitlines()[0]
    import ginsim
    for L, b in parts.items():
        lds = int(re.search(r'LDS Size \[bytes/block\]: (\d+)', b).group(1))
        assert lds == ginsim.csd_plan(L, 1, L, 1.0, 1, L)['lds_bytes'], L            # the plan reports what the kernel takes
