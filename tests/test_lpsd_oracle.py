"""The multi-resolution PSD without a device: the half-band table against its generator and its two figures, the restatement of
tests/lpsd_ref.py against analysis (a tone, white noise, the tiling of the octaves), its float64 arithmetic against long double
on every shape the device is held to, the plan of ginsim_lpsd_plan through the built library, every refusal that needs no context,
the fourth header, the Python surface and the build's resource report.

Measured here (CPU): the table's passband deviation 2.998e-5 and stopband level 1.560e-10 on the 20 001-point grids (the bounds
are 3.0e-5 and 1.92e-10); the tone's integrated power is off by 2.4e-5 of itself (bound 9.0e-5); the white level's worst
octave of eight is at 0.34 of its five standard errors; the float64 restatement's figures are lpsd_cases.DEV."""
import ctypes as C
import importlib.util
import math
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import lpsd_cases as lc
import lpsd_ref as ref
import psd_exact as px

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'gnss-ins-sim_amd')
GEN = os.path.join(REPO, 'tools', 'gen_halfband_table.py')
FS = 100.0
PASSBAND, STOPBAND = 2.5e-5, 1.6e-10            # the design's two figures; the table is held to 1.2 times each


def _gen():
    spec = importlib.util.spec_from_file_location('gen_halfband_table', GEN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the table
def test_the_committed_table_is_what_its_generator_writes():
    r = subprocess.run([sys.executable, GEN, '--check'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout
    np.testing.assert_array_equal(_gen().taps(), ref.taps())


def test_table_is_symmetric_half_band_and_of_unit_gain():
    h = ref.taps()
    assert h.size == 27 and np.all(h == h[::-1])
    m = np.arange(27) - 13
    assert np.all(h[(m % 2 == 0) & (m != 0)] == 0.0) and np.count_nonzero(h) == 15
    assert abs(h[13] - 0.5) < 1e-5                              # exactly 0.5 before the division by the sum
    assert abs(math.fsum(h) - 1.0) <= 2.0 ** -52
    hl = ref.taps(np.longdouble)
    assert hl.dtype == np.longdouble and np.all(hl.astype(np.float64) == h)


def test_table_meets_the_designs_two_figures():
    p, s = _gen().figures(ref.taps(), 20001)
    print('half-band table: passband deviation %.4g (bound %.4g), stopband %.4g (bound %.4g)' % (p, 1.2 * PASSBAND, s, 1.2 * STOPBAND))
    assert p <= 1.2 * PASSBAND
    assert s <= 1.2 * STOPBAND


# ---- one decimation
def test_decimation_counts_and_float64_against_long_double():
    assert [ref.n_out(n) for n in (0, 26, 27, 28, 29, 30)] == [0, 0, 1, 1, 2, 2]
    for n, seed in ((27, 1), (28, 2), (500, 3), (2 * ref.TILE + 27, 4)):
        for kind in ('white', 'offset', 'walk'):
            x = px.series(kind, n, seed)
            y, e = ref.decimate(x), ref.decimate(x, np.longdouble)
            assert y.shape == e.shape == (ref.n_out(n),) and y.dtype == np.float64 and e.dtype == np.longdouble
            assert np.all(np.abs(y - e) <= ref.decimate_bound(x))
            direct = np.array([np.dot(ref.taps(np.longdouble), x[2 * i:2 * i + 27].astype(np.longdouble)) for i in range(min(y.size, 9))])
            assert np.all(np.abs(direct - e[:direct.size]) <= ref.decimate_bound(x)[:direct.size] * 2.0 ** -8)
    assert ref.decimate(np.ones(26)).size == 0
    assert np.all(np.abs(ref.decimate(np.ones(100)) - 1.0) <= 4 * 2.0 ** -53)          # unit gain at f = 0


def test_a_non_finite_sample_reaches_the_outputs_whose_taps_touch_it():
    n = 200
    x = px.series('white', n, 5)
    clean = ref.decimate(x)
    for bad, val in (([0], np.nan), ([n - 1], np.inf), ([n - 2], np.nan), ([80], np.inf), ([81], -np.inf), ([70, 72], [np.inf, -np.inf])):
        z = x.copy()
        z[bad] = val
        y = ref.decimate(z)
        hit = ref.touched(n, bad)
        np.testing.assert_array_equal(~np.isfinite(y), hit)
        np.testing.assert_array_equal(y[~hit], clean[~hit])
    # an odd sample is the centre of one output and nothing else; an even one is a pair tap of up to 14
    assert ref.touched(n, [81]).sum() == 1 and ref.touched(n, [80]).sum() == 14 and ref.touched(n, [0]).sum() == 1


# ---- the restatement against analysis
def test_a_tone_is_found_in_the_octave_of_its_level_with_its_power():
    """A pure tone of amplitude A at 2.2 Hz, L = 256 at 100 Hz, five levels: level 3 (12.5 Hz) reports 1.5625 .. 3.08 Hz and no
    other level reports 2.2 Hz; the tone sits 13 bins from either edge of that octave.  The octave's integrated density is A^2/2
    up to (a) the gain of the three filters it has passed, each within 1.2 * 2.5e-5 of 1 below an eighth of its input rate, and
    (b) the Hann window's leakage past 12 bins, sum over |d| >= 12 of |W(d)|^2 / (1.5 |W(0)|^2) with |W(d) / W(0)| = 1 / (pi d
    (d^2 - 1)) at most: 2 / (1.5 pi^2) * sum_{d >= 12} 1 / (d^2 (d^2 - 1)^2) < 6e-8, doubled for the image at negative
    frequencies and the window's own term at twice the frequency."""
    L, D, A, f0 = 256, 128, 3.0, 2.2
    n = ref.shortest(4, L, D, 4)
    x = A * np.sin(2 * np.pi * f0 / FS * np.arange(n) + 0.4)
    p, f, lev = ref.lpsd(x, FS, L, D, 'hann', True, 4)
    assert lev.max() == 4 and np.all(np.diff(f) > 0)
    assert lev[np.argmin(np.abs(f - f0))] == 3 and set(lev[(f > 1.6) & (f < 3.0)]) == {3}
    k = int(np.argmax(p))
    assert lev[k] == 3 and abs(f[k] - f0) <= FS / 8 / L
    octave = lev == 3
    power = p[octave].sum() * (FS / 8 / L)
    leak = 2 * 2 / (1.5 * math.pi ** 2) * sum(1.0 / (d * d * (d * d - 1) ** 2) for d in range(12, 4000))
    bound = 3 * 1.2 * PASSBAND + leak
    print('lpsd tone: integrated power off by %.3g of itself, bound %.3g' % (abs(power / (A * A / 2) - 1), bound))
    assert abs(power / (A * A / 2) - 1.0) <= bound
    # and nowhere else: what the other bins hold is the segment mean that detrending takes out of a tone of at least 45 cycles
    # per segment, at most A / (45 pi), in the two lowest bins of the last level
    elsewhere = (p * FS / 2.0 ** lev / L)[~octave].sum()
    assert elsewhere <= (A / (45 * math.pi)) ** 2


def test_white_noise_has_one_level_in_every_octave():
    """White noise of variance 1: 2 / fs in every octave.  Standard error of an octave's mean, as in test_gpu_psd.py's white
    level: over K_j Hann segments at half overlap the average has variance (1 + 2/36 (K_j - 1) / K_j) / K_j, and the mean over M_j
    neighbouring bins (1 + 8/9 + 2/36) / M_j of that.  The two lowest bins of the last level (detrend, window) and level 0's
    last are left out."""
    L, D, n = 256, 128, 1 << 17
    x = np.random.default_rng(7).standard_normal(n)
    p, f, lev = ref.lpsd(x, FS, L, D, 'hann', True, 4)
    ns = ref.level_lengths(n, L, D, 4)
    assert len(ns) == lev.max() + 1 >= 8
    worst = 0.0
    for j, nj in enumerate(ns):
        K = px.segments(nj, L, D)
        sel = (lev == j) & (f > 1.5 * FS / 2 ** j / L) & (f < FS / 2)
        M = int(sel.sum())
        se = math.sqrt((1 + 2 / 36 * (K - 1) / K) / K * (1 + 8 / 9 + 2 / 36) / M)
        got = p[sel].mean() / (2.0 / FS)
        worst = max(worst, abs(got - 1) / (5 * se))
        assert abs(got - 1.0) <= 5 * se, (j, K, M, got, se)
    print('lpsd white level over %d octaves: worst error / (5 standard errors) %.3g' % (len(ns), worst))


def test_a_single_level_is_welch_on_all_bins():
    for L in (8, 64, 1024):
        for n in (L, 2 * L + 24):
            x = px.series('walk', n, L)
            assert ref.level_lengths(n, L, L // 2) == [n]
            p, f, lev = ref.lpsd(x, FS, L, L // 2, 'hann', True)
            np.testing.assert_array_equal(p, px.restated(x, FS, L, L // 2, 'hann', True))
            np.testing.assert_array_equal(f, px.freqs(FS, L))
            assert np.all(lev == 0)
        assert len(ref.level_lengths(2 * L + 25, L, L // 2)) == 2       # the shortest series with a level 1: n_1 = L


def test_the_octaves_tile_the_band_for_every_segment_length():
    for k in range(3, 14):
        L = 1 << k
        for levels in (1, 2, 3, 7, 32):
            b = ref.bands(levels, L)
            edges = []
            for j in reversed(range(levels)):
                lo, hi = b[j]
                assert lo <= hi
                edges.append((Fraction(lo, L * 2 ** j), Fraction(hi + 1, L * 2 ** j), Fraction(1, L * 2 ** j)))
            assert edges[0][0] == 0 and edges[-1][1] - edges[-1][2] == Fraction(1, 2)          # from 0 to fs / 2, in units of fs
            for (_, end, _), (start, _, _) in zip(edges, edges[1:]):
                assert end == start                                                           # no gap, no overlap
            if levels >= 3:
                assert b[1][1] - b[1][0] + 1 == L // 8
    assert ref.bands(3, 8)[1] == (1, 1)                                                       # one bin per middle level at L = 8


# ---- the float64 restatement against the long-double one, on every shape the device is held to
@pytest.mark.parametrize('case', lc.CASES, ids=lc.IDS)
def test_recorded_deviation_of_the_float64_restatement(case):
    name, L, D, J, K_last, short, extra, kinds, pad, win, det, ms, levels = case
    n, S, stride = lc.shape(case)
    assert len(ref.level_lengths(n, L, D, ms)) == levels
    if not short and not extra:
        assert px.segments(ref.level_lengths(n, L, D, ms)[-1], L, D) == K_last
    a = lc.rows(case)
    e, t, f, lev = lc.reference(case)
    assert e.shape == t.shape == (S, f.size) and np.all(np.diff(f) > 0) and lev.max() == levels - 1
    worst = np.zeros(levels)
    for s in range(S):
        p, f2, lev2 = ref.lpsd(a[s, :n], lc.FS, L, D, win, det, ms)
        np.testing.assert_array_equal(f2, f)
        np.testing.assert_array_equal(lev2, lev)
        for j in range(levels):
            worst[j] = max(worst[j], px.ratio(p[lev == j], e[s][lev == j], t[s][lev == j]))
    print('lpsd restatement %s: float64 against long double, error / tol per level %s (recorded %s)'
          % (name, ' '.join('%.3g' % w for w in worst), ' '.join('%.3g' % d for d in lc.DEV[name])))
    assert len(lc.DEV[name]) == levels and np.all(worst <= np.asarray(lc.DEV[name]))
    assert np.all(worst >= 0.5 * np.asarray(lc.DEV[name]))            # and the record is the measurement, not a loose cover
    assert lc.allowed(case).shape == f.shape


# ---- the plan, through the built library
def _edge_lengths(L):
    return [L, 2 * L + 24, 2 * L + 25, 2 * L + 26, 2 * L + 27, 2 * L + 28]


def test_plan_follows_the_restatement():
    import ginsim
    for L, D in ((8, 4), (8, 1), (64, 32), (1024, 512), (8192, 8192)):
        for n in _edge_lengths(L) + [5 * L + 1000, 1440000]:
            for S in (1, 3, 192):
                for ms in (1, 3):
                    if px.segments(n, L, D) < ms:
                        continue
                    assert ginsim.lpsd_plan(n, S, n + 5, FS, L, D, ms) == ref.plan(n, S, L, D, ms), (L, D, n, S, ms)
        assert len(ginsim.lpsd_plan(2 * L + 24, 1, 2 * L + 24, FS, L, D)['levels']) == 1
        assert [l['n'] for l in ginsim.lpsd_plan(2 * L + 25, 1, 2 * L + 25, FS, L, D)['levels']] == [2 * L + 25, L]
    for case in lc.CASES:
        n, S, stride = lc.shape(case)
        g = ginsim.lpsd_plan(n, S, stride, lc.FS, case[1], case[2], case[11])
        assert g == ref.plan(n, S, case[1], case[2], case[11]) and len(g['levels']) == case[12], case[0]
    # the cap of 32 levels: 2^40 samples at L = 8 would have 37
    n = 1 << 40
    g = ginsim.lpsd_plan(n, 1, n, FS, 8, 8)
    assert len(g['levels']) == 32 == ref.MAX_LEVELS and g == ref.plan(n, 1, 8, 8)
    assert g['nbins'] == 4 + 30 * 1 + 2
    # the bench's buffer: the cascade reads fewer than twice level 0's samples and its scratch is under level 0's bytes
    g = ginsim.lpsd_plan(1440000, 192, 1440000, 100.0, 8192)
    assert len(g['levels']) == 8 and sum(l['n'] for l in g['levels']) < 2 * 1440000 and g['scratch_bytes'] < 8 * 192 * 1440000
    assert g['levels'][0]['bins'] == 3073 and g['levels'][3]['bins'] == 1024 and g['levels'][7]['first_bin'] == 0


def _err():
    from ginsim import _lib
    return _lib.lib.ginsim_last_error().decode()


def test_plan_refusals_their_order_and_what_they_leave():
    from ginsim import _lib
    g = _lib.LpsdGeometry()
    size = C.sizeof(g)
    assert size == 16 + 32 * 32

    def call(n=100, S=1, stride=None, fs=1.0, L=64, D=32, ms=1, gp=True):
        C.memset(C.byref(g), 0xA5, size)
        rc = _lib.lib.ginsim_lpsd_plan(n, S, n if stride is None else stride, fs, L, D, ms, C.byref(g) if gp else None)
        if rc != _lib.OK:
            assert C.string_at(C.byref(g), size) == b'\xa5' * size          # a refused plan leaves *g as it was
        return rc
    assert call(n=0, L=7, D=0, ms=0, gp=False) == _lib.ERR_ARG and _err() == 'lpsd_plan: NULL argument'
    for kw in (dict(n=0), dict(S=0), dict(stride=99), dict(fs=0.0), dict(fs=float('nan'))):
        assert call(L=7, D=0, ms=0, **kw) == _lib.ERR_ARG and _err() == 'lpsd_plan: bad sizes', kw
    for L in (0, 4, 12, 16384):
        assert call(L=L, D=0, ms=0) == _lib.ERR_ARG and _err() == 'lpsd_plan: nperseg %d is not a power of two in [8, 8192]' % L
    for D in (0, 65):
        assert call(n=10, D=D, ms=0) == _lib.ERR_ARG and _err() == 'lpsd_plan: step %d outside [1, 64]' % D
    assert call(n=63, ms=0) == _lib.ERR_RANGE and _err() == 'lpsd_plan: a series of n = 63 samples is shorter than one segment of nperseg = 64'
    for ms in (0, -1):
        assert call(ms=ms) == _lib.ERR_ARG and _err() == 'lpsd_plan: min_segments %d must be at least 1' % ms
    assert call(n=100, ms=3) == _lib.ERR_RANGE and _err() == 'lpsd_plan: 2 segments at level 0 are fewer than min_segments = 3'
    assert call(n=100, ms=2) == _lib.OK and (g.levels, g.nbins, g.level[0].segments) == (1, 33, 2)
    assert g.level[1].n == 0 and g.level[31].bins == 0                       # the levels a call does not have are zero
    # the parts of level 0 before the cascade's own limits; the tiles of level 1 behind min_segments
    big = 2 ** 62
    assert call(n=big, L=8, D=1, ms=0) == _lib.ERR_RANGE and _err().startswith('lpsd_plan: ') and 'parts' in _err()
    n = 2 ** 43
    assert call(n=n, L=8192, D=8192, ms=0) == _lib.ERR_ARG and 'min_segments' in _err()
    assert call(n=n, L=8192, D=8192) == _lib.ERR_RANGE
    assert _err().startswith('lpsd_plan: level 1 of %d samples is %d tiles of 1024' % (ref.n_out(n), -(-ref.n_out(n) // 1024)))
    import ginsim
    with pytest.raises(ValueError, match='lpsd_plan: nperseg 100'):
        ginsim.lpsd_plan(1000, 1, 1000, 1.0, 100)


def test_call_refusals_with_a_null_context():
    from ginsim import _lib
    freq, p, lev, nb = np.empty(4), np.empty(4), np.empty(4, dtype=np.int32), C.c_int32(-7)
    fn = _lib.lib.ginsim_lpsd
    ok = (1 << 30, _lib.dptr(freq), _lib.dptr(p), lev.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nb))
    for hole in range(5):
        x, f, o, l, q = [None if i == hole else a for i, a in enumerate(ok)]
        assert fn(None, x, 0, 0, 0, -1.0, 7, 0, 5, 5, 0, f, o, l, q, 0) == _lib.ERR_ARG
        assert _err() == 'lpsd: NULL argument' and nb.value == -7
    no = C.c_int64(-7)
    assert _lib.lib.ginsim_decimate2(None, 1 << 30, 10, 0, 0, 1 << 31, 0, C.byref(no)) == _lib.ERR_ARG
    assert _err() == 'decimate2: NULL argument' and no.value == -7


# ---- the fourth header and the surface
def test_header_compiles_as_c99_and_its_names_are_exported_and_bound(tmp_path):
    import ginsim
    src = tmp_path / 'h.c'
    src.write_text('#include "ginsim_lpsd.h"\n'
                   'int main(void) { ginsim_lpsd_geometry g; g.levels = 1; g.level[GINSIM_LPSD_MAX_LEVELS - 1].bins = 2;\n'
                   '  return g.levels + g.level[31].bins + GINSIM_LPSD_TAPS + (GINSIM_ABI_VERSION == 9 ? 0 : 1); }\n')
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I' + os.path.join(REPO, 'include'),
                    '-fsyntax-only', str(src)], check=True, timeout=120)
    hdr = open(os.path.join(REPO, 'include', 'ginsim_lpsd.h')).read()
    declared = set(re.findall(r'\b(ginsim_[a-z0-9_]+)\s*\(', hdr))
    assert declared == {'ginsim_decimate2', 'ginsim_lpsd', 'ginsim_lpsd_plan'} == set(ginsim.LPSD_EXPORTS)
    raw = C.CDLL(ginsim.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name) and getattr(ginsim.lib, name).argtypes is not None
    others = set(ginsim.EXPORTS) | set(ginsim.OALLAN_EXPORTS) | set(ginsim.PSD_EXPORTS)
    assert not declared & others and len(ginsim.EXPORTS) == 86 and len(ginsim.OALLAN_EXPORTS) == len(ginsim.PSD_EXPORTS) == 2
    for h, count in (('ginsim.h', 86), ('ginsim_oallan.h', 2), ('ginsim_psd.h', 2)):
        text = open(os.path.join(REPO, 'include', h)).read()
        assert len(set(re.findall(r'\b(ginsim_[a-z0-9_]+)\s*\(', text))) == count, h
    assert ginsim.lib.ginsim_abi_version() == 9
    from ginsim import _lib
    assert C.sizeof(_lib.LpsdLevel) == 32 and _lib.LPSD_MAX_LEVELS == ref.MAX_LEVELS == 32
    assert 'ginsim_lpsd.h' in open(os.path.join(REPO, 'README.md')).read()


def test_python_surface():
    import ginsim
    from ginsim import multi
    from demo_algorithms import psd_analysis
    for name in ('lpsd', 'lpsd_host', 'lpsd_plan', 'decimate2', 'model_psd'):
        assert callable(getattr(ginsim, name))
    assert callable(ginsim.MonteCarloJob.lpsd) and callable(multi.JobSet.lpsd)
    with pytest.raises(ValueError, match='window'):
        ginsim.lpsd(None, 0, 100, 1, 100, 1.0, 64, window='hamming')
    p = psd_analysis.Psd()
    assert p.multires is False and p.output == ['psd_freq', 'psd_accel', 'psd_gyro']
    q = psd_analysis.Psd(nperseg=256, multires=True, min_segments=2)
    assert q.multires is True and q.min_segments == 2 and q.output == p.output and q.input == p.input


def test_model_density_integrates_to_the_models_variance():
    import ginsim
    fs = 100.0
    err = {'b': np.zeros(3), 'b_drift': np.array([2e-3, 1e-3, 5e-4]), 'b_corr': np.array([2.0, 50.0, np.inf]), 'arw': np.full(3, 1e-4)}
    m = ginsim.sensor_model(err, 'arw', fs)
    f = np.linspace(0.0, fs / 2, 2_000_001)
    d = ginsim.model_psd(err, 'arw', fs, f)
    assert d.shape == (f.size, 3)
    for i in range(3):
        var = m.white[i] ** 2 + m.gm_b[i] ** 2 / (1.0 - m.gm_a[i] ** 2)
        total = np.sum(0.5 * (d[1:, i] + d[:-1, i])) * (f[1] - f[0])
        assert abs(total / var - 1.0) <= 1e-6, i
    corner = 1.0 / (2 * math.pi * 2.0)
    white = 2 * m.white[0] ** 2 / fs
    lo, at = ginsim.model_psd(err, 'arw', fs, [0.0, corner])[:, 0] - white
    assert abs(at / lo - 0.5) <= 0.01                           # half the plateau at 1 / (2 pi Tc)


def test_resource_report_has_the_kernels_and_no_scratch():
    path = os.path.join(PKG, 'build', 'lpsd.resources.txt')
    assert os.path.exists(path), 'build.py writes it next to the object'
    blocks = open(path).read().split('Function Name: ')[1:]
    assert len(blocks) == 2 and sum('decimate2_kernel' in b for b in blocks) == 1 and sum('lpsd_report_kernel' in b for b in blocks) == 1
    for b in blocks:
        assert re.search(r'ScratchSize \[bytes/lane\]: (\d+)', b).group(1) == '0'
        assert int(re.search(r'^VGPRs: (\d+)', b, re.M).group(1)) <= 64        # eight wavefronts per SIMD
    b = [b for b in blocks if 'decimate2_kernel' in b][0]
    assert int(re.search(r'LDS Size \[bytes/block\]: (\d+)', b).group(1)) == 8 * (1048 + 1040)
