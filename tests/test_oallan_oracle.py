"""The overlapping Allan variance without a device: the exact values and the tolerance of tests/oallan_exact.py, the plan of
ginsim_oallan_plan through the built library, every refusal of the two entry points, and the second header.

Measured here (CPU, long double of 64 mantissa bits): the float64 restatement with a sequential global cumsum reaches 0.0018 of
``bound`` at worst with this file's draws (n = 30 000, white noise plus a random walk; 0.061 at worst over the draws of
oallan_exact's text); the across-series scatter of the overlapping estimator at the longest tau over 192 white series of 36 000
samples (numpy default_rng(1), m = 4000) is 0.645 of the non-overlapping estimator's (0.735 with the draw quoted in DESIGN 4.3b)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import allan_exact as ax
import oallan_exact as ox

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _series(kind, n, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n)
    if kind == 'offset':
        x += 1e6
    elif kind == 'walk':
        x += np.cumsum(rng.standard_normal(n))
    return x


def test_longdouble_and_fsum_paths_agree():
    if not ax.WIDE:
        pytest.skip('no long double wider than a double: exact() takes the fsum path alone')
    for n, fs in ((18, 1.0), (27, 1.0), (99, 1.0), (400, 2.0), (1500, 10.0)):
        for kind in ('white', 'offset', 'walk'):
            x = _series(kind, n, n)
            a, b = ox.exact_longdouble(x, fs), ox.exact_fsum(x, fs)
            assert a.size == len(ox.factors(n, fs)) > 0
            np.testing.assert_allclose(a, b, rtol=1e-15, atol=0)
    only = ox.exact_fsum(_series('white', 400, 3), 1.0, only={1, 40})
    assert np.isnan(only).sum() == only.size - 2


def test_factors_are_the_reference_list():
    for n, fs in ((9, 1.0), (17, 1.0), (18, 1.0), (89, 1.0), (90, 1.0), (99, 1.0), (36000, 1.0), (1440000, 400.0), (1000, 1000.0)):
        assert ox.factors(n, fs) == ax.factors(n, fs)[0]
        assert all(n // m >= 9 and n - 2 * m + 1 > 0 for m in ox.factors(n, fs))
    assert ox.factors(90, 1.0) == list(range(1, 10))        # n // 9 == 10 yields 1 .. 9 only
    assert ox.factors(9, 1.0) == [] and ox.factors(17, 1.0) == [] and ox.factors(18, 1.0) == [1, 2]
    assert len(ox.factors(1440000, 400.0)) == 46


@pytest.mark.parametrize('n,fs', [(18, 1.0), (30000, 1.0), (1440000, 400.0)])
def test_float64_restatement_stays_within_the_bound(n, fs):
    worst = 0.0
    for kind in ('white', 'offset', 'walk'):
        x = _series(kind, n, 7)
        e, tau = ox.exact(x, fs)
        m = np.array(ox.factors(n, fs))
        np.testing.assert_array_equal(tau, m * (1.0 / fs))
        r = ox.ratio(ox.restated(x, fs), e, ox.bound(x, e, m))
        print('oallan restatement n %d %s: error / bound %.3g' % (n, kind, r))
        worst = max(worst, r)
    assert worst <= 1.0       # 0.0018 at worst (module text)


def test_theta_may_gain_a_line():
    """d is unchanged when theta gains a + b k: evaluated in long double on integers, where every operation is exact."""
    rng = np.random.default_rng(5)
    n = 500
    th = np.concatenate([[0], np.cumsum(rng.integers(-1000, 1000, n))]).astype(np.longdouble)
    k = np.arange(n + 1).astype(np.longdouble)
    for m in ox.factors(n, 1.0):
        d0 = th[2 * m:] - 2 * th[m:n + 1 - m] + th[:n + 1 - 2 * m]
        t2 = th + 12345 + 678 * k
        d1 = t2[2 * m:] - 2 * t2[m:n + 1 - m] + t2[:n + 1 - 2 * m]
        np.testing.assert_array_equal(d0, d1)
    # and through exact(): a constant offset of x that is exactly representable changes nothing
    x = rng.integers(-1000, 1000, n).astype(np.float64)
    np.testing.assert_array_equal(ox.exact(x, 1.0)[0], ox.exact(x + 4096.0, 1.0)[0])


def test_scatter_at_the_longest_tau_is_below_the_binned_estimator():
    """192 white series of 36 000 samples, seed 1, fs 1 Hz, m = 4000: std over the series of the overlapping estimate against the
    non-overlapping one.  Measured 0.645 with this draw (relative scatter 0.58 -> 0.38)."""
    x = np.random.default_rng(1).standard_normal((192, 36000))
    assert ox.factors(36000, 1.0)[-1] == 4000
    o = np.array([ox.exact(r, 1.0)[0][-1] for r in x])
    a = np.array([ax.exact(r, 1.0)[0][-1] for r in x])
    ratio = o.std() / a.std()
    print('oallan scatter ratio at m = 4000: %.3f (relative %.2f -> %.2f)' % (ratio, a.std() / a.mean(), o.std() / o.mean()))
    assert ratio < 1.0


# ---- the plan, through the built library
def test_plan_forms_terms_and_the_all_stream_switch(monkeypatch):
    import ginsim
    monkeypatch.delenv('GINSIM_OALLAN_TILE', raising=False)
    n, fs = 36000, 1.0
    f, g = ginsim.oallan_plan(0, n, 3, n, fs)
    mult = ox.factors(n, fs)
    Cp, H = g['tile_payload'], g['tile_halo']
    assert Cp >= 1 and H >= 2
    assert [e['m'] for e in f] == mult
    assert [e['terms'] for e in f] == [n - 2 * m + 1 for m in mult]
    assert [e['form'] for e in f] == [0 if 2 * m <= H else 1 for m in mult]
    assert g['tile_factors'] == sum(2 * m <= H for m in mult) and g['tile_factors'] + g['stream_factors'] == len(mult)
    assert all(e['nparts'] == -(-e['terms'] // Cp) for e in f if e['form'] == 0)
    assert all(e['nparts'] >= 1 for e in f) and g['scratch_bytes'] > 0
    assert ginsim.OALLAN_FORMS == ('tile', 'stream')
    monkeypatch.setenv('GINSIM_OALLAN_TILE', '0')           # read per call
    f0, g0 = ginsim.oallan_plan(0, n, 3, n, fs)
    assert [e['form'] for e in f0] == [1] * len(mult) and g0['tile_factors'] == 0 and g0['stream_factors'] == len(mult)
    assert (g0['tile_payload'], g0['tile_halo']) == (Cp, H) and [e['m'] for e in f0] == mult
    monkeypatch.setenv('GINSIM_OALLAN_TILE', '1')
    assert ginsim.oallan_plan(0, n, 3, n, fs)[0] == f
    monkeypatch.delenv('GINSIM_OALLAN_TILE')
    for n0, fs0 in ((17, 1.0), (9, 1.0), (8, 1.0), (1000, 1000.0), (8999, 1000.0)):       # ceil(log10(1)) = 0 levels; n fs too short
        assert ginsim.oallan_plan(0, n0, 1, n0, fs0)[0] == [] == ox.factors(n0, fs0)
    f1, g1 = ginsim.oallan_plan(0, 18, 1, 18, 1.0)
    assert [(e['m'], e['terms'], e['form'], e['nparts']) for e in f1] == [(1, 17, 0, 1), (2, 15, 0, 1)]


def _plan_call():
    from ginsim import _lib
    nt, g = C.c_int32(-7), _lib.OallanGeometry()
    f = (_lib.OallanFactor * 64)()

    def call(n=100, S=1, stride=None, fs=1.0, ntp=True, fp=True, cap=64, gp=True):
        return _lib.lib.ginsim_oallan_plan(0, n, S, n if stride is None else stride, fs, C.byref(nt) if ntp else None,
                                           f if fp else None, cap, C.byref(g) if gp else None)
    return call, nt


def _err():
    from ginsim import _lib
    return _lib.lib.ginsim_last_error().decode()


BAD_SIZES = [dict(n=0), dict(S=0), dict(S=-1), dict(stride=99), dict(fs=0.0), dict(fs=-1.0), dict(fs=float('inf')),
             dict(fs=float('nan'))]


def test_plan_refusals_and_their_order():
    from ginsim import _lib
    call, nt = _plan_call()
    for kw in (dict(ntp=False), dict(gp=False), dict(fp=False), dict(cap=-1)):
        assert call(n=0, **kw) == _lib.ERR_ARG and _err().startswith('oallan_plan: bad arguments'), kw     # before the sizes
    assert call(fp=False, cap=0) == _lib.ERR_RANGE and nt.value == 10          # no array needed with capacity 0; ntau still reported
    for kw in BAD_SIZES:
        assert call(cap=0, **kw) == _lib.ERR_ARG and _err() == 'oallan: bad sizes', kw                      # before the capacity
    assert call(cap=9) == _lib.ERR_RANGE and _err() == 'oallan_plan: 10 averaging factors but capacity 9'
    assert call(cap=10) == _lib.OK
    assert call(n=8, cap=0) == _lib.OK and nt.value == 0


def test_call_refusals_with_a_null_context_and_their_order():
    from ginsim import _lib
    tau, ov, nt = np.empty(4), np.empty(4), C.c_int32(-7)
    fn = _lib.lib.ginsim_oallan
    # NULL first, with everything else wrong too; nothing is written.  (The refusals behind it need a context:
    # tests/test_gpu_oallan.py.)
    ok = (1 << 30, _lib.dptr(tau), _lib.dptr(ov), C.byref(nt))
    for hole in range(4):
        x, t, o, p = [None if i == hole else a for i, a in enumerate(ok)]
        assert fn(None, x, 0, 0, 0, -1.0, t, o, p, 0) == _lib.ERR_ARG
        assert _err() == 'oallan: NULL argument' and nt.value == -7
    assert fn(None, *ok[:1], 100, 1, 100, 1.0, *ok[1:], 128) == _lib.ERR_ARG and _err() == 'oallan: NULL argument'
    with pytest.raises(ValueError, match='oallan: NULL argument'):
        _lib.check(fn(None, None, 100, 1, 100, 1.0, None, None, None, 128))


def test_header_compiles_as_c99_and_its_names_are_exported_and_bound(tmp_path):
    import ginsim
    src = tmp_path / 'h.c'
    src.write_text('#include "ginsim_oallan.h"\n'
                   'int main(void) { ginsim_oallan_factor f; ginsim_oallan_geometry g; f.m = 1; g.tile_halo = 2;\n'
                   '  return (int)(f.m + g.tile_halo) + (GINSIM_ABI_VERSION == 9 ? 0 : 1); }\n')
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I' + os.path.join(REPO, 'include'),
                    '-fsyntax-only', str(src)], check=True, timeout=120)
    hdr = open(os.path.join(REPO, 'include', 'ginsim_oallan.h')).read()
    declared = set(re.findall(r'\b(ginsim_[a-z0-9_]+)\s*\(', hdr))
    assert declared == {'ginsim_oallan', 'ginsim_oallan_plan'} == set(ginsim.OALLAN_EXPORTS)
    raw = C.CDLL(ginsim.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name) and getattr(ginsim.lib, name).argtypes is not None
    from ginsim import _lib
    assert C.sizeof(_lib.OallanFactor) == 24 and C.sizeof(_lib.OallanGeometry) == 32
    readme = open(os.path.join(REPO, 'README.md')).read()
    assert '86 entry points' in readme and 'ginsim_oallan.h' in readme
    for name in ('oallan_var', 'oallan_var_host', 'oallan_plan'):
        assert callable(getattr(ginsim, name))


def test_the_first_header_and_its_exports_are_what_they_were():
    import ginsim
    hdr = open(os.path.join(REPO, 'include', 'ginsim.h')).read()
    declared = set(re.findall(r'\b(ginsim_[a-z0-9_]+)\s*\(', hdr))
    assert len(declared) == 86 and 'ginsim_oallan' not in declared
    assert len(ginsim.EXPORTS) == 86 and set(ginsim.EXPORTS) <= declared and not set(ginsim.OALLAN_EXPORTS) & set(ginsim.EXPORTS)
    assert ginsim.lib.ginsim_abi_version() == 9
