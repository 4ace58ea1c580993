"""Welch's power spectral density without a device: the exact values and the tolerance of tests/psd_exact.py, the plan of
ginsim_psd_plan through the built library, every refusal of the two entry points, the third header, the plugin's surface and the
build's resource report.

Measured here (CPU, long double of 64 mantissa bits): the float64 restatement reaches 0.35 of ``tol`` at worst over this file's
cases (L = 8192, D = L, boxcar, no detrend, the offset of 1e6); with the first form of the tolerance (sqrt(L) at every bin, see
psd_exact's text) the same cases reached 5.6 at bin 0 (L = 4096, D = L/2, boxcar, detrend, the offset of 1e6).  On the 25 shapes of tests/psd_cases.py, the ones the device is held
to, it reaches 0.184 (L1024_K2_quarter_step_raw), 0.115 on the eleven appended last (L8192_no_overlap_two_parts_plus_1)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import psd_cases as pc
import psd_exact as px

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'gnss-ins-sim_amd')
FS = 100.0


@pytest.mark.parametrize('L', [8, 64, 1024, 4096, 8192])
def test_float64_restatement_stays_within_the_tolerance(L):
    worst = (0.0, None)
    for D in (L // 4, L // 2, L):
        for kind in px.KINDS:
            n = min(3 * L + 5 * D + 7, 40000)
            x = px.series(kind, n, L + D)
            for win in px.WINDOWS:
                for det in (True, False):
                    e, f = px.exact(x, FS, L, D, win, det)
                    assert e.shape == f.shape == (L // 2 + 1,) and f[1] == FS / L
                    r = px.ratio(px.restated(x, FS, L, D, win, det), e, px.tol(x, FS, L, D, win, det, e))
                    worst = max(worst, (r, (D, kind, win, det)))
    print('psd restatement L %d: error / tol %.3g at %s' % (L, worst[0], worst[1]))
    assert worst[0] <= 1.0


def test_float64_restatement_on_every_gpu_shape():
    """The reference's own margin on every shape the device is held to (tests/psd_cases.py): the float64 restatement against the
    exact values, under the tolerance and the bound of test_gpu_psd.py::test_parity_with_exact."""
    worst = (0.0, None)
    for case in pc.CASES:
        name, L, D, K, tail, kinds, pad, win, det, _ = case
        n, S, stride = pc.shape(case)
        a = pc.rows(case)
        here = 0.0
        for s in range(S):
            x = a[s, :n]
            e, _ = px.exact(x, FS, L, D, win, det)
            here = max(here, px.ratio(px.restated(x, FS, L, D, win, det), e, px.tol(x, FS, L, D, win, det, e)))
        assert here <= 1.0, (name, here)
        worst = max(worst, (here, name))
    print('psd restatement on the %d device shapes: error / tol %.3g at %s' % (len(pc.CASES), worst[0], worst[1]))
    assert worst[0] <= 1.0


def test_the_tolerance_is_the_first_form_wherever_the_windows_transform_is_small():
    """g[k] > sqrt(L) at bin 0 (boxcar) and bins 0, 1 (Hann) only: everywhere else the tolerance is the issue's formula."""
    for L in (8, 64, 4096):
        x = px.series('offset', 3 * L, L)
        for win, raised in (('boxcar', [0]), ('hann', [0, 1])):
            e, _ = px.exact(x, FS, L, L // 2, win, True)
            seg = np.lib.stride_tricks.sliding_window_view(x, L)[::L // 2]
            w = px.window(L, win, np.float64)
            y = (seg - seg.mean(axis=1, keepdims=True)) * w
            d = 2.0 ** -53 * (4 * math.log2(L) * np.sqrt((y * y).sum(axis=1)) + (2 + math.log2(L)) * math.sqrt(L) * np.abs(seg).max(axis=1))
            c = np.full(L // 2 + 1, 2.0)
            c[0] = c[-1] = 1.0
            e1 = c * np.mean(d * d) / (FS * (w * w).sum())
            first = 1e-10 * e + 2 * np.sqrt(e * e1) + e1
            t = px.tol(x, FS, L, L // 2, win, True, e)
            keep = np.ones(L // 2 + 1, dtype=bool)
            keep[raised] = False
            if L == 8 and win == 'hann':            # sqrt(8) > L/4: bin 1 is not raised at this length
                keep[1] = True
            np.testing.assert_allclose(t[keep], first[keep], rtol=1e-12)
            assert np.all(t >= first * (1 - 1e-12)) and t[0] > first[0]


def test_exact_agrees_with_scipy():
    signal = pytest.importorskip('scipy.signal')
    for L, n in ((64, 1000), (1024, 9000)):
        for kind in ('white', 'tone', 'offset'):
            x = px.series(kind, n, 5)
            for win in px.WINDOWS:
                for det in (True, False):
                    for D in (L // 2, L):
                        e, f = px.exact(x, FS, L, D, win, det)
                        fr, p = signal.welch(x, FS, window=win, nperseg=L, noverlap=L - D, detrend='constant' if det else False,
                                             scaling='density')
                        np.testing.assert_allclose(fr, f, rtol=1e-15, atol=0)
                        assert np.max(np.abs(p - e)) <= 1e-9 * np.max(e), (L, kind, win, det, D)


def test_parseval():
    for L, n in ((8, 100), (1024, 5000), (8192, 20000)):
        x = px.series('walk', n, 3)
        p, _ = px.exact(x, FS, L, L, 'boxcar', False)
        read = x[:px.segments(n, L, L) * L]
        assert abs(np.sum(p) * FS / L / np.mean(read * read) - 1.0) <= 1e-12


# ---- the plan, through the built library
def test_plan_follows_the_formulas_on_every_gpu_shape():
    import ginsim
    for case in pc.CASES:
        _, L, D, K, tail, kinds, pad, _, _, where = case
        n, S, stride = pc.shape(case)
        assert px.segments(n, L, D) == K, case[0]
        g = ginsim.welch_plan(n, S, stride, FS, L, D)
        spp = pc.segs_per_part(L, D)
        assert (g['segments'], g['segs_per_part'], g['nparts']) == (K, spp, -(-K // spp)), case[0]
        assert spp % 2 == 0 and spp >= 4 * L // D - 1
        if where is not None:
            assert K == where[0] * spp + where[1], case[0]
        assert g['threads'] == min(max(L // 4, 64), 512) and g['lds_bytes'] <= 160 * 1024
        assert g['scratch_bytes'] >= 8 * S * g['nparts'] * (L // 2 + 1)
        for S2 in (1, 7, 192):             # the partition does not depend on the number of series
            g2 = ginsim.welch_plan(n, S2, n, FS, L, D)
            assert [g2[k] for k in ('segments', 'segs_per_part', 'nparts', 'threads', 'lds_bytes')] == \
                [g[k] for k in ('segments', 'segs_per_part', 'nparts', 'threads', 'lds_bytes')]
    g = ginsim.welch_plan(1440000, 192, 1440000, 400.0, 1024)          # step defaults to half a segment
    assert (g['segments'], g['segs_per_part'], g['nparts']) == (2811, 32, 88)
    assert g['scratch_bytes'] <= 8 * 192 * 1440000 // 8
    assert ginsim.PSD_WINDOWS == ('boxcar', 'hann')


def _err():
    from ginsim import _lib
    return _lib.lib.ginsim_last_error().decode()


BAD_SIZES = [dict(n=0), dict(S=0), dict(S=-1), dict(stride=99), dict(fs=0.0), dict(fs=-1.0), dict(fs=float('inf')),
             dict(fs=float('nan'))]
BAD_NPERSEG = [0, -8, 4, 7, 12, 1000, 16384, 8193]
BAD_STEP = [0, -1, 65]


def test_plan_refusals_and_their_order():
    from ginsim import _lib
    g = _lib.PsdGeometry()

    def call(n=100, S=1, stride=None, fs=1.0, L=64, D=32, gp=True):
        return _lib.lib.ginsim_psd_plan(n, S, n if stride is None else stride, fs, L, D, C.byref(g) if gp else None)
    assert call(n=0, L=7, D=0, gp=False) == _lib.ERR_ARG and _err() == 'psd_plan: NULL argument'       # before everything else
    for kw in BAD_SIZES:
        assert call(L=7, D=0, **kw) == _lib.ERR_ARG and _err() == 'psd_plan: bad sizes', kw             # before nperseg
    for L in BAD_NPERSEG:
        assert call(L=L, D=0) == _lib.ERR_ARG and _err() == 'psd_plan: nperseg %d is not a power of two in [8, 8192]' % L     # before step
    for D in BAD_STEP:
        assert call(n=10, D=D) == _lib.ERR_ARG and _err() == 'psd_plan: step %d outside [1, 64]' % D    # before the series' length
    assert call(n=63) == _lib.ERR_RANGE and _err() == 'psd_plan: a series of n = 63 samples is shorter than one segment of nperseg = 64'
    assert call(n=64) == _lib.OK and (g.segments, g.nparts) == (1, 1)
    assert call(n=64, D=1) == _lib.OK and call(n=64, D=64) == _lib.OK
    for L in (8, 8192):
        assert call(n=8192, L=L, D=L) == _lib.OK


# L = 8, D = 1: parts of 16384 segments; N_LAST is the longest series of 2^31 - 1 parts, all of them full
MAX_PARTS = 2 ** 31 - 1
N_LAST = MAX_PARTS * 16384 + 7


def _plan_raw(n, S, g, L=8, D=1):
    from ginsim import _lib
    return _lib.lib.ginsim_psd_plan(n, S, n, 1.0, L, D, C.byref(g))


def test_plan_states_the_last_length_it_can():
    from ginsim import _lib
    assert pc.segs_per_part(8, 1) == 16384
    g = _lib.PsdGeometry()
    assert _plan_raw(N_LAST, 1, g) == _lib.OK
    assert g.segments == MAX_PARTS * 16384 == N_LAST - 8 + 1
    assert (g.segs_per_part, g.nparts) == (16384, MAX_PARTS)
    assert g.scratch_bytes == (8 * MAX_PARTS * 5 + 255) // 256 * 256
    assert _plan_raw(N_LAST - 16384, 1, g) == _lib.OK and g.nparts == MAX_PARTS - 1
    assert _plan_raw(N_LAST - 16384 + 1, 1, g) == _lib.OK and g.nparts == MAX_PARTS      # a last part of one segment
    # the largest batch of that length whose records stay below 2^63 bytes
    S = (2 ** 63 - 256) // (40 * MAX_PARTS)
    assert _plan_raw(N_LAST, S, g) == _lib.OK and g.scratch_bytes == (40 * MAX_PARTS * S + 255) // 256 * 256 < 2 ** 63
    # another shape at its own edge: L = 8192, D = 8192, parts of 4 segments
    n = MAX_PARTS * 4 * 8192
    assert _plan_raw(n, 1, g, 8192, 8192) == _lib.OK and (g.segments, g.segs_per_part, g.nparts) == (MAX_PARTS * 4, 4, MAX_PARTS)
    assert g.scratch_bytes == (8 * MAX_PARTS * 4097 + 255) // 256 * 256


def test_plan_refuses_what_it_cannot_state():
    """Any n is a legal question (host arithmetic only); an answer that does not fit the geometry is refused, not narrowed: the
    parent of this test answered n = 2^62 with GINSIM_OK and nparts == 0."""
    from ginsim import _lib
    fields = [k for k, _ in _lib.PsdGeometry._fields_]

    def refused(n, S, parts, L=8, D=1, words=()):
        g = _lib.PsdGeometry(-11, -12, -13, -14, -15, -16)
        before = [getattr(g, k) for k in fields]
        assert _plan_raw(n, S, g, L, D) == _lib.ERR_RANGE, (n, S, g.nparts)
        msg = _err()
        assert msg.startswith('psd_plan: ') and '%d parts' % parts in msg and all(w in msg for w in words), msg
        assert [getattr(g, k) for k in fields] == before
    refused(N_LAST + 1, 1, 2 ** 31)                                  # one segment past the last full part
    refused(N_LAST + 1, 2 ** 31 - 1, 2 ** 31)
    refused(2 ** 62, 1, 2 ** 48)
    refused(2 ** 63 - 1, 1, 2 ** 49)                                 # the longest series there is
    refused(N_LAST, 2 ** 31 - 1, MAX_PARTS, words=('2^63 bytes',))   # the parts fit, the records' bytes do not
    S = (2 ** 63 - 256) // (40 * MAX_PARTS)
    refused(N_LAST, S + 1, MAX_PARTS, words=('2^63 bytes',))
    refused(MAX_PARTS * 4 * 8192 + 8192, 1, 2 ** 31, L=8192, D=8192)
    import ginsim
    with pytest.raises(ValueError, match='psd_plan: .* 281474976710656 parts'):
        ginsim.welch_plan(2 ** 62, 1, 2 ** 62, 1.0, 8, 1)


def test_plan_refusal_sits_behind_the_arguments_and_the_short_series():
    """The new refusal's place in the order of include/ginsim_psd.h: after the arguments and after "n < nperseg".  (Before the
    grid's y limit: tests/test_gpu_psd.py::test_device_refuses_what_the_plan_cannot_state, which needs the context.)"""
    from ginsim import _lib
    g = _lib.PsdGeometry()
    big = 2 ** 62
    for kw, msg in ((dict(S=0), 'psd_plan: bad sizes'), (dict(L=12), 'psd_plan: nperseg 12 is not a power of two in [8, 8192]'),
                    (dict(D=9), 'psd_plan: step 9 outside [1, 8]')):
        L, D = kw.get('L', 8), kw.get('D', 1)
        assert _lib.lib.ginsim_psd_plan(big, kw.get('S', 1), big, 1.0, L, D, C.byref(g)) == _lib.ERR_ARG and _err() == msg
    assert _lib.lib.ginsim_psd_plan(7, 2 ** 31 - 1, big, 1.0, 8, 1, C.byref(g)) == _lib.ERR_RANGE
    assert _err() == 'psd_plan: a series of n = 7 samples is shorter than one segment of nperseg = 8'
    hdr = open(os.path.join(REPO, 'include', 'ginsim_psd.h')).read()
    order = [hdr.index(w) for w in ('n < nperseg;', '2^31 - 1 parts', "device's maxGridSize[1]", 'cap below')]
    assert order == sorted(order)


def test_call_refusals_with_a_null_context_and_their_order():
    from ginsim import _lib
    freq, p, nf = np.empty(4), np.empty(4), C.c_int32(-7)
    fn = _lib.lib.ginsim_psd_welch
    # NULL first, with everything else wrong too; nothing is written.  (The refusals behind it need a context:
    # tests/test_gpu_psd.py.)
    ok = (1 << 30, _lib.dptr(freq), _lib.dptr(p), C.byref(nf))
    for hole in range(4):
        x, f, o, q = [None if i == hole else a for i, a in enumerate(ok)]
        assert fn(None, x, 0, 0, 0, -1.0, 7, 0, 5, 5, f, o, q, 0) == _lib.ERR_ARG
        assert _err() == 'psd: NULL argument' and nf.value == -7
    assert fn(None, ok[0], 100, 1, 100, 1.0, 64, 32, 1, 1, *ok[1:], 33) == _lib.ERR_ARG and _err() == 'psd: NULL argument'
    with pytest.raises(ValueError, match='psd: NULL argument'):
        _lib.check(fn(None, None, 100, 1, 100, 1.0, 64, 32, 1, 1, None, None, None, 33))


def test_python_arguments():
    import ginsim
    with pytest.raises(ValueError, match='window'):
        ginsim.welch_psd(None, 0, 100, 1, 100, 1.0, 64, window='hamming')
    with pytest.raises(ValueError, match='psd_plan: nperseg 100'):
        ginsim.welch_plan(1000, 1, 1000, 1.0, 100)


def test_header_compiles_as_c99_and_its_names_are_exported_and_bound(tmp_path):
    import ginsim
    src = tmp_path / 'h.c'
    src.write_text('#include "ginsim_psd.h"\n'
                   'int main(void) { ginsim_psd_geometry g; g.segments = 1; g.nparts = 2;\n'
                   '  return (int)(g.segments + g.nparts) + GINSIM_PSD_HANN + (GINSIM_ABI_VERSION == 9 ? 0 : 1); }\n')
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I' + os.path.join(REPO, 'include'),
                    '-fsyntax-only', str(src)], check=True, timeout=120)
    hdr = open(os.path.join(REPO, 'include', 'ginsim_psd.h')).read()
    declared = set(re.findall(r'\b(ginsim_[a-z0-9_]+)\s*\(', hdr))
    assert declared == {'ginsim_psd_welch', 'ginsim_psd_plan'} == set(ginsim.PSD_EXPORTS)
    raw = C.CDLL(ginsim.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name) and getattr(ginsim.lib, name).argtypes is not None
    from ginsim import _lib
    assert C.sizeof(_lib.PsdGeometry) == 32
    readme = open(os.path.join(REPO, 'README.md')).read()
    assert '86 entry points' in readme and 'ginsim_oallan.h' in readme and 'ginsim_psd.h' in readme
    for name in ('welch_psd', 'welch_psd_host', 'welch_plan'):
        assert callable(getattr(ginsim, name))
    assert callable(ginsim.MonteCarloJob.psd)
    from ginsim import multi
    assert callable(multi.JobSet.psd)


def test_the_first_header_and_its_exports_are_what_they_were():
    import ginsim
    hdr = open(os.path.join(REPO, 'include', 'ginsim.h')).read()
    declared = set(re.findall(r'\b(ginsim_[a-z0-9_]+)\s*\(', hdr))
    assert len(declared) == 86 and not any(n.startswith('ginsim_psd') for n in declared)
    assert len(ginsim.EXPORTS) == 86 and set(ginsim.EXPORTS) <= declared
    assert not set(ginsim.PSD_EXPORTS) & (set(ginsim.EXPORTS) | set(ginsim.OALLAN_EXPORTS))
    assert ginsim.lib.ginsim_abi_version() == 9


def test_plugin_surface_and_registry():
    from demo_algorithms import psd_analysis
    from gnss_ins_sim.sim import ins_data_manager
    p = psd_analysis.Psd()
    assert p.input == ['fs', 'accel', 'gyro'] and p.output == ['psd_freq', 'psd_accel', 'psd_gyro']
    assert (p.nperseg, p.step, p.window, p.detrend) == (1024, None, 'hann', True)
    assert all(callable(getattr(p, m)) for m in ('run', 'run_device', 'get_results', 'reset')) and p.get_results() is None
    q = psd_analysis.Psd(nperseg=256, step=64, window='boxcar', detrend=False)
    assert (q.nperseg, q.step, q.window, q.detrend) == (256, 64, 'boxcar', False)
    d = ins_data_manager.InsDataMgr([100.0, None, None], 0)
    for name in p.output:
        assert d.is_supported(name)
    d.set_algo_output(p.output)
    for name, unit in (('psd_accel', '(m/s^2)^2/Hz'), ('psd_gyro', '(rad/s)^2/Hz')):
        sd = d.get_data_all(name)
        assert sd.units == [unit] * 3 and sd.output_units == sd.units          # a density is not a rate: no rad -> deg on output
        assert sd.logx and sd.logy and len(sd.legend) == 3
    assert d.get_data_all('psd_freq').units == ['Hz'] and d.get_data_all('psd_freq').logx
    assert not os.path.exists(os.path.join(PKG, 'gnss_ins_sim', 'psd'))         # the reference's module of that name stays reachable


def test_resource_report_has_every_segment_length_and_no_scratch():
    path = os.path.join(PKG, 'build', 'psd.resources.txt')
    assert os.path.exists(path), 'build.py writes it next to the object'
    text = open(path).read()
    blocks = text.split('Function Name: ')[1:]
    parts = {int(m.group(1)): b for b in blocks for m in [re.search(r'psd_part_kernelILi(\d+)E', b)] if m}
    assert sorted(parts) == [1 << k for k in range(3, 14)]
    assert any('psd_finish_kernel' in b for b in blocks)
    for b in blocks:
        assert re.search(r'ScratchSize \[bytes/lane\]: (\d+)', b).group(1) == '0', b.splitlines()[0]
    import ginsim
    for L, b in parts.items():
        lds = int(re.search(r'LDS Size \[bytes/block\]: (\d+)', b).group(1))
        assert lds == ginsim.welch_plan(L, 1, L, 1.0, L)['lds_bytes'], L           # the plan reports what the kernel takes


def test_requested_spectrum_chain_in_numpy():
    """The margin of test_gpu_psd.py's last test: the generator's chain in float64 NumPy against the requested PSD."""
    import ginsim
    fs, n = pc.REQUESTED_FS, pc.REQUESTED_N
    vib = dict(type='psd', freq=pc.REQUESTED_FREQ, **pc.REQUESTED_PSD)
    N, amp, on_grid = ginsim.psd_amplitudes(vib, fs, n)
    assert N == n and not on_grid and amp.shape == (3, n // 2 + 1)
    worst = 0.0
    for draw in range(8):
        rng = np.random.default_rng(draw)
        for c, axis in enumerate('xyz'):
            phase = np.pi * rng.standard_normal(n // 2 + 1)
            x = np.fft.irfft(amp[c] * np.exp(1j * phase), n) + (-9.794841972265039 if axis == 'z' else 0.0)
            want = pc.requested_on_grid(axis)
            got = px.restated(x, fs, n, n, 'boxcar', True)
            t = px.tol(x, fs, n, n, 'boxcar', True, want)
            worst = max(worst, px.ratio(got[1:], want[1:], t[1:]))
    print('requested spectrum, NumPy chain: error / tol %.3g' % worst)
    assert worst <= pc.REQUESTED_NUMPY
