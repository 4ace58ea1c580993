"""The overlapping Allan variance on the device (csrc/oallan.hip through ginsim_oallan): every result is held to the exact values
of tests/oallan_exact.py within the tolerance derived there, and every case asserts from ginsim.oallan_plan WHICH form (tile or
stream) ran each factor.  The shapes come from the geometry the library reports (tile payload C, halo H, and the stream form's
work-item length, found from the plan's nparts), never from numbers written here.

Sections: the smallest lengths; one tile and its edges; the form boundary with and without GINSIM_OALLAN_TILE=0; the stream
form's work-item edges; batches, strides, base alignment and repeatability; inputs that break naive forms; non-finite samples;
the refusals; the Python layers; one full-size case."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oallan_exact as ox

pytestmark = pytest.mark.gpu

TILE, STREAM = 0, 1


@pytest.fixture(scope='module')
def ctx():
    import ginsim
    c = ginsim.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _default_forms(monkeypatch):
    monkeypatch.delenv('GINSIM_OALLAN_TILE', raising=False)


def _geometry():
    import ginsim
    g = ginsim.oallan_plan(0, 100, 1, 100, 1.0)[1]
    return g['tile_payload'], g['tile_halo']


def _both_forms_n(H):
    """The shortest series (plus an odd bit) that has a stream-form factor: 9 m for the first factor with 2 m > H."""
    m = next(m for m in ox.factors(10 ** 7, 1.0) if 2 * m > H)
    return 9 * m + 37


def _stream_item():
    """The stream form's shifts per work item, from the plan: the largest number of terms of factor 1 that is still one part."""
    import ginsim
    os.environ['GINSIM_OALLAN_TILE'] = '0'
    try:
        parts = lambda n: ginsim.oallan_plan(0, n, 1, n, 1.0)[0][0]['nparts']      # noqa: E731  factor 1: terms = n - 1
        lo, hi = 18, 1 << 26
        assert parts(lo) == 1 and parts(hi) > 1
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if parts(mid) == 1 else (lo, mid)
        return lo - 1
    finally:
        del os.environ['GINSIM_OALLAN_TILE']


def rows(kinds, n, seed):
    """One series per kind: white, offset (1e6), walk (white + random walk), ramp, const."""
    rng = np.random.default_rng(seed)
    out = []
    for kind in kinds:
        x = rng.standard_normal(n)
        if kind == 'offset':
            x += 1e6
        elif kind == 'walk':
            x += np.cumsum(rng.standard_normal(n))
        elif kind == 'ramp':
            x = 3.0 + 0.5 * np.arange(n)
        elif kind == 'const':
            x = np.full(n, 7.25)
        out.append(x)
    return out


def pack(rws, stride, off=0):
    """The rows at `stride` entries apart behind `off` leading entries, the gaps and the tail filled with NaN: a kernel that reads
    outside its series shows it."""
    n = rws[0].size
    flat = np.full(off + stride * len(rws) + 4, np.nan)
    for s, x in enumerate(rws):
        flat[off + s * stride:off + s * stride + n] = x
    return flat


def run(ctx, rws, fs, stride=None, off=0, forms=None, ref=None, what=''):
    """Upload, assert the plan of exactly this call, run it, hold every row to its exact values.  Returns (oavar, ref)."""
    import ginsim
    n, S = rws[0].size, len(rws)
    stride = n if stride is None else stride
    buf = ctx.upload(pack(rws, stride, off))
    try:
        ptr = buf.ptr + 8 * off
        f, g = ginsim.oallan_plan(ptr, n, S, stride, fs)
        mult = ox.factors(n, fs)
        assert [e['m'] for e in f] == mult and [e['terms'] for e in f] == [n - 2 * m + 1 for m in mult]
        want = [TILE if 2 * m <= g['tile_halo'] else STREAM for m in mult] if forms is None else [forms] * len(mult)
        assert [e['form'] for e in f] == want, (n, f)
        oavar, tau = ginsim.oallan_var(ctx, ptr, n, S, stride, fs)
    finally:
        buf.free()
    assert oavar.shape == (S, len(mult))
    np.testing.assert_array_equal(tau, np.array([m * (1.0 / fs) for m in mult]))
    if ref is None:
        ref = [ox.exact(x, fs)[0] for x in rws]
    worst = 0.0
    for s, x in enumerate(rws):
        assert np.isfinite(oavar[s]).all(), (what, s)
        worst = max(worst, ox.ratio(oavar[s], ref[s], ox.bound(x, ref[s], np.array(mult))))
    print('oallan %s n %d x %d: error / bound %.3g' % (what, n, S, worst))
    assert worst <= 1.0, (what, n, worst)
    return oavar, ref


# ---- the smallest lengths
@pytest.mark.parametrize('n', [18, 19, 26, 27, 89, 90, 99])
def test_smallest_lengths(ctx, n, monkeypatch):
    """n // 9 crossing 2, 3, 9, 10 (90: the factors 1 .. 9 only) and 11 (99: the factor 10), in both forms."""
    rws = rows(('white', 'offset', 'walk'), n, n)
    assert ox.factors(n, 1.0) == {18: [1, 2], 19: [1, 2], 26: [1, 2], 27: [1, 2, 3], 89: list(range(1, 10)), 90: list(range(1, 10)),
                                  99: list(range(1, 11))}[n]
    a, ref = run(ctx, rws, 1.0, what='smallest tile')
    monkeypatch.setenv('GINSIM_OALLAN_TILE', '0')
    run(ctx, rws, 1.0, forms=STREAM, ref=ref, what='smallest stream')


def test_short_series_have_no_factor(ctx):
    import ginsim
    for n, fs in ((17, 1.0), (9, 1.0), (1000, 1000.0)):
        oavar, tau = ginsim.oallan_var_host(ctx, np.arange(float(n)), fs)
        assert oavar.size == 0 and tau.size == 0


# ---- one tile and its edges
def test_tile_edges(ctx):
    """n around C, C + H and 2 C: the last valid shift n - 2m of every tile-form factor falls in the payload, on its last entry and
    in the halo of the first tile, and in a second and a third tile."""
    Cp, H = _geometry()
    for n in (Cp - 1, Cp, Cp + 1, Cp + H - 1, Cp + H, Cp + H + 1, 2 * Cp, 2 * Cp + 1):
        run(ctx, rows(('white', 'walk'), n, n), 1.0, what='tile edge')


# ---- the form boundary
def test_form_boundary_both_forms_against_the_same_exact_values(ctx, monkeypatch):
    import ginsim
    Cp, H = _geometry()
    n = _both_forms_n(H)                # the largest tile-form factor and the smallest stream-form factor are both present
    mult = ox.factors(n, 1.0)
    assert any(2 * m <= H for m in mult) and any(2 * m > H for m in mult)
    rws = rows(('white', 'offset', 'walk'), n, 11)
    a, ref = run(ctx, rws, 1.0, what='boundary')
    monkeypatch.setenv('GINSIM_OALLAN_TILE', '0')
    b, _ = run(ctx, rws, 1.0, forms=STREAM, ref=ref, what='boundary all-stream')
    f = ginsim.oallan_plan(0, n, 3, n, 1.0)[0]
    monkeypatch.delenv('GINSIM_OALLAN_TILE')
    f1 = ginsim.oallan_plan(0, n, 3, n, 1.0)[0]
    stream = [i for i, e in enumerate(f1) if e['form'] == STREAM]
    assert stream and all(e['form'] == STREAM for e in f)
    np.testing.assert_array_equal(a[:, stream], b[:, stream])      # the same kernel on the same prefix


# ---- the stream form's work items
def test_stream_work_item_edges(ctx, monkeypatch):
    """n - 2m + 1 of the largest factor one less than, exactly and one more than the stream form's work-item length."""
    import ginsim
    W = _stream_item()
    found = {}
    for n in range(W, 3 * W):
        d = n - 2 * ox.factors(n, 1.0)[-1] + 1 - W
        if d in (-1, 0, 1) and d not in found:
            found[d] = n
    assert sorted(found) == [-1, 0, 1], (W, found)
    monkeypatch.setenv('GINSIM_OALLAN_TILE', '0')
    for d, n in sorted(found.items()):
        last = ginsim.oallan_plan(0, n, 2, n, 1.0)[0][-1]
        assert last['terms'] == W + d and last['nparts'] == (2 if d == 1 else 1)
        run(ctx, rows(('white', 'walk'), n, n), 1.0, forms=STREAM, what='stream item %+d' % d)


# ---- batches and layout
def test_batches_strides_alignment_and_repeatability(ctx):
    Cp, H = _geometry()
    n = _both_forms_n(H)                # both forms, a few tiles, odd
    kinds = ('white', 'offset', 'walk')
    rws = rows([kinds[s % 3] for s in range(65)], n, 21)
    ref = [ox.exact(x, 1.0)[0] for x in rws[:3]]
    full, _ = run(ctx, rws, 1.0, ref=ref + [ox.exact(x, 1.0)[0] for x in rws[3:]], what='batch 65')
    again, _ = run(ctx, rws, 1.0, ref=[r for r in full], what='batch 65 again')        # held to the first launch: ratio 0
    np.testing.assert_array_equal(full, again)
    for S in (1, 2, 3, 64):
        for stride, off in ((n, 0), (n + 3, 0), (n, 1), (n + 3, 1)):        # off 1: the base address at 8 modulo 16
            if S == 64 and (stride, off) != (n + 3, 1):
                continue
            got, _ = run(ctx, rws[:S], 1.0, stride=stride, off=off, ref=list(full[:S]), what='batch %d stride %d off %d' % (S, stride, off))
            np.testing.assert_array_equal(got, full[:S])                    # alone or in any batch: the same bits
    alone, _ = run(ctx, [rws[64]], 1.0, ref=[full[64]], what='last alone')
    np.testing.assert_array_equal(alone[0], full[64])


# ---- inputs that break naive forms
@pytest.mark.parametrize('stream', [False, True])
def test_offset_ramp_constant_and_walk(ctx, stream, monkeypatch):
    Cp, H = _geometry()
    n = 9 * H // 2 + 1001
    if stream:
        monkeypatch.setenv('GINSIM_OALLAN_TILE', '0')
    rws = rows(('offset', 'ramp', 'const', 'walk'), n, 31)
    oavar, ref = run(ctx, rws, 1.0, forms=STREAM if stream else None, what='inputs')
    m = np.array(ox.factors(n, 1.0), dtype=np.float64)
    closed = 0.25 * m * m / 2.0                                             # d = m^2 slope exactly: oavar = slope^2 m^2 / 2
    np.testing.assert_allclose(ref[1], closed, rtol=1e-15)
    assert ox.ratio(oavar[1], closed, ox.bound(rws[1], closed, m)) <= 1.0
    assert np.array_equal(oavar[2], np.zeros(m.size))


# ---- non-finite samples
@pytest.mark.parametrize('stream', [False, True])
@pytest.mark.parametrize('bad', [np.nan, np.inf])
def test_a_non_finite_sample_spoils_its_series_alone(ctx, stream, bad, monkeypatch):
    import ginsim
    Cp, H = _geometry()
    n = Cp + H + 19
    if stream:
        monkeypatch.setenv('GINSIM_OALLAN_TILE', '0')
    rws = rows(('white', 'walk', 'offset'), n, 41)
    clean, _ = run(ctx, rws, 1.0, forms=STREAM if stream else None, what='clean')
    for at in (0, Cp, n - 1):
        x = [r.copy() for r in rws]
        x[1][at] = bad
        got, _ = ginsim.oallan_var_host(ctx, np.stack(x), 1.0)
        assert np.isnan(got[1]).all(), (at, got[1])
        np.testing.assert_array_equal(got[[0, 2]], clean[[0, 2]])


# ---- refusals
def test_refusals_in_order_and_one_series_too_many(ctx):
    """The refusals of ginsim_allan with the prefix oallan:, in its order: NULL, sizes, (no factor: nothing to refuse), the grid
    limit, the capacity.  No refused call may launch on the pointer, which is not one."""
    import ginsim
    from ginsim import _lib
    tau, ov, nt = np.empty(128), np.empty(128), C.c_int32(0)
    fake = 1 << 30
    err = lambda: _lib.lib.ginsim_last_error().decode()                      # noqa: E731
    call = lambda S, n, cap=128, fs=10.0, stride=None, x=fake: _lib.lib.ginsim_oallan(    # noqa: E731
        ctx.handle, x, n, S, n if stride is None else stride, fs, _lib.dptr(tau), _lib.dptr(ov), C.byref(nt), cap)
    assert call(0, 0, 0, x=None) == _lib.ERR_ARG and err() == 'oallan: NULL argument'
    for kw in (dict(S=1, n=0), dict(S=0, n=100), dict(S=1, n=100, stride=99), dict(S=1, n=100, fs=0.0), dict(S=1, n=100, fs=-1.0),
               dict(S=1, n=100, fs=float('inf')), dict(S=1, n=100, fs=float('nan'))):
        assert call(cap=0, **kw) == _lib.ERR_ARG and err() == 'oallan: bad sizes', kw
    assert call(2 ** 31 - 1, 89, 0) == _lib.OK and nt.value == 0             # 89 samples at 10 Hz: no factor, nothing to do
    assert call(2 ** 31 - 1, 2521, 0) == _lib.ERR_RANGE                      # the grid limit before the capacity
    found = re.search(r'the device takes (\d+)', err())
    assert found, err()
    limit = int(found.group(1))
    assert 65535 <= limit < 2 ** 31 - 1
    assert call(limit + 1, 2521) == _lib.ERR_RANGE and nt.value == 0
    msg = err()
    assert msg.startswith('oallan:') and '%d series' % (limit + 1) in msg and 'takes %d' % limit in msg and 'split the batch' in msg
    with pytest.raises(ValueError, match='split the batch'):
        _lib.check(call(limit + 1, 2521))
    ntau = len(ox.factors(2521, 10.0))
    assert call(limit, 2521, ntau - 1) == _lib.ERR_RANGE and err() == 'oallan: %d averaging factors but capacity %d' % (ntau, ntau - 1)
    assert nt.value == 0


# ---- through the layers
def test_job_keyword_module_and_plugin(ctx):
    import ginsim
    from ginsim import workloads
    from gnss_ins_sim.allan import allan
    from demo_algorithms import allan_analysis
    fs, runs, n = 100.0, 2, 2000
    text = open(workloads.profile_path('static_1800s')).read().split('\n')
    ini, _ = workloads.parse_motion('\n'.join(text[:4]))
    raw = ginsim.pathgen(ini, np.array([[1.0, 0, 0, 0, 0, 0, 0, n / fs, 0.0]]), fs, 0.0, workloads.HIGH_MOBILITY, 1)
    truth = {'ref_accel': np.ascontiguousarray(raw['imu'][:, 1:4]), 'ref_gyro': np.ascontiguousarray(raw['imu'][:, 4:7]),
             'ref_pos': raw['nav'][:, 1:4], 'ref_vel': raw['nav'][:, 4:7], 'ref_att': raw['nav'][:, 7:10]}
    assert truth['ref_accel'].shape[0] == n
    acc, gyr = workloads.imu_grade('mid-accuracy')
    job = ginsim.MonteCarloJob(ctx, fs, 1, truth, acc, gyr, None, runs=runs, algos=(), seed=77, keep_sensors=True).run()
    host = {nm: job.sensors(nm, list(range(runs))) for nm in ('accel', 'gyro')}             # (runs, n, 3)
    series = np.concatenate([host[nm].transpose(0, 2, 1).reshape(3 * runs, n) for nm in ('accel', 'gyro')])     # [sensor][run][axis][n]
    tau, ad = job.allan(fs, overlapping=True)
    ov, t2 = ginsim.oallan_var_host(ctx, series, fs)
    np.testing.assert_array_equal(tau, t2)
    for i, nm in enumerate(('accel', 'gyro')):
        assert ad[nm].shape == (runs, tau.size, 3)
        np.testing.assert_array_equal(ad[nm], np.sqrt(ov).reshape(2, runs, 3, -1)[i].transpose(0, 2, 1))
    for s in (0, 5, 11):
        e = ox.exact(series[s], fs)[0]
        assert ox.ratio(ov[s], e, ox.bound(series[s], e, np.array(ox.factors(n, fs)))) <= 1.0
    # without the keyword: today's path, the bits of allan_var on the same series
    tau0, ad0 = job.allan(fs)
    av, t0 = ginsim.allan_var_host(ctx, series, fs)
    np.testing.assert_array_equal(tau0, t0)
    np.testing.assert_array_equal(tau0, tau)                                 # the two curves share their tau
    for i, nm in enumerate(('accel', 'gyro')):
        np.testing.assert_array_equal(ad0[nm], np.sqrt(av).reshape(2, runs, 3, -1)[i].transpose(0, 2, 1))
    assert not np.array_equal(ad0['gyro'], ad['gyro'])
    job.release()
    # the module function and the plugin on host arrays
    o1, t1 = allan.oallan_var(series[3], fs)
    np.testing.assert_array_equal(o1, ov[3])
    assert allan.oallan_var(series[3][:50], fs) == ([], [])
    a = allan_analysis.Allan(overlapping=True)
    assert a.input == ['fs', 'accel', 'gyro'] and a.output == ['algo_time', 'ad_accel', 'ad_gyro']
    a.run([fs, host['accel'][0], host['gyro'][0]])
    t3, ad_a, ad_g = a.get_results()
    np.testing.assert_array_equal(ad_a, np.sqrt(ov[0:3].T))
    np.testing.assert_array_equal(ad_g, np.sqrt(ov[3 * runs:3 * runs + 3].T))
    assert allan_analysis.Allan().overlapping is False


def test_sim_with_the_overlapping_plugin(ctx):
    from gnss_ins_sim.sim import imu_model, ins_sim
    from demo_algorithms import allan_analysis
    from conftest import PKG
    with open(os.path.join(PKG, 'motion_profiles', 'static_1800s.csv')) as f:
        lines = f.read().splitlines()
    short = os.path.join(os.environ.get('TMPDIR', '/tmp'), 'static_oallan_%d.csv' % os.getpid())
    cmd = lines[3].split(',')
    cmd[7] = '20'
    with open(short, 'w') as f:
        f.write('\n'.join(lines[:3] + [','.join(cmd)]) + '\n')
    try:
        fs, runs = 100.0, 2
        imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=False)
        sims = {}
        for over in (True, False):
            sim = ins_sim.Sim([fs, 0.0, 0.0], short, ref_frame=1, imu=imu, mode=None, env=None,
                              algorithm=allan_analysis.Allan(overlapping=over), seed=5)
            sim.run(runs)
            sims[over] = sim
        ntau = len(ox.factors(sims[True].dmgr.gyro.data[0].shape[0], fs))
        assert ntau > 0
        for r in range(runs):
            key = 'algo0_%d' % r
            d = sims[True].dmgr
            assert d.ad_accel.data[key].shape == (ntau, 3) and d.ad_gyro.data[key].shape == (ntau, 3)
            np.testing.assert_array_equal(d.algo_time.data[key], sims[False].dmgr.algo_time.data[key])
            g = d.gyro.data[r]
            for ax in range(3):
                e = ox.exact(g[:, ax], fs)[0]
                tol = ox.bound(g[:, ax], e, np.array(ox.factors(g.shape[0], fs)))
                assert ox.ratio(d.ad_gyro.data[key][:, ax] ** 2, e, 2 * tol + 4 * 2.0 ** -53) <= 1.0      # sqrt and square: two roundings more
    finally:
        os.remove(short)


# ---- one full-size case
def test_full_size_six_series(ctx):
    """6 x 1 440 000 at 400 Hz: 46 factors up to m = 100 000, 256 tiles and 88 work items per series."""
    n, fs = 1440000, 400.0
    assert len(ox.factors(n, fs)) == 46 and ox.factors(n, fs)[-1] == 100000
    rws = rows(('white', 'offset', 'walk', 'white', 'walk', 'offset'), n, 51)
    run(ctx, rws, fs, what='full size')
