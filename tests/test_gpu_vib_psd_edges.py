"""ginsim_vib_psd_series (csrc/vib_psd.hip: the spectrum kernel, a batched complex-to-real hipFFT behind a plan cache, the tiled
transposition) called directly and held to the exact series of tests/vib_psd_exact.py: every period, tile and block edge of
vib_psd_exact.CASES, the halving rule at its first and last bin and past its underflow, the 32768-run cap of a block of runs, the
plan cache, both sensors, every axis -- and the launch that reads the series, through MonteCarloJob.

Every test prints its error over its bound; the bound per sample is A 2^-53 (1 + 16 DEV[id]) against the long-double sum and
A 2^-53 (1 + 17 DEV[id]) against the float64 restatement (vib_psd_exact has the derivation), and 1e-12 A in any event.

Measured on one MI355X (error / bound, the largest per section; DESIGN 4.1c has them): parity 0.21 (N62_R65_acc_off2p32_rand: 7.1
units of 34.6; 0.16 at N = 4098 and 16382, 0.15 at 16384), the closed form of the edge bins 0.061, halving 0.11 (halve_N512_from8),
blocks of runs 0.065, a run alone 0.065 and against its batch 0, the launch 0.0056 of the sensor tolerances; the same-bits tests
are bitwise.  No case is held to the ceiling in place of the margin.  The whole file: 14 s, hipFFT's plans of seventeen periods
included; the slowest test 1.9 s (N16384_R129)."""
import numpy as np
import pytest

import vib_psd_exact as vx
from test_gpu_edge_cases import _cut, _psd_def

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = -7.25e300                        # no sample can be that large: a place the call left alone shows
SENSOR = {'acc': 0, 'gyr': 1}


@pytest.fixture(scope='module')
def ctx():
    import ginsim
    c = ginsim.Context(0)
    yield c
    c.close()


def series(ctx, case, runs=None, off=None, halve=None, amp=None):
    """One ginsim_vib_psd_series call for the case (or for other runs of it): (3, N, runs).  The output lies in front of a guard of
    64 doubles, which must survive, in a buffer filled beforehand, of which every place must have been written."""
    import ginsim
    from ginsim import _lib
    runs = case.runs if runs is None else runs
    off = case.off if off is None else off
    halve = case.halve if halve is None else halve
    amp = np.ascontiguousarray(vx.case_amplitudes(case) if amp is None else amp)
    assert amp.shape == (3, case.N // 2 + 1)
    size = 3 * case.N * runs
    buf = ctx.upload(np.full(size + GUARD, FILL))
    try:
        _lib.check(ginsim.lib.ginsim_vib_psd_series(ctx.handle, amp.ctypes.data, case.N, runs, off, case.seed, SENSOR[case.sensor], halve, buf.ptr))
        out = ctx.download(buf, (size + GUARD,))
    finally:
        buf.free()
    assert np.all(out[size:] == FILL), 'the guard behind the output was written'
    out = out[:size].reshape(3, case.N, runs)
    assert np.all(np.isfinite(out)) and not np.any(out == FILL)
    return out


def hold(case, got, ref=None, what=''):
    """Parity of a (3, N, len(ref['runs'])) result: every position against the float64 restatement, the sampled ones against the
    long-double sum, and the ceiling.  Returns the larger error / bound."""
    ref = vx.reference(case) if ref is None else ref
    assert got.shape == ref['f64'].shape
    if not ref['A'].any():
        assert not got.any(), 'a table of zeros must give zeros'
    e64, eld = vx.deviation_f64(got, ref), vx.deviation(got, ref)
    r64, rld = e64 / vx.allowed(case, vx.MARGIN + 1), eld / vx.allowed(case)
    print('%s%s: %.3g units of A 2^-53 from the long-double sum (bound %.3g), %.3g from the restatement; error / bound %.3g'
          % (case.id, what, eld, vx.allowed(case), e64, max(r64, rld)))
    assert rld <= 1.0 and r64 <= 1.0, (case.id, eld, e64)
    assert max(e64, eld) * vx.UNIT <= vx.CEILING
    return max(r64, rld)


# ---- parity
@pytest.mark.parametrize('cid', [c.id for c in vx.CASES + vx.RESEEDED + vx.OTHER_SENSOR + vx.SWAPPED])
def test_series_parity_at_every_period_tile_and_block_edge(ctx, cid):
    """Each case of the square {1, 63, 64, 65, 129 runs} x {tiny, tile-edge, block-edge, composite, capped period}, and the ones
    derived from them: another seed (other imaginary parts of bins 0 and N/2, which must not matter: N = 64, 4098), the other
    sensor, two rows of the table swapped.  First, on the reference alone: the case can see a swap of the axes' normals, a lost
    (-1)^j, a lost run offset, and its derived cases are not the case itself."""
    case = vx.BY_ID[cid]
    if case.table == 'rand' and case.N > 2:
        assert vx.moved(case, 'swap_axes') > 1e3 and vx.moved(case, 'no_alternation') > 1e3
    if case.off and case.table != 'zero':
        assert vx.moved(case, 'local_run') > 1e3
    if case.base:
        base = vx.reference(vx.BY_ID[case.base])
        d = np.abs(vx.reference(case)['exact'] - base['exact']).astype(np.float64)
        assert vx._ratio(d, base['A'][:, None, base['at']]) > 1e3 * vx.allowed(case)
    hold(case, series(ctx, case))


def test_the_edge_bins_alone_in_closed_form(ctx):
    """a[0] and a[L-1] alone: x[j] = (a0 cos(pi z0) + (-1)^j aL cos(pi zL)) / N, whatever the sines of z0 and zL are -- the
    imaginary parts the spectrum kernel writes into bins 0 and N/2 are ignored by the transform."""
    for cid in ('N4_R65_gyr_off37_edges', 'N130_R65_gyr_off37_edges'):
        case = vx.BY_ID[cid]
        got, a, N = series(ctx, case), vx.case_amplitudes(case).astype(vx.LD), case.N
        worst = 0.0
        for r in (0, 63, 64):
            z = vx.normals(case, r).astype(vx.LD)
            assert np.abs(np.sin(vx.PI * z[[0, -1]])).min() > 1e-3              # there IS an imaginary part to ignore
            c = np.cos(vx.PI * z)
            want = (a[:, 0] * c[0])[:, None] + np.where(np.arange(N) % 2 == 0, 1, -1)[None, :] * (a[:, -1] * c[-1])[:, None]
            worst = max(worst, vx._ratio(np.abs(got[:, :, r] - want / N).astype(np.float64), vx.unit(a)[:, None]))
        print('%s: closed form of bins 0 and N/2, error / bound %.3g' % (cid, worst / vx.allowed(case)))
        assert worst <= vx.allowed(case)


# ---- the halving rule
@pytest.mark.parametrize('cid', [c.id for c in vx.HALVING])
def test_halving_at_the_first_and_last_interior_bin_and_past_its_underflow(ctx, cid):
    """halve_per_run: global run g sees a[1 .. L-2] sqrt(0.5^(g + 1)), bins 0 and L-1 as given -- at N = 4, 6, 66, 512 (one interior
    bin, two, many, the bin past the spectrum kernel's first block) and the run ids 0, 1, 2, 9, 1000, 2300, each through
    run_offset.  First, on the reference alone: a halving of bin 0 or bin L-1, or none of bin 1 or L-2, would show."""
    case = vx.BY_ID[cid]
    for fault in ('halve_bin0', 'halve_last', 'skip_bin1', 'skip_last_interior', 'local_run'):
        if fault != 'local_run' or case.off:
            assert vx.moved(case, fault) > 1e3, fault
    got = series(ctx, case)
    hold(case, got)
    if case.off == 2299:                    # 0.5^2301 is zero: the closed form of bins 0 and N/2 alone, which nothing has scaled
        a, N = vx.case_amplitudes(case).astype(vx.LD), case.N
        for r in range(3):
            c = np.cos(vx.PI * vx.normals(case, r).astype(vx.LD))
            want = (a[:, 0] * c[0])[:, None] + np.where(np.arange(N) % 2 == 0, 1, -1)[None, :] * (a[:, -1] * c[-1])[:, None]
            A = (a[:, 0] + a[:, -1]).astype(np.float64) / N
            assert vx._ratio(np.abs(got[:, :, r] - want / N).astype(np.float64), A[:, None]) <= vx.allowed(case)


def test_halving_has_nothing_to_halve_at_period_2(ctx):
    case = vx.BY_ID['N2_R1_gyr_off37_rand']
    plain = series(ctx, case, runs=65, off=0, halve=0)
    assert np.array_equal(series(ctx, case, runs=65, off=0, halve=1), plain)
    print('period 2 with and without halve_per_run: error / bound 0 (bitwise)')


# ---- blocks of runs
@pytest.mark.parametrize('cid', [c.id for c in vx.BLOCKS])
def test_blocks_of_32768_runs(ctx, cid):
    """More runs than the spectrum kernel's grid.y takes: 32768 + 65 runs of period 8 (two blocks, the second of 65 runs), 2 x 32768
    + 1 runs of period 2 (three blocks, the last of one run).  The first and the last run of every block to parity; every other
    run finite, written and no larger than A.  First, on the reference alone: a run id counted within its block would show."""
    case = vx.BY_ID[cid]
    ref = vx.reference(case)
    assert vx.moved(case, 'block_local_run') > 1e3 and ref['runs'].tolist() == list(case.rr)
    got = series(ctx, case)
    assert got.shape == (3, case.N, case.runs)
    hold(case, np.ascontiguousarray(got[:, :, ref['runs']]), ref)
    A = vx.unit(ref['a'])
    assert np.all(np.abs(got) <= (A * (1.0 + vx.allowed(case) * vx.UNIT))[:, None, None])
    # no two runs share their series: a block written over another, or the same ids twice, would
    flat = got.reshape(-1, case.runs)
    assert np.unique(flat, axis=1).shape[1] == case.runs


# ---- the same bits
def test_same_bits_call_after_call_with_a_cached_plan_and_on_a_fresh_context(ctx):
    """Two calls of one case; N = 64 with 65 runs, then 64, then 65 again on one context (the third call is served by the plan the
    first one made, the second made another for the same period); the same case on a fresh Context after another was closed."""
    import ginsim
    case = vx.BY_ID['N64_R63_gyr_off0_rand']
    first = series(ctx, case, runs=65)
    second = series(ctx, case, runs=64)
    third = series(ctx, case, runs=65)
    assert np.array_equal(first, third)
    assert np.array_equal(series(ctx, case, runs=64), second)
    big = vx.BY_ID['N4098_R65_gyr_off0_rand']
    assert np.array_equal(series(ctx, big), series(ctx, big))
    c2 = ginsim.Context(0)
    try:
        assert np.array_equal(series(c2, case, runs=65), first)
    finally:
        c2.close()
    c3 = ginsim.Context(0)                  # its stream may have the address of c2's: c2's plans went with c2
    try:
        assert np.array_equal(series(c3, case, runs=65), first)
        assert np.array_equal(series(c3, case, runs=64), second)
    finally:
        c3.close()
    assert np.array_equal(series(ctx, case, runs=65), first)           # and the first context's plans are still its own
    print('repeated calls, cached plans, fresh contexts: error / bound 0 (bitwise)')


def test_a_run_of_a_batch_against_the_same_run_alone(ctx):
    """Run r of a 129-run call and the same global run made alone (run_offset + r, one run): the batch size may change the FFT
    kernel, so the two agree within the bound, not to the bit; both are held to the reference."""
    case = vx.BY_ID['N66_R129_acc_off37_rand_halved']
    ref = vx.reference(case)
    batch = series(ctx, case)
    worst = 0.0
    for r in (0, 63, 64, 128):
        alone = series(ctx, case, runs=1, off=case.off + r)
        one = dict(ref, runs=np.array([r]), f64=ref['f64'][:, :, [r]], A=ref['A'][:, [r]], rr=np.array([r]), at=np.array([0]),
                   exact=ref['exact'][:, :, ref['rr'].tolist().index(r)][:, :, None])
        hold(case, alone, one, ' run %d alone' % r)
        worst = max(worst, vx._ratio(np.abs(alone[:, :, 0] - batch[:, :, r]), ref['A'][:, None, r]))
    print('%s: a run alone against the run in its batch, error / bound %.3g' % (case.id, worst / vx.allowed(case)))
    assert worst <= vx.allowed(case)


# ---- axes
def test_swapping_two_rows_of_the_table_leaves_the_third_axis_alone(ctx):
    """The rows are the axes' amplitudes, the normals stay with the axis: with rows p and q swapped, the third axis keeps its
    bits (parity of the two swapped ones: the rows cases of the parity test)."""
    base = vx.BY_ID[vx.SWAPPED[0].base]
    plain = series(ctx, base)
    for case in vx.SWAPPED:
        got = series(ctx, case)
        kept = [c for c in range(3) if case.perm[c] == c][0]
        assert np.array_equal(got[kept], plain[kept])
        for c in set(range(3)) - {kept}:
            assert not np.array_equal(got[c], plain[c]) and not np.array_equal(got[c], plain[case.perm[c]])
    print('rows swapped: the third axis, error / bound 0 (bitwise)')


# ---- through the launch that reads the series
def _long(truth, n):
    reps = -(-n // 1000)
    return {k: (np.concatenate([v] * reps)[:n] if hasattr(v, 'shape') and v.shape and v.shape[0] == 1000 else v) for k, v in truth.items()}


RANDOM = {'type': 'random', 'x': 2e-3, 'y': 1e-3, 'z': 3e-3}
SINUS = {'type': 'sinusoidal', 'x': 0.3, 'y': 0.1, 'z': 0.2, 'freq': 7.0}


@pytest.mark.parametrize('n, runs, off, acc_psd, gyr_psd, other', [
    (2, 65, 2 ** 32 + 5, 'interpolated', None, 'random'),           # the accelerometer has a PSD, the gyroscope a 'random' term
    (3, 65, 0, None, 'grid', 'sinusoidal'),                         # the reverse, with 'sinusoidal'; given on the grid: halved per run
    (999, 129, 37, 'interpolated', None, None),                     # one sensor has a PSD, the other nothing
    (16385, 65, 0, None, 'interpolated', None),
])
def test_the_launch_reads_the_series_at_every_period(ctx, n, runs, off, acc_psd, gyr_psd, other):
    """MonteCarloJob on the turn profile cut (or repeated) to n samples, sensors only: period 2; period 4 for n = 3, whose last
    sample is never read; period 1000 for n = 999; period 16384 for n = 16385, whose last sample is the period's first again.
    Against oracle.ins_np.mc_sensors at the sensor tolerances of tests/test_gpu_edge_cases.py."""
    import ginsim
    from ginsim import workloads
    from oracle import ins_np
    _, truth, _ = workloads.truth_from_profile('turn_90deg', 100.0, 1)
    t = _cut(truth, n) if n <= 1000 else _long(truth, n)
    assert t['ref_accel'].shape[0] == n
    period = min(n + n % 2, 16384)
    mk = {'interpolated': lambda u: _psd_def(u), 'grid': lambda u: _psd_def(u, grid=period // 2 + 1), None: lambda u: None}
    extra = {'random': RANDOM, 'sinusoidal': SINUS, None: None}[other]
    va = mk[acc_psd](1.0) if acc_psd else (extra if gyr_psd and other == 'sinusoidal' else None)
    vg = mk[gyr_psd](1e-3) if gyr_psd else (extra if acc_psd and other == 'random' else None)
    acc, gyr = workloads.imu_grade('low-accuracy')
    seed = 2 ** 40 + 77
    job = ginsim.MonteCarloJob(ctx, 100.0, 1, t, acc, gyr, None, runs=runs, run_offset=off, algos=(), seed=seed, keep_sensors=True,
                               vib_accel=va, vib_gyro=vg).run()
    name = job.kernel_name()
    print('n %d, %d runs: %s' % (n, runs, name))
    assert name.startswith('ginsim::mc_kernel<') and name.endswith('true>') and job.sensor_layout == 'runs'
    for v, psd, d in ((job.params.vib_accel, acc_psd, va), (job.params.vib_gyro, gyr_psd, vg)):
        assert v.type == (3 if psd else 2 if d is SINUS else 1 if d is RANDOM else 0)
        assert v.period == period or not psd
    assert bool(getattr(job, 'psd_given_on_grid', False)) == (gyr_psd == 'grid')
    pick = np.array(sorted({0, 1, 63, 64, runs - 1}))
    a_ref, g_ref = ins_np.mc_sensors(seed, off + pick, 100.0, t['ref_accel'], t['ref_gyro'], acc, gyr, va, vg)
    ga, gg = job.sensors('accel', pick), job.sensors('gyro', pick)
    ea, eg = np.max(np.abs(ga - a_ref)), np.max(np.abs(gg - g_ref))
    print('n %d: accelerometer %.3g of 1e-12, gyroscope %.3g of 1e-14; error / bound %.3g' % (n, ea, eg, max(ea / 1e-12, eg / 1e-14)))
    np.testing.assert_allclose(ga, a_ref, rtol=0, atol=1e-12)
    np.testing.assert_allclose(gg, g_ref, rtol=0, atol=1e-14)
    # the term is there, and the sample past the period is the period's first
    a0, g0 = ins_np.mc_sensors(seed, off + pick, 100.0, t['ref_accel'], t['ref_gyro'], acc, gyr)
    vib = (ga - a0) if acc_psd else (gg - g0)
    assert np.abs(vib).max() > (1e-3 if acc_psd else 1e-6)
    if n > 16384:
        np.testing.assert_allclose(vib[:, 16384], vib[:, 0], rtol=0, atol=1e-12 if acc_psd else 1e-14)
        assert np.abs(vib[:, 16384] - vib[:, 1]).max() > 1e3 * (1e-12 if acc_psd else 1e-14)
    job.release()
