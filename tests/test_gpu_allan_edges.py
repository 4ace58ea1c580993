"""The Allan kernels (csrc/allan.hip) at every edge of the host's level plan: each case asserts through ginsim.allan_plan WHICH
kernel form ran at every level (the table of tests/allan_cases.py, pinned without a device by test_allan_plan.py), and compares
every series with the exact Allan variance of tests/allan_exact.py under the tolerance derived there -- 1e-10 plus what an fp64
implementation may lose to an offset, 2.8e-7 at most and 1e-10 on rows without one.  The largest error-to-tolerance ratio of a
group is printed and recorded.

Sections: (a) the forms of level 0 by length, stride parity and base alignment; (b) the fuse boundary, fused against two
launches; (c) chunked levels 2 and 3; (d) the number of levels at powers of ten; (e) several chunks per workgroup of the pair
kernel and more than 1024 series; (f) the register-staged kernel with three chunks per wavefront, forced in a child process;
(g) non-finite samples; and the refusal of more series than the grid's y dimension takes."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import allan_cases as ac
import allan_exact as ax
from allan_cases import L, T, ALIGNED, ODD, OFF8
from test_gpu_full_size import _record

pytestmark = pytest.mark.gpu

WORST = {}
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def ctx():
    import ginsim
    c = ginsim.Context(0)
    yield c
    c.close()


def _note(group, case, r):
    WORST[group] = max(WORST.get(group, 0.0), r)
    print('allan edges %s %s: error / bound %.3g (worst of the group so far %.3g)' % (group, case, r, WORST[group]))
    _record('allan_edges_' + group, ratio=WORST[group])
    assert r <= 1.0, (group, case, r)


def _modes(lv):
    return tuple(l['mode'] for l in lv)


def _exact(rws, fs):
    """[(exact avar, tolerance)] per row."""
    levels = ax.factors(rws[0].size, fs)[1]
    out = []
    for x in rws:
        ea, _ = ax.exact(x, fs)
        out.append((ea, ax.bound(x, ea, levels)))
    return out


def _ratio(avar, ref):
    """Largest error over tolerance of the device's rows against [(exact, tolerance)]; every evaluated factor must be finite."""
    worst = 0.0
    for s, (ea, tol) in enumerate(ref):
        assert np.isfinite(avar[s]).all(), s
        worst = max(worst, ax.ratio(avar[s], ea, tol))
    return worst


def _run(ctx, flat, n, S, stride, fs, offset, plan, ntau=None):
    """Upload, assert the plan of exactly this call, run it."""
    import ginsim
    buf = ctx.upload(flat)
    assert buf.ptr % 256 == 0
    ptr = buf.ptr + offset
    nt, lv = ginsim.allan_plan(ptr, n, S, stride, fs)
    assert _modes(lv) == tuple(plan), (n, S, stride, offset, lv)
    avar, tau = ginsim.allan_var(ctx, ptr, n, S, stride, fs)
    mult = ax.factors(n, fs)[0]
    assert nt == len(mult) == tau.size and (ntau is None or nt == ntau)
    np.testing.assert_array_equal(tau, np.array([m * (1.0 / fs) for m in mult]))
    return avar, tau, lv, buf


# ---- a
@pytest.mark.parametrize('n', sorted(ac.LEVEL0))
def test_level0_forms_every_placement(ctx, n, monkeypatch):
    """2520 (one chunk: tail), 2521 and 2559 (chunked, below the DMA stage), 2560 / 2561 (the first DMA chunk, and a second chunk of
    one entry), 5039 .. 5041 (two chunks to a third of one entry), 5079 / 5080 (the second chunk staged through registers / the
    first length at which the DMA takes it) -- on an aligned even-stride buffer, with an odd stride, and at 8 modulo 16: the last
    two run the register-staged kernel on doubles that are not 16-byte aligned."""
    monkeypatch.delenv('GINSIM_ALLAN_FUSE', raising=False)
    fs = ac.fs_of(n)
    rws = ac.rows(100, n, fs)
    ref = _exact(rws, fs)
    got = {}
    for where in (ALIGNED, ODD, OFF8):
        stride, off = ac.placement(n, where)
        plan = ac.level0_plan(n, where)
        avar, tau, lv, buf = _run(ctx, ac.pack(rws, stride, off), n, 4, stride, fs, off, plan, ac.LEVEL0_NTAU[n])
        if where != ALIGNED:
            assert lv[0]['mode'] in (L, T)
        _note('a', '%d %s' % (n, where), _ratio(avar, ref))
        got[where] = avar
        buf.free()
    np.testing.assert_array_equal(got[ODD], got[OFF8])          # the same kernel on the same values
    np.testing.assert_allclose(got[ALIGNED], got[ODD], rtol=1e-11)


# ---- b
@pytest.mark.parametrize('n', sorted(ac.FUSE))
def test_fuse_boundary_fused_and_two_launches(ctx, n, monkeypatch):
    """25 209: level 1 is exactly one chunk, pair + tail.  25 210: fused, the second workgroup's level-0 share is 10 entries and its
    level-1 chunk ONE entry.  27 720 = 11 chunks, 27 760 the first length whose 11th chunk the DMA takes, 50 400 = two full
    workgroups, 50 410 a third with one chunk of ten entries."""
    fs = 100.0
    rws = ac.rows(200, n, fs)
    ref = _exact(rws, fs)
    stride, off = ac.placement(n, ALIGNED)
    flat = ac.pack(rws, stride)
    monkeypatch.delenv('GINSIM_ALLAN_FUSE', raising=False)
    fused, _, lv, buf = _run(ctx, flat, n, 4, stride, fs, 0, ac.FUSE[n][0])
    assert lv[0]['nparts'] == ac.FUSE_PARTS[n]
    buf.free()
    monkeypatch.setenv('GINSIM_ALLAN_FUSE', '0')
    two, _, lv, buf = _run(ctx, flat, n, 4, stride, fs, 0, ac.FUSE[n][1])
    assert lv[0]['nparts'] == -(-n // 2520)
    buf.free()
    np.testing.assert_allclose(fused, two, rtol=1e-11)
    _note('b', '%d fused' % n, _ratio(fused, ref))
    _note('b', '%d two launches' % n, _ratio(two, ref))


# ---- c
@pytest.mark.parametrize('key', sorted(ac.DEEP))
def test_deeper_levels(ctx, key, monkeypatch):
    """Level 2 of 2520 / 2521 / 2559 / 2560 / 2561 entries behind the fused launch (tail, the window below the DMA stage twice,
    pair, register-staged because 2561 is odd); an odd first stride with level 1 of 36 000 (pair) and 36 001 (register-staged)
    entries; one series of 2 521 000 and 2 560 000 samples: level 3 chunked (register-staged, pair), the ping / pong buffers
    flipped three times."""
    monkeypatch.delenv('GINSIM_ALLAN_FUSE', raising=False)
    n, S, where = key
    fs = 100.0
    rws = ac.rows(300, n, fs, S)
    ref = _exact(rws, fs)
    stride, off = ac.placement(n, where)
    avar, tau, lv, buf = _run(ctx, ac.pack(rws, stride, off), n, S, stride, fs, off, ac.DEEP[key])
    buf.free()
    _note('c', '%d x %d %s' % (S, n, where), _ratio(avar, ref))


# ---- d
@pytest.mark.parametrize('key', sorted(ac.POWERS))
def test_powers_of_ten_of_the_largest_factor(ctx, key, monkeypatch):
    """ntau and tau equal the oracle's exactly where floor(n / 9) is a power of ten or one more: 9009 samples have a 28th factor
    (1000) that lives in a tail level of nine entries; 899 samples at 100 Hz have none."""
    from oracle import ins_np
    monkeypatch.delenv('GINSIM_ALLAN_FUSE', raising=False)
    n, fs = key
    ntau, plan = ac.POWERS[key]
    rws = ac.rows(400, n, fs)
    stride, off = ac.placement(n, ALIGNED)
    avar, tau, lv, buf = _run(ctx, ac.pack(rws, stride), n, 4, stride, fs, 0, plan, ntau)
    buf.free()
    assert avar.shape == (4, ntau)
    for s in range(4):
        oa, ot = ins_np.allan_var(rws[s], fs)
        assert ot.size == ntau
        np.testing.assert_array_equal(tau, ot)
    if ntau:
        _note('d', '%d at %g Hz' % (n, fs), _ratio(avar, _exact(rws, fs)))


# ---- e
@pytest.mark.parametrize('key', sorted(ac.BATCH))
def test_chunks_per_workgroup_and_series_counts(ctx, key, monkeypatch):
    """The pair kernel's pipeline over 3 and 4 chunks of one workgroup (two requests in flight, the request into the stage just
    read, a ragged last chunk staged through registers behind DMA chunks), 1025 series (the branch past 1024) and the capped regime
    (18 chunks x 1024 series: four per workgroup, five workgroups, the last with two).  Eight distinct rows tiled: the distinct ones
    against the exact reference, EVERY series against its twin eight rows earlier bit for bit -- a series that read a neighbour's
    chunk or record would differ."""
    monkeypatch.setenv('GINSIM_ALLAN_FUSE', '0')
    S, n = key
    plan, cpb, parts = ac.BATCH[key]
    fs = ac.fs_of(n)
    rws = ac.rows(500, n, fs, 8)
    ref = _exact(rws, fs)
    flat = np.resize(np.stack(rws), (S, n))             # row s = distinct row s % 8
    assert np.array_equal(flat[S - 1], rws[(S - 1) % 8])
    avar, tau, lv, buf = _run(ctx, flat, n, S, n, fs, 0, plan)
    buf.free(pool=False)
    assert (lv[0]['chunks_per_block'], lv[0]['nparts']) == (cpb, parts)
    _note('e', '%d x %d' % (S, n), _ratio(avar[:8], ref))
    np.testing.assert_array_equal(avar[8:], avar[:-8])


# ---- f
def _forced_child(setting):
    env = dict(os.environ)
    for k in ('GINSIM_ALLAN_DMA', 'GINSIM_ALLAN_CPW', 'GINSIM_ALLAN_FUSE'):
        env.pop(k, None)
    env.update(ac.FORCED_ENV[setting])
    env['PYTHONPATH'] = os.pathsep.join([p for p in sys.path if p])
    out = subprocess.run([sys.executable, os.path.join(HERE, 'allan_forced_child.py'), setting], env=env, stdout=subprocess.PIPE,
                         timeout=300, check=True, universal_newlines=True)
    got = json.loads(out.stdout.strip().splitlines()[-1])
    return {int(n): np.array(v) for n, v in got.items()}


@pytest.fixture(scope='module')
def forced_reference(ctx):
    """Per n: the rows' exact values and what the default plan gives for the same buffers."""
    import ginsim
    ref = {}
    for n in ac.FORCED:
        fs = ac.fs_of(n)
        rws = ac.rows(600, n, fs, ac.FORCED_S)
        stride, _ = ac.placement(n, ALIGNED)
        buf = ctx.upload(ac.pack(rws, stride))
        avar, _ = ginsim.allan_var(ctx, buf, n, ac.FORCED_S, stride, fs)
        buf.free()
        ref[n] = (_exact(rws, fs), avar)
    return ref


@pytest.mark.parametrize('setting', sorted(ac.FORCED_ENV))
def test_register_staged_form_forced_in_a_child_process(forced_reference, setting):
    """GINSIM_ALLAN_DMA=0 with and without GINSIM_ALLAN_CPW=3 (read once per process: a fresh child each, which asserts mode 0 and
    the chunks per wavefront at every chunked level -- tests/allan_forced_child.py): a wavefront's loop over three chunks with the
    stage reused between fences, at 2 chunks (one wavefront takes both), 4 (the second wavefront gets a chunk of ONE entry), 7, 40
    and 101 / 11 / 2 chunks at levels 0 / 1 / 2."""
    got = _forced_child(setting)
    for n in ac.FORCED:
        exact, default = forced_reference[n]
        assert got[n].shape == default.shape
        _note('f', '%d %s' % (n, setting), _ratio(got[n], exact))
        np.testing.assert_allclose(got[n], default, rtol=1e-11)


# ---- g
@pytest.mark.parametrize('n', sorted(ac.NONFINITE))
def test_nonfinite_samples_poison_exactly_the_factors_that_hold_them(ctx, n, monkeypatch):
    """The reference drops the tail x[nb * m:] per factor, so a NaN near the end leaves most factors finite; the kernels subtract
    each chunk's first entry and mask absent bin pairs with selects -- a multiply where a select belongs would turn every factor
    NaN.  Per row and factor: finite exactly where the NumPy oracle is finite and there within the tolerance, NaN where it is NaN,
    non-finite where it is inf.  Plans: tail only, pair, fused, fused + a chunked level 2."""
    import ginsim
    from oracle import ins_np
    monkeypatch.delenv('GINSIM_ALLAN_FUSE', raising=False)
    fs = ac.fs_of(n)
    rws = ac.nonfinite_rows(n, fs)
    stride, _ = ac.placement(n, ALIGNED)
    avar, tau, lv, buf = _run(ctx, ac.pack(rws, stride), n, 7, stride, fs, 0, ac.NONFINITE[n])
    levels = len(lv)
    worst = 0.0
    for s, x in enumerate(rws):
        oa, _ = ins_np.allan_var(x, fs)
        fin = np.isfinite(oa)
        if s in (1, 2, 4) and n > 2000:             # a condition on the inputs: these rows tell a select from a multiply
            assert fin.any() and np.isnan(oa).any(), (s, fin.sum())
        np.testing.assert_array_equal(np.isfinite(avar[s]), fin, err_msg='row %d' % s)
        assert np.isnan(avar[s][np.isnan(oa)]).all(), s
        if fin.any():
            ea, _ = ax.exact(x, fs)
            assert np.isfinite(ea[fin]).all()
            tol = ax.bound(x, ea, levels)
            worst = max(worst, ax.ratio(avar[s][fin], ea[fin], tol[fin]))
    assert np.isfinite(avar[0]).all() and not np.isfinite(avar[3]).any() and not np.isfinite(avar[5]).all()
    np.testing.assert_array_equal(avar[0], avar[6])
    alone, _ = ginsim.allan_var(ctx, buf, n, 1, stride, fs)
    np.testing.assert_array_equal(alone[0], avar[0])
    buf.free()
    _note('g', '%d' % n, worst)


# ---- the grid's y dimension
def test_more_series_than_the_grid_takes_are_refused_before_any_launch(ctx):
    """The three chunked kernels have the series on the grid's y dimension (the Allan plugin passes 3 x runs series per sensor:
    21 846 runs reach 65 536).  One series more than the device's maxGridSize[1] is refused with the count, the limit and the
    advice; the pointer is never followed.  A tail-only call has the series on x and is planned as ever."""
    import ginsim
    from ginsim import _lib
    tau, avar, nt = np.empty(128), np.empty(128), C.c_int32(-1)
    fake = 1 << 30
    call = lambda S, n, cap=128: _lib.lib.ginsim_allan(ctx.handle, fake, n, S, n, 10.0, _lib.dptr(tau), _lib.dptr(avar), C.byref(nt), cap)  # noqa: E731
    # the limit from the refusal itself; with no room for a single factor this call is refused whatever the limit is, so nothing
    # can be launched on the pointer even where the check is missing
    assert call(2 ** 31 - 1, 2521, 0) == _lib.ERR_RANGE
    found = re.search(r'the device takes (\d+)', _lib.lib.ginsim_last_error().decode())
    assert found, _lib.lib.ginsim_last_error()
    limit = int(found.group(1))
    assert 65535 <= limit < 2 ** 31 - 1
    assert call(limit + 1, 2521) == _lib.ERR_RANGE and nt.value == 0
    msg = _lib.lib.ginsim_last_error().decode()
    assert msg.startswith('allan:') and '%d series' % (limit + 1) in msg and 'takes %d' % limit in msg and 'split the batch' in msg
    with pytest.raises(ValueError, match='split the batch'):
        _lib.check(call(limit + 1, 2521))
    _, lv = ginsim.allan_plan(fake, 2520, limit + 1, 2520, 10.0)
    assert _modes(lv) == (T, T, T)
    _, lv = ginsim.allan_plan(fake, 2521, limit + 1, 2521, 10.0)
    assert _modes(lv) == (L, T, T)
    # the context still works
    x = ac.rows(700, 2521, 10.0, 1)[0]
    got, _ = ginsim.allan_var_host(ctx, x, 10.0)
    assert ax.ratio(got, *_exact([x], 10.0)[0]) <= 1.0
