"""Which kernel form an Allan call runs, without a device: ginsim_allan_plan is the planning code ginsim_allan launches from
(csrc/api_series.hip allan_plan), so this table pins the constants the GPU cases of test_gpu_allan_edges.py rely on -- kChunk
2520, kDmaStage 2560, kFuseChunks 10, 1024 workgroups in a round, 16 chunks each, total / 4096 capped at 8, the 16-byte and
stride-parity conditions of the LDS-DMA.  A retuned constant fails HERE, by name, and does not quietly turn a GPU case into a
test of another kernel."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import allan_cases as ac
import allan_exact
from allan_cases import L, P, F0, T, ALIGNED, ODD, OFF8
from conftest import REPO

BASE = 1 << 20          # stands for a 256-byte aligned device pointer; never followed


def _plan(n, S, stride, fs, offset=0):
    import ginsim
    ntau, lv = ginsim.allan_plan(BASE + offset, n, S, stride, fs)
    return ntau, lv


def _modes(lv):
    return tuple(l['mode'] for l in lv)


def _levels_are_the_decades(n, stride, lv):
    for k, l in enumerate(lv):
        assert l['n_in'] == n // 10 ** k
        assert l['in_stride'] == (stride if k == 0 else n // 10 ** k)
        if l['mode'] == T:
            assert l['n_in'] <= 2520 and (l['chunks_per_block'], l['nparts']) == (1, 1)
        else:
            assert l['n_in'] > 2520


def test_plan_entry_point_is_declared_bound_and_needs_no_device():
    import ginsim
    hdr = open(os.path.join(REPO, 'include', 'ginsim.h')).read()
    assert 'int ginsim_allan_plan(' in hdr and 'ginsim_allan_plan' in ginsim.EXPORTS
    assert callable(ginsim.allan_plan) and ginsim.ALLAN_MODES == ('level', 'pair', 'fused0', 'fused1', 'tail')
    for bad in (dict(n=0), dict(S=0), dict(stride=99), dict(fs=0.0)):
        kw = dict(n=100, S=1, stride=100, fs=1.0)
        kw.update(bad)
        with pytest.raises(ValueError, match='allan: bad sizes'):
            ginsim.allan_plan(BASE, kw['n'], kw['S'], kw['stride'], kw['fs'])
    from ginsim import _lib
    nt, nl = C.c_int32(-1), C.c_int32(-1)
    lv = (_lib.AllanLevel * 2)()
    assert _lib.lib.ginsim_allan_plan(BASE, 90009, 1, 90010, 1.0, C.byref(nt), C.byref(nl), lv, 2) == _lib.ERR_RANGE
    assert (nt.value, nl.value) == (37, 5) and b'5 levels but capacity 2' in _lib.lib.ginsim_last_error()
    assert _lib.lib.ginsim_allan_plan(BASE, 90009, 1, 90010, 1.0, None, C.byref(nl), lv, 2) == _lib.ERR_ARG


@pytest.mark.parametrize('n', sorted(ac.LEVEL0))
@pytest.mark.parametrize('where', [ALIGNED, ODD, OFF8])
def test_level0_forms_by_length_stride_parity_and_base(n, where):
    """kChunk and kDmaStage: 2520 is one chunk (tail), 2521..2559 chunked but below the DMA stage, from 2560 the wave-pair kernel --
    unless the stride is odd or the base sits at 8 modulo 16."""
    stride, off = ac.placement(n, where)
    ntau, lv = _plan(n, 4, stride, ac.fs_of(n), off)
    assert _modes(lv) == ac.level0_plan(n, where), (n, where)
    assert ntau == ac.LEVEL0_NTAU[n] == len(allan_exact.factors(n, ac.fs_of(n))[0])
    _levels_are_the_decades(n, stride, lv)
    if where != ALIGNED:
        assert lv[0]['mode'] in (L, T)
    nchunks = -(-n // 2520)
    if lv[0]['mode'] == P:          # 4 series: 256 workgroups per series in a round -> one chunk each
        assert (lv[0]['chunks_per_block'], lv[0]['nparts']) == (1, nchunks)
    if lv[0]['mode'] == L:          # two wavefronts per workgroup, one chunk each
        assert (lv[0]['chunks_per_block'], lv[0]['nparts']) == (1, (nchunks + 1) // 2 * 2)


def test_only_the_base_modulo_16_counts():
    for off in range(0, 64, 8):
        _, lv = _plan(5080, 4, 5092, 10.0, off)
        assert lv[0]['mode'] == (P if off % 16 == 0 else L), off


@pytest.mark.parametrize('n', sorted(ac.FUSE))
def test_fuse_boundary_both_forms(n, monkeypatch):
    """kFuseChunks and the fuse condition (level 1 of more than one chunk): 25 209 is pair + tail, 25 210 fused with a second
    workgroup; GINSIM_ALLAN_FUSE=0 (read per call) gives level 0 to the pair kernel and level 1 to the form its parity allows."""
    stride, _ = ac.placement(n, ALIGNED)
    monkeypatch.delenv('GINSIM_ALLAN_FUSE', raising=False)
    _, lv = _plan(n, 4, stride, 100.0)
    assert _modes(lv) == ac.FUSE[n][0]
    assert lv[0]['nparts'] == ac.FUSE_PARTS[n]
    if lv[0]['mode'] == F0:
        assert lv[0]['chunks_per_block'] == 10 and lv[1]['nparts'] == lv[0]['nparts'] and lv[1]['chunks_per_block'] == 1
    _levels_are_the_decades(n, stride, lv)
    monkeypatch.setenv('GINSIM_ALLAN_FUSE', '0')
    _, lv = _plan(n, 4, stride, 100.0)
    assert _modes(lv) == ac.FUSE[n][1]
    assert (lv[0]['chunks_per_block'], lv[0]['nparts']) == (1, -(-n // 2520))
    monkeypatch.setenv('GINSIM_ALLAN_FUSE', '1')
    assert _modes(_plan(n, 4, stride, 100.0)[1]) == ac.FUSE[n][0]
    # the fused form needs the LDS-DMA at level 0
    assert _modes(_plan(n, 4, stride + 1, 100.0)[1])[0] == L and _modes(_plan(n, 4, stride, 100.0, 8)[1])[0] == L


@pytest.mark.parametrize('key', sorted(ac.DEEP))
def test_deeper_levels_window_and_stride_parity(key, monkeypatch):
    """Levels past the first have their own length as stride and a 256-byte aligned base: 2521 and 2559 entries fall into the
    window below the DMA stage, 2560 is even (pair), 2561 odd (register-staged); an odd first stride leaves level 1 to the parity of
    n / 10; n / 1000 of 2521 and 2560 is a chunked level 3."""
    monkeypatch.delenv('GINSIM_ALLAN_FUSE', raising=False)
    n, S, where = key
    stride, off = ac.placement(n, where)
    _, lv = _plan(n, S, stride, 100.0, off)
    assert _modes(lv) == ac.DEEP[key]
    _levels_are_the_decades(n, stride, lv)


@pytest.mark.parametrize('key', sorted(ac.POWERS))
def test_number_of_levels_at_powers_of_ten(key, monkeypatch):
    monkeypatch.delenv('GINSIM_ALLAN_FUSE', raising=False)
    n, fs = key
    stride, _ = ac.placement(n, ALIGNED)
    ntau, lv = _plan(n, 4, stride, fs)
    assert (ntau, _modes(lv)) == ac.POWERS[key]
    _levels_are_the_decades(n, stride, lv)


@pytest.mark.parametrize('key', sorted(ac.NTAU))
def test_ntau_is_the_oracles(key):
    """ceil(log10(floor(n / 9))) levels: 9000 and 9008 give 27 factors, 9009 gives 28; 89 and 90 samples at 1 Hz nine each (the
    tenth factor needs a second level, which floor(n / 9) = 10 does not open)."""
    from oracle import ins_np
    n, fs = key
    ntau, lv = _plan(n, 1, n, fs)
    assert ntau == ac.NTAU[key] == ins_np.allan_var(np.zeros(n), fs)[1].size == len(allan_exact.factors(n, fs)[0])
    assert len(lv) == allan_exact.factors(n, fs)[1]


@pytest.mark.parametrize('key', sorted(ac.BATCH))
def test_chunks_per_workgroup_and_series_counts(key, monkeypatch):
    """The two regimes of the pair kernel: one round of 1024 workgroups with ceil(chunks / (1024 / S)) <= 16 chunks each (3 at 512
    series x 6 chunks, 4 at 1024 and at 1025 series x 4 chunks -- the latter through the S > 1024 branch), else total / 4096 capped
    at 8 (18 chunks x 1024 series -> 4)."""
    monkeypatch.setenv('GINSIM_ALLAN_FUSE', '0')
    S, n = key
    plan, cpb, parts = ac.BATCH[key]
    _, lv = _plan(n, S, n, ac.fs_of(n))
    assert _modes(lv) == plan and (lv[0]['chunks_per_block'], lv[0]['nparts']) == (cpb, parts)
    _levels_are_the_decades(n, n, lv)
    # the caps themselves: 16 chunks in one round, then 8
    assert _plan(2520 * 16, 1024, 2520 * 16, 100.0)[1][0]['chunks_per_block'] == 16
    assert _plan(2520 * 17, 1024, 2520 * 17 + 2, 100.0)[1][0]['chunks_per_block'] == 4          # 17 * 1024 / 4096
    assert _plan(2520 * 40, 1024, 2520 * 40, 100.0)[1][0]['chunks_per_block'] == 8              # 10, capped
    # the register-staged form serialises chunks in a wavefront only from 65 536 chunks on
    assert _plan(2521, 32767, 2523, 10.0)[1][0]['chunks_per_block'] == 1
    assert _plan(2521, 32768, 2523, 10.0)[1][0]['chunks_per_block'] == 2


@pytest.mark.parametrize('n', sorted(ac.NONFINITE))
def test_plans_of_the_nonfinite_cases(n, monkeypatch):
    monkeypatch.delenv('GINSIM_ALLAN_FUSE', raising=False)
    stride, _ = ac.placement(n, ALIGNED)
    _, lv = _plan(n, 7, stride, ac.fs_of(n))
    assert _modes(lv) == ac.NONFINITE[n]


def forced_plans(setting):
    """The plans of the forced register-staged cases from a fresh process (GINSIM_ALLAN_DMA / _CPW are read once per process)."""
    code = ('import json, sys; sys.path[:0] = %r; import ginsim, allan_cases as ac\n'
            'print(json.dumps({str(n): ginsim.allan_plan(1 << 20, n, ac.FORCED_S, ac.placement(n, ac.ALIGNED)[0], ac.fs_of(n))[1]'
            ' for n in ac.FORCED}))' % [p for p in sys.path if p])
    env = dict(os.environ)
    for k in ('GINSIM_ALLAN_DMA', 'GINSIM_ALLAN_CPW', 'GINSIM_ALLAN_FUSE'):
        env.pop(k, None)
    env.update(ac.FORCED_ENV[setting])
    out = subprocess.run([sys.executable, '-c', code], env=env, stdout=subprocess.PIPE, timeout=120, check=True, universal_newlines=True)
    return {int(k): v for k, v in json.loads(out.stdout.strip().splitlines()[-1]).items()}


@pytest.mark.parametrize('setting', sorted(ac.FORCED_ENV))
def test_forced_register_staged_plans(setting):
    """GINSIM_ALLAN_DMA=0 puts every chunked level on allan_level_kernel (and rules the fused form out), GINSIM_ALLAN_CPW=3 three
    chunks on a wavefront: 2 x 3 chunks per workgroup decide the records per series."""
    plans = forced_plans(setting)
    for n, (plan, parts3, parts0) in ac.FORCED.items():
        lv = plans[n]
        assert _modes(lv) == plan, n
        chunked = [l for l in lv if l['mode'] != T]
        assert all(l['mode'] == L and l['chunks_per_block'] == (3 if setting == 'cpw3' else 1) for l in chunked), n
        assert tuple(l['nparts'] for l in chunked) == (parts3 if setting == 'cpw3' else parts0), n


def test_more_series_than_the_grid_takes_are_planned_all_the_same():
    """The limit belongs to the device (ginsim_allan refuses, test_gpu_allan_edges.py); the host-only query has none."""
    _, lv = _plan(2521, 65536, 2522, 10.0)
    assert _modes(lv) == (L, T, T)
    _, lv = _plan(2520, 65536, 2520, 10.0)
    assert _modes(lv) == (T, T, T)
