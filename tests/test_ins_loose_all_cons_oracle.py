"""CPU: consistency checkpoints for every InsLoose family: the new header, its two entry points, their refusals and
dispatch, the build's resource reports of loose_all_cons_kernel, the job's keyword (checkpoints=, scale_truth=), the restatement
(tests/ins_loose_all_cons_ref.py) against the restatement of the 15-state record, against a direct evaluation of the scale columns
and against the recorded consistency ratios of the combined filter (ins_loose_all_cases.CONSISTENCY_RATIOS), which it reproduces
in ONE run with two checkpoints where the table took two truncated runs and their kept trajectories; and the cases
tests/test_gpu_ins_loose_all_cons_edges.py chooses (the tilted stops profile's checkpoints, a non-finite truth of the scale factor) on the
restatement alone."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import ins_loose_aided_cases as ac
import ins_loose_all_cases as ls
import ins_loose_all_cons_ref as acons
import ins_loose_all_ref as aref
import ins_loose_cases as cs
import ins_loose_cons_ref as cref
import ins_loose_mag_cases as mc
import ins_loose_ref as ref
import ins_loose_still_cases as sc
import test_ins_loose_all_oracle as allt
from conftest import REPO
from test_ins_loose_all_oracle import FakeContext, _drop, _set

NEW = {'ginsim_loose_all_cons_run', 'ginsim_loose_all_cons_kernel_name'}
N, RUNS = allt.N, allt.RUNS
SUBSETS = [w for k in range(4) for w in itertools.combinations(('mag', 'scale', 'still'), k)]


# ------------------------------------------------------------------------------------------------- C ABI
def test_the_header_declares_exactly_the_new_names_and_the_library_exports_them():
    import ginsim
    from ginsim import _lib
    hdr = open(os.path.join(REPO, 'include', 'ginsim_loose_all_cons.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert set(re.findall(r'\b(ginsim_[a-z0-9_]+)\s*\(', code)) == NEW
    assert set(ginsim.LOOSE_ALL_CONS_EXPORTS) == NEW and not NEW & set(ginsim.EXPORTS) and len(ginsim.EXPORTS) == 86
    assert set(ginsim.LOOSE_ALL_EXPORTS) == allt.NEW
    so = ctypes.CDLL(ginsim.LIB_PATH)
    assert all(hasattr(so, name) for name in NEW)
    assert ginsim.lib.ginsim_abi_version() == 9
    for other in ('ginsim.h', 'ginsim_loose_all.h'):
        text = open(os.path.join(REPO, 'include', other)).read()
        assert not any(name in text for name in NEW), other
    # the whole kernarg segment: two base blocks, two pointers, the three family blocks, the checkpoint arguments (a pointer, a
    # count, a pointer) and the truth pointer -- under HIP's 4 KB
    cons_args = 3 * 8
    assert ctypes.sizeof(_lib.McParams) + ctypes.sizeof(_lib.LooseParams) + 16 + ctypes.sizeof(_lib.LooseAllParams) + cons_args + 8 <= 4096
    assert _lib.CONS_RECORD == 43 == ginsim.ConsistencyResult.WIDTH == acons.RECORD


class Blocks(allt.Blocks):
    """The combined entry point's valid blocks and a valid checkpoint block (three checkpoints) next to them."""

    def __init__(self, given):
        from ginsim import _lib as L
        super().__init__(given)
        self.samples = np.array([0, 10, N - 1], dtype=np.int64)
        self.mc.ref_nav = self.d
        c = self.cons = L.LooseConsParams()
        c.cons_sample, c.cons_m, c.out_cons, c.cons_work = self.samples.ctypes.data, 3, self.d, self.d
        self.truth = None

    def _args(self):
        ref_ = lambda s: None if s is None else ctypes.byref(s)
        return tuple(ref_(s) for s in (self.mc, self.p, self.mag, self.scale, self.still, self.cons)) + (self.truth,)

    def name(self):
        from ginsim import _lib as L
        buf = ctypes.create_string_buffer(256)
        rc = L.lib.ginsim_loose_all_cons_kernel_name(*(self._args() + (buf, 256)))
        return [rc, (buf.value if rc == L.OK else L.lib.ginsim_last_error()).decode()]

    def all_name(self):
        return allt.Blocks.name(self)


def made(given, *fns):
    b = Blocks(given)
    for f in fns:
        f(b)
    return b


@pytest.mark.parametrize('name', list(allt.CASES))
def test_everything_the_combined_entry_point_refuses_is_refused_with_its_message(name):
    """Every case of tests/test_ins_loose_all_oracle.py with a valid checkpoint block next to it: a refusal is ginsim_loose_all_run's,
    code and text; a legal case names loose_all_cons_kernel, with 16 states where the scale block is held -- whatever number of
    blocks is left."""
    from ginsim import _lib as L
    form, fns = allt.CASES[name]
    b = made(form == 'given', *fns)
    rc, text = b.name()
    want_rc, want = b.all_name()
    if want_rc != L.OK:
        assert [rc, text] == [want_rc, want]
    else:
        ns = 16 if b.scale is not None else 15
        assert [rc, text] == [L.OK, 'ginsim::loose_all_cons_kernel<0, %s, false, %d>' % ('true' if form == 'given' else 'false', ns)], want


CONS = {
    'cons NULL': (_drop('cons'), 'loose_cons_run: NULL argument'),
    'cons_m=-1': (_set('cons.cons_m', -1), 'loose_cons_run: cons_m=-1 must be >= 0'),
    'cons_m>n': (_set('cons.cons_m', N + 1), 'loose_cons_run: cons_m=%d checkpoints for n=%d samples' % (N + 1, N)),
    'cons_sample NULL': (_set('cons.cons_sample', None), 'loose_cons_run: cons_sample, out_cons or cons_work missing'),
    'out_cons NULL': (_set('cons.out_cons', None), 'loose_cons_run: cons_sample, out_cons or cons_work missing'),
    'cons_work NULL': (_set('cons.cons_work', None), 'loose_cons_run: cons_sample, out_cons or cons_work missing'),
    'ref_nav NULL': (_set('mc.ref_nav', None), 'loose_cons_run: checkpoints need ref_nav'),
    'out_proc': (lambda b: setattr(b.p, 'out_proc', b.d),
                 'loose_cons_run: online process statistics (out_proc) and checkpoints in one launch are refused'),
    'sample=n': (lambda b: b.samples.__setitem__(2, N), 'loose_cons_run: checkpoint 2 (%d) is outside [0, %d)' % (N, N)),
    'sample=-1': (lambda b: b.samples.__setitem__(0, -1), 'loose_cons_run: checkpoint 0 (-1) is outside [0, %d)' % N),
    'repeated': (lambda b: b.samples.__setitem__(1, 0), 'loose_cons_run: the checkpoints are not strictly increasing at 1'),
    'descending': (lambda b: b.samples.__setitem__(2, 5), 'loose_cons_run: the checkpoints are not strictly increasing at 2'),
}
TRUTH = lambda b: setattr(b, 'truth', ctypes.c_void_p(b.d))
NO_SCALE_TRUTH = 'loose_all_cons_run: scale_truth without a scale block'


@pytest.mark.parametrize('what', list(CONS))
@pytest.mark.parametrize('given', [False, True], ids=['gen', 'given'])
def test_the_checkpoint_block_is_checked_as_its_own_entry_point_checks_it(what, given):
    from ginsim import _lib as L
    fn, message = CONS[what]
    assert made(given, fn).name() == [L.ERR_ARG, message]
    # the same block through ginsim_loose_cons_kernel_name: the same text
    b = made(given, fn)
    buf = ctypes.create_string_buffer(256)
    rc = L.lib.ginsim_loose_cons_kernel_name(ctypes.byref(b.mc), ctypes.byref(b.p), None if b.cons is None else ctypes.byref(b.cons), buf, 256)
    assert [rc, L.lib.ginsim_last_error().decode()] == [L.ERR_ARG, message]


def test_the_order_of_the_checks_and_the_truth_without_a_scale_block():
    from ginsim import _lib as L
    # a family block before the checkpoint block, the checkpoint block before the truth
    for first, text in ((_set('mag.mag_every', -1), 'loose_mag_run: '), (_set('scale.scale0', 0.0), 'loose_scale_run: '),
                        (_set('still.still_mask', 4), 'loose_still_run: '), (_set('mc.precision', 1), 'loose_run: the filter kernel is fp64 only'),
                        (_set('p.aid_mask', 6), 'loose_scale_run: aid_mask=6 has no bit 0')):
        rc, got = made(False, first, CONS['cons_m=-1'][0]).name()
        assert rc == L.ERR_ARG and got.startswith(text), got
    assert made(False, _drop('scale'), TRUTH, CONS['repeated'][0]).name() == [L.ERR_ARG, CONS['repeated'][1]]
    assert made(False, _drop('scale'), TRUTH).name() == [L.ERR_ARG, NO_SCALE_TRUTH]
    assert made(True, _drop('scale', 'mag', 'still'), TRUTH).name() == [L.ERR_ARG, NO_SCALE_TRUTH]
    assert made(False, _drop('scale'), TRUTH, _set('cons.cons_m', 0)).name() == [L.ERR_ARG, NO_SCALE_TRUTH]
    assert made(False, TRUTH).name() == [L.OK, 'ginsim::loose_all_cons_kernel<0, false, false, 16>']
    # cons_m == 0 is ginsim_loose_all_run: its kernel, whatever else the checkpoint block holds
    for drop in ((), ('mag',), ('mag', 'still'), ('mag', 'scale', 'still')):
        b = made(False, _drop(*drop), _set('cons.cons_m', 0), _set('cons.cons_sample', None), _set('mc.ref_nav', None))
        assert b.name() == b.all_name() and b.name()[0] == L.OK and '_cons_' not in b.name()[1], drop
    # the run entry point makes the same checks before it touches a device
    b = Blocks(False)
    assert L.lib.ginsim_loose_all_cons_run(None, *b._args()) == L.ERR_ARG
    assert L.lib.ginsim_last_error().decode().startswith('loose_all_cons_run: NULL argument')
    assert L.lib.ginsim_loose_all_cons_kernel_name(*(b._args() + (None, 0))) == L.ERR_ARG


@pytest.mark.parametrize('rf, source, scale', list(itertools.product((0, 1), ('gen', 'vib', 'given'), (False, True))))
def test_all_cons_dispatch(rf, source, scale):
    """The 12 names ginsim::loose_all_cons_kernel<RF, GIVEN, VIB, NS>, with every number of blocks left."""
    for drop in ((), ('mag',), ('still',), ('mag', 'still')):
        b = made(source == 'given', _drop(*(drop + (() if scale else ('scale',)))))
        b.mc.ref_frame = rf
        if source == 'vib':
            b.mc.vib_gyro.type = 1
        want = 'ginsim::loose_all_cons_kernel<%d, %s, %s, %d>' % (rf, allt.TF[source == 'given'], allt.TF[source == 'vib'], 16 if scale else 15)
        assert b.name() == [0, want]
    b = made(source == 'given', _drop('mag', 'scale', 'still'), _set('p.aid_mask', 0))
    b.mc.ref_frame = rf
    assert b.name()[1].endswith('15>') and 'loose_all_cons_kernel<%d' % rf in b.name()[1]


def test_build_reports_no_scratch_for_any_instantiation_of_the_checkpoint_kernel():
    """build/ins_loose_all_cons.resources.txt and build/ins_loose_all_cons16.resources.txt (written by build.py): the 12
    instantiations <RF, GIVEN, VIB, NS> of loose_all_cons_kernel by name, each with 0 bytes of scratch, at most 256 VGPRs, an
    occupancy of at least 1 and the static LDS bound of the sibling kernels."""
    from conftest import PKG
    kernels = {}
    for stem in ('ins_loose_all_cons', 'ins_loose_all_cons16'):
        path = os.path.join(PKG, 'build', stem + '.resources.txt')
        assert os.path.exists(path), 'run gnss-ins-sim_amd/build.py (it writes %s)' % path
        cur = None
        for line in open(path):
            k, _, v = line.strip().partition(':')
            if k == 'Function Name':
                cur = kernels.setdefault(v.strip(), {'file': stem})
            elif cur is not None and v.strip():
                cur[k.split('[')[0].strip()] = v.strip()
    found = {n: r for n, r in kernels.items() if '21loose_all_cons_kernelI' in n}
    seen = set(re.search(r'loose_all_cons_kernelILi(\d)ELb(\d)ELb(\d)ELi(\d+)E', n).groups() for n in found)
    want = set((rf, g, v, ns) for rf in '01' for g in '01' for v in '01' for ns in ('15', '16') if not (g == '1' and v == '1'))
    assert seen == want and len(found) == 12, seen ^ want
    for n, r in found.items():
        print(n, {k: r[k] for k in ('VGPRs', 'AGPRs', 'ScratchSize', 'Occupancy', 'LDS Size') if k in r})
        assert r['file'] == ('ins_loose_all_cons16' if 'Li16E' in n else 'ins_loose_all_cons'), n
        assert int(r['ScratchSize']) == 0, '%s: %s bytes of scratch per lane' % (n, r['ScratchSize'])
        assert int(r['Occupancy']) >= 1 and int(r['VGPRs']) <= 256, (n, r)
        assert int(r['LDS Size']) <= 8192 + 4 * 4, (n, r['LDS Size'])


# ------------------------------------------------------------------------------------------------- the job's surface
@pytest.fixture(scope='module')
def job_args():
    import ginsim
    ini, truth, _ = ls.stops_truth(20.0, 1, 2.0, 200)
    acc_e, gyr_e = cs.imu_errors()
    return lambda given=None, **kw: ginsim.InsLooseJob(FakeContext(), 20.0, 1, truth, acc_e, gyr_e, cs.GPS_ERR, ini, 4, given=given, **kw)


CONS_MESSAGES = {      # what cons_samples= says today of a job that holds these blocks
    (): None,
    ('mag',): r'^cons_samples: consistency checkpoints of the magnetometer-aided filter are not built \(mag=...\)$',
    ('scale',): r'^odo_scale_state: consistency checkpoints \(cons_samples=...\) of the filter with the scale-factor state are not built$',
    ('still',): r'^still: consistency checkpoints \(cons_samples=...\) of the filter with the standstill block are not built$',
    2: r'^combined: consistency checkpoints \(cons_samples=...\) of the combined family are not built$',
}


@pytest.mark.parametrize('held', SUBSETS, ids=['+'.join(w) or 'none' for w in SUBSETS])
def test_the_job_launches_the_checkpoint_family_with_any_subset_of_the_blocks(job_args, held):
    from ginsim.ins_loose import ALL_CONS, COMBINED, COMBINED_BLOCKS, FAMILIES
    assert [s for _, s in FAMILIES] == ['_cons', '_mag', '_scale', '_still'] and COMBINED == ('allp', '_all') and ALL_CONS == ('consp', '_all_cons')
    kw = ls.job_kw(ls.MASK, mc.MAG_ERR if 'mag' in held else None, 'scale' in held, 3 if 'still' in held else 0)
    if len(held) >= 2:
        kw['combined'] = True
    job = job_args(checkpoints=[10], **kw)
    assert job._family[0] == '_all_cons' and job.cons is None and job.consp is not None and job.consp.cons_m == 1
    assert job._family[1][:3] == tuple(getattr(job, a) for a in COMBINED_BLOCKS)
    assert [b is not None for b in job._family[1][:3]] == [k in held for k in ('mag', 'scale', 'still')]
    assert job.kernel_name() == 'ginsim::loose_all_cons_kernel<1, false, false, %d>' % (16 if 'scale' in held else 15)
    # the truth of the scale factor: what the lane makes its odometer with in the generated form
    assert ('scale_truth' in job._bufs) == ('scale' in held)
    # the argument rules of cons_samples: any order, repeats, mapped back
    many = job_args(checkpoints=[150, 3, 150, 0], **kw)
    assert list(many._cons_samples) == [0, 3, 150] and list(many._cons_back) == [2, 1, 2, 0] and many.consp.cons_m == 3
    for bad in ([], [200], [-1]):
        with pytest.raises(ValueError, match=r'^checkpoints must be sample indices in \[0, 200\), at least one$'):
            job_args(checkpoints=bad, **kw)
    # cons_samples keeps what it says today
    message = CONS_MESSAGES[2 if len(held) >= 2 else held]
    if message is None:
        assert job_args(cons_samples=[10], **kw).kernel_name() == 'ginsim::loose_cons_kernel<1, false, false, true>'
    else:
        with pytest.raises(ValueError, match=message):
            job_args(cons_samples=[10], **kw)
    if len(held) >= 2:                              # two blocks still need the opt-in
        with pytest.raises(ValueError, match=allt.PAIR_MESSAGES[held]):
            job_args(checkpoints=[10], **dict(kw, combined=False))


def test_the_new_refusals_of_the_keyword(job_args):
    kw = ls.job_kw(ls.MASK, None, True, 0)
    with pytest.raises(ValueError, match=r'^checkpoints: not together with cons_samples'):
        job_args(checkpoints=[10], cons_samples=[10])
    with pytest.raises(ValueError, match=r'^checkpoints: online process statistics \(proc_first\) and checkpoints in one launch are refused$'):
        job_args(checkpoints=[10], proc_first=0, **kw)
    with pytest.raises(ValueError, match=r'^checkpoints: scale_truth without the scale-factor state'):
        job_args(checkpoints=[10], scale_truth=1.0, **ls.job_kw(ls.MASK, None, False, 3))
    for bad in (np.ones(5), np.ones((4, 1)), np.ones(3)):
        with pytest.raises(ValueError, match=r'^checkpoints: scale_truth must be a scalar or \(runs,\) = \(4,\)'):
            job_args(checkpoints=[10], scale_truth=bad, **kw)
    for good in (0.99, np.full(4, 0.99), [1.0, 0.99, 0.98, 1.01]):
        assert 'scale_truth' in job_args(checkpoints=[10], scale_truth=good, **kw)._bufs
    # the given form has no truth of its own
    given = {k: allt.FakeBuffer(1 << 20) for k in ('accel', 'gyro', 'gps', 'odo')}
    job = job_args(given=given, checkpoints=[10], **kw)
    assert 'scale_truth' not in job._bufs and job._family[1][-1] is None
    assert job.kernel_name() == 'ginsim::loose_all_cons_kernel<1, true, false, 16>'
    assert 'scale_truth' in job_args(given=given, checkpoints=[10], scale_truth=0.985, **kw)._bufs
    # without the keyword nothing of the job changes
    plain = job_args(**kw)
    assert plain.consp is None and plain.cons is None and plain._family[0] == '_scale'
    with pytest.raises(ValueError, match='was not requested'):
        plain.consistency()


def test_the_result_carries_the_scale_columns_through_pack_unpack_merge_and_allgather():
    import ginsim
    from ginsim import distributed
    rng = np.random.default_rng(2)
    a, b = rng.random((5, 43)) + 1.0, rng.random((5, 43)) + 1.0
    a[:, 0], b[:, 0] = 7.0, 9.0
    r = ginsim.ConsistencyResult(a)
    assert r.pbar.shape == (5, 15) and r.e2.shape == r.nes.shape == r.ratio.shape == (5, 9) and r.nees.shape == (5, 3)
    for name in ('pbar_scale', 'e2_scale', 'nes_scale', 'sigma_scale', 'rms_scale', 'ratio_scale'):
        assert getattr(r, name).shape == (5,), name
    assert np.array_equal(r.pbar_scale, a[:, 37] / 7) and np.array_equal(r.e2_scale, a[:, 38] / 7) and np.array_equal(r.nes_scale, a[:, 39] / 7)
    assert np.array_equal(r.ratio_scale, np.sqrt(a[:, 38] / 7) / np.sqrt(a[:, 37] / 7))
    assert np.array_equal(ginsim.ConsistencyResult.unpack(r.pack()).records, a)
    m = ginsim.ConsistencyResult.merge([a, b])
    assert np.array_equal(m.records, a + b) and np.array_equal(m.e2_scale, (a + b)[:, 38] / 16)
    assert np.array_equal(distributed.allgather_consistency(r).records, a)        # not distributed: the identity, 43 columns wide
    z = ginsim.ConsistencyResult.zero(3)
    assert z.records.shape == (3, 43) and np.all(np.isnan(z.ratio_scale))


def test_the_sim_has_a_method_of_its_own_for_every_family_and_consistency_curve_keeps_its_signature():
    import inspect
    from gnss_ins_sim.sim import ins_sim
    old, new = inspect.signature(ins_sim.Sim.consistency_curve), inspect.signature(ins_sim.Sim.consistency_curve_any_family)
    assert list(old.parameters)[1:] == list(new.parameters)[1:] == ['every', 'samples']
    assert [p.kind for p in new.parameters.values()][1:] == [inspect.Parameter.KEYWORD_ONLY] * 2
    assert "'scale'" in ins_sim.Sim.consistency_curve_any_family.__doc__
    assert list(inspect.signature(ins_sim._McResults.consistency).parameters)[1:] == ['name', 'samples', 'any_family']


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.fixture(scope='module', params=[1, 0], ids=['rf1', 'rf0'])
def small(request):
    """5 runs of the stops profile's first 25 s at 20 Hz, every sensor drawn from the model; the true scale of every run drawn."""
    from ginsim.ins_loose import filter_model
    rf, fs, n, R = request.param, 20.0, 500, 5
    ini, truth, stamps = ls.stops_truth(fs, rf, 2.0, n)
    acc_e, gyr_e = cs.imu_errors()
    rng = np.random.default_rng(5)
    accel, gyro, _, _ = ref.sample_sensors(rng, fs, truth['ref_accel'], truth['ref_gyro'], acc_e, gyr_e, R)
    gps = cs.sample_gps(rng, truth, rf, R)
    scales = 1.0 + 0.02 * rng.standard_normal(R)
    odo = scales[:, None] * np.asarray(truth['ref_odo'])[None] + ls.ODO_ERR['stdv'] * rng.standard_normal((R, n))
    mag = ref.sample_mag(rng, truth['ref_mag'], mc.MAG_ERR_SKEW, R)
    model = filter_model(fs, acc_e, gyr_e, cs.GPS_ERR)
    flags = sc.flags_of(truth)
    nav = np.concatenate([truth['ref_att'], truth['ref_pos'], truth['ref_vel']], axis=1)
    return {'rf': rf, 'fs': fs, 'n': n, 'model': model, 'flags': flags, 'odo': odo, 'mag': mag, 'scales': scales, 'nav': nav,
            'head': (rf, fs, gyro, accel, ini, model), 'tail': (gps, stamps, truth['gps_visibility'])}


SAMPLES = [0, 1, 200, 499, 260, 200]


@pytest.mark.parametrize('mask', [0, 7])
def test_without_a_block_the_record_is_the_15_state_restatement_s(small, mask):
    aid = ac.aid(mask, 3) if mask else None
    got = acons.run(*small['head'], small['nav'], SAMPLES, *small['tail'], odo=small['odo'], aid=aid)
    want = cref.run(*small['head'], small['nav'], SAMPLES, *small['tail'], odo=small['odo'], aid=aid)
    assert got.shape == (6, 43) and np.array_equal(got, want) and not got[:, 37:].any() and np.all(got[:, 0] == 5)
    assert np.array_equal(got[2], got[5])


@pytest.mark.parametrize('which', [('scale',), ('mag', 'scale', 'still')], ids=['scale', 'all'])
@pytest.mark.parametrize('dtype', [np.float64, np.longdouble], ids=['f64', 'long'])
def test_the_scale_columns_against_a_direct_evaluation(small, which, dtype):
    """Columns 37-39 from the series ins_loose_all_ref.run keeps (k_est and the 16-entry diagonal of P at every stored row); columns
    1-15 from the same diagonal; without a truth 38 and 39 are 0 and the others do not move."""
    kw = ls.blocks(small['model'], small['fs'], small['rf'], ls.MASK, mc.MAG_ERR_SKEW if 'mag' in which else None, True,
                   3 if 'still' in which else 0, flags=small['flags'])
    kw.update(odo=small['odo'], mag=small['mag'] if 'mag' in which else None)
    rec = acons.run(*small['head'], small['nav'], SAMPLES, *small['tail'], dtype=dtype, scale_truth=small['scales'], **kw)
    o = aref.run(*small['head'], *small['tail'], dtype=dtype, keep_pdiag=True, **kw)
    assert rec.dtype == dtype and np.all(rec[:, 0] == 5) and not rec[:, 40:].any()
    for row, j in zip(rec, SAMPLES):
        ek = o['k_est'][:, j] - small['scales'].astype(dtype)
        assert np.array_equal(row[1:16], o['pdiag'][:, j, :15].sum(axis=0))
        assert row[37] == o['pdiag'][:, j, 15].sum() and row[38] == (ek * ek).sum() and row[39] == (ek * ek / o['pdiag'][:, j, 15]).sum()
    assert rec[0, 38] > 0 and rec[3, 37] < 0.5 * rec[0, 37]                     # the state is learnt while GPS is visible
    blind = acons.run(*small['head'], small['nav'], SAMPLES, *small['tail'], dtype=dtype, **kw)
    assert not blind[:, 38:].any() and np.array_equal(blind[:, :38], rec[:, :38])
    one = acons.run(*small['head'], small['nav'], SAMPLES, *small['tail'], dtype=dtype, scale_truth=0.99, **kw)
    assert np.array_equal(one[:, :38], rec[:, :38]) and not np.array_equal(one[:, 38], rec[:, 38])
    m = acons.means(rec)
    assert m['ratio_scale'].shape == (6,) and np.allclose(np.asarray(m['ratio_scale'], dtype=np.float64),
                                                          np.sqrt(np.asarray(rec[:, 38] / rec[:, 37], dtype=np.float64)))


def test_a_run_with_a_bad_scale_variance_or_a_non_finite_scale_error_is_left_out(small):
    import ins_loose_scale_ref as sref
    scale = {'scale0': 1.0, 'p0_scale': 0.02, 'q_k': 0.0}
    f = sref.ScaleFilter(small['rf'], small['fs'], small['head'][4], 5, small['model'], scale)
    t = small['nav'][0]
    truth = np.array([1.0, 0.99, 1.01, 1.0, 0.98])
    whole = acons.record(f, t, truth)
    assert whole[0] == 5 and whole[37] == 5 * 0.02 * 0.02 and np.isclose(whole[38], np.sum((1.0 - truth) ** 2))
    f.pkk[1] = 0.0                                      # P[15][15] = 0: out, with or without a truth
    assert acons.record(f, t, truth)[0] == 4 and acons.record(f, t)[0] == 4
    f.pkk[1], f.k_est[3] = 4e-4, np.inf                 # a non-finite estimate: out with a truth only
    with np.errstate(all='ignore'):
        got = acons.record(f, t, truth)
    assert got[0] == 4 and np.isclose(got[38], np.sum((1.0 - truth[[0, 1, 2, 4]]) ** 2)) and acons.record(f, t)[0] == 5


def test_one_run_with_two_checkpoints_reproduces_the_recorded_ratios_of_the_combined_filter():
    """ins_loose_all_cases.consistency_draw, 1024 runs, every block on the 16-state filter: ONE run with checkpoints at the last
    sample of the first stop and at the profile's end gives CONSISTENCY_RATIOS of the nine navigation states and, as ratio_scale,
    entry 15 of the table, at both tags, to the 2e-3 tests/test_ins_loose_all_oracle.py holds the table to."""
    c = ls.consistency_draw(1, cs.CONSISTENCY_FS, cs.CONSISTENCY_RUNS)
    n = c['truth']['ref_accel'].shape[0]
    at = {'stop': sc.windows(c['flags'])[0][1], 'end': n - 1}
    kw = ls.blocks(c['model'], c['fs'], c['rf'], ls.CONSISTENCY_MASK, mc.MAG_ERR, True, 3, flags=c['flags'])
    t = c['truth']
    nav = np.concatenate([t['ref_att'], t['ref_pos'], t['ref_vel']], axis=1)
    rec = acons.run(c['rf'], c['fs'], c['gyro'], c['accel'], c['ini'], c['model'], nav, [at['stop'], at['end']], c['gps'], c['stamps'],
                    t['gps_visibility'], odo=c['odo'], mag=c['mag'], scale_truth=c['scales'], **kw)
    assert np.all(rec[:, 0] == 1024)
    m = acons.means(rec)
    for k, tag in enumerate(('stop', 'end')):
        print('%s: ratios' % tag, np.array2string(m['ratio'][k], precision=3, separator=', '), 'scale %.3f' % m['ratio_scale'][k],
              'nees', np.array2string(m['nees'][k], precision=3, separator=', '))
    for k, tag in enumerate(('stop', 'end')):
        np.testing.assert_allclose(m['ratio'][k], ls.CONSISTENCY_RATIOS[tag][:9], rtol=0, atol=2e-3)
        np.testing.assert_allclose(m['ratio_scale'][k], ls.CONSISTENCY_RATIOS[tag][15], rtol=0, atol=2e-3)


# ------------------------------------------------------------------------------------------------- the cases of the edges file
def host_draw(rf, n, R, profile, geo, seed):
    """R runs of a stops profile at 20 Hz, every sensor drawn on the host from the model (as `small`); the odometer reads ls.READS."""
    from ginsim.ins_loose import filter_model
    ini, truth, stamps = ls.stops_truth(20.0, rf, 2.0, n, profile, geo)
    n = truth['ref_accel'].shape[0]
    acc_e, gyr_e = cs.imu_errors()
    rng = np.random.default_rng(seed)
    accel, gyro, _, _ = ref.sample_sensors(rng, 20.0, truth['ref_accel'], truth['ref_gyro'], acc_e, gyr_e, R)
    gps = cs.sample_gps(rng, truth, rf, R)
    odo = ls.READS * np.asarray(truth['ref_odo'])[None] + ls.ODO_ERR['stdv'] * rng.standard_normal((R, n))
    mag = ref.sample_mag(rng, truth['ref_mag'], mc.MAG_ERR_SKEW, R)
    model = filter_model(20.0, acc_e, gyr_e, cs.GPS_ERR)
    nav = np.concatenate([truth['ref_att'], truth['ref_pos'], truth['ref_vel']], axis=1)
    return {'rf': rf, 'n': n, 'ini': ini, 'truth': truth, 'stamps': stamps, 'model': model, 'flags': sc.flags_of(truth), 'odo': odo, 'mag': mag,
            'nav': nav, 'head': (rf, 20.0, gyro, accel, ini, model), 'tail': (gps, stamps, truth['gps_visibility'])}


@pytest.mark.parametrize('rf', [0, 1])
def test_the_checkpoints_of_the_tilted_stops_profile_exist_and_exclude_no_run(rf):
    """What tests/test_gpu_ins_loose_all_cons_edges.py chooses on the tilted stops profile (41 S, parked on a slope, yaw through +-180
    deg), without a GPU: ls.edge_checkpoints asserts the profile's preconditions and that every named sample exists; here each of them
    is shown again from the truth, and the float64 restatement alone, on 8 host-drawn runs with every block at ls.SCHEDULE's periods,
    includes all 8 at every one of them -- a count below the run count on the device is then the device's."""
    ini, truth, stamps = ls.stops_truth(20.0, rf, 2.0, None, sc.TILTED_STOPS_CSV, mc.GEO_SOUTH)
    n = truth['ref_accel'].shape[0]
    flags = sc.flags_of(truth)
    samples = ls.edge_checkpoints(ini, truth, stamps, flags)
    print('tilted stops rf%d: n %d, checkpoints %s, standstill windows %s' % (rf, n, samples, sc.windows(flags)))
    assert n == 960 and ini[0] < 0 and np.degrees(np.max(np.abs(truth['ref_att'][:, 1]))) >= 10.0
    assert len(sc.windows(flags)) == 2 and samples[:2] == [0, 1] and samples[-2:] == [n - 2, n - 1]
    fires = ls.schedule(n, ls.SCHEDULE, stamps, truth['gps_visibility'], flags)
    yaw = truth['ref_att'][:, 0]
    assert any(fires[j] == ls.FIX | ls.AID | ls.MAG | ls.STILL for j in samples)
    assert any(fires[j] & ls.STILL and not fires[j] & ls.FIX and sc.windows(flags)[1][0] <= j <= sc.windows(flags)[1][1] for j in samples)
    assert any(abs(yaw[j] - yaw[j - 1]) > np.pi for j in samples[1:])
    assert sc.windows(flags)[0][1] in samples and flags[sc.windows(flags)[0][1] + 1] == 0
    c = host_draw(rf, None, 8, sc.TILTED_STOPS_CSV, mc.GEO_SOUTH, 7)
    kw = ls.blocks(c['model'], 20.0, rf, ls.MASK, mc.MAG_ERR_SKEW, True, 3, every=ls.SCHEDULE, geo=mc.GEO_SOUTH, flags=flags)
    rec = acons.run(*c['head'], c['nav'], samples, *c['tail'], odo=c['odo'], mag=c['mag'], scale_truth=ls.READS, **kw)
    assert rec.shape == (8, 43) and np.all(rec[:, 0] == 8) and np.all(np.isfinite(rec)) and np.all(rec[2:, 38] > 0)


def test_a_non_finite_truth_of_the_scale_factor_excludes_exactly_its_two_runs():
    """ls.bad_scale_truth (NaN in run 7, +inf in run 40) on 65 host-drawn runs of the level stops profile: the restatement alone counts
    63 at every checkpoint of the device test's list, and its sums are those over the other 63 runs."""
    samples = [50, 100, 101, 200, 299]
    c = host_draw(1, 300, 65, sc.STOPS_CSV, mc.GEO, 8)
    kw = ls.blocks(c['model'], 20.0, 1, ls.MASK, mc.MAG_ERR_SKEW, True, 3, every=2, flags=c['flags'])
    truth = ls.bad_scale_truth(65)
    assert np.count_nonzero(~np.isfinite(truth)) == 2
    rec = acons.run(*c['head'], c['nav'], samples, *c['tail'], odo=c['odo'], mag=c['mag'], scale_truth=truth, **kw)
    assert np.all(rec[:, 0] == 63) and np.all(np.isfinite(rec))
    keep = np.setdiff1d(np.arange(65), [7, 40])
    head = c['head'][:2] + (c['head'][2][keep], c['head'][3][keep]) + c['head'][4:]
    part = acons.run(*head, c['nav'], samples, c['tail'][0][keep], *c['tail'][1:], odo=c['odo'][keep], mag=c['mag'][keep],
                     scale_truth=truth[keep], **kw)
    assert np.array_equal(part[:, 0], rec[:, 0]) and np.allclose(part, rec, rtol=1e-12, atol=0)
    clean = acons.run(*c['head'], c['nav'], samples, *c['tail'], odo=c['odo'], mag=c['mag'], scale_truth=ls.READS, **kw)
    assert np.all(clean[:, 0] == 65)
