"""CPU: InsLoose with all its aids in one launch: the new header, its two entry points, their refusals and dispatch, the
build's resource reports of loose_all_kernel, the job's and the plugin's opt-in (combined=True), the restatement
(tests/ins_loose_all_ref.py) against the restatements it composes, against what information can only do to P and against the
statistics of its own covariance.

Recorded in ins_loose_all_cases (measured by test_restatement_consistency; 1024 runs drawn from the filter's own model, the stops
profile at 20 Hz with 2 Hz GPS, 'mid-accuracy' IMU, ref_frame 1, the true scale of every run drawn from N(1, 0.02^2)):
CONSISTENCY_RATIOS of the 16 states at the last sample of the first stop and at the profile's end."""
import ctypes
import itertools
import json
import os
import re

import numpy as np
import pytest

import ins_loose_all_cases as ls
import ins_loose_all_ref as aref
import ins_loose_cases as cs
import ins_loose_mag_cases as mc
import ins_loose_ref as ref
import ins_loose_scale_cases as kc
import ins_loose_scale_ref as sref
import ins_loose_still_cases as sc
from conftest import GOLDEN, REPO

NEW = {'ginsim_loose_all_run', 'ginsim_loose_all_kernel_name'}
FIXTURE = os.path.join(GOLDEN, 'api_refusals_all.json')
NAN = float('nan')
N, RUNS = 30, 4
TF = {False: 'false', True: 'true'}


# ------------------------------------------------------------------------------------------------- C ABI
def test_the_header_declares_exactly_the_new_names_and_the_library_exports_them():
    import ginsim
    from ginsim import _lib
    hdr = open(os.path.join(REPO, 'include', 'ginsim_loose_all.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert set(re.findall(r'\b(ginsim_[a-z0-9_]+)\s*\(', code)) == NEW
    assert set(ginsim.LOOSE_ALL_EXPORTS) == NEW and not NEW & set(ginsim.EXPORTS) and len(ginsim.EXPORTS) == 86
    so = ctypes.CDLL(ginsim.LIB_PATH)
    assert all(hasattr(so, name) for name in NEW)
    assert ginsim.lib.ginsim_abi_version() == 9
    main = open(os.path.join(REPO, 'include', 'ginsim.h')).read()
    assert not any(name in main for name in NEW) and 'ginsim_loose_all_params' not in main
    # the by-value block: the three family blocks one after the other, no padding
    body = re.search(r'typedef struct \{(.*?)\}\s*ginsim_loose_all_params\s*;', code, re.S).group(1)
    assert re.findall(r'(ginsim_loose_\w+_params)\s+(\w+)\s*;', body) == [('ginsim_loose_mag_params', 'mag'), ('ginsim_loose_scale_params', 'scale'),
                                                                          ('ginsim_loose_still_params', 'still')]
    A = _lib.LooseAllParams
    sizes = [ctypes.sizeof(t) for t in (_lib.LooseMagParams, _lib.LooseScaleParams, _lib.LooseStillParams)]
    assert [A.mag.offset, A.scale.offset, A.still.offset] == [0, sizes[0], sizes[0] + sizes[1]] and ctypes.sizeof(A) == sum(sizes) == 392
    # the whole kernarg segment: two base blocks, two pointers, the block -- under HIP's 4 KB
    assert ctypes.sizeof(_lib.McParams) + ctypes.sizeof(_lib.LooseParams) + 16 + ctypes.sizeof(A) <= 4096


class Blocks(object):
    """The valid parameter blocks of the combined entry point: mc, p (odometer and constraints on), mag, scale, still."""

    def __init__(self, given):
        from ginsim import _lib as L
        self.dummy = np.zeros(64)
        self.stamps = np.array([0, 10, 20], dtype=np.int64)
        d = self.d = self.dummy.ctypes.data
        m = self.mc = L.McParams()
        m.n, m.runs, m.fs, m.n_ini, m.ini = N, RUNS, 100.0, 1, d
        if given:
            m.given_sensors, m.in_accel, m.in_gyro, m.in_odo = 1, d, d, d
        else:
            m.ref_accel, m.ref_gyro, m.ref_odo = d, d, d
        p = self.p = L.LooseParams()
        p.m, p.gps_stamp, p.n_list = 3, self.stamps.ctypes.data, RUNS
        p.in_gps, p.ref_gps = (d, None) if given else (None, d)
        p.r_diag[:], p.p0[:] = [1.0] * 6, [1.0] * 5
        p.decay_g[:], p.decay_a[:] = [1.0] * 3, [1.0] * 3
        p.aid_mask, p.aid_every, p.r_odo, p.odo_scale_f, p.r_nhc = 7, 1, 0.01, 1.0, 0.0025
        g = self.mag = L.LooseMagParams()
        g.mag_every = 1
        g.in_mag, g.ref_mag = (d, None) if given else (None, d)
        g.mag_si[:], g.cal_si[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1], [1, 0, 0, 0, 1, 0, 0, 0, 1]
        g.mag_n[:], g.r_mag[:] = [30.0, -3.0, 40.0], [1e-4] * 3
        s = self.scale = L.LooseScaleParams()
        s.scale0, s.p0_scale = 1.0, 0.02
        q = self.still = L.LooseStillParams()
        q.still_mask, q.still_every, q.still_flags, q.r_zupt = 3, 1, d, 4e-4
        q.r_zaru[:] = [1e-8] * 3

    def name(self):
        """(return code, kernel name or the refusal's message)"""
        from ginsim import _lib as L
        buf = ctypes.create_string_buffer(256)
        ref_ = lambda s: None if s is None else ctypes.byref(s)
        rc = L.lib.ginsim_loose_all_kernel_name(ref_(self.mc), ref_(self.p), ref_(self.mag), ref_(self.scale), ref_(self.still), buf, 256)
        return [rc, (buf.value if rc == L.OK else L.lib.ginsim_last_error()).decode()]


def _set(path, value, index=None):
    def apply(b):
        obj, names = b, path.split('.')
        for k in names[:-1]:
            obj = getattr(obj, k)
        if index is None:
            setattr(obj, names[-1], value)
        else:
            getattr(obj, names[-1])[index] = value
    return apply


def _all(*fns):
    def apply(b):
        for f in fns:
            f(b)
    return apply


def _drop(*attrs):
    def apply(b):
        for a in attrs:
            setattr(b, a, None)
    return apply


SINGLE = {
    'gen': {
        # absent and degenerate blocks: fewer than two left is the single family's launch, or the aided one
        'mag NULL is legal': _drop('mag'), 'scale NULL is legal': _drop('scale'), 'still NULL is legal': _drop('still'),
        'mag alone is legal: the mag launch': _drop('scale', 'still'), 'scale alone is legal: the scale launch': _drop('mag', 'still'),
        'still alone is legal: the still launch': _drop('mag', 'scale'), 'no block is legal: the aided launch': _drop('mag', 'scale', 'still'),
        'no block and aid_mask=0 is legal: the plain launch': _all(_drop('mag', 'scale', 'still'), _set('p.aid_mask', 0)),
        'mag_every=0 is legal: scale + still': _set('mag.mag_every', 0),
        'mag_every=0 is legal and reads nothing else': _all(_set('mag.mag_every', 0), _set('mag.ref_mag', None), _set('mag.r_mag', NAN, 1)),
        'still_mask=0 is legal: scale + mag': _set('still.still_mask', 0),
        'still_mask=0 is legal and reads nothing else': _all(_set('still.still_mask', 0), _set('still.still_flags', None), _set('still.r_zupt', NAN)),
        'both degenerate is legal: the scale launch': _all(_set('mag.mag_every', 0), _set('still.still_mask', 0)),
        'degenerate mag, no scale is legal: the still launch': _all(_set('mag.mag_every', 0), _drop('scale')),
        'mag_every=2^40 is legal': _set('mag.mag_every', 2 ** 40), 'still_every=2^40 is legal': _set('still.still_every', 2 ** 40),
        # each block as its own family checks it
        'mag_every=-1': _set('mag.mag_every', -1), 'ref_mag NULL': _set('mag.ref_mag', None), 'r_mag=0': _set('mag.r_mag', 0.0, 2),
        'mag_n zero': _all(_set('mag.mag_n', 0.0, 0), _set('mag.mag_n', 0.0, 1), _set('mag.mag_n', 0.0, 2)), 'cal_si nan': _set('mag.cal_si', NAN, 4),
        'aid_mask=6 with scale': _set('p.aid_mask', 6), 'aid_mask=6 without scale is legal': _all(_set('p.aid_mask', 6), _drop('scale')),
        'scale0=0': _set('scale.scale0', 0.0), 'p0_scale<0': _set('scale.p0_scale', -1.0), 'q_k nan': _set('scale.q_k', NAN),
        'still_mask=4': _set('still.still_mask', 4), 'still_every=0': _set('still.still_every', 0), 'r_zupt nan': _set('still.r_zupt', NAN),
        'r_zaru<0': _set('still.r_zaru', -1e-300, 2), 'still_flags NULL': _set('still.still_flags', None),
        # the filter's own blocks
        'runs=0': _set('mc.runs', 0), 'ref_gps NULL': _set('p.ref_gps', None), 'vib_accel psd': _set('mc.vib_accel.type', 3), 'aid_mask=8': _set('p.aid_mask', 8),
        'precision=1': _set('mc.precision', 1), 'mc NULL': _drop('mc'), 'p NULL': _drop('p'),
    },
    'given': {'in_mag NULL': _set('mag.in_mag', None), 'in_gps NULL': _set('p.in_gps', None), 'in_odo NULL': _set('mc.in_odo', None),
              'still_flags NULL': _set('still.still_flags', None), 'ref_mag NULL is legal': _set('mag.ref_mag', None)},
}
# two violations at once: the message is that of the check that comes first
PAIRS = [
    # the filter's block before every family block
    ('gen', 'aid_mask=8', 'mag_every=-1'), ('gen', 'runs=0', 'scale0=0'), ('gen', 'precision=1', 'still_mask=4'), ('given', 'in_gps NULL', 'in_mag NULL'),
    # mag before scale before still
    ('gen', 'r_mag=0', 'scale0=0'), ('gen', 'ref_mag NULL', 'still_flags NULL'), ('gen', 'p0_scale<0', 'still_every=0'),
    ('gen', 'aid_mask=6 with scale', 'r_zupt nan'), ('given', 'in_mag NULL', 'still_flags NULL'),
]


def _cases():
    out = {}
    for form, table in SINGLE.items():
        out['all %s: valid' % form] = (form, [])
        for what, fn in table.items():
            out['all %s: %s' % (form, what)] = (form, [fn])
    for form, a, b in PAIRS:
        out['all %s: %s + %s' % (form, a, b)] = (form, [SINGLE[form][a], SINGLE[form][b]])
    return out


CASES = _cases()


def outcome(name):
    form, fns = CASES[name]
    b = Blocks(form == 'given')
    for f in fns:
        f(b)
    return b.name()


def test_fixture_lists_every_case():
    """GINSIM_RECORD_REFUSALS=1: write the fixture (at the commit that adds the family, once); otherwise only check it is complete."""
    if os.environ.get('GINSIM_RECORD_REFUSALS') == '1':
        with open(FIXTURE, 'w') as f:
            f.write('{\n' + ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(outcome(k))) for k in CASES) + '\n}\n')
    with open(FIXTURE) as f:
        assert sorted(json.load(f)) == sorted(CASES)


@pytest.fixture(scope='module')
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize('name', list(CASES))
def test_refusal_is_the_recorded_one(name, recorded):
    assert outcome(name) == recorded[name]


def test_every_refusal_is_an_argument_error_in_the_order_filter_mag_scale_still(recorded):
    from ginsim import _lib as L
    prefixes = ('loose_run', 'loose_mag_run', 'loose_scale_run', 'loose_still_run')
    refused = 0
    for name, (rc, text) in recorded.items():
        if name.endswith('valid') or 'legal' in name:
            assert rc == L.OK and text.startswith('ginsim::'), name
        else:
            assert rc == L.ERR_ARG and text.split(':')[0] in prefixes, (name, text)
            refused += 1
    assert refused >= 25
    for form, a, b in PAIRS:
        assert recorded['all %s: %s + %s' % (form, a, b)] == recorded['all %s: %s' % (form, a)], (a, b)
    for form, a, _ in PAIRS[:4]:
        assert recorded['all %s: %s' % (form, a)][1].startswith('loose_run: '), a
    assert recorded['all gen: precision=1'][1] == 'loose_run: the filter kernel is fp64 only'
    assert 'without the odometer is refused' in recorded['all gen: aid_mask=6 with scale'][1]
    want = {'valid': 'loose_all_kernel<0, false, false, false, 16>', 'mag NULL is legal': 'loose_all_kernel<0, false, false, false, 16>',
            'scale NULL is legal': 'loose_all_kernel<0, false, false, false, 15>', 'still NULL is legal': 'loose_all_kernel<0, false, false, false, 16>',
            'mag alone is legal: the mag launch': 'loose_mag_kernel<0, false, false, false>',
            'scale alone is legal: the scale launch': 'loose_scale_kernel<0, false, false, false>',
            'still alone is legal: the still launch': 'loose_still_kernel<0, false, false, false>',
            'no block is legal: the aided launch': 'loose_aided_kernel<0, false, false, false>',
            'no block and aid_mask=0 is legal: the plain launch': 'loose_kernel<0, false, false, false>',
            'mag_every=0 is legal: scale + still': 'loose_all_kernel<0, false, false, false, 16>',
            'mag_every=0 is legal and reads nothing else': 'loose_all_kernel<0, false, false, false, 16>',
            'still_mask=0 is legal: scale + mag': 'loose_all_kernel<0, false, false, false, 16>',
            'both degenerate is legal: the scale launch': 'loose_scale_kernel<0, false, false, false>',
            'degenerate mag, no scale is legal: the still launch': 'loose_still_kernel<0, false, false, false>',
            'aid_mask=6 without scale is legal': 'loose_all_kernel<0, false, false, false, 15>'}
    for what, kernel in want.items():
        assert recorded['all gen: ' + what][1] == 'ginsim::' + kernel, what
    assert recorded['all given: valid'][1] == 'ginsim::loose_all_kernel<0, true, false, false, 16>'
    # the run entry point makes the same checks before it touches a device
    b = Blocks(False)
    run = lambda: L.lib.ginsim_loose_all_run(None, ctypes.byref(b.mc), ctypes.byref(b.p), ctypes.byref(b.mag), ctypes.byref(b.scale), ctypes.byref(b.still))
    assert run() == L.ERR_ARG and L.lib.ginsim_last_error().decode().startswith('loose_all_run: NULL argument')
    assert L.lib.ginsim_loose_all_kernel_name(ctypes.byref(b.mc), ctypes.byref(b.p), None, None, None, None, 0) == L.ERR_ARG


@pytest.mark.parametrize('rf, source, flag, scale', list(itertools.product((0, 1), ('gen', 'vib', 'given'), (False, True), (False, True))))
def test_all_dispatch(rf, source, flag, scale):
    """The 24 names ginsim::loose_all_kernel<RF, GIVEN, VIB, PS, NS>; with one block left the name is the single family's, the one its
    own entry point reports."""
    from ginsim import _lib as L
    b = Blocks(source == 'given')
    b.mc.ref_frame = rf
    if source == 'vib':
        b.mc.vib_gyro.type = 1
    if flag:
        b.p.out_proc, b.mc.ref_nav = b.d, b.d
    if not scale:
        b.scale = None
    args = (rf, TF[source == 'given'], TF[source == 'vib'], TF[flag])
    assert b.name() == [0, 'ginsim::loose_all_kernel<%d, %s, %s, %s, %d>' % (args + (16 if scale else 15,))]
    buf = ctypes.create_string_buffer(256)
    for keep, fn in (('mag', L.lib.ginsim_loose_mag_kernel_name), ('still', L.lib.ginsim_loose_still_kernel_name)):
        one = Blocks(source == 'given')
        one.mc, one.p = b.mc, b.p
        for other in {'mag', 'scale', 'still'} - {keep}:
            setattr(one, other, None)
        assert fn(ctypes.byref(b.mc), ctypes.byref(b.p), ctypes.byref(getattr(one, keep)), buf, 256) == 0
        assert one.name() == [0, buf.value.decode()] == [0, 'ginsim::loose_%s_kernel<%d, %s, %s, %s>' % ((keep,) + args)]


def test_build_reports_no_scratch_for_any_instantiation_of_the_combined_kernel():
    """build/ins_loose_all.resources.txt and build/ins_loose_all16.resources.txt (written by build.py): the 24 instantiations
    <RF, GIVEN, VIB, PS, NS> of loose_all_kernel, each with 0 bytes of scratch, at most 256 VGPRs and the static LDS bound the sibling
    kernels are held to (the covariance is dynamic LDS: nothing new in static LDS)."""
    from conftest import PKG
    kernels = {}
    for stem in ('ins_loose_all', 'ins_loose_all16'):
        path = os.path.join(PKG, 'build', stem + '.resources.txt')
        assert os.path.exists(path), 'run gnss-ins-sim_amd/build.py (it writes %s)' % path
        cur = None
        for line in open(path):
            k, _, v = line.strip().partition(':')
            if k == 'Function Name':
                cur = kernels.setdefault(v.strip(), {'file': stem})
            elif cur is not None and v.strip():
                cur[k.split('[')[0].strip()] = v.strip()
    found = {n: r for n, r in kernels.items() if '16loose_all_kernelI' in n}
    seen = set(re.search(r'loose_all_kernelILi(\d)ELb(\d)ELb(\d)ELb(\d)ELi(\d+)E', n).groups() for n in found)
    want = set((rf, g, v, ps, ns) for rf in '01' for g in '01' for v in '01' for ps in '01' for ns in ('15', '16') if not (g == '1' and v == '1'))
    assert seen == want and len(found) == 24, seen ^ want
    for n, r in found.items():
        print(n, {k: r[k] for k in ('VGPRs', 'AGPRs', 'ScratchSize', 'Occupancy', 'LDS Size') if k in r})
        assert r['file'] == ('ins_loose_all16' if 'Li16E' in n else 'ins_loose_all'), n
        assert int(r['ScratchSize']) == 0, '%s: %s bytes of scratch per lane' % (n, r['ScratchSize'])
        assert int(r['Occupancy']) >= 1 and int(r['VGPRs']) <= 256, (n, r)
        assert int(r['LDS Size']) <= 8192 + 4 * 4, (n, r['LDS Size'])


# ------------------------------------------------------------------------------------------------- the job's and the plugin's surface
PAIR_MESSAGES = {
    ('mag', 'scale'): r'^odo_scale_state: the scale-factor state together with the magnetometer block \(mag=...\) is not built$',
    ('mag', 'still'): r'^still: the standstill block together with the magnetometer block \(mag=...\) is not built$',
    ('scale', 'still'): r'^still: the standstill block together with the scale-factor state \(odo_scale_state=...\) is not built$',
    ('mag', 'scale', 'still'): r'^odo_scale_state: the scale-factor state together with the magnetometer block \(mag=...\) is not built$',
}


def test_the_job_s_table_of_combinations_with_the_opt_in():
    from ginsim.ins_loose import COMBINED, COMBINED_BLOCKS, FAMILIES, refuse_combinations
    assert [s for _, s in FAMILIES] == ['_cons', '_mag', '_scale', '_still'] and COMBINED == ('allp', '_all')
    assert COMBINED_BLOCKS == ('magp', 'scalep', 'stillp')
    base = dict(scale=False, keep_scale=False, odo=True, mag=False, cons=False, proc=False, still=False)
    for held, message in PAIR_MESSAGES.items():
        kw = dict(base, **{k: True for k in held})
        refuse_combinations(combined=True, **kw)                                # accepted with the opt-in
        refuse_combinations(combined=True, **dict(kw, proc=True, keep_scale='scale' in held))
        for without in (dict(), dict(combined=False)):                          # refused with today's exact message without it
            with pytest.raises(ValueError, match=message):
                refuse_combinations(**dict(kw, **without))
        with pytest.raises(ValueError, match=r'^combined: consistency checkpoints \(cons_samples=...\) of the combined family are not built$'):
            refuse_combinations(combined=True, **dict(kw, cons=True))
        if 'scale' in held:
            with pytest.raises(ValueError, match=r"^combined: a scale-factor state without the odometer \(aid\['odo'\]\) is refused by the combined family too$"):
                refuse_combinations(combined=True, **dict(kw, odo=False))
    # with one block or none the opt-in changes no row and no message
    for one in ('mag', 'scale', 'still'):
        kw = dict(base, **{one: True})
        refuse_combinations(combined=True, **kw)
        for combined in (False, True):
            with pytest.raises(ValueError, match=r'^(still|odo_scale_state|cons_samples): .*consistency checkpoints'):
                refuse_combinations(combined=combined, **dict(kw, cons=True))
    for combined in (False, True):
        with pytest.raises(ValueError, match=r"^odo_scale_state: a scale-factor state without the odometer \(aid\['odo'\]\) is refused$"):
            refuse_combinations(combined=combined, **dict(base, scale=True, odo=False))
        with pytest.raises(ValueError, match=r'^keep_scale: '):
            refuse_combinations(combined=combined, **dict(base, keep_scale=True))


class FakeBuffer(object):
    def __init__(self, nbytes):
        self.ptr, self.nbytes, self.placed = 4096, int(nbytes), False

    def at(self, offset):
        return self.ptr + int(offset)

    def free(self):
        pass


class FakeContext(object):
    """What InsLooseJob's constructor asks of a Context, without a device: nothing is launched, kernel_name() needs no device."""
    PLACED_MIN_JOB = 1 << 62

    def upload(self, a):
        return FakeBuffer(np.asarray(a).nbytes)

    def malloc(self, nbytes, placed=False):
        return FakeBuffer(nbytes)


@pytest.fixture(scope='module')
def job_args():
    import ginsim
    ini, truth, _ = ls.stops_truth(20.0, 1, 2.0, 200)
    acc_e, gyr_e = cs.imu_errors()
    return lambda **kw: ginsim.InsLooseJob(FakeContext(), 20.0, 1, truth, acc_e, gyr_e, cs.GPS_ERR, ini, 4, **kw)


@pytest.mark.parametrize('held', [(), ('mag',), ('scale',), ('still',), ('mag', 'scale'), ('mag', 'still'), ('scale', 'still'), ('mag', 'scale', 'still')])
def test_the_job_launches_the_combined_family_with_two_or_more_blocks_and_the_single_family_otherwise(job_args, held):
    kw = ls.job_kw(ls.MASK, mc.MAG_ERR if 'mag' in held else None, 'scale' in held, 3 if 'still' in held else 0)
    if len(held) >= 2:
        with pytest.raises(ValueError, match=PAIR_MESSAGES[held]):
            job_args(**kw)                                                      # without the keyword: today's refusal
        job = job_args(combined=True, **kw)
        assert job._family[0] == '_all' and job.allp == (job.magp, job.scalep, job.stillp)
        assert [b is not None for b in job.allp] == [k in held for k in ('mag', 'scale', 'still')]
        assert job.kernel_name() == 'ginsim::loose_all_kernel<1, false, false, false, %d>' % (16 if 'scale' in held else 15)
        with pytest.raises(ValueError, match='^combined: consistency checkpoints'):
            job_args(combined=True, cons_samples=[10], **kw)
        job.mc.precision = 1                                                    # fp32: the glue's check, whatever the family
        with pytest.raises(Exception, match='loose_run: the filter kernel is fp64 only'):
            job.kernel_name()
    else:
        job, plain = job_args(combined=True, **kw), job_args(**kw)
        assert job.allp is None and job._family[0] == plain._family[0] == ('_' + held[0] if held else '')
        assert job.kernel_name() == plain.kernel_name() == 'ginsim::loose_%s_kernel<1, false, false, false>' % (held[0] if held else 'aided')
    if 'scale' in held:
        with pytest.raises(ValueError, match='without the odometer'):
            job_args(combined=True, **dict(kw, aid={'nhc': True}))


def test_plugin_surface():
    from demo_algorithms.ins_loose_device import InsLoose
    plain = InsLoose()
    assert plain.combined is False and plain.combined_arguments() == {} and InsLoose(combined=True).combined_arguments() == {'combined': True}
    assert InsLoose(combined=True).input == plain.input and InsLoose(combined=True).output == plain.output
    every = InsLoose(odo=True, nhc=True, odo_scale_state=True, mag=True, zupt=True, zaru=True, combined=True, mag_every=2, still_every=3, odo_every=4,
                     odo_scale_p0=0.05)
    assert every.input == plain.input + ['odo', 'mag'] and every.output == plain.output + ['odo_scale'] and (every.batch, every.mc_algo) == (True, 'loose')
    assert every.aid() == {'odo': True, 'nhc': True, 'every': 4, 'odo_std': None, 'nhc_std': 0.05, 'scale': None}
    assert every.mag_options() == {'every': 2, 'std': None, 'si': None, 'hi': None}
    assert every.scale_options() == {'scale0': 1.0, 'p0': 0.05, 'q': 0.0}
    assert every.still_options() == {'zupt': True, 'zaru': True, 'every': 3, 'speed': 0.01, 'rate': 2e-4, 'zupt_std': 0.02, 'zaru_std': None, 'flags': None}
    pairs = {'mag + still': dict(mag=True, zupt=True), 'mag + scale': dict(mag=True, odo=True, odo_scale_state=True),
             'scale + still': dict(odo=True, odo_scale_state=True, zaru=True)}
    for name, kw in pairs.items():
        with pytest.raises(ValueError, match='is not built'):
            InsLoose(**kw)                                                      # today's refusals without the keyword
        a = InsLoose(combined=True, **kw)
        assert a.input == plain.input + (['odo'] if kw.get('odo') else []) + (['mag'] if kw.get('mag') else []), name
        assert a.output == plain.output + (['odo_scale'] if kw.get('odo_scale_state') else []), name
    with pytest.raises(ValueError, match='needs odo=True'):
        InsLoose(odo_scale_state=True, mag=True, combined=True)                 # still refused with the keyword
    with pytest.raises(ValueError, match='odo_scale0='):
        InsLoose(odo=True, odo_scale_state=True, odo_scale=0.99, zupt=True, combined=True)


def test_sim_takes_the_combined_plugin_next_to_the_plain_one_and_refuses_fp32():
    from gnss_ins_sim.sim import imu_model, ins_sim
    from demo_algorithms.ins_loose_device import InsLoose
    algos = lambda: [InsLoose(), InsLoose(odo=True, nhc=True, odo_scale_state=True, mag=True, zupt=True, zaru=True, combined=True)]
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=9, gps=True, odo=True)
    sim = ins_sim.Sim([100.0, 10.0, 100.0], sc.STOPS_CSV, ref_frame=1, imu=imu, geo_mag_n=list(mc.GEO), algorithm=algos())
    assert ins_sim._plugin_roles(sim, [getattr(a, 'mc_algo', None) for a in sim.amgr.algo]).loose == [0, 1]
    f32 = ins_sim.Sim([100.0, 10.0, 100.0], sc.STOPS_CSV, ref_frame=1, imu=imu, geo_mag_n=list(mc.GEO), algorithm=algos(), precision='f32')
    with pytest.raises(NotImplementedError, match='fp64 only'):
        f32.run(2)


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.fixture(scope='module', params=[1, 0], ids=['rf1', 'rf0'])
def small(request):
    """5 runs of the stops profile's first 25 s at 20 Hz (the first stop and 8 s after it), every sensor drawn from the model."""
    from ginsim.ins_loose import filter_model
    rf, fs, n, R = request.param, 20.0, 500, 5
    ini, truth, stamps = ls.stops_truth(fs, rf, 2.0, n)
    acc_e, gyr_e = cs.imu_errors()
    rng = np.random.default_rng(5)
    accel, gyro, _, _ = ref.sample_sensors(rng, fs, truth['ref_accel'], truth['ref_gyro'], acc_e, gyr_e, R)
    gps = cs.sample_gps(rng, truth, rf, R)
    odo = ref.sample_odo(rng, truth['ref_odo'], ls.ODO_ERR, R)
    mag = ref.sample_mag(rng, truth['ref_mag'], mc.MAG_ERR_SKEW, R)
    model = filter_model(fs, acc_e, gyr_e, cs.GPS_ERR)
    flags = sc.flags_of(truth)
    assert len(sc.windows(flags)) == 1

    def kw(mag_on=True, scale=True, smask=3, p0=kc.P0_SCALE, **more):
        out = ls.blocks(model, fs, rf, ls.MASK, mc.MAG_ERR_SKEW if mag_on else None, scale, smask, flags=flags, p0=p0)
        return dict(dict(out, odo=odo, mag=mag if mag_on else None), **more)
    return {'args': (rf, fs, gyro, accel, ini, model, gps, stamps, truth['gps_visibility']), 'kw': kw, 'n': n, 'model': model, 'fs': fs, 'rf': rf,
            'flags': flags}


def same(a, b, keys, what):
    for k in keys:
        assert np.array_equal(a[k], b[k]), (what, k)


def test_without_a_scale_the_wrapper_is_the_15_state_restatement_and_with_one_the_scale_restatement(small):
    a = aref.run(*small['args'], **small['kw'](scale=False))
    kw = small['kw'](scale=False)
    b = ref.run(*small['args'], **kw)
    same(a, b, cs.PARITY_KEYS + ('P_end',), 'no scale')
    kw = small['kw'](mag_on=False, smask=0)
    a, b = aref.run(*small['args'], **kw), sref.run(*small['args'], odo=kw['odo'], aid=kw['aid'], scale=kw['scale'])
    same(a, b, kc.PARITY_KEYS + ('P_end',), 'scale alone')


def test_a_scale_state_that_cannot_move_is_the_15_state_combined_run_bit_for_bit(small):
    """p0_scale = 0, q_k = 0: c and pkk stay 0, x[15] stays 0 through every block, and every output is the 15-state run's with
    odo_scale_f = scale0."""
    kw16 = small['kw'](p0=0.0)
    assert kw16['scale']['p0_scale'] == 0.0 and kw16['scale']['q_k'] == 0.0
    a = aref.run(*small['args'], **kw16)
    b = aref.run(*small['args'], **dict(kw16, scale=None))                      # the same aid: odo_scale_f = scale0, r_odo as the state's
    same(a, b, cs.PARITY_KEYS, 'frozen scale')
    assert np.array_equal(a['P_end'][:, :15, :15], b['P_end']) and not a['P_end'][:, 15].any() and np.all(a['k_est'] == kc.SCALE0)
    moving = aref.run(*small['args'], **small['kw']())
    assert not np.array_equal(moving['vel'], a['vel']) and not np.all(moving['k_est'] == kc.SCALE0)


def test_a_block_that_never_fires_leaves_the_run_of_the_others_bit_for_bit(small):
    n, flags = small['n'], small['flags']
    zero = np.zeros(n, dtype=np.int32)
    keys = kc.PARITY_KEYS + ('P_end',)
    full = aref.run(*small['args'], **small['kw']())
    # all flags 0: the scale + mag run
    a, b = aref.run(*small['args'], **small['kw'](flags=zero)), aref.run(*small['args'], **small['kw'](smask=0))
    same(a, b, keys, 'all flags 0')
    assert not np.array_equal(a['vel'], full['vel'])
    # mag_every >= n: the scale + still run
    never = small['kw']()
    never['mag_model'] = dict(never['mag_model'], mag_every=n)
    a, b = aref.run(*small['args'], **never), aref.run(*small['args'], **small['kw'](mag_on=False))
    same(a, b, keys, 'mag_every >= n')
    assert not np.array_equal(a['att'], full['att'])
    # both: ins_loose_scale_ref.run
    never['flags'] = zero
    kw = small['kw'](mag_on=False, smask=0)
    a, b = aref.run(*small['args'], **never), sref.run(*small['args'], odo=kw['odo'], aid=kw['aid'], scale=kw['scale'])
    same(a, b, keys, 'mask and period degenerate')
    never['still'] = dict(never['still'], still_mask=0)
    never['flags'] = flags
    same(aref.run(*small['args'], **never), b, keys, 'still_mask 0')
    # the 16-state covariance stays symmetric and positive semi-definite through every block
    d, dd = full['P_end'], np.sqrt(np.concatenate([full['pdiag_end'], full['scale_end'][:, 1:2]], axis=1))
    assert np.max(np.abs(d - np.swapaxes(d, 1, 2)) / (dd[:, :, None] * dd[:, None, :])) < 1e-12
    assert np.all(np.linalg.eigvalsh(d / (dd[:, :, None] * dd[:, None, :])) > -1e-9)


def test_every_block_s_feedback_moves_the_scale_estimate(small):
    """One sample by hand: after a standstill block and after a magnetometer block of the 16-state filter, k_est has moved by
    -x[15] of that block, which is not zero once the state is correlated with the others."""
    rf, fs, gyro, accel, ini, model, gps, stamps, vis = small['args']
    kw = small['kw']()
    f = sref.ScaleFilter(rf, fs, ini, gyro.shape[0], model, kw['scale'])
    first = sc.windows(small['flags'])[0][0]
    aref.ref.run(rf, fs, gyro[:, :first], accel[:, :first], ini, model, gps, stamps[stamps < first], vis[:np.sum(stamps < first)], odo=kw['odo'][:, :first],
                 aid=kw['aid'], filt=f)
    assert np.any(f.c != 0.0)
    smask, _, r_zupt, r_zaru = ref.still_numbers(kw['still'])
    before = f.k_est.copy()
    x = f.still(gyro[:, first - 1], smask, r_zupt, r_zaru)
    assert x.shape[1] == 16 and np.all(x[:, 15] != 0.0) and np.array_equal(f.k_est, before - x[:, 15])
    _, m_n, cal_si, cal_hi, r_mag = ref.mag_numbers(kw['mag_model'])
    before = f.k_est.copy()
    x = f.mag(kw['mag'][:, first], m_n, cal_si, cal_hi, r_mag)
    assert x.shape[1] == 16 and np.all(x[:, 15] != 0.0) and np.array_equal(f.k_est, before - x[:, 15])


def test_information_only_adds():
    """P does not depend on the noise draw beyond the linearisation: at the outage's last sample the predicted 1 sigma of yaw, of the
    horizontal position and of dbg_z with every aid is not larger than with any subset of {mag, scale-aided odometer, standstill}
    (the 16-state filters; 'none' is the odometer-aided filter with the scale state alone)."""
    from ins_loose_aided_cases import outage_samples
    c = ls.consistency_draw(1, 20.0, 8)
    j = outage_samples(c['truth'], c['stamps'], 20.0, cs.CONSISTENCY_FS_GPS)[1]
    sig = {}
    for mag, still in itertools.product((False, True), (False, True)):
        o = ls.restate(c, ls.MASK, mag, True, 3 if still else 0, keep_pdiag=True)
        p = o['pdiag'][:, j]
        sig[(mag, still)] = {'yaw': np.sqrt(p[:, 8]), 'horizontal': np.sqrt(p[:, 0] + p[:, 1]), 'dbg_z': np.sqrt(p[:, 11])}
        print('mag %d still %d:' % (mag, still), {k: float(np.mean(v)) for k, v in sig[(mag, still)].items()})
    unaided = ls.restate(c, 0, False, False, 0, keep_pdiag=True)['pdiag'][:, j]
    sig['gps'] = {'yaw': np.sqrt(unaided[:, 8]), 'horizontal': np.sqrt(unaided[:, 0] + unaided[:, 1]), 'dbg_z': np.sqrt(unaided[:, 11])}
    everything = sig[(True, True)]
    for subset, s in sig.items():
        if subset == (True, True):
            continue
        for k in ('yaw', 'horizontal', 'dbg_z'):
            assert np.all(everything[k] <= s[k] * (1 + 1e-6)), (subset, k, everything[k], s[k])
    assert np.all(everything['yaw'] < 0.5 * sig['gps']['yaw']) and np.all(everything['horizontal'] < 0.5 * sig['gps']['horizontal'])


@pytest.fixture(scope='module')
def consistency():
    """The 1024-run case once: every block on the 16-state filter; ratios at the last sample of the first stop (the profile truncated
    there: the filter is causal) and at the profile's end."""
    c = ls.consistency_draw(1, cs.CONSISTENCY_FS, cs.CONSISTENCY_RUNS)
    j = sc.windows(c['flags'])[0][1]
    out = {}
    for tag, n in (('stop', j + 1), ('end', c['truth']['ref_accel'].shape[0])):
        out[tag] = ls.ratios16(c, ls.restate(c, ls.CONSISTENCY_MASK, True, True, 3, n), n - 1)
    return out


def test_restatement_consistency(consistency):
    """RMS error over sqrt(mean P_kk) of the 16 states, runs drawn from the filter's own model, every block on.  The cap is DESIGN
    4.11g's: every ratio below 1.4 at both instants.  The recorded ratios are held to 2e-3; tests/test_gpu_ins_loose_all.py holds the
    device to the same."""
    for tag in ('stop', 'end'):
        print('combined %s:' % tag, np.array2string(consistency[tag], precision=3, separator=', '))
    for tag in ('stop', 'end'):
        assert np.all(consistency[tag] < ls.CAP), (tag, consistency[tag])
        np.testing.assert_allclose(consistency[tag], ls.CONSISTENCY_RATIOS[tag], rtol=0, atol=2e-3)
