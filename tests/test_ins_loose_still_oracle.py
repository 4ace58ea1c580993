"""CPU: InsLoose's standstill aiding, ZUPT and ZARU: the C ABI's new block, entry points, refusals and dispatch, the
build's resource report of loose_still_kernel, the restatement (tests/ins_loose_ref.py) against the aided restatement, against
what information can only do to P and against the statistics of its own covariance, still_model, standstill_flags, the job's
combination refusals, the plugin's surface and the stops profile's windows.

Recorded in ins_loose_still_cases (measured by test_restatement_consistency; 1024 runs drawn from the filter's own model, the stops
profile at 20 Hz with 2 Hz GPS, 'mid-accuracy' IMU, the default block, ref_frame 1): CONSISTENCY_RATIOS at the last sample of the
first stop and at the profile's end, for the unaided filter and the filter with both rows."""
import ctypes
import itertools
import json
import os
import re

import numpy as np
import pytest

import ins_loose_aided_cases as ac
import ins_loose_cases as cs
import ins_loose_ref as ref
import ins_loose_still_cases as sc
from conftest import GOLDEN, REPO

NEW = {'ginsim_loose_still_run', 'ginsim_loose_still_kernel_name'}
FIELDS = [('still_mask', ctypes.c_int32), ('reserved', ctypes.c_int32), ('still_every', ctypes.c_int64), ('still_flags', ctypes.c_void_p),
          ('r_zupt', ctypes.c_double), ('r_zaru', ctypes.c_double * 3)]
FIXTURE = os.path.join(GOLDEN, 'api_refusals_still.json')
NAN, INF = float('nan'), float('inf')
N, RUNS = 30, 4


# ------------------------------------------------------------------------------------------------- C ABI
def test_the_standstill_block_is_declared_exported_bound_and_mirrored():
    import ginsim
    from ginsim import _lib
    hdr = open(os.path.join(REPO, 'include', 'ginsim.h')).read()
    declared = set(re.findall(r'\b(ginsim_[a-z0-9_]+)\s*\(', hdr))
    so = ctypes.CDLL(ginsim.LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(so, name) and name in ginsim.EXPORTS
    assert ginsim.lib.ginsim_abi_version() == 9
    assert int(re.search(r'#define GINSIM_ABI_VERSION (\d+)', hdr).group(1)) == 9
    body = re.search(r'typedef struct \{((?:(?!typedef struct).)*?)\}\s*ginsim_loose_still_params\s*;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    members = []                                                                # (name, C type, array length or None)
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        ctype = re.match(r'^(?:const\s+)?(\w+)\s*(\*?)', decl)
        rest = re.sub(r'^(?:const\s+)?\w+\s*\*?', '', decl, count=1)
        for x in rest.split(','):
            dim = re.search(r'\[(\d+)\]', x)
            members.append((re.sub(r'\[.*', '', x).strip(' *'), ctype.group(1) + ctype.group(2), int(dim.group(1)) if dim else None))
    assert [m[0] for m in members] == [f[0] for f in _lib.LooseStillParams._fields_] == [f[0] for f in FIELDS]
    scalar = {'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'int32_t*': ctypes.c_void_p}
    for (name, ctype, dim), (_, want) in zip(members, _lib.LooseStillParams._fields_):
        if dim is None and ctype != 'double':
            assert want is scalar[ctype], name
        elif dim is None:
            assert want is ctypes.c_double, name
        else:
            assert ctype == 'double' and want._type_ is ctypes.c_double and want._length_ == dim, name
    # natural alignment, no padding the header does not spell: the offsets the kernel reads the by-value block at
    assert [getattr(_lib.LooseStillParams, f[0]).offset for f in FIELDS] == [0, 4, 8, 16, 24, 32]
    assert ctypes.sizeof(_lib.LooseStillParams) == 56
    assert hasattr(ginsim, 'still_model') and hasattr(ginsim, 'standstill_flags')
    # the README's count of entry points follows the header
    readme = open(os.path.join(REPO, 'README.md')).read()
    assert '%d entry points' % len(declared) in readme


class Blocks(object):
    """The valid parameter blocks of the standstill entry point (tests/test_api_refusals.py's Blocks for this family): mc, p, q."""

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
        q = self.q = L.LooseStillParams()
        q.still_mask, q.still_every, q.still_flags, q.r_zupt = 3, 1, d, 4e-4
        q.r_zaru[:] = [1e-8] * 3

    def name(self):
        """(return code, kernel name or the refusal's message)"""
        from ginsim import _lib as L
        buf = ctypes.create_string_buffer(256)
        ref_ = lambda s: None if s is None else ctypes.byref(s)
        rc = L.lib.ginsim_loose_still_kernel_name(ref_(self.mc), ref_(self.p), ref_(self.q), buf, 256)
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


def _drop(attr):
    def apply(b):
        setattr(b, attr, None)
    return apply


AIDED = _all(_set('p.aid_mask', 6), _set('p.aid_every', 1), _set('p.r_nhc', 0.0025))
SINGLE = {
    'gen': {
        'q NULL': _drop('q'), 'still_mask=-1': _set('q.still_mask', -1), 'still_mask=4': _set('q.still_mask', 4),
        'still_mask=0 is legal: the plain launch': _set('q.still_mask', 0),
        'still_mask=0 is legal: the aided launch': _all(_set('q.still_mask', 0), AIDED),
        'still_mask=0 is legal and reads nothing else': _all(_set('q.still_mask', 0), _set('q.still_flags', None), _set('q.still_every', 0),
                                                             _set('q.r_zupt', NAN), _set('q.r_zaru', -1.0, 1)),
        'still_every=0': _set('q.still_every', 0), 'still_every=-3': _set('q.still_every', -3),
        'still_every=2^40 is legal': _set('q.still_every', 2 ** 40),
        'r_zupt=0': _set('q.r_zupt', 0.0), 'r_zupt nan': _set('q.r_zupt', NAN), 'r_zupt inf': _set('q.r_zupt', INF), 'r_zupt<0': _set('q.r_zupt', -1.0),
        'r_zupt=0 without its bit is legal': _all(_set('q.still_mask', 2), _set('q.r_zupt', 0.0)),
        'r_zaru=0': _set('q.r_zaru', 0.0, 0), 'r_zaru nan': _set('q.r_zaru', NAN, 1), 'r_zaru inf': _set('q.r_zaru', INF, 2), 'r_zaru<0': _set('q.r_zaru', -1e-300, 2),
        'r_zaru nan without its bit is legal': _all(_set('q.still_mask', 1), _set('q.r_zaru', NAN, 1)),
        'still_flags NULL': _set('q.still_flags', None),
        'runs=0': _set('mc.runs', 0), 'ref_gps NULL': _set('p.ref_gps', None), 'vib_accel psd': _set('mc.vib_accel.type', 3), 'aid_mask=8': _set('p.aid_mask', 8),
        'precision=1': _set('mc.precision', 1),
    },
    'given': {'still_flags NULL': _set('q.still_flags', None), 'in_gps NULL': _set('p.in_gps', None), 'r_zupt nan': _set('q.r_zupt', NAN),
              'in_odo NULL is legal without the odometer': _set('mc.in_odo', None)},
}
# two violations at once: the message is that of the check that comes first
PAIRS = [
    # the filter's block before the standstill block
    ('gen', 'aid_mask=8', 'still_mask=4'), ('gen', 'vib_accel psd', 'q NULL'), ('gen', 'runs=0', 'still_flags NULL'), ('gen', 'ref_gps NULL', 'r_zupt=0'),
    ('gen', 'precision=1', 'still_every=0'), ('given', 'in_gps NULL', 'still_flags NULL'),
    # the order inside the standstill block: mask, period, r_zupt, r_zaru, flags
    ('gen', 'still_mask=4', 'still_every=0'), ('gen', 'still_every=0', 'r_zupt nan'), ('gen', 'r_zupt=0', 'r_zaru nan'), ('gen', 'r_zaru=0', 'still_flags NULL'),
    ('given', 'r_zupt nan', 'still_flags NULL'),
]


def _cases():
    out = {}
    for form, table in SINGLE.items():
        out['still %s: valid' % form] = (form, [])
        for what, fn in table.items():
            out['still %s: %s' % (form, what)] = (form, [fn])
    for form, a, b in PAIRS:
        out['still %s: %s + %s' % (form, a, b)] = (form, [SINGLE[form][a], SINGLE[form][b]])
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


def test_every_refusal_is_an_argument_error_with_its_prefix_and_the_filter_s_block_comes_first(recorded):
    from ginsim import _lib as L
    refused = 0
    for name, (rc, text) in recorded.items():
        if name.endswith('valid') or 'legal' in name:
            assert rc == L.OK and text.startswith('ginsim::'), name
        else:
            assert rc == L.ERR_ARG and text.split(':')[0] in ('loose_run', 'loose_still_run'), name
            refused += 1
    assert refused >= 25
    for form, a, b in PAIRS[:6]:                                                # the filter's block before the standstill block
        assert recorded['still %s: %s + %s' % (form, a, b)][1].startswith('loose_run: '), (a, b)
    for form, a, b in PAIRS[6:]:
        assert recorded['still %s: %s + %s' % (form, a, b)] == recorded['still %s: %s' % (form, a)], (a, b)
    assert recorded['still gen: precision=1'][1].startswith('loose_run: ')
    assert recorded['still gen: still_mask=0 is legal: the plain launch'][1] == 'ginsim::loose_kernel<0, false, false, false>'
    assert recorded['still gen: still_mask=0 is legal: the aided launch'][1] == 'ginsim::loose_aided_kernel<0, false, false, false>'
    assert recorded['still gen: still_mask=0 is legal and reads nothing else'][1] == 'ginsim::loose_kernel<0, false, false, false>'
    # the run entry point makes the same checks before it touches a device
    b = Blocks(False)
    b.q.still_mask = 4
    assert L.lib.ginsim_loose_still_run(None, ctypes.byref(b.mc), ctypes.byref(b.p), ctypes.byref(b.q)) == L.ERR_ARG
    b.q.still_mask = 3
    assert L.lib.ginsim_loose_still_run(None, ctypes.byref(b.mc), ctypes.byref(b.p), ctypes.byref(b.q)) == L.ERR_ARG
    assert L.lib.ginsim_last_error().decode().startswith('loose_still_run: NULL argument')
    assert L.lib.ginsim_loose_still_kernel_name(ctypes.byref(b.mc), ctypes.byref(b.p), ctypes.byref(b.q), None, 0) == L.ERR_ARG


TF = {False: 'false', True: 'true'}


@pytest.mark.parametrize('rf, source, flag, aided', list(itertools.product((0, 1), ('gen', 'vib', 'given'), (False, True), (False, True))))
def test_still_dispatch(rf, source, flag, aided):
    """The 12 names ginsim::loose_still_kernel<RF, GIVEN, VIB, PS>, with and without the odometer / non-holonomic block next to the
    standstill block (the same kernel); still_mask = 0 names the plain or the aided kernel."""
    b = Blocks(source == 'given')
    b.mc.ref_frame = rf
    if source == 'vib':
        b.mc.vib_gyro.type = 1
    if aided:
        AIDED(b)
    if flag:
        b.p.out_proc, b.mc.ref_nav = b.d, b.d
    args = (rf, TF[source == 'given'], TF[source == 'vib'], TF[flag])
    for mask in (1, 2, 3):
        b.q.still_mask = mask
        assert b.name() == [0, 'ginsim::loose_still_kernel<%d, %s, %s, %s>' % args]
    b.q.still_mask = 0
    assert b.name() == [0, 'ginsim::%s<%d, %s, %s, %s>' % (('loose_aided_kernel' if aided else 'loose_kernel',) + args)]


def test_build_reports_no_scratch_for_any_instantiation_of_the_standstill_kernel():
    """build/ins_loose_still.resources.txt (written by build.py): the 12 instantiations <RF, GIVEN, VIB, PS> of loose_still_kernel, each
    with 0 bytes of scratch, at most 256 VGPRs and the static LDS bound the sibling kernels are held to (nothing new in LDS)."""
    from conftest import PKG
    path = os.path.join(PKG, 'build', 'ins_loose_still.resources.txt')
    assert os.path.exists(path), 'run gnss-ins-sim_amd/build.py (it writes %s)' % path
    kernels, cur = {}, None
    for line in open(path):
        k, _, v = line.strip().partition(':')
        if k == 'Function Name':
            cur = kernels.setdefault(v.strip(), {})
        elif cur is not None and v.strip():
            cur[k.split('[')[0].strip()] = v.strip()
    still = {n: r for n, r in kernels.items() if '18loose_still_kernelI' in n}
    seen = set(re.search(r'loose_still_kernelILi(\d)ELb(\d)ELb(\d)ELb(\d)E', n).groups() for n in still)
    want = set((rf, g, v, ps) for rf in '01' for g in '01' for v in '01' for ps in '01' if not (g == '1' and v == '1'))
    assert seen == want and len(still) == 12, seen ^ want
    for n, r in still.items():
        print(n, {k: r[k] for k in ('VGPRs', 'AGPRs', 'ScratchSize', 'Occupancy', 'LDS Size') if k in r})
        assert int(r['ScratchSize']) == 0, '%s: %s bytes of scratch per lane' % (n, r['ScratchSize'])
        assert int(r['Occupancy']) >= 1 and int(r['VGPRs']) <= 256, (n, r)
        assert int(r['LDS Size']) <= 8192 + 4 * 4, (n, r['LDS Size'])


# ------------------------------------------------------------------------------------------------- the profile
@pytest.mark.parametrize('rf', [0, 1])
def test_the_stops_profile_has_two_standstill_windows_one_inside_the_outage(rf):
    """55 s; at speed 0.02 m/s and rate 1e-3 rad/s the truth is still at 10.5-17.1 s and 33.5-40.1 s (20 Hz) and at 9.15-17.06 s and
    32.15-40.06 s (100 Hz); GPS is hidden from 27 s to 45 s.  The default thresholds give shorter windows inside those."""
    for fs, want in ((20.0, [(10.5, 17.1), (33.5, 40.1)]), (100.0, [(9.15, 17.06), (32.15, 40.06)])):
        ini, truth, stamps = sc.stops_truth(fs, rf, 2.0)
        n = truth['ref_accel'].shape[0]
        assert n == int(55 * fs)
        w = sc.windows(sc.flags_of(truth, 0.02, 1e-3))
        np.testing.assert_allclose(np.array(w) / fs, want, rtol=0, atol=1e-9)
        d = sc.windows(sc.flags_of(truth))
        assert len(d) == 2 and all(a0 <= a and b <= b0 and b - a > 5 * fs for (a, b), (a0, b0) in zip(d, w))
        speed = np.linalg.norm(truth['ref_vel'], axis=1)
        assert speed[w[0][0]] <= 0.02 and speed[w[0][1] - int(fs)] < 1e-6 and speed[w[0][0] - 1] > 0.02      # rest is approached, not hit
        rate = np.linalg.norm(truth['ref_gyro'][d[0][0]:d[0][1]], axis=1)
        assert np.all(np.abs(rate - (7.292115e-5 if rf == 0 else 0.0)) < 2e-6)
        hidden = stamps[np.asarray(truth['gps_visibility']) == 0] / fs
        assert hidden.min() == 27.0 and hidden.max() == 44.5
        assert hidden.min() < d[1][0] / fs and d[1][1] / fs < hidden.max()     # the second stop lies inside the outage
        assert d[0][1] / fs < hidden.min()                                      # the first one has GPS


@pytest.mark.parametrize('rf', [0, 1])
def test_the_tilted_stops_profile_parks_twice_on_a_slope_once_inside_the_outage(rf):
    """tests/golden/ins_loose/motion_def_tilted_stops.csv, what tests/test_gpu_ins_loose_tilted_aids.py and the B7' test of
    tests/test_ins_loose_attitude_oracle.py rely on: 48 s at 20 Hz with 2 Hz fixes; the default flags give the windows 180-301 and
    600-721; the vehicle stands at (170, 12, -10) deg and at (-160, -8, 5) deg, 41 S; the yaw wraps after samples 422 and 875; the
    fixes 48-79 are hidden and the second stop lies inside that outage."""
    fs = 20.0
    ini, truth, stamps = sc.stops_truth(fs, rf, 2.0, None, sc.TILTED_STOPS_CSV)
    n = truth['ref_accel'].shape[0]
    assert n == 960 and stamps.size == 96 and np.array_equal(stamps, np.arange(96) * 10)
    w = sc.windows(sc.flags_of(truth))
    assert w == [(180, 301), (600, 721)]
    att = np.rad2deg(truth['ref_att'])
    for (a, b), want in zip(w, ((170.0, 12.0, -10.0), (-160.0, -8.0, 5.0))):
        np.testing.assert_allclose(att[a:b + 1], np.tile(want, (b + 1 - a, 1)), rtol=0, atol=1e-3)
        assert np.max(np.linalg.norm(truth['ref_vel'][a:b + 1], axis=1)) <= 0.01
    assert np.nonzero(np.abs(np.diff(truth['ref_att'][:, 0])) > np.pi)[0].tolist() == [422, 875]
    assert np.rad2deg(ini[0]) == pytest.approx(-41.0)                             # the southern hemisphere
    hidden = np.nonzero(np.asarray(truth['gps_visibility']) == 0)[0]
    assert hidden.tolist() == list(range(48, 80))
    assert stamps[hidden[0]] < w[1][0] and w[1][1] < stamps[hidden[-1]]           # the second stop lies inside the outage
    assert w[0][1] < stamps[hidden[0]]                                            # the first one has GPS


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.fixture(scope='module', params=[(1, 0), (0, 7)], ids=['rf1', 'rf0-aided'])
def small(request):
    """5 runs of the stops profile's first 25 s at 20 Hz (the first stop and 8 s after it), sensors drawn from the model."""
    from ginsim.ins_loose import filter_model
    rf, mask = request.param
    fs, n, R = 20.0, 500, 5
    ini, truth, stamps = sc.stops_truth(fs, rf, 2.0, n)
    acc_e, gyr_e = cs.imu_errors()
    rng = np.random.default_rng(5)
    accel, gyro, _, _ = ref.sample_sensors(rng, fs, truth['ref_accel'], truth['ref_gyro'], acc_e, gyr_e, R)
    gps = cs.sample_gps(rng, truth, rf, R)
    odo = ref.sample_odo(rng, truth['ref_odo'], ac.ODO_ERR, R)
    model = filter_model(fs, acc_e, gyr_e, cs.GPS_ERR)
    return {'args': (rf, fs, gyro, accel, ini, model, gps, stamps, truth['gps_visibility']), 'kw': dict(odo=odo, aid=ac.aid(mask) if mask else None),
            'model': model, 'fs': fs, 'n': n, 'flags': sc.flags_of(truth), 'truth': truth}


def test_a_block_that_never_fires_is_the_aided_restatement_bit_for_bit(small):
    n, flags = small['n'], small['flags']
    a = ref.run(*small['args'], **small['kw'])
    still = sc.model(small['model'], small['fs'], 3)
    only_first = np.zeros(n, dtype=np.int32)
    only_first[0] = 1
    for name, kw in (('no block', dict()), ('all flags 0', dict(still=still, flags=np.zeros(n, dtype=np.int32))),
                     ('a flag at j = 0 only', dict(still=still, flags=only_first)),
                     ('every >= n', dict(still=sc.model(small['model'], small['fs'], 3, every=n), flags=flags)),
                     ('every = 2^40', dict(still=sc.model(small['model'], small['fs'], 3, every=2 ** 40), flags=flags)),
                     ('mask 0', dict(still=dict(still, still_mask=0), flags=flags))):
        o = ref.run(*small['args'], **dict(small['kw'], **kw))
        for k in cs.PARITY_KEYS + ('P_end',):
            assert np.array_equal(a[k], o[k]), (name, k)
    c = ref.run(*small['args'], still=still, flags=flags, **small['kw'])
    assert not np.array_equal(a['vel'], c['vel']) and not np.array_equal(a['wb'], c['wb'])
    d, dd = c['P_end'], np.sqrt(c['pdiag_end'])
    assert np.max(np.abs(d - np.swapaxes(d, 1, 2)) / (dd[:, :, None] * dd[:, None, :])) < 1e-12
    assert np.all(np.linalg.eigvalsh(d / (dd[:, :, None] * dd[:, None, :])) > -1e-9)


def test_one_bit_alone_is_the_full_block_with_the_other_bit_clear(small):
    """ZUPT only = the block whose ZARU rows are switched off by their variance being unreadable (and the reverse): the mask alone
    selects the rows, the other rows' numbers are not read."""
    flags = small['flags']
    both = sc.model(small['model'], small['fs'], 3)
    for mask in (1, 2):
        alone = ref.run(*small['args'], still=sc.model(small['model'], small['fs'], mask), flags=flags, **small['kw'])
        cleared = ref.run(*small['args'], still=dict(both, still_mask=mask), flags=flags, **small['kw'])
        poisoned = dict(both, still_mask=mask, **({'r_zaru': np.full(3, np.nan)} if mask == 1 else {'r_zupt': np.nan}))
        unread = ref.run(*small['args'], still=poisoned, flags=flags, **small['kw'])
        full = ref.run(*small['args'], still=both, flags=flags, **small['kw'])
        for k in cs.PARITY_KEYS + ('P_end',):
            assert np.array_equal(alone[k], cleared[k]) and np.array_equal(alone[k], unread[k]), (mask, k)
        assert not np.array_equal(alone['pdiag_end'], full['pdiag_end'])


def test_zaru_uses_the_raw_sample_before_and_the_rest_rate():
    """One block by hand: z = wb + w_rest - gyro[j - 1] (raw), w_rest = D (W cos lat, 0, -W sin lat) in ref_frame 0 with earth_rot and
    zero otherwise; a filter at rest whose gyro reads bias + earth rate learns exactly that bias."""
    from oracle import ins_np
    from ginsim.ins_loose import filter_model
    acc_e, gyr_e = cs.imu_errors()
    fs = 20.0
    model = filter_model(fs, acc_e, gyr_e, cs.GPS_ERR, p0=(1e-3, 1e-3, 1e-5, 1e-3, 1e-5))
    ini = np.array([0.6, 2.0, 10.0, 0.0, 0.0, 0.0, 0.7, -0.2, 0.3])
    bias = np.array([[2e-4, -1e-4, 3e-4]])
    for rf, earth in ((0, True), (0, False), (1, True)):
        f = ref.LooseFilter(rf, fs, ini, 1, model, earth)
        w = f.rest_rate()
        if rf == 0 and earth:
            want = ref.dcm_zyx(ini[None, 6:9])[0] @ (ins_np.W_IE * np.array([np.cos(0.6), 0.0, -np.sin(0.6)]))
            np.testing.assert_allclose(w[0], want, rtol=1e-14)
            assert abs(np.linalg.norm(w) - ins_np.W_IE) < 1e-18
        else:
            assert np.all(w == 0.0)
        x = f.still(w + bias, 2, 1.0, np.full(3, 1e-12))                       # a nearly noise-free ZARU
        np.testing.assert_allclose(f.wb, bias, rtol=2e-6)                       # truth = estimate - error: wb rises to the bias
        np.testing.assert_allclose(x[:, 9:12], -bias, rtol=2e-6)
        assert np.all(x[:, 0:9] == 0.0) and np.all(x[:, 12:15] == 0.0)          # P0 is diagonal: nothing else moves


def test_information_only_adds():
    """P does not depend on the noise draw beyond the linearisation: at the end of the first stop the predicted 1 sigma of dbg_z with
    ZARU is strictly below the one without, and the predicted 1 sigma of every dv with ZUPT strictly below the one without.  (The states
    a row does not observe can differ in the seventh digit either way: the two filters linearise about different estimates.)"""
    c = sc.consistency_draw(1, 20.0, 8)
    j = sc.windows(c['flags'])[0][1]
    o = {name: sc.restate_filter(c, name, keep_pdiag=True) for name in sc.FILTERS}
    sig = {name: np.sqrt(v['pdiag'][:, j]) for name, v in o.items()}
    for name in ('gps', 'zupt', 'zaru', 'still'):
        print(name, 'sigma dv', sig[name][0, 3:6], 'sigma dbg', sig[name][0, 9:12])
    assert np.all(sig['zaru'][:, 11] < sig['gps'][:, 11]) and np.all(sig['still'][:, 11] < sig['zupt'][:, 11])
    assert np.all(sig['zaru'][:, 9:12] < sig['gps'][:, 9:12])
    assert np.all(sig['zupt'][:, 3:6] < sig['gps'][:, 3:6]) and np.all(sig['still'][:, 3:6] < sig['zaru'][:, 3:6])
    assert np.all(sig['zupt'][:, 3:5] < 0.5 * sig['gps'][:, 3:5])               # the horizontal velocity: by far
    # and before the first flagged sample nothing differs
    first = sc.windows(c['flags'])[0][0]
    for name in ('zupt', 'zaru', 'still'):
        for k in ('att', 'pos', 'vel', 'wb', 'ab', 'pdiag'):
            assert np.array_equal(o[name][k][:, :first], o['gps'][k][:, :first]), (name, k)


@pytest.fixture(scope='module')
def consistency():
    """The 1024-run case once: the unaided filter and the filter with both rows; ratios at the last sample of the first stop (the state
    is that of the profile truncated there: the filter is causal) and at the profile's end."""
    c = sc.consistency_draw(1, cs.CONSISTENCY_FS, cs.CONSISTENCY_RUNS)
    j = sc.windows(c['flags'])[0][1]
    out = {}
    for name in ('gps', 'still'):
        o = sc.restate_filter(c, name, keep_pdiag=True)
        out[name] = {'stop': sc.ratios(sc.error_at(c, o, j), o['pdiag'][:, j]), 'end': sc.ratios(sc.error_at(c, o, -1), o['pdiag'][:, -1])}
    return out


def test_restatement_consistency(consistency):
    """RMS error over sqrt(mean pdiag) per state, runs drawn from the filter's own model.  The unaided filter lies in BAND = [0.7, 1.4]
    at both instants.  The filter with both rows: every state <= 1.4 at both instants (it never claims more than it has), and
    >= 0.7 in psi, dbg and dba; dr and dv are bounded above only, as the project bounds the non-holonomic rows.  Outside the unaided
    filter's band, on the LOW side, fall dr_z (0.51-0.54 at both instants; the unaided filter's own is 0.79 at the stop) and, at the
    end of the stop, dv (0.50-0.69): r_zupt = (0.02 m/s)^2 is a pseudo-noise, twice the largest true speed the flags admit, while
    the true speed in the window decays to 1e-8 m/s and is the same in every run -- the rows are far more exact than the filter is
    told, so P stays above the error, as the non-holonomic rows do.  The known correlation of the ZARU sample's
    noise with the process noise is on the optimistic side and small: dbg stays within 1.07."""
    for name in ('gps', 'still'):
        for tag in ('stop', 'end'):
            print('%s %s:' % (name, tag), np.array2string(consistency[name][tag], precision=3, separator=', '))
    lo, hi = sc.BAND
    for tag in ('stop', 'end'):
        g, s = consistency['gps'][tag], consistency['still'][tag]
        assert np.all(g >= lo) and np.all(g <= hi), (tag, g)
        assert np.all(s <= hi), (tag, s)
        assert np.all(s[6:15] >= lo), (tag, s)
        np.testing.assert_allclose(g, sc.CONSISTENCY_RATIOS['gps'][tag], rtol=0, atol=2e-3)
        np.testing.assert_allclose(s, sc.CONSISTENCY_RATIOS['still'][tag], rtol=0, atol=2e-3)


def test_restatement_consistency_on_the_tilted_stops_profile():
    """The same on tests/golden/ins_loose/motion_def_tilted_stops.csv (ref_frame 1, 1024 runs, both rows): what the level test asserts
    of the filter with both rows -- every state <= 1.4 at both instants, psi, dbg and dba >= 0.7 -- and the ratios recorded in
    ins_loose_still_cases.CONSISTENCY_BY_PROFILE['tilted'], which tests/test_gpu_ins_loose_tilted_aids.py holds the device to.
    Measured: dr and dv lie low as on the level profile and for the same reason (dr_y 0.63, dr_z 0.49, dv 0.50-0.69 at the end of
    the stop, dr_z 0.52 at the end); psi, dbg and dba stay in 0.81-1.07."""
    c = sc.consistency_draw(1, cs.CONSISTENCY_FS, cs.CONSISTENCY_RUNS, profile=sc.TILTED_STOPS_CSV)
    j = sc.windows(c['flags'])[0][1]
    o = sc.restate_filter(c, 'still', keep_pdiag=True)
    got = {'stop': sc.ratios(sc.error_at(c, o, j), o['pdiag'][:, j]), 'end': sc.ratios(sc.error_at(c, o, -1), o['pdiag'][:, -1])}
    for tag in ('stop', 'end'):
        print('tilted stops, still %s:' % tag, np.array2string(got[tag], precision=3, separator=', '))
    lo, hi = sc.BAND
    for tag in ('stop', 'end'):
        assert np.all(got[tag] <= hi), (tag, got[tag])
        assert np.all(got[tag][6:15] >= lo), (tag, got[tag])
        np.testing.assert_allclose(got[tag], sc.CONSISTENCY_BY_PROFILE['tilted']['still'][tag], rtol=0, atol=2e-3)


# ------------------------------------------------------------------------------------------------- Python surface
def test_still_model_defaults_and_refusals():
    from ginsim.ins_loose import filter_model, still_model
    acc_e, gyr_e = cs.imu_errors()
    fm = filter_model(20.0, acc_e, gyr_e, cs.GPS_ERR)
    assert still_model(fm, 20.0, None) is None
    a = still_model(fm, 20.0, {})
    assert sorted(a) == ['r_zaru', 'r_zupt', 'rate', 'speed', 'still_every', 'still_mask']
    assert (a['still_mask'], a['still_every'], a['speed'], a['rate']) == (3, 1, 0.01, 2e-4)
    assert a['r_zupt'] == 0.02 ** 2
    np.testing.assert_allclose(a['r_zaru'], fm['q_psi'] * 20.0 ** 2, rtol=1e-15)
    t = still_model(fm, 20.0, True)
    assert all(np.array_equal(t[k], a[k]) for k in a) and sorted(t) == sorted(a)
    assert still_model(fm, 20.0, {'zaru': False})['still_mask'] == 1 and np.all(still_model(fm, 20.0, {'zaru': False})['r_zaru'] == 0.0)
    b = still_model(fm, 20.0, {'zupt': False, 'every': 4, 'zaru_std': 1e-4, 'speed': 0.0, 'rate': 1e-3})
    assert (b['still_mask'], b['still_every'], b['r_zupt'], b['speed'], b['rate']) == (2, 4, 0.0, 0.0, 1e-3)
    np.testing.assert_allclose(b['r_zaru'], [1e-8] * 3, rtol=1e-15)
    assert still_model(fm, 20.0, {'zupt': False, 'zaru': False})['still_mask'] == 0
    np.testing.assert_allclose(still_model(fm, 20.0, {'zaru_std': [1e-4, 2e-4, 3e-4]})['r_zaru'], [1e-8, 4e-8, 9e-8], rtol=1e-15)
    for bad in ({'evry': 1}, {'every': 0}, {'every': 1.5}, {'zupt_std': 0.0}, {'zupt_std': -0.02}, {'zupt_std': NAN}, {'zaru_std': 0.0},
                {'zaru_std': [1e-4, 1e-4]}, {'zaru_std': [1e-4, INF, 1e-4]}, {'speed': -0.01}, {'speed': NAN}, {'rate': -1.0}, {'rate': INF}):
        with pytest.raises(ValueError):
            still_model(fm, 20.0, bad)
    with pytest.raises(ValueError, match='unknown keys'):
        still_model(fm, 20.0, {'evry': 1})


def test_standstill_flags():
    from ginsim.ins_loose import standstill_flags
    vel = np.array([[0.0, 0.0, 0.0], [0.006, 0.008, 0.0], [0.006, 0.008, 0.001], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    gyro = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 2e-4], [0.0, 0.0, 0.0], [1e-4, 0.0, 2e-4], [0.0, 0.0, 0.0]])
    f = standstill_flags({'ref_vel': vel, 'ref_gyro': gyro})
    assert f.dtype == np.int32 and f.tolist() == [1, 1, 0, 0, 0]                # the norms, each against its threshold, inclusive
    assert standstill_flags({'ref_vel': vel, 'ref_gyro': gyro}, 0.02, 1e-3).tolist() == [1, 1, 1, 1, 0]
    assert standstill_flags({'ref_vel': vel, 'ref_gyro': gyro}, 0.0, 0.0).tolist() == [1, 0, 0, 0, 0]
    for bad in ((-1.0, 1.0), (1.0, NAN), (INF, 1.0)):
        with pytest.raises(ValueError):
            standstill_flags({'ref_vel': vel, 'ref_gyro': gyro}, *bad)
    with pytest.raises(ValueError):
        standstill_flags({'ref_vel': vel, 'ref_gyro': gyro[:3]})


def test_the_job_s_table_of_combinations():
    from ginsim.ins_loose import FAMILIES, refuse_combinations
    assert FAMILIES[-1] == ('stillp', '_still') and [s for _, s in FAMILIES] == ['_cons', '_mag', '_scale', '_still']
    base = dict(scale=False, keep_scale=False, odo=False, mag=False, cons=False, proc=False)
    refuse_combinations(**base)
    refuse_combinations(still=True, **base)
    refuse_combinations(still=True, **dict(base, odo=True, proc=True))
    with pytest.raises(ValueError, match=r'^still: the standstill block together with the magnetometer block \(mag=...\) is not built$'):
        refuse_combinations(still=True, **dict(base, mag=True))
    with pytest.raises(ValueError, match=r'^still: consistency checkpoints \(cons_samples=...\) of the filter with the standstill block are not built$'):
        refuse_combinations(still=True, **dict(base, cons=True))
    with pytest.raises(ValueError, match=r'^still: the standstill block together with the scale-factor state \(odo_scale_state=...\) is not built$'):
        refuse_combinations(still=True, **dict(base, scale=True, odo=True))
    # every existing message still wins, and is what it was
    with pytest.raises(ValueError, match=r'^odo_scale_state: the scale-factor state together with the magnetometer block \(mag=...\) is not built$'):
        refuse_combinations(still=True, **dict(base, scale=True, odo=True, mag=True))
    with pytest.raises(ValueError, match=r'^cons_samples: consistency checkpoints of the magnetometer-aided filter are not built \(mag=...\)$'):
        refuse_combinations(still=True, **dict(base, mag=True, cons=True))
    with pytest.raises(ValueError, match=r'^cons_samples: online process statistics \(proc_first\) and checkpoints in one launch are refused$'):
        refuse_combinations(still=True, **dict(base, cons=True, proc=True))
    with pytest.raises(ValueError, match=r'^cons_samples: online process statistics'):
        refuse_combinations(**dict(base, cons=True, proc=True))                 # the old signature, without `still`


def test_plugin_surface():
    from demo_algorithms.ins_loose_device import InsLoose
    plain = InsLoose()
    assert plain.still_options() is None and (plain.zupt, plain.zaru) == (False, False)
    a = InsLoose(zupt=True, zaru=True)
    assert a.input == plain.input and a.output == plain.output and (a.batch, a.mc_algo) == (True, 'loose')
    assert a.still_options() == {'zupt': True, 'zaru': True, 'every': 1, 'speed': 0.01, 'rate': 2e-4, 'zupt_std': 0.02, 'zaru_std': None,
                                 'flags': None}
    b = InsLoose(odo=True, nhc=True, zaru=True, still_every=3, still_speed=0.02, still_rate=1e-3, zupt_std=0.05, zaru_std=[1e-4, 1e-4, 2e-4],
                 standstill=[0, 1, 1, 0])
    o = b.still_options()
    assert (o['zupt'], o['zaru'], o['every'], o['speed'], o['rate'], o['zupt_std']) == (False, True, 3, 0.02, 1e-3, 0.05)
    assert o['flags'].dtype == np.int32 and o['flags'].tolist() == [0, 1, 1, 0] and b.input == plain.input + ['odo']
    assert InsLoose(still_every=4, zupt_std=0.1, standstill=[1, 0]).still_options() is None     # the numbers alone switch nothing on
    for bad in (dict(still_every=0), dict(still_every=2.5), dict(zupt_std=0.0), dict(zupt_std=INF), dict(zaru_std=[1e-4, 1e-4]),
                dict(zaru_std=-1e-4), dict(still_speed=-1.0), dict(still_rate=NAN), dict(mag=True), dict(odo=True, odo_scale_state=True)):
        with pytest.raises((ValueError, TypeError)):
            InsLoose(zupt=True, zaru=True, **bad)
    from gnss_ins_sim.sim import imu_model
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=True)
    series = [100.0, np.zeros((10, 3)), np.zeros((10, 3)), np.arange(10) / 100.0, np.zeros(1), np.zeros((1, 6))]
    with pytest.raises(ValueError, match='standstill='):                        # a logged series has no truth to derive the flags from
        InsLoose(ini_pos_vel_att=np.zeros(9), ref_frame=1, imu=imu, zupt=True).run(series)


def test_sim_takes_the_standstill_plugin_next_to_the_plain_one():
    from gnss_ins_sim.sim import imu_model, ins_sim
    from demo_algorithms.ins_loose_device import InsLoose
    sim = ins_sim.Sim([100.0, 10.0, 0.0], sc.STOPS_CSV, ref_frame=1, imu=imu_model.IMU(accuracy='mid-accuracy', axis=6, gps=True),
                      algorithm=[InsLoose(), InsLoose(zupt=True, zaru=True)])
    assert ins_sim._plugin_roles(sim, [getattr(a, 'mc_algo', None) for a in sim.amgr.algo]).loose == [0, 1]
