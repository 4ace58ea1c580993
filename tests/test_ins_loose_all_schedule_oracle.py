"""CPU: what tests/test_gpu_ins_loose_all_schedule.py relies on, shown on the restatement (tests/ins_loose_all_ref.py) without a device.

a. The schedule case (ins_loose_all_cases.SCHEDULE: aid 4, mag 3, still 5 on the first 600 samples of the stops profile at 20 Hz with a
   fix every 10 samples and ins_loose_all_cases.schedule_flags) makes every one of the 15 non-empty subsets of {fix applied, aiding,
   magnetometer, standstill block} fire on some sample j > 0, the four-way meeting with a visible fix among them, and blocks inside the
   GPS outage; the count from the periods is the list of block methods the restatement calls, sample by sample.
b. The closed form of the scale state's random walk: with q_k > 0 and an aiding block that never fires, P[15][15] is the Python loop
   p = p0 * p0; p += q_k (n - 1 times) to the bit, k_est stays scale0, the cross column stays 0 and the other 15 states are the 15-state
   restatement's.
c. q matters where it should: with the odometer row (mask 1) q = 1e-3 /sqrt(s) ends with a larger P[15][15] in every run than q = 0 and
   another k_est; the two end sigmas are recorded in ins_loose_all_cases.SCALE_END_SIGMA."""
import itertools

import numpy as np
import pytest

import ins_loose_all_cases as ls
import ins_loose_all_ref as aref
import ins_loose_cases as cs
import ins_loose_mag_cases as mc
import ins_loose_ref as ref
import ins_loose_scale_cases as kc
import ins_loose_scale_ref as sref

FS, FS_GPS, N, RUNS = 20.0, 2.0, ls.SCHEDULE_N, 4
NAMES = {ls.FIX: 'correct', ls.AID: 'aid', ls.MAG: 'mag', ls.STILL: 'still'}


@pytest.fixture(scope='module', params=[1, 0], ids=['rf1', 'rf0'])
def case(request):
    """4 runs of the schedule case, every sensor drawn from the model."""
    from ginsim.ins_loose import filter_model
    rf = request.param
    ini, truth, stamps = ls.stops_truth(FS, rf, FS_GPS, N)
    acc_e, gyr_e = cs.imu_errors()
    rng = np.random.default_rng(11)
    accel, gyro, _, _ = ref.sample_sensors(rng, FS, truth['ref_accel'], truth['ref_gyro'], acc_e, gyr_e, RUNS)
    gps = cs.sample_gps(rng, truth, rf, RUNS)
    odo = ref.sample_odo(rng, truth['ref_odo'], ls.ODO_ERR, RUNS)
    mag = ref.sample_mag(rng, truth['ref_mag'], mc.MAG_ERR_SKEW, RUNS)
    model = filter_model(FS, acc_e, gyr_e, cs.GPS_ERR)
    flags = ls.schedule_flags(truth, stamps, N)

    def kw(mask=ls.MASK, mag_on=True, scale=True, smask=3, every=ls.SCHEDULE, **more):
        out = ls.blocks(model, FS, rf, mask, mc.MAG_ERR_SKEW if mag_on else None, scale, smask, every=every, flags=flags, **more)
        return dict(out, odo=odo, mag=mag if mag_on else None)
    return {'args': (rf, FS, gyro, accel, ini, model, gps, stamps, truth['gps_visibility']), 'kw': kw, 'rf': rf, 'flags': flags, 'truth': truth,
            'stamps': stamps, 'ini': ini, 'model': model}


# ------------------------------------------------------------------------------------------------- a. the schedule
def test_the_helpers_take_a_period_per_block_and_keep_today_s_behaviour_for_an_int(case):
    model, rf = case['model'], case['rf']
    assert ls.periods(3) == (3, 3, 3) and ls.periods(ls.SCHEDULE) == (4, 3, 5) and ls.periods(ls.ROTATED) == (5, 4, 3)
    assert set(ls.periods(ls.SCHEDULE)) == set(ls.periods(ls.ROTATED))          # the same periods with the roles rotated: no block keeps its own
    assert all(a != b for a, b in zip(ls.periods(ls.SCHEDULE), ls.periods(ls.ROTATED)))
    assert all(np.gcd(a, b) == 1 for a, b in itertools.combinations(ls.periods(ls.SCHEDULE), 2))
    b = ls.blocks(model, FS, rf, ls.MASK, mc.MAG_ERR_SKEW, True, 3, every=ls.SCHEDULE, q=1e-3)
    assert (b['aid']['aid_every'], b['mag_model']['mag_every'], b['still']['still_every']) == (4, 3, 5)
    assert b['scale'] == {'scale0': kc.SCALE0, 'p0_scale': kc.P0_SCALE, 'q_k': 1e-3 * 1e-3 / FS}
    j = ls.job_kw(ls.MASK, mc.MAG_ERR_SKEW, True, 3, every=ls.SCHEDULE, q=1e-3)
    assert (j['aid']['every'], j['mag']['every'], j['still']['every']) == (4, 3, 5) and j['odo_scale_state']['q'] == 1e-3
    same = ls.blocks(model, FS, rf, ls.MASK, mc.MAG_ERR_SKEW, True, 3, every=2)
    assert (same['aid']['aid_every'], same['mag_model']['mag_every'], same['still']['still_every'], same['scale']['q_k']) == (2, 2, 2, 0.0)
    assert ls.job_kw(ls.MASK, None, True, 0)['odo_scale_state'] == {'scale0': kc.SCALE0, 'p0': kc.P0_SCALE}


def test_every_subset_of_the_blocks_fires_on_some_sample(case):
    """All 15 non-empty subsets of {fix applied, aid, mag, still} on samples j > 0 of the 600-sample case; the four together on a sample
    whose fix is visible; blocks inside the GPS outage, a standstill block among them."""
    truth, stamps, flags = case['truth'], case['stamps'], case['flags']
    assert truth['ref_accel'].shape[0] == N == 600 and np.array_equal(stamps, np.arange(0, N, 10))
    s = ls.schedule(N, ls.SCHEDULE, stamps, truth['gps_visibility'], flags)
    count = np.bincount(s[1:], minlength=16)
    print('samples per subset (bits fix 1, aid 2, mag 4, still 8):', count.tolist())
    assert np.all(count[1:] > 0), np.nonzero(count[1:] == 0)[0] + 1
    hidden = stamps[np.asarray(truth['gps_visibility']) == 0]
    first = int(hidden[0])
    assert hidden.size and np.array_equal(hidden, np.arange(first, N, 10))      # one outage, to the case's end
    four = np.nonzero(s == ls.FIX | ls.AID | ls.MAG | ls.STILL)[0]
    assert four.size and np.all(four < first) and np.all(np.isin(four, stamps))
    inside = s[first:]
    assert not np.any(inside & ls.FIX) and all(np.any(inside & b) for b in (ls.AID, ls.MAG, ls.STILL))
    assert np.any(inside == ls.AID | ls.MAG | ls.STILL)                         # the three meet where no fix is applied
    # the truth's own signal alone cannot: its standstill samples all lie before the outage
    own = ls.schedule(N, ls.SCHEDULE, stamps, truth['gps_visibility'], ls.sc.flags_of(truth))
    assert not np.any(own[first:] & ls.STILL) and not np.any(own[1:] == ls.AID | ls.STILL)


class Recorder(object):
    """Wraps the block methods of a filter of the restatement: calls[j] is the set of bits of the methods ins_loose_ref.run called at
    sample j (the hook runs after the blocks of a sample and closes it)."""

    def __init__(self, filt, n):
        self.calls, self.j = np.zeros(n, dtype=np.int64), 0
        for bit, name in NAMES.items():
            setattr(filt, name, self._wrap(getattr(filt, name), bit))

    def _wrap(self, fn, bit):
        def call(*args, **kw):
            assert not self.calls[self.j] & bit and self.calls[self.j] < bit    # once per sample, in the order fix, aid, mag, still
            self.calls[self.j] |= bit
            return fn(*args, **kw)
        return call

    def hook(self, f, j):
        assert j == self.j
        self.j += 1


@pytest.mark.parametrize('every', [ls.SCHEDULE, ls.ROTATED], ids=['aid4 mag3 still5', 'aid5 mag4 still3'])
@pytest.mark.parametrize('scale', [True, False], ids=['16 states', '15 states'])
def test_the_count_is_what_the_restatement_calls(case, every, scale):
    rf, fs, gyro, accel, ini, model, gps, stamps, vis = case['args']
    kw = case['kw'](scale=scale, every=every)
    state = kw.pop('scale', None)
    f = sref.ScaleFilter(rf, fs, ini, RUNS, model, state) if scale else ref.LooseFilter(rf, fs, ini, RUNS, model)
    rec = Recorder(f, N)
    ref.run(rf, fs, gyro, accel, ini, model, gps, stamps, vis, hook=rec.hook, filt=f, **kw)
    assert rec.j == N
    assert np.array_equal(rec.calls, ls.schedule(N, every, stamps, vis, case['flags']))
    assert rec.calls[0] == ls.FIX                                              # nothing but the fix at sample 0


# ------------------------------------------------------------------------------------------------- b. the closed form
def closed_form(p0, q_k, n):
    p = p0 * p0
    for _ in range(n - 1):
        p += q_k
    return p


@pytest.mark.parametrize('q', [1e-3, 0.05])
def test_closed_form_of_the_random_walk_when_the_aiding_block_never_fires(case, q):
    """aid_every = n: no odometer row ever makes the scale state observable.  P[15][15] is n - 1 additions of q_k to the bit, k_est
    stays scale0 at every row, the cross column is exactly 0, and states 0-14 are the 15-state restatement's with the same blocks."""
    kw = case['kw'](every={'aid': N, 'mag': 3, 'still': 5}, q=q)
    q_k = kw['scale']['q_k']
    assert q_k == q * q / FS > 0.0
    o = aref.run(*case['args'], **kw)
    want = closed_form(kc.P0_SCALE, q_k, N)
    assert want > kc.P0_SCALE ** 2 and np.all(o['scale_end'][:, 1] == want)
    assert np.all(o['k_est'] == kc.SCALE0) and np.all(o['scale_end'][:, 0] == kc.SCALE0)
    assert not o['pcross_end'].any() and not o['P_end'][:, 15, :15].any()
    b = aref.run(*case['args'], **dict(kw, scale=None))
    for k in cs.PARITY_KEYS:
        assert np.array_equal(o[k], b[k]), k
    assert np.array_equal(o['P_end'][:, :15, :15], b['P_end'])
    # and the scale family's own restatement
    single = sref.run(*case['args'], odo=kw['odo'], aid=kw['aid'], scale=kw['scale'])
    assert np.all(single['scale_end'][:, 1] == want) and np.all(single['k_est'] == kc.SCALE0) and not single['pcross_end'].any()


# ------------------------------------------------------------------------------------------------- c. q matters
def test_the_random_walk_keeps_the_scale_state_open(case):
    """Mask 1 (the odometer row), the schedule's periods, all three blocks: q = 1e-3 /sqrt(s) against q = 0."""
    a = aref.run(*case['args'], **case['kw'](mask=1, q=ls.SCALE_Q))
    b = aref.run(*case['args'], **case['kw'](mask=1))
    sa, sb = np.sqrt(a['scale_end'][:, 1]), np.sqrt(b['scale_end'][:, 1])
    print('rf%d end sigma of the scale state: q = 0 %.6f, q = 1e-3 %.6f' % (case['rf'], sb.mean(), sa.mean()))
    assert np.all(sa > sb) and np.all(sb < kc.P0_SCALE) and np.all(a['scale_end'][:, 0] != b['scale_end'][:, 0])
    assert not np.array_equal(a['k_est'], b['k_est']) and np.array_equal(a['k_est'][:, :4], b['k_est'][:, :4])   # until the first aiding block
    np.testing.assert_allclose([sb.mean(), sa.mean()], ls.SCALE_END_SIGMA[case['rf']], rtol=0, atol=5e-7)
