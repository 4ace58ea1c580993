"""Shared inputs of the tests of InsLoose with all its aids in one launch (tests/test_ins_loose_all_oracle.py on the CPU,
tests/test_gpu_ins_loose_all.py on the device): the stops profiles' truth with the magnetometer's, every block's numbers, the draw of
the consistency test and the ratios it measures and records; and the schedule case of tests/test_ins_loose_all_schedule_oracle.py and
tests/test_gpu_ins_loose_all_schedule.py: a period per block, the count of what fires on every sample, its standstill signal; and the two choices of
tests/test_gpu_ins_loose_all_cons_edges.py that tests/test_ins_loose_all_cons_oracle.py holds without a GPU: the checkpoints of the tilted
stops profile (edge_checkpoints) and a truth of the scale factor with two non-finite entries (bad_scale_truth)."""
import functools

import numpy as np

import ins_loose_aided_cases as ac
import ins_loose_cases as cs
import ins_loose_mag_cases as mc
import ins_loose_scale_cases as kc
import ins_loose_still_cases as sc

READS = 0.985                                       # what the odometer of the device dumps reads; the filter starts from 1.0
ODO_ERR = {'scale': READS, 'stdv': kc.ODO_STDV}
MASK = 7                                            # odometer and both constraints next to the other blocks

# Measured by tests/test_ins_loose_all_oracle.py::test_restatement_consistency: 1024 runs drawn from the filter's own model with
# np.random.default_rng(ins_loose_cases.CONSISTENCY_SEED) (accel, gyro, GPS as the unaided case draws them, then the true scales
# ~ N(1, 0.02^2), the odometer's noise and the magnetometer as ref_mag + 0.01 N), the stops profile at 20 Hz with 2 Hz GPS,
# 'mid-accuracy' IMU, ref_frame 1; the odometer row alone (mask 1, as ins_loose_scale_cases: the constraint rows are pessimistic by
# construction), the scale-factor state (scale0 1, p0 0.02, q 0), the magnetometer (MAG_ERR, GEO) and both standstill rows, every
# block at every sample.  RMS error over sqrt(mean P_kk) of the 16 states, the 16th k_est - k, at the LAST SAMPLE OF THE FIRST STOP
# ('stop': the profile truncated there) and at the profile's end ('end').  The cap is DESIGN 4.11g's: every ratio below CAP.
CAP = 1.4
CONSISTENCY_MASK = 1
CONSISTENCY_RATIOS = {
    'stop': (0.618, 0.667, 0.513, 0.706, 0.539, 0.695, 0.855, 0.977, 0.846, 1.028, 1.025, 1.000, 0.980, 0.935, 0.951, 0.974),
    'end': (0.594, 0.871, 0.536, 0.904, 0.960, 0.871, 0.982, 1.028, 1.002, 1.055, 1.044, 1.077, 1.016, 0.953, 1.019, 0.947),
}
# at the end of the stop: RMS of k_est - k 0.00178, sqrt(mean P[15][15]) 0.00183; at the profile's end 0.00095 and 0.00101 (from 0.02).
# The largest ratio is dbg_z at the profile's end, 1.077 (the standstill filter alone: 1.061, ins_loose_still_cases): the known
# correlation of the ZARU sample's noise with q_psi, on the optimistic side and small.  The low ratios are dr and dv, as for the
# standstill rows alone (r_zupt is a cautious pseudo-noise).  With the constraint rows too (mask 7) the end ratios are 0.572, 0.651,
# 0.402, 0.900, 0.677, 0.792, 0.923, 1.027, 0.940, 1.054, 1.045, 1.069, 1.016, 0.953, 1.015, 0.934: lower in dr and dv, as mask 7 always is.


# The schedule case (tests/test_ins_loose_all_schedule_oracle.py, tests/test_gpu_ins_loose_all_schedule.py): the first SCHEDULE_N samples
# of the stops profile at 20 Hz with 2 Hz GPS (a fix every 10 samples; the outage begins at sample 540) and a period of its own for
# every block, pairwise coprime.  ROTATED gives every block another block's period: a counter that borrows a period fails under one of
# the two.  OUTAGE_FLAGS: see schedule_flags.
SCHEDULE = {'aid': 4, 'mag': 3, 'still': 5}
ROTATED = {'aid': 5, 'mag': 4, 'still': 3}
SCHEDULE_N = 600
OUTAGE_FLAGS = (540, 545, 560, 585)     # aid + mag + still, still alone, aid + still, mag + still: none with a fix applied
FIX, AID, MAG, STILL = 1, 2, 4, 8       # the bits of schedule()
# Measured by tests/test_ins_loose_all_schedule_oracle.py::test_the_random_walk_keeps_the_scale_state_open: 4 runs drawn from the model
# (np.random.default_rng(11)), the schedule case with mask 1 and all three blocks.  The mean end sigma sqrt(P[15][15]) of the scale
# state with q = 0 and with q = SCALE_Q [1/sqrt(s)], from the initial 0.02, by ref_frame.
SCALE_Q = 1e-3
SCALE_END_SIGMA = {0: (0.002544, 0.003827), 1: (0.002539, 0.003818)}


@functools.lru_cache(maxsize=None)
def stops_truth(fs, ref_frame, fs_gps, n=None, profile=sc.STOPS_CSV, geo=mc.GEO):
    """(ini_pva, truth with 'ref_odo' and 'ref_mag', gps stamps) of a stops profile, cut to the first n samples."""
    return mc.outage_truth(fs, ref_frame, fs_gps, n, profile, geo)


def periods(every):
    """(aid, mag, still): the period of each block.  every: one int for all three, or {'aid': a, 'mag': m, 'still': s}."""
    if isinstance(every, dict):
        assert set(every) == {'aid', 'mag', 'still'}, every
        return int(every['aid']), int(every['mag']), int(every['still'])
    return every, every, every


def blocks(model, fs, rf, mask=MASK, mag=None, scale=False, smask=0, every=1, geo=mc.GEO, flags=None, scale0=kc.SCALE0, p0=kc.P0_SCALE, q=0.0):
    """The keyword arguments of ins_loose_all_ref.run that describe the blocks (without the per-run series odo and mag): aid, and
    mag_model (mag: the magnetometer's error dict), scale (scale: True), still and flags (smask: the standstill rows) where given.
    every: the period of every block, or one per block (periods).  q: the scale state's random walk [1/sqrt(s)]."""
    ea, em, es = periods(every)
    kw = {'aid': (kc.aid(mask, ea, scale0) if scale else ac.aid(mask, ea, odo_err=ODO_ERR)) if mask else None}
    if mag is not None:
        kw['mag_model'] = mc.model(mag, rf, em, geo)
    if scale:
        kw['scale'] = kc.scale(scale0, p0, q, fs)
    if smask:
        kw['still'], kw['flags'] = sc.model(model, fs, smask, es), flags
    return kw


def job_kw(mask=MASK, mag=None, scale=False, smask=0, every=1, geo=mc.GEO, flags=None, scale0=kc.SCALE0, p0=kc.P0_SCALE, keep=True, q=0.0):
    """The same case as the keywords of an InsLooseJob (over odo_err=ODO_ERR)."""
    ea, em, es = periods(every)
    kw = {'odo_err': ODO_ERR}
    if mask:
        kw['aid'] = ac.aid_options(mask, ea)
    if mag is not None:
        kw = mc.mag_kw(mag, geo, em, **kw)
    if scale:
        kw.update(odo_scale_state=dict({'scale0': scale0, 'p0': p0}, **({'q': q} if q else {})), keep_scale=keep)
    if smask:
        kw['still'] = sc.options(smask, es, flags=flags)
    return kw


def schedule(n, every, stamps, visible, flags, mask=MASK, mag=True, smask=3):
    """(n,) int: which of {fix applied, aiding, magnetometer, standstill block} fires at every sample, as the bits FIX, AID, MAG, STILL;
    counted from the periods, the stamps, the visibility and the flags alone (the kernel's and the restatement's rule: a block fires
    at j > 0 with j % period == 0, the standstill block only where flags[j] != 0; a fix is applied where its visibility is not 0).
    tests/test_ins_loose_all_schedule_oracle.py holds it to the block methods the restatement calls."""
    ea, em, es = periods(every)
    j = np.arange(n)
    s = np.zeros(n, dtype=np.int64)
    stamps, visible = np.asarray(stamps), np.asarray(visible)
    s[stamps[(visible != 0) & (stamps < n)]] |= FIX
    later = j > 0
    if mask:
        s[later & (j % ea == 0)] |= AID
    if mag:
        s[later & (j % em == 0)] |= MAG
    if smask:
        s[later & (j % es == 0) & (np.asarray(flags)[:n] != 0)] |= STILL
    return s


def schedule_flags(truth, stamps, n=SCHEDULE_N):
    """The standstill signal of the schedule case: the truth's own over the first n samples and, constructed, the samples OUTAGE_FLAGS
    inside the GPS outage, where the vehicle moves.  Parity does not need the signal to be physical; without them no standstill
    block of these n samples falls into the outage, and an aiding and a standstill block (every 20 samples with SCHEDULE) always
    meet a visible fix."""
    flags = np.array(sc.flags_of(truth)[:n], dtype=np.int32)
    hidden = np.asarray(stamps)[np.asarray(truth['gps_visibility']) == 0]
    assert hidden.size and all(int(hidden[0]) <= j < n for j in OUTAGE_FLAGS)
    flags[list(OUTAGE_FLAGS)] = 1
    return flags


def edge_checkpoints(ini, truth, stamps, flags, every=SCHEDULE):
    """The checkpoints of the tilted stops profile (tests/test_gpu_ins_loose_all_cons_edges.py, held on the CPU by
    tests/test_ins_loose_all_cons_oracle.py), each from the truth and asserted to exist: samples 0 and 1, the last flagged sample of
    the first standstill window, the first sample at which the truth's yaw has wrapped through +-180 deg, a sample inside the GPS
    outage at which the standstill block fires and no fix is applied, a sample at which fix, aiding, magnetometer and standstill
    block all fire, and the last two.  Asserts the profile's preconditions: a southern latitude, |pitch| of 10 deg and more, two
    standstill windows, one outage.  Returns the sorted list (eight samples)."""
    n = truth['ref_accel'].shape[0]
    att, visible, stamps = np.asarray(truth['ref_att']), np.asarray(truth['gps_visibility']), np.asarray(stamps)
    assert ini[0] < 0.0, 'the profile lies south of the equator'
    assert np.max(np.abs(att[:, 1])) >= np.radians(10.0)
    win = sc.windows(flags)
    assert len(win) == 2, win
    hidden = np.nonzero(visible == 0)[0]
    assert hidden.size and np.array_equal(hidden, np.arange(hidden[0], hidden[-1] + 1)) and hidden[-1] + 1 < stamps.size      # one outage
    first, after = int(stamps[hidden[0]]), int(stamps[hidden[-1] + 1])
    assert first <= win[1][0] and win[1][1] < after                             # the second stop lies inside it
    wrap = np.nonzero(np.abs(np.diff(att[:, 0])) > np.pi)[0]
    assert wrap.size
    fires = schedule(n, every, stamps, visible, flags)
    j = np.arange(n)
    blind = np.nonzero((fires & STILL != 0) & (fires & FIX == 0) & (j >= first) & (j < after))[0]
    meet = np.nonzero(fires == FIX | AID | MAG | STILL)[0]
    assert blind.size and meet.size
    samples = sorted({0, 1, int(win[0][1]), int(wrap[0]) + 1, int(blind[0]), int(meet[0]), n - 2, n - 1})
    assert len(samples) == 8 and flags[win[0][1]] != 0
    return samples


def bad_scale_truth(runs=65):
    """A truth of the scale factor that excludes exactly two runs from every checkpoint: NaN in run 7, +inf in run 40."""
    truth = np.full(runs, READS)
    truth[7], truth[40] = np.nan, np.inf
    return truth


def deviation(a, b):
    """ins_loose_scale_cases.deviation where the case has the 16th state, ins_loose_cases.deviation where not."""
    return kc.deviation(a, b) if 'scale_end' in b else cs.deviation(a, b)


def consistency_draw(rf, fs, runs, n=None):
    """One draw for every subset of the blocks: accel, gyro, fixes, the true scales, the odometer's noise, the magnetometer, in that
    order from np.random.default_rng(ins_loose_cases.CONSISTENCY_SEED); 2 Hz GPS, 'mid-accuracy' IMU, the stops profile cut to n."""
    import ins_loose_ref as ref
    from ginsim.ins_loose import filter_model
    ini, truth, stamps = stops_truth(fs, rf, cs.CONSISTENCY_FS_GPS, n)
    acc_e, gyr_e = cs.imu_errors()
    c = {'rf': rf, 'fs': fs, 'ini': ini, 'truth': truth, 'stamps': stamps, 'acc_e': acc_e, 'gyr_e': gyr_e, 'runs': runs,
         'model': filter_model(fs, acc_e, gyr_e, cs.GPS_ERR), 'flags': sc.flags_of(truth)}
    rng = np.random.default_rng(cs.CONSISTENCY_SEED)
    c['accel'], c['gyro'], c['tba'], c['tbg'] = ref.sample_sensors(rng, fs, truth['ref_accel'], truth['ref_gyro'], acc_e, gyr_e, runs)
    c['gps'] = cs.sample_gps(rng, truth, rf, runs)
    c['scales'] = 1.0 + kc.P0_SCALE * rng.standard_normal(runs)
    c['odo'] = c['scales'][:, None] * np.asarray(truth['ref_odo'])[None] + kc.ODO_STDV * rng.standard_normal((runs, truth['ref_odo'].shape[0]))
    c['mag'] = ref.sample_mag(rng, truth['ref_mag'], mc.MAG_ERR, runs)
    return c


def restate(c, mask, mag, scale, smask, n=None, keep_pdiag=False):
    """ins_loose_all_ref.run on (the first n samples of) a consistency_draw with the named blocks."""
    import ins_loose_all_ref as aref
    n = c['truth']['ref_accel'].shape[0] if n is None else n
    m = int(np.searchsorted(c['stamps'], n))
    kw = blocks(c['model'], c['fs'], c['rf'], mask, mc.MAG_ERR if mag else None, scale, smask, flags=c['flags'][:n])
    if kw['aid'] is not None and not scale:            # the 15-state filter is told the mean of the true scales
        kw['aid'] = ac.aid(mask, 1, odo_err={'scale': 1.0, 'stdv': kc.ODO_STDV})
    return aref.run(c['rf'], c['fs'], c['gyro'][:, :n], c['accel'][:, :n], c['ini'], c['model'], c['gps'][:, :m], c['stamps'][:m],
                    c['truth']['gps_visibility'][:m], odo=c['odo'][:, :n], mag=c['mag'][:, :n] if mag else None, keep_pdiag=keep_pdiag, **kw)


def ratios16(c, o, j):
    """RMS error over sqrt(mean P_kk) of the 16 states at sample j = the last of a result o whose run ended there."""
    e = sc.error_at(c, o, j)
    se = np.asarray(o['scale_end'], dtype=np.float64)
    e = np.concatenate([e, (se[:, 0] - c['scales'])[:, None]], axis=1)
    p = np.concatenate([np.asarray(o['pdiag_end'], dtype=np.float64), se[:, 1:2]], axis=1)
    return np.sqrt(np.mean(e * e, axis=0)) / np.sqrt(np.mean(p, axis=0))
