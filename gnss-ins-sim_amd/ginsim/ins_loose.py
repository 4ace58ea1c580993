"""InsLooseJob: the loosely coupled GPS/INS Kalman filter (the interface demo_algorithms/ins_loose.py::InsLoose declares, whose
prediction and correction are `pass` in the reference) over a batch of Monte-Carlo runs on one device (csrc/ins_loose.hip,
ginsim_loose_run).  One launch: every lane makes its own IMU samples and GPS fixes again from the run's Philox streams (the bits
MonteCarloJob and AuxSensorJob would store), mechanises them with the free-integration step on bias-corrected samples and runs a
15-state closed-loop error-state filter next to it.  tests/ins_loose_ref.py restates the arithmetic in NumPy.
With aid=... the filter also uses the odometer and the non-holonomic constraints of a land vehicle (csrc/ins_loose_aided.hip,
aiding_model; restated by tests/ins_loose_ref.py).  With cons_samples=... the launch also reduces, across its runs, the
filter's covariance and its actual error at those samples (csrc/ins_loose_cons.hip, consistency(); restated by
tests/ins_loose_cons_ref.py).  With mag=... the filter also uses the magnetometer, a three-row block on the attitude error
(csrc/ins_loose_mag.hip, mag_model; restated by tests/ins_loose_ref.py).  With odo_scale_state=... the odometer's scale factor is
a 16th state that the filter estimates (csrc/ins_loose_scale.hip, scale_model; restated by tests/ins_loose_scale_ref.py).
With still=... the filter also uses what it may assume while the vehicle stands still, the zero-velocity and the zero-angular-rate
update (csrc/ins_loose_still.hip, still_model, standstill_flags; restated by tests/ins_loose_ref.py).
What one launch does not combine is stated once (refuse_combinations); the job records the family it launches once (FAMILIES).
With combined=True the magnetometer block, the scale-factor state and the standstill block go together in one launch
(csrc/ins_loose_all.hip, COMBINED; restated by tests/ins_loose_all_ref.py, which composes the two restatements above).
With checkpoints=... any of these filters reduces the consistency record, the scale state's columns included
(csrc/ins_loose_all_cons.hip, ALL_CONS; restated by tests/ins_loose_all_cons_ref.py).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib, check
from .engine import DeviceView, StatsResult, ConsistencyResult, ini_table
from .job import BatchJob

P0_FLOOR = (1e-3, 1e-3, 1e-5, 1e-7, 1e-5)      # m, m/s, rad, rad/s, m/s^2


def filter_model(fs, accel_err, gyro_err, gps_err, q_scale=1.0, p0=None):
    """The numbers of ginsim_loose_params that describe the filter, from the error dicts the run is generated with.

      r_diag    gps_err['stdp']^2, gps_err['stdv']^2 (stdp in metres in both frames)
      q_v/q_psi (vrw^2 | arw^2) dt per body axis; an axis whose drift is white (b_corr = inf: pathgen.bias_drift draws an
                independent drift every sample) adds that sample noise, b_drift^2 dt^2, and its bias state is a constant
      q_bg/q_ba the driving noise of the Gauss-Markov drift as pathgen.bias_drift generates it, 2 sigma^2 / tau dt
      decay_*   1 - dt / tau (1 for a random walk)
      p0        initial 1 sigma of (dr, dv, psi, dbg, dba).  Default: the runs start ON the truth with zero drift, so the floor
                P0_FLOOR = (1e-3 m, 1e-3 m/s, 1e-5 rad, 1e-7 rad/s, 1e-5 m/s^2), and for the two bias states the largest constant
                bias |b| of the sensor where that is larger
    q_scale multiplies every Qd."""
    dt = 1.0 / float(fs)
    m = {'r_diag': np.concatenate([(np.asarray(gps_err['stdp'], dtype=np.float64) * np.ones(3)) ** 2,
                                   (np.asarray(gps_err['stdv'], dtype=np.float64) * np.ones(3)) ** 2])}
    for err, rw, qn, qb, dec in ((accel_err, 'vrw', 'q_v', 'q_ba', 'decay_a'), (gyro_err, 'arw', 'q_psi', 'q_bg', 'decay_g')):
        w = np.asarray(err[rw], dtype=np.float64) * np.ones(3)
        sig = np.asarray(err['b_drift'], dtype=np.float64) * np.ones(3)
        tau = np.asarray(err['b_corr'], dtype=np.float64) * np.ones(3)
        inf = np.isinf(tau)
        tau_f = np.where(inf, 1.0, tau)
        m[qn] = (w * w * dt + np.where(inf, sig * sig * dt * dt, 0.0)) * float(q_scale)
        m[qb] = np.where(inf, 0.0, 2.0 * sig * sig / tau_f * dt) * float(q_scale)
        m[dec] = np.where(inf, 1.0, 1.0 - dt / tau_f)
    if p0 is None:
        p0 = list(P0_FLOOR)
        p0[3] = max(p0[3], float(np.max(np.abs(np.asarray(gyro_err['b'], dtype=np.float64)))))
        p0[4] = max(p0[4], float(np.max(np.abs(np.asarray(accel_err['b'], dtype=np.float64)))))
    m['p0'] = np.asarray(p0, dtype=np.float64).reshape(5)
    return m


def gps_sigma(gps_err, ref_gps, ref_frame):
    """ginsim_aux_params.gps_sigma as AuxSensorJob makes it (pathgen.py:616-619: metres -> rad at the FIRST fix in ref_frame 0)."""
    from gnss_ins_sim.geoparams import geoparams
    sig = np.concatenate([np.asarray(gps_err['stdp'], dtype=np.float64) * np.ones(3),
                          np.asarray(gps_err['stdv'], dtype=np.float64) * np.ones(3)])
    if ref_frame == 0:
        rm, rn, _, _, cl, _ = geoparams.geo_param(ref_gps[0, 0:3])
        sig[0] = sig[0] / rm
        sig[1] = sig[1] / rn / cl
    return sig


def aiding_model(odo_err, aid):
    """The five aiding numbers of ginsim_loose_params, {'aid_mask', 'aid_every', 'odo_scale_f', 'r_odo', 'r_nhc'}, from the
    odometer's error dict {'scale', 'stdv'} (None without an odometer) and the options
    aid = {'odo': bool, 'nhc': bool, 'every': int, 'odo_std': float | None, 'nhc_std': float, 'scale': float | None}:

      aid_mask     bit 0 'odo' (z = v_b[0] - odo / scale), bits 1 and 2 'nhc' (z = v_b[1], v_b[2])
      odo_scale_f  'scale': the scale factor the FILTER assumes; default odo_err['scale'].  It is a parameter, not a state: a
                   filter that assumes 1.0 of an odometer that reads 0.99 is inconsistent by a factor of tens;
                   InsLooseJob(odo_scale_state=...) estimates it instead (scale_model)
      r_odo        'odo_std'^2 [m/s]: of the SCALED sample; default odo_err['stdv'] / scale
      r_nhc        'nhc_std'^2 [m/s]; default 0.05: a pseudo-noise, how far the vehicle may slide
      aid_every    'every': a block every so many IMU samples; default 1
    aid None or without 'odo' and 'nhc': no aiding (aid_mask 0)."""
    aid = dict(aid or {})
    unknown = set(aid) - {'odo', 'nhc', 'every', 'odo_std', 'nhc_std', 'scale'}
    if unknown:
        raise ValueError('aid: unknown keys %s' % sorted(unknown))
    odo, nhc = bool(aid.get('odo', False)), bool(aid.get('nhc', False))
    out = {'aid_mask': (1 if odo else 0) | (6 if nhc else 0), 'aid_every': 0, 'odo_scale_f': 0.0, 'r_odo': 0.0, 'r_nhc': 0.0}
    if not out['aid_mask']:
        return out
    every = aid.get('every', 1)
    if int(every) != every or int(every) < 1:
        raise ValueError("aid['every'] must be an integer >= 1")
    out['aid_every'] = int(every)

    def positive(name, v):
        v = float(v)
        if not (v > 0.0 and np.isfinite(v)):
            raise ValueError('aid[%r] must be positive and finite' % (name,))
        return v
    if nhc:
        out['r_nhc'] = positive('nhc_std', aid.get('nhc_std', 0.05)) ** 2
    if odo:
        scale, std = aid.get('scale'), aid.get('odo_std')
        if (scale is None or std is None) and odo_err is None:
            raise ValueError("aid['odo'] needs odo_err={'scale', 'stdv'} or both aid['scale'] and aid['odo_std']")
        scale = positive('scale', odo_err['scale'] if scale is None else scale)
        out['odo_scale_f'] = scale
        out['r_odo'] = positive('odo_std', float(odo_err['stdv']) / scale if std is None else std) ** 2
    return out


def mag_field(geo_mag_n, ref_frame):
    """The geomagnetic field [uT] in the navigation frame of ref_frame, (3,): the NED vector in ref_frame 0; in ref_frame 1 the
    virtual-inertial x axis points along the horizontal field, (hypot(bx, by), 0, bz), as pathgen forms it (pathgen.py:169-171)."""
    g = np.asarray(geo_mag_n, dtype=np.float64).reshape(-1)
    if g.size != 3 or not np.all(np.isfinite(g)):
        raise ValueError('geo_mag_n must be three finite numbers [uT]')
    if int(ref_frame) == 1:
        g = np.array([np.hypot(g[0], g[1]), 0.0, g[2]])
    return g.copy()


def mag_model(mag_err, geo_mag_n, ref_frame, mag=None):
    """The numbers of the magnetometer block of ginsim_loose_mag_params that describe the FILTER,
    {'mag_every', 'mag_n', 'cal_si', 'cal_hi', 'r_mag'}, from the magnetometer's error dict {'si', 'hi', 'std'} (None: every
    number must come from the options), the geomagnetic field geo_mag_n [uT, NED] and the options
    mag = {'every': int, 'std': 3 floats | float, 'si': (3, 3), 'hi': (3,), 'field': (3,)}:

      mag_every  'every': a block every so many IMU samples; default 1
      cal_si     inv('si'), cal_hi = 'hi': the calibration the filter ASSUMES, m_cal = cal_si . mag - cal_hi; default mag_err's own
                 soft- and hard-iron.  Parameters, not states (as the odometer's scale factor): MagCal's result can be passed here
      r_mag      diag(cal_si diag('std'^2) cal_si^T) [uT^2]; 'std' defaults to mag_err['std'].  The calibrated sample's noise
                 covariance is that full matrix; the rows are processed as independent scalars, so its off-diagonal terms are
                 dropped.  The expression is exact for a diagonal soft-iron matrix
      mag_n      'field': the field the filter assumes in the navigation frame; default geo_mag_n in the frame's form
                 (mag_field: as it is in ref_frame 0, (hypot(bx, by), 0, bz) in ref_frame 1)
    """
    mag = dict(mag or {})
    unknown = set(mag) - {'every', 'std', 'si', 'hi', 'field'}
    if unknown:
        raise ValueError('mag: unknown keys %s' % sorted(unknown))
    every = mag.get('every', 1)
    if int(every) != every or int(every) < 1:
        raise ValueError("mag['every'] must be an integer >= 1")

    def pick(name, size):
        v = mag.get(name)
        if v is None:
            if mag_err is None:
                raise ValueError("mag[%r] is needed without mag_err={'si', 'hi', 'std'}" % (name,))
            v = mag_err[name]
        v = np.asarray(v, dtype=np.float64)
        v = v * np.ones(3) if (name != 'si' and v.size == 1) else v
        if v.size != size or not np.all(np.isfinite(v)):
            raise ValueError('mag[%r] must be %d finite numbers' % (name, size))
        return v.reshape(-1)
    si, hi, std = pick('si', 9).reshape(3, 3), pick('hi', 3), pick('std', 3)
    if not np.all(std > 0.0):
        raise ValueError("mag['std'] must be positive and finite")
    if not abs(np.linalg.det(si)) > 1e-12 * max(np.abs(si).max(), np.finfo(np.float64).tiny) ** 3:
        raise ValueError("mag['si'] is singular: the filter cannot undo that soft-iron matrix")
    cal_si = np.linalg.inv(si)
    field = mag.get('field')
    if field is None:
        if geo_mag_n is None:
            raise ValueError("the magnetometer block needs the geomagnetic field: geo_mag_n or mag['field']")
        field = mag_field(geo_mag_n, ref_frame)
    field = np.asarray(field, dtype=np.float64).reshape(-1)
    if field.size != 3 or not np.all(np.isfinite(field)) or not np.any(field != 0.0):
        raise ValueError("mag['field'] must be three finite numbers, not all zero")
    return {'mag_every': int(every), 'mag_n': field.copy(), 'cal_si': cal_si, 'cal_hi': hi.copy(),
            'r_mag': np.einsum('ik,k,ik->i', cal_si, std * std, cal_si)}


def scale_model(odo_err, opts, fs=None):
    """The three numbers of ginsim_loose_scale_params that describe the FILTER, {'scale0', 'p0_scale', 'q_k'}, from the odometer's
    error dict {'scale', 'stdv'} (not read: the filter does not know the odometer's scale -- that is the point of the state) and
    the options opts = {'scale0': float, 'p0': float, 'q': float}:

      scale0    the scale factor the filter starts from; default 1.0
      p0_scale  'p0': the initial 1 sigma of the scale-factor error; default 0.02; 0 (with q 0) is the filter that assumes scale0
      q_k       'q'^2 / fs: 'q' [1/sqrt(s)] is the random walk of the scale factor; default 0, a constant.  'q' > 0 needs fs
    opts None: no scale state (None is returned); {} or True takes every default."""
    if opts is None or opts is False:
        return None
    opts = {} if opts is True else dict(opts)
    unknown = set(opts) - {'scale0', 'p0', 'q'}
    if unknown:
        raise ValueError('odo_scale_state: unknown keys %s' % sorted(unknown))
    scale0, p0, q = float(opts.get('scale0', 1.0)), float(opts.get('p0', 0.02)), float(opts.get('q', 0.0))
    if not (scale0 > 0.0 and np.isfinite(scale0)):
        raise ValueError("odo_scale_state['scale0'] must be positive and finite")
    if not (p0 >= 0.0 and np.isfinite(p0)):
        raise ValueError("odo_scale_state['p0'] must be finite and not negative")
    if not (q >= 0.0 and np.isfinite(q)):
        raise ValueError("odo_scale_state['q'] must be finite and not negative")
    if q > 0.0 and fs is None:
        raise ValueError("odo_scale_state['q'] > 0 needs the sample rate fs")
    return {'scale0': scale0, 'p0_scale': p0, 'q_k': q * q / float(fs) if q > 0.0 else 0.0}


STILL_KEYS = ('zupt', 'zaru', 'every', 'speed', 'rate', 'zupt_std', 'zaru_std', 'flags')


def still_model(model, fs, still=None):
    """The numbers of ginsim_loose_still_params that describe the FILTER, {'still_mask', 'still_every', 'r_zupt', 'r_zaru'}, and the
    two thresholds of standstill_flags, {'speed', 'rate'}, from the filter's model (filter_model: 'q_psi' is read), the sample rate
    and the options still = {'zupt': bool, 'zaru': bool, 'every': int, 'speed': float, 'rate': float, 'zupt_std': float,
    'zaru_std': 3 floats | float, 'flags': (n,)}:

      still_mask   bit 0 'zupt' (z = vel, on dv), bit 1 'zaru' (z = bg_est + w_rest - gyro, on dbg); default both
      still_every  'every': a block is possible every so many IMU samples; default 1
      speed, rate  the standstill signal of standstill_flags: |ref_vel| <= speed [m/s] and |ref_gyro| <= rate [rad/s]; defaults
                   0.01 and 2e-4.  Not read when 'flags' gives the signal (the job reads 'flags', not this function)
      r_zupt       'zupt_std'^2 [m/s]; default 0.02: twice the largest true speed the default flags admit
      r_zaru       'zaru_std'^2 [rad/s] per body axis; default sqrt(q_psi) fs: the per-sample rate noise the filter already believes in
    still None: no block (None is returned); {} or True takes every default."""
    if still is None or still is False:
        return None
    still = {} if still is True else dict(still)
    unknown = set(still) - set(STILL_KEYS)
    if unknown:
        raise ValueError('still: unknown keys %s' % sorted(unknown))
    zupt, zaru = bool(still.get('zupt', True)), bool(still.get('zaru', True))
    every = still.get('every', 1)
    if int(every) != every or int(every) < 1:
        raise ValueError("still['every'] must be an integer >= 1")

    def positive(name, v, size=1, zero=False):
        v = np.asarray(v, dtype=np.float64).reshape(-1)
        v = v * np.ones(size) if v.size == 1 else v
        if v.size != size or not np.all(np.isfinite(v)) or not np.all(v >= 0.0 if zero else v > 0.0):
            raise ValueError('still[%r] must be %s%s and finite' % (name, '%d numbers, ' % size if size > 1 else '',
                                                                   'not negative' if zero else 'positive'))
        return v
    speed, rate = positive('speed', still.get('speed', 0.01), zero=True)[0], positive('rate', still.get('rate', 2e-4), zero=True)[0]
    out = {'still_mask': (1 if zupt else 0) | (2 if zaru else 0), 'still_every': int(every), 'speed': float(speed), 'rate': float(rate),
           'r_zupt': 0.0, 'r_zaru': np.zeros(3)}
    if zupt:
        out['r_zupt'] = float(positive('zupt_std', still.get('zupt_std', 0.02))[0]) ** 2
    if zaru:
        std = still.get('zaru_std')
        if std is None:
            std = np.sqrt(np.asarray(model['q_psi'], dtype=np.float64) * np.ones(3)) * float(fs)
        out['r_zaru'] = positive('zaru_std', std, 3) ** 2
    return out


def standstill_flags(truth, speed=0.01, rate=2e-4):
    """(n,) int32: flag[j] = |ref_vel[j]| <= speed and |ref_gyro[j]| <= rate, from the truth's 'ref_vel' and 'ref_gyro' (n, 3): the
    standstill signal a vehicle would supply, one per IMU sample for all runs.  A detector on each run's own noisy sensors would
    differ from lane to lane and is not built."""
    speed, rate = float(speed), float(rate)
    if not (speed >= 0.0 and np.isfinite(speed) and rate >= 0.0 and np.isfinite(rate)):
        raise ValueError('standstill_flags: speed and rate must be finite and not negative')
    vel, gyro = np.asarray(truth['ref_vel'], dtype=np.float64), np.asarray(truth['ref_gyro'], dtype=np.float64)
    if vel.ndim != 2 or vel.shape[1] != 3 or gyro.shape != vel.shape:
        raise ValueError("standstill_flags: truth['ref_vel'] and truth['ref_gyro'] must be (n, 3)")
    return np.ascontiguousarray((np.linalg.norm(vel, axis=1) <= speed) & (np.linalg.norm(gyro, axis=1) <= rate), dtype=np.int32)


# the family blocks a job can hold, in the order the C glue picks among them: (the job's attribute, the entry points' suffix)
FAMILIES = (('cons', '_cons'), ('magp', '_mag'), ('scalep', '_scale'), ('stillp', '_still'))
# the combined family, looked at before FAMILIES: a job made with combined=True that holds two or three of COMBINED_BLOCKS launches
# through the entry points with this suffix, which take the three blocks (None: NULL) and not one
COMBINED = ('allp', '_all')
COMBINED_BLOCKS = ('magp', 'scalep', 'stillp')
# checkpoints for every family (checkpoints=...), looked at before both: the entry points with this suffix take COMBINED_BLOCKS
# (None: NULL), the checkpoint block and the device pointer of the scale factor's truth
ALL_CONS = ('consp', '_all_cons')


def refuse_combinations(scale, keep_scale, odo, mag, cons, proc, still=False, combined=False):
    """The options of InsLooseJob that one launch does not combine, stated once: (applies, message), the first row that applies is
    raised.  Arguments: is the option given (scale: odo_scale_state, odo: aid['odo'], cons: cons_samples, proc: proc_first,
    still: still).  combined: the job was made with combined=True: the three rows that name two of the magnetometer block, the
    scale-factor state and the standstill block do not apply; what the combined family refuses comes first and says so."""
    pair = not combined
    more = sum(map(bool, (scale, mag, still))) >= 2
    rows = (
        (combined and more and cons, 'combined: consistency checkpoints (cons_samples=...) of the combined family are not built'),
        (combined and more and scale and not odo,"combined: a scale-factor state without the odometer (aid['odo']) is refused by the combined family too"),
        (keep_scale and not scale, 'keep_scale: the scale-factor series exists with odo_scale_state=... only'),
        (pair and scale and mag, 'odo_scale_state: the scale-factor state together with the magnetometer block (mag=...) is not built'),
        (scale and cons, 'odo_scale_state: consistency checkpoints (cons_samples=...) of the filter with the scale-factor state are not built'),
        (scale and not odo, "odo_scale_state: a scale-factor state without the odometer (aid['odo']) is refused"),
        (mag and cons, 'cons_samples: consistency checkpoints of the magnetometer-aided filter are not built (mag=...)'),
        (cons and proc, 'cons_samples: online process statistics (proc_first) and checkpoints in one launch are refused'),
        (pair and still and mag, 'still: the standstill block together with the magnetometer block (mag=...) is not built'),
        (still and cons, 'still: consistency checkpoints (cons_samples=...) of the filter with the standstill block are not built'),
        (pair and still and scale, 'still: the standstill block together with the scale-factor state (odo_scale_state=...) is not built'),
    )
    for applies, text in rows:
        if applies:
            raise ValueError(text)


class InsLooseJob(BatchJob):
    """One batch of runs of the loosely coupled filter on one device.

    truth: dict with 'ref_accel', 'ref_gyro', 'ref_att', 'ref_pos', 'ref_vel' (n, 3) and 'ref_gps' (m, 6), 'gps_time' (m,)
    [seconds: fix k is applied at IMU sample round(gps_time[k] fs)], 'gps_visibility' (m,) as workloads.truth_from_profile(gps=True)
    makes them.  ini: the initial states FreeIntegration takes.  gps_err: {'stdp', 'stdv'}.
    given: None (samples and fixes are regenerated per lane: same seed and run ids as MonteCarloJob / AuxSensorJob, same bits) or a
    dict of device buffers {'accel', 'gyro'} [3][n][runs] and 'gps' [6][m][runs] (and 'odo' [n][runs] for aid['odo']).
    odo_err, aid: the odometer's error dict {'scale', 'stdv'} and the aiding options of aiding_model() (csrc/ins_loose_aided.hip;
    None: the filter without aiding).  aid['odo'] needs truth['ref_odo'] (n,) and odo_err in the generated form: the lane makes the
    odometer sample MonteCarloJob(keep_sensors) would store for the same seed and run ids.
    model: filter_model(...) or None (made from the error dicts, q_scale and p0).
    keep_traj: materialise att / pos / vel ([9][n][runs]) and wb, ab ([3][n][runs] each).
    proc_first: None, or the first sample of the online process-error window.  end_pos_ned / proc_ned (ref_frame 0): position
    errors of the end-point record / of the process statistics in local NED metres; end_ned: a second end-point record in NED metres.
    placed: as MonteCarloJob (kept planes of Context.PLACED_MIN_JOB bytes or more come from the placed arena).
    cons_samples: None, or the IMU sample indices (any order, repeats allowed) at which the launch reduces the consistency record
    across its runs (consistency()): the filter's P against its error in its own coordinates.  Not together with proc_first.
    mag_err, geo_mag_n, mag: the magnetometer's error dict {'si', 'hi', 'std'}, the geomagnetic field [uT, NED] and the options of
    mag_model() (csrc/ins_loose_mag.hip; mag None: the filter without the magnetometer block; {} takes every default).  The
    generated form needs truth['ref_mag'] (n, 3) and mag_err: the lane makes the magnetometer sample AuxSensorJob would store for
    the same seed and run ids.  The given form reads given['mag'] [3][n][runs].  Not together with cons_samples.
    odo_scale_state: None, or the options of scale_model() ({} takes every default): the odometer's scale factor is the filter's
    16th state (csrc/ins_loose_scale.hip).  Needs aid['odo']; aid['scale'] is then not read (the filter starts from 'scale0'), and
    r_odo defaults to (odo_err['stdv'] / scale0)^2.  Together with mag and still through combined=True; not with cons_samples or fp32.  keep_scale: materialise the
    k_est series ([n][runs]; series('odo_scale', ...)).
    still: None, or the options of still_model() ({} takes every default): the zero-velocity and the zero-angular-rate update at the
    samples the standstill signal marks (csrc/ins_loose_still.hip).  The signal is still['flags'] (n,), or standstill_flags() of the
    truth with still['speed'] and still['rate']; it is the job's own device array in the generated and in the given form (nothing
    is read from `given`).  Together with mag and odo_scale_state through combined=True; not with cons_samples.
    combined: True lifts the three "not together" rules among mag, odo_scale_state and still: a job that holds two or three of them
    launches the combined family (csrc/ins_loose_all.hip), one kernel that runs every block in the order fix, odometer /
    constraints, magnetometer, standstill.  With one of them or none the job launches exactly what it launches without the keyword.
    Still refused: cons_samples, fp32 (the C glue's check), odo_scale_state without aid['odo'].
    checkpoints: None, or sample indices with cons_samples' rules (any order, repeats allowed): the consistency record
    (consistency()) of a filter with any of mag, odo_scale_state and still -- with combined=True, with a single block or with
    none -- through one kernel family that has every block and the checkpoints (csrc/ins_loose_all_cons.hip; restated
    by tests/ins_loose_all_cons_ref.py).  cons_samples keeps its own kernel and every refusal it has.  Not together with
    cons_samples or proc_first.
    scale_truth: with checkpoints and odo_scale_state, the true scale factor the record's scale columns compare k_est with: a scalar
    or (runs,), indexed by the run id.  None: odo_err['scale'] in the generated form (what the lane makes its odometer with); no
    truth in the given form (e2_scale and nes_scale are then 0).
    """

    algos = ('loose',)

    def __init__(self, ctx, fs, ref_frame, truth, accel_err, gyro_err, gps_err, ini, runs, seed=0, run_offset=0, ini_first=0,
                 earth_rot=True, given=None, model=None, q_scale=1.0, p0=None, keep_traj=False, proc_first=None, proc_ned=False,
                 end_pos_ned=False, end_ned=False, vib_accel=None, vib_gyro=None, placed=None, gps_stamps=None, odo_err=None, aid=None,
                 cons_samples=None, mag_err=None, geo_mag_n=None, mag=None, odo_scale_state=None, keep_scale=False, still=None,
                 combined=False, checkpoints=None, scale_truth=None):
        self.ctx, self._bufs = ctx, {}
        self.combined = bool(combined)
        if checkpoints is not None and cons_samples is not None:
            raise ValueError('checkpoints: not together with cons_samples (one list of checkpoints per launch)')
        if checkpoints is not None and proc_first is not None:
            raise ValueError('checkpoints: online process statistics (proc_first) and checkpoints in one launch are refused')
        if scale_truth is not None and (odo_scale_state is None or odo_scale_state is False):
            raise ValueError('checkpoints: scale_truth without the scale-factor state (odo_scale_state=...)')
        if scale_truth is not None and checkpoints is None:
            raise ValueError('checkpoints: scale_truth is read at checkpoints (checkpoints=...) only')
        self.keep_traj, self.keep_scale = bool(keep_traj), bool(keep_scale)
        self.proc_first, self.proc_ned, self.end_ned = proc_first, bool(proc_ned), bool(end_ned)
        table, ref_gps = self._sizes_and_stamps(fs, ref_frame, truth, ini, runs, seed, run_offset, ini_first, earth_rot, end_pos_ned,
                                                gps_stamps)
        self.model = model if model is not None else filter_model(fs, accel_err, gyro_err, gps_err, q_scale, p0)
        self.scale = scale_model(odo_err, odo_scale_state, fs)
        self.still = still_model(self.model, fs, still)
        refuse_combinations(scale=self.scale is not None, keep_scale=self.keep_scale, odo=bool(aid and aid.get('odo')),
                            mag=mag is not None, cons=cons_samples is not None, proc=proc_first is not None, still=self.still is not None,
                            combined=self.combined)
        for k in ('r_diag', 'p0', 'q_v', 'q_psi', 'q_bg', 'q_ba', 'decay_g', 'decay_a'):     # the filter numbers
            getattr(self.params, k)[:] = [float(x) for x in np.asarray(self.model[k], dtype=np.float64).reshape(-1)]
        self._family_blocks(ref_frame, odo_err, aid, mag_err, geo_mag_n, mag)
        self._standstill(truth, still)
        self._inputs(table, ref_gps, truth, fs, accel_err, gyro_err, gps_err, odo_err, mag_err, vib_accel, vib_gyro, given)
        self._outputs(placed)
        self._checkpoints(cons_samples)
        # the family the job launches, once: the first block of FAMILIES that the job has (the order of the C glue), else the plain entry
        self._family = next(((suffix, getattr(self, attr)) for attr, suffix in FAMILIES if getattr(self, attr) is not None), ('', None))
        # the combined family first: two or three of its blocks in a job that opted in
        held = tuple(getattr(self, attr) for attr in COMBINED_BLOCKS)
        self.allp = held if self.combined and sum(b is not None for b in held) >= 2 else None
        if self.allp is not None:
            self._family = (COMBINED[1], self.allp)
        # checkpoints=: whatever blocks the job holds (none to three) go through the one entry point that has checkpoints for all
        # of them (csrc/ins_loose_all_cons.hip); cons_samples= above keeps its own
        self.consp = None
        if checkpoints is not None:
            self._checkpoints(checkpoints, 'checkpoints')
            self.consp, self.cons = self.cons, None
            self._scale_truth(scale_truth, given, odo_err)
            truth_ptr = None if 'scale_truth' not in self._bufs else C.c_void_p(self._bufs['scale_truth'].ptr)
            self._family = (ALL_CONS[1], held + (self.consp, truth_ptr))

    # ------------------------------------------------------------------ the constructor's steps
    def _sizes_and_stamps(self, fs, ref_frame, truth, ini, runs, seed, run_offset, ini_first, earth_rot, end_pos_ned, gps_stamps):
        """n, runs, m and the fields of the two base blocks that say which runs a launch makes and when its fixes arrive (the stamps
        and the visibility flags stay host arrays: every launch copies them).  Returns the initial-state table and ref_gps (m, 6)."""
        self.n, self.runs = int(truth['ref_accel'].shape[0]), int(runs)
        if self.runs < 1:
            raise ValueError('runs must be >= 1')
        if self.end_ned and int(ref_frame) != 0:
            raise ValueError('end_ned: ref_frame 0 only')
        self._ref_frame = int(ref_frame)
        m = self.mc = _lib.McParams()
        self._fill_batch(m, fs, run_offset, seed)
        m.ref_frame, m.earth_rot, m.end_pos_ned = int(ref_frame), int(bool(earth_rot)), int(bool(end_pos_ned))
        table, has_g = ini_table(ini)
        m.n_ini, m.ini_first, m.ini_has_g = table.shape[0], int(ini_first), int(has_g)
        ref_gps = np.ascontiguousarray(truth['ref_gps'], dtype=np.float64).reshape(-1, 6) if 'ref_gps' in truth else np.zeros((0, 6))
        self.m = int(ref_gps.shape[0])
        if gps_stamps is None:
            gps_stamps = np.rint(np.asarray(truth['gps_time'], dtype=np.float64) * float(fs)) if self.m else np.zeros(0)
        self._stamps = np.ascontiguousarray(gps_stamps, dtype=np.int64).reshape(-1)
        vis = truth['gps_visibility'] if 'gps_visibility' in truth else np.ones(self.m)
        self._visible = np.ascontiguousarray(np.asarray(vis) != 0, dtype=np.int32).reshape(-1)
        if self._stamps.size != self.m or self._visible.size != self.m:
            raise ValueError('gps_time / gps_visibility do not match ref_gps')
        p = self.params = _lib.LooseParams()
        p.m, p.n_list = self.m, self.runs
        p.gps_stamp, p.gps_visible = self._stamps.ctypes.data, self._visible.ctypes.data
        return table, ref_gps

    def _family_blocks(self, ref_frame, odo_err, aid, mag_err, geo_mag_n, mag):
        """The numbers of the aiding fields (aid), of the scale-factor block (scale, scalep) and of the magnetometer block (mag, magp);
        their device pointers come with the inputs and the outputs."""
        self.scalep = self.mag = self.magp = None
        if self.scale is not None:
            # what the 15-state filter is told (aid['scale']) the 16-state filter starts from (scale0); r_odo's default follows it
            aid = dict(aid, scale=self.scale['scale0'])
            if aid.get('odo_std') is None and odo_err is None:
                raise ValueError("odo_scale_state needs odo_err={'scale', 'stdv'} or aid['odo_std']")
            g = self.scalep = _lib.LooseScaleParams()
            g.scale0, g.p0_scale, g.q_k = self.scale['scale0'], self.scale['p0_scale'], self.scale['q_k']
        self.aid = aiding_model(odo_err, aid)
        for k, v in self.aid.items():
            setattr(self.params, k, v)
        if mag is not None:
            self.mag = mag_model(mag_err, geo_mag_n, ref_frame, mag)
            g = self.magp = _lib.LooseMagParams()
            g.mag_every = self.mag['mag_every']
            for k in ('mag_n', 'cal_si', 'cal_hi', 'r_mag'):
                getattr(g, k)[:] = [float(x) for x in np.asarray(self.mag[k], dtype=np.float64).reshape(-1)]

    def _standstill(self, truth, still):
        """The standstill block (still, stillp) and the device copy of its signal: the caller's still['flags'] or standstill_flags()
        of the truth."""
        self.stillp = self.still_flags = None
        if self.still is None:
            return
        flags = None if still is True else dict(still).get('flags')
        if flags is None:
            flags = standstill_flags(truth, self.still['speed'], self.still['rate'])
        flags = np.asarray(flags)
        if flags.shape != (self.n,):
            raise ValueError("still['flags'] must be (n,): one standstill signal per IMU sample")
        self.still_flags = np.ascontiguousarray(flags != 0, dtype=np.int32)
        self._bufs['still_flags'] = self.ctx.upload(self.still_flags)
        g = self.stillp = _lib.LooseStillParams()
        g.still_mask, g.still_every, g.r_zupt = self.still['still_mask'], self.still['still_every'], self.still['r_zupt']
        g.r_zaru[:] = [float(x) for x in self.still['r_zaru']]
        g.still_flags = self._bufs['still_flags'].ptr

    def _inputs(self, table, ref_gps, truth, fs, accel_err, gyro_err, gps_err, odo_err, mag_err, vib_accel, vib_gyro, given):
        """Where the lanes take their samples from, and the one upload of what they read: the initial-state table and, in the generated
        form, the truth's series behind it."""
        m, p, use_odo = self.mc, self.params, bool(self.aid['aid_mask'] & 1)
        self._ref_nav = np.ascontiguousarray(np.concatenate([truth['ref_att'], truth['ref_pos'], truth['ref_vel']], axis=1))
        m.ref_end[:] = [float(x) for x in self._ref_nav[-1]]
        need = (('accel', 3, self.n), ('gyro', 3, self.n), ('gps', 6, self.m)) + ((('odo', 1, self.n),) if use_odo else ()) + \
            ((('mag', 3, self.n),) if self.mag is not None else ())
        self._sensor_source(m, fs, accel_err, gyro_err, vib_accel, vib_gyro, given, need, 'filter')
        parts = [(m, 'ini', table.reshape(-1))]             # (block, pointer field, host array) of everything uploaded, in order
        if given is None:
            parts += self._truth_series(truth, ref_gps, gps_err, odo_err, mag_err, use_odo)
        else:
            p.in_gps = given['gps'].ptr if self.m else None
            if use_odo:
                m.in_odo = given['odo'].ptr
            if self.mag is not None:
                self.magp.in_mag = given['mag'].ptr
        buf = self._bufs['inputs'] = self.ctx.upload(np.concatenate([q for _, _, q in parts]))
        offs = np.cumsum([0] + [q.size for _, _, q in parts]) * 8
        for (block, field, q), o in zip(parts, offs):
            setattr(block, field, buf.at(o) if q.size else None)

    def _truth_series(self, truth, ref_gps, gps_err, odo_err, mag_err, use_odo):
        """The generated form: [(block, pointer field, flat host array)] of the truth's series the lanes make their samples from, in
        upload order, and the numbers of the sensors that only this form has (gps_sigma, the odometer's and the magnetometer's model)."""
        m, p = self.mc, self.params
        parts = [(m, 'ref_accel', np.asarray(truth['ref_accel'], dtype=np.float64).reshape(-1)),
                 (m, 'ref_gyro', np.asarray(truth['ref_gyro'], dtype=np.float64).reshape(-1)), (p, 'ref_gps', ref_gps.reshape(-1))]
        if self.m:
            p.gps_sigma[:] = [float(x) for x in gps_sigma(gps_err, ref_gps, self._ref_frame)]
        if use_odo:
            if 'ref_odo' not in truth or odo_err is None:
                raise ValueError("aid['odo'] in the generated form needs truth['ref_odo'] and odo_err")
            ref_odo = np.asarray(truth['ref_odo'], dtype=np.float64).reshape(-1)
            if ref_odo.size != self.n:
                raise ValueError("truth['ref_odo'] must have one value per IMU sample")
            m.odo_scale, m.odo_stdv = float(odo_err['scale']), float(odo_err['stdv'])
            parts.append((m, 'ref_odo', ref_odo))
        if self.mag is not None:
            if 'ref_mag' not in truth or mag_err is None:
                raise ValueError("mag in the generated form needs truth['ref_mag'] and mag_err")
            ref_mag = np.asarray(truth['ref_mag'], dtype=np.float64)
            if ref_mag.shape != (self.n, 3):
                raise ValueError("truth['ref_mag'] must be (n, 3): one row per IMU sample")
            g = self.magp
            g.mag_si[:] = [float(x) for x in np.asarray(mag_err['si'], dtype=np.float64).reshape(9)]
            g.mag_hi[:] = [float(x) for x in np.asarray(mag_err['hi'], dtype=np.float64) * np.ones(3)]
            g.mag_std[:] = [float(x) for x in np.asarray(mag_err['std'], dtype=np.float64) * np.ones(3)]
            parts.append((g, 'ref_mag', ref_mag.reshape(-1)))
        return parts

    def _outputs(self, placed):
        """The device buffers a launch writes: the per-run end records, the online process statistics (proc_first), the kept series
        (keep_traj) and the records of the scale-factor state."""
        m, p, R = self.mc, self.params, self.runs
        # end [9][R], bias_end [6][R], pdiag_end [15][R], run list [R], the NED end record [9][R]
        small = self._bufs['small'] = self.ctx.malloc((9 + 6 + 15 + 1 + 9) * R * 8)
        if self.end_ned:
            p.out_end_ned = small.at(31 * R * 8)
        p.out_end, p.out_bias_end, p.out_pdiag_end, self._list = small.ptr, small.at(9 * R * 8), small.at(15 * R * 8), small.at(30 * R * 8)
        if self.proc_first is not None:
            if not 0 <= int(self.proc_first) < self.n:
                raise ValueError('proc_first must be a sample index of the run')
            if self.proc_ned and self._ref_frame != 0:
                raise ValueError('NED position errors exist in ref_frame 0 only')
            m.ref_nav, m.proc_first, m.proc_pos_ned = self._nav(), int(self.proc_first), int(self.proc_ned)
            self._bufs['proc'] = self.ctx.malloc(27 * R * 8)
            p.out_proc = self._bufs['proc'].ptr
        if self.keep_traj:
            plane = self.n * R * 8
            total = 15 * plane
            self._bufs['series'] = self.ctx.malloc(total, placed=self._use_placed(placed, total))
            self._bufs['traj_loose'] = DeviceView(self._bufs['series'], 0, 9 * plane)
            self._bufs['wb'] = DeviceView(self._bufs['series'], 9 * plane, 3 * plane)
            self._bufs['ab'] = DeviceView(self._bufs['series'], 12 * plane, 3 * plane)
            p.out_traj, p.out_wb, p.out_ab = self._bufs['traj_loose'].ptr, self._bufs['wb'].ptr, self._bufs['ab'].ptr
        if self.scalep is not None:
            g = self.scalep
            # scale_end [2][R], pcross_end [15][R], and the kept series [n][R]
            self._bufs['scale'] = self.ctx.malloc((17 + (self.n if self.keep_scale else 0)) * R * 8)
            g.out_scale_end, g.out_pcross_end = self._bufs['scale'].ptr, self._bufs['scale'].at(2 * R * 8)
            if self.keep_scale:
                g.out_scale = self._bufs['scale'].at(17 * R * 8)

    def _scale_truth(self, scale_truth, given, odo_err):
        """The device copy [runs] of the scale factor's truth that the checkpoints of a filter with the scale-factor state compare
        k_est with: a scalar or (runs,); None: what the lane itself generates the odometer with (odo_err['scale']) in the generated
        form, no truth in the given form."""
        if self.scalep is None:
            return
        if scale_truth is None:
            if given is not None or odo_err is None:
                return
            scale_truth = float(odo_err['scale'])
        v = np.asarray(scale_truth, dtype=np.float64)
        if v.ndim == 0:
            v = np.full(self.runs, float(v))
        if v.shape != (self.runs,):
            raise ValueError('checkpoints: scale_truth must be a scalar or (runs,) = (%d,), one true scale factor per run' % self.runs)
        self._bufs['scale_truth'] = self.ctx.upload(np.ascontiguousarray(v))

    def _checkpoints(self, cons_samples, who='cons_samples'):
        """The checkpoint block (cons) and its record and work buffers."""
        self.cons = None
        if cons_samples is None:
            return
        asked = np.asarray(cons_samples, dtype=np.int64).reshape(-1)
        if asked.size == 0 or asked.min() < 0 or asked.max() >= self.n:
            raise ValueError('%s must be sample indices in [0, %d), at least one' % (who, self.n))
        # the kernel walks a strictly increasing list; _cons_back maps its records to the caller's order
        self._cons_samples, self._cons_back = np.unique(asked, return_inverse=True)
        self._cons_samples = np.ascontiguousarray(self._cons_samples, dtype=np.int64)
        mu, waves = self._cons_samples.size, (self.runs + 63) // 64
        self._bufs['cons'] = self.ctx.malloc((1 + waves) * mu * _lib.CONS_RECORD * 8)
        self.mc.ref_nav = self._nav()
        c = self.cons = _lib.LooseConsParams()
        c.cons_sample, c.cons_m = self._cons_samples.ctypes.data, mu
        c.out_cons, c.cons_work = self._bufs['cons'].ptr, self._bufs['cons'].at(mu * _lib.CONS_RECORD * 8)

    # ------------------------------------------------------------------ launches
    def _entry(self, what, *head):
        """The family's entry point ginsim_loose[_cons | _mag | _scale | _still | _all]_<what> and its arguments: head, the two base
        blocks, the family's block (the combined family's three, None for one the job does not hold)."""
        suffix, block = self._family
        blocks = () if block is None else block if isinstance(block, tuple) else (block,)
        args = head + (C.byref(self.mc), C.byref(self.params)) + \
            tuple(C.byref(b) if isinstance(b, C.Structure) else b for b in blocks)       # None: NULL; a device pointer as it is
        return getattr(lib, 'ginsim_loose%s_%s' % (suffix, what)), args

    def kernel_name(self):
        buf = C.create_string_buffer(256)
        fn, args = self._entry('kernel_name')
        check(fn(*(args + (buf, 256))))
        return buf.value.decode()

    def variant(self):
        v = C.c_int32(0)
        check(lib.ginsim_loose_variant(C.byref(self.mc), C.byref(self.params), C.byref(v)))
        return v.value

    def launch(self, ids=None):
        """Enqueue the kernel (asynchronous).  ids: launch these runs only (lane i filters run ids[i]); the others keep what they hold,
        and the consistency record is over the listed runs."""
        self._put_run_list(self.params, ids)
        fn, args = self._entry('run', self.ctx.handle)
        check(self.ctx.retry_oom(lambda: fn(*args)))

    def run(self, ids=None):
        self.launch(ids)
        self.ctx.sync()
        return self

    def placement(self):
        b = self._bufs.get('series')
        return {'placed': ['series'] if b is not None and b.placed else [], 'unplaced': ['series'] if b is not None and not b.placed else []}

    # ------------------------------------------------------------------ results
    def stats(self, algo='loose', ned=False):
        """End-point statistics (att3 wrapped, pos3, vel3) of the last launch.  ned: the job must have end_pos_ned=True."""
        s = _lib.Stats()
        check(lib.ginsim_end_stats(self.ctx.handle, self._end_ptr(ned), self.runs, C.byref(s)))
        return StatsResult(s)

    def _end_ptr(self, ned):
        if ned and not (self.end_ned or self.mc.end_pos_ned):
            raise ValueError('the NED end-point record was not requested (end_ned=True)')
        return self.params.out_end_ned if (ned and self.end_ned) else self.params.out_end

    def end_errors(self, algo='loose', ned=False):
        """(runs, 9) end-point errors [att3 wrapped, pos3, vel3]; ned=True: the NED record (end_ned=True)."""
        return self.ctx.download(self._end_ptr(ned), (9, self.runs)).T.copy()

    def process_stats_online(self, algo='loose'):
        """(runs, 3, 9) = max|e|, mean, std of the error over samples >= proc_first."""
        if self.proc_first is None:
            raise ValueError('online process statistics were not requested (proc_first=...)')
        return self.ctx.download(self._bufs['proc'], (3, 9, self.runs)).transpose(2, 0, 1)

    def final_biases(self):
        """(wb, ab), each (runs, 3): the bias estimates at the last sample."""
        a = self.ctx.download(self.params.out_bias_end, (6, self.runs))
        return a[0:3].T.copy(), a[3:6].T.copy()

    def final_pdiag(self):
        """(runs, 15): the diagonal of P at the last sample."""
        return self.ctx.download(self.params.out_pdiag_end, (15, self.runs)).T.copy()

    def final_sigmas(self):
        """(runs, 15): the 1 sigma of every state at the last sample, sqrt(final_pdiag()); (runs, 16) with odo_scale_state, the
        scale-factor error the last."""
        sig = np.sqrt(self.final_pdiag())
        return sig if self.scalep is None else np.concatenate([sig, self.final_scale()[1][:, None]], axis=1)

    def _need_scale(self):
        if self.scalep is None:
            raise ValueError('the filter has no scale-factor state (odo_scale_state=...)')

    def final_scale(self):
        """(k_est, sigma), each (runs,): the scale-factor estimate at the last sample and its 1 sigma, sqrt(P[15][15])."""
        self._need_scale()
        a = self.ctx.download(self.scalep.out_scale_end, (2, self.runs))
        return a[0].copy(), np.sqrt(a[1])

    def final_pcross(self):
        """(runs, 15): P[k][15], the covariance of the scale-factor error with the 15 other states, at the last sample."""
        self._need_scale()
        return self.ctx.download(self.scalep.out_pcross_end, (15, self.runs)).T.copy()

    def consistency(self):
        """ConsistencyResult of the last launch at cons_samples, in the caller's order: across the runs launched, the filter's
        mean P_kk next to the mean squared error of the navigation states in the filter's own coordinates, and the normalised
        errors (per state and per 3x3 block)."""
        if self.cons is None and self.consp is None:
            raise ValueError('the consistency record was not requested (cons_samples=...)')
        rec = self.ctx.download(self._bufs['cons'], (self._cons_samples.size, _lib.CONS_RECORD))
        return ConsistencyResult(rec[self._cons_back])

    def series(self, name, run_ids):
        """Kept series of selected runs, each (k, n, 3): 'att', 'pos', 'vel', 'wb', 'ab'; 'odo_scale' (k, n): k_est (keep_scale)."""
        if name == 'odo_scale':
            self._need_scale()
            if not self.keep_scale:
                raise ValueError('the scale-factor series was not kept (keep_scale=True)')
            return self._gather(self.scalep.out_scale, self.n, 1, run_ids)[:, :, 0]
        if not self.keep_traj:
            raise ValueError('the series were not kept (keep_traj=True)')
        plane = self.n * self.runs * 8
        if name in ('wb', 'ab'):
            return self._gather(self._bufs[name].ptr, self.n, 3, run_ids)
        k = ('att', 'pos', 'vel').index(name)
        return self._gather(self._bufs['traj_loose'].ptr + 3 * k * plane, self.n, 3, run_ids)

    def trajectories(self, algo='loose', run_ids=(0,), displacement=False):
        return tuple(self.series(k, run_ids) for k in ('att', 'pos', 'vel'))
