"""Constructed inputs that drive nav_step (csrc/nav.hpp) and Att::step (csrc/ins_math.hpp) through their rare branches: the pitch
fold over +-pi/2, the single +-2 pi wrap of yaw and roll, attitude and latitude steps on both sides of 2^-6 rad (short / long series)
and of 0.25 rad (series / exact trig), steps of 2 rad and more (where a series in place of the exact trig is off by > 1e-7), and all
of these on, one before and one after a resync step (j + 1 = 0 mod 32).  Infrastructure of tests/test_nav_branch_oracle.py (CPU) and
tests/test_gpu_nav_branches.py (device): no test in this file.

Every case is small (n <= 900 samples, <= 257 runs), names the branch events it is there for with a minimum count (`want`; a key
'free:...' holds for that algorithm only), and is
described by the sensor series every run sees, so that the same numbers go through the given-data kernels (as they are) and the
generate-mode kernels (as the truth of a zero-error IMU, which reproduces them exactly; or with the noise the case names).  The
odometer is exact (scale 1, stdv 0) everywhere: the forward speed of a run is the truth's.

The events are counted from the C oracle's trajectory (`events`): the oracle has no series and no cache, so a step's size and the
fold / wrap decisions are recomputed from its state at sample j and the rates of that sample exactly as attitude.euler_update_zyx
forms them (`steps`, checked against the oracle's own next sample in the CPU test).

Which runs are compared (`compared`): the Euler-rate integration divides by cos(pitch), so a run that comes close to the pole
amplifies rounding differences, and one that passes +-pi/2 (or +-pi) within rounding takes a branch on one side only.  A run is
compared when the oracle ALONE shows that neither happens: with the gyro series scaled by 1 + 2^-40 (60 times the largest relative
deviation the device's arithmetic admits, rcp_n1's 2^-46) no fold or wrap decision changes and no value moves by more than a tenth
of the tolerance, and pitch stays >= 1e-6 from +-pi/2, yaw and roll >= 1e-6 from +-pi, after every step (but for a yaw or roll that
sits ON +-pi: ON_PI below).  The oracle has no other
branch: which series the device rotates its cache with is not a decision of the mechanisation and may differ at a threshold row.
"""
import functools
import math

import numpy as np

from conftest import load_golden

D2R = np.pi / 180.0
ZERO = {'b': np.zeros(3), 'b_drift': np.zeros(3), 'b_corr': np.full(3, 100.0), 'arw': np.zeros(3), 'vrw': np.zeros(3)}
ODO_EXACT = {'scale': 1.0, 'stdv': 0.0}
SMALL, BIG, HUGE = 2.0 ** -6, 0.25, 2.0
UP = np.nextafter                      # UP(x, inf): the next double above x
PERTURB = 1.0 + 2.0 ** -40
MARGIN = 1e-6
# A yaw or roll that sits ON +-pi: the tumble fixture and case (a) start with roll = 0 and turn about the pitch axis alone, so the
# first fold makes the roll pi to the bit (0 + pi) and it stays within an ulp or two of it until the next fold.  Which side of the
# wrap such a step takes is decided by rounding and changes nothing that is compared: +pi and -pi are the same angle (the
# comparison is modulo 2 pi) and the trig that carries the state on differs by 1e-16.  Such steps have no margin to hold and
# their wrap decision is not among those that must not change; within (ON_PI, MARGIN) a run is left out like any other.
ON_PI = 1e-12
EVENTS = ('fold_up', 'fold_down', 'yaw_wrap_pos', 'yaw_wrap_neg', 'roll_wrap_pos', 'roll_wrap_neg', 'step_mid', 'step_big', 'step_huge',
          'on_resync', 'before_resync', 'after_resync', 'at_small', 'above_small', 'at_big', 'above_big',
          'lat_small', 'lat_mid', 'lat_big', 'lat_huge', 'lat_on_resync', 'lat_before_resync', 'lat_after_resync', 'fold_next_to_huge', 'straddle_small', 'straddle_big')


def tolerance(n):
    """SURVEY 8(c) as tests/test_gpu_fuzz.py applies it: per sample, on attitude (mod 2 pi) and on position / velocity relative to
    max(1, |x|)"""
    return 1e-9 * max(1.0, n / 1000.0)


class Case(object):
    """gyro / accel (n, 3), odo (n,): what every run sees (before the noise of gyr_err / acc_err); ini (9,) or (9, runs): one
    initial state or a table with one column per run; given_gyro (runs, n, 3): per-run series for the given-data kernels only
    (generate=False); bad: {run: first non-finite sample of its attitude}."""

    def __init__(self, name, rf, fs, gyro, accel, odo, ini, want, runs=1, off=0, seed=1, gyr_err=ZERO, acc_err=ZERO, earth_rot=True,
                 strict=True, run_counts=None, given_gyro=None, generate=True, bad=None, clean_ini=None):
        self.name, self.rf, self.fs, self.runs, self.off, self.seed = name, int(rf), float(fs), int(runs), int(off), int(seed)
        self.gyro, self.accel, self.odo = (np.ascontiguousarray(x, dtype=np.float64) for x in (gyro, accel, odo))
        self.n = self.gyro.shape[0]
        self.ini = np.asarray(ini, dtype=np.float64)
        self.want, self.gyr_err, self.acc_err, self.earth_rot, self.strict = dict(want), gyr_err, acc_err, bool(earth_rot), bool(strict)
        self.run_counts = tuple(run_counts or (self.runs,))
        self.given_gyro, self.generate, self.bad = given_gyro, bool(generate), dict(bad or {})
        self.clean_ini = clean_ini          # (f): the table without the bad run's NaN
        self.noisy = gyr_err is not ZERO or acc_err is not ZERO
        assert self.n <= 900 and self.runs <= 257
        for x in (self.gyro, self.accel, self.odo, self.ini):
            x.setflags(write=False)

    @property
    def truth(self):
        z = np.zeros((self.n, 3))
        return {'ref_accel': self.accel, 'ref_gyro': self.gyro, 'ref_odo': self.odo, 'ref_att': z, 'ref_pos': z, 'ref_vel': z}

    def ini_of(self, r):
        return self.ini if self.ini.ndim == 1 else self.ini[:, r]


# ----------------------------------------------------------------------------------------------------------------- the cases
def _case_a():
    """Pure pitch tumble in ref_frame 1, roll = 0, w_x = w_z = 0, 64 Hz: dp = w_y / 64 exactly, q = 0, so |dp| is the step's size to
    the bit.  Ordinary steps of 0.0086 .. 0.0195 rad (both sides of 2^-6) fold the pitch up, down and up again; rows 20 .. 27 and
    the rows around the resyncs at 32 and 64 carry w_y = +-1, +-nextafter(1), +-16, +-nextafter(16): steps of exactly 2^-6, the
    next double, 0.25 and the next double.  After the first fold the roll is pi to the bit (0 + pi) and stays within rounding of it
    until the next fold takes it to 0 (ON_PI)."""
    n, fs = 700, 64.0
    j = np.arange(n)
    wy = 0.9 + 0.35 * np.sin(2 * np.pi * j / 37.0)
    one, sixteen = UP(1.0, 2.0), UP(16.0, 17.0)
    special = {20: 1.0, 21: one, 22: 16.0, 23: sixteen, 24: -1.0, 25: -one, 26: -16.0, 27: -sixteen,
               30: 16.0, 31: -sixteen, 32: 1.0, 62: one, 63: sixteen, 64: -16.0, 94: 1.0, 95: 16.0, 96: one,
               300: 1.0, 301: one, 302: -16.0, 303: sixteen}
    for k, v in special.items():
        wy[k] = v
    gyro = np.stack([np.zeros(n), wy, np.zeros(n)], axis=1)
    accel = np.stack([0.3 * np.sin(j / 11.0), np.zeros(n), -9.79 + 0.1 * np.cos(j / 7.0)], axis=1)
    ini = np.array([0.6, -1.1, 120.0, 4.0, 0.1, -0.2, 0.3, 0.35, 0.0])
    want = {'fold_up': 2, 'fold_down': 1, 'step_mid': 100, 'step_big': 4, 'at_small': 4, 'above_small': 4, 'at_big': 4, 'above_big': 4,
            'on_resync': 3, 'before_resync': 3, 'after_resync': 3, 'yaw_wrap_pos': 1}
    return Case('a_pitch_thresholds', 1, fs, gyro, accel, np.full(n, 4.0), ini, want)


def _tumble():
    g = load_golden('t1_fixture_tumble')
    return g['gyro'], g['accel'], g['ini'][:9], float(g['fs'])


def _case_b(rf):
    """The rates of the tumble fixture (tests/golden/make_golden.py, t1_tumble): a fold in either direction, wraps of yaw and roll
    and steps above 2^-6 rad where the rates divide by a small cos(pitch) (0.0026 at the least)."""
    gyro, accel, ini, fs = _tumble()
    want = {'fold_up': 1, 'fold_down': 1, 'yaw_wrap_pos': 3, 'roll_wrap_pos': 1, 'step_mid': 200, 'on_resync': 8, 'before_resync': 8, 'after_resync': 8}
    return Case('b_tumble_rf%d' % rf, rf, fs, gyro, accel, np.full(gyro.shape[0], 5.0), ini, want)


RUN_COUNTS = (1, 63, 64, 65, 257)


def _case_c_ini():
    """The tumble, 257 runs, each with its own initial pitch and yaw spread over four steps' worth (4 x 0.0106 rad): neighbouring
    lanes fold and wrap at different samples.  No noise: generate mode reproduces the rates."""
    gyro, accel, ini, fs = _tumble()
    R = 257
    table = np.repeat(ini[:, None], R, axis=1)
    k = np.arange(R)
    spread = 4 * 61.0 * D2R / fs
    table[7] = ini[7] + spread * ((k * 37) % R) / R         # neighbours far apart within the spread
    table[6] = ini[6] + spread * ((k * 101) % R) / R
    want = {'fold_up': R // 2, 'fold_down': R // 2, 'yaw_wrap_pos': R // 2, 'roll_wrap_pos': R // 2, 'step_mid': 50000, 'straddle_small': 10}
    return Case('c_ini_table', 1, fs, gyro, accel, np.full(gyro.shape[0], 5.0), table, want, runs=R, strict=False, run_counts=RUN_COUNTS)


def _case_c_noise():
    """Gyro noise as in test_shard_invariance_with_steps_across_the_series_threshold (0.005 rad per step) on a pitch rate of
    +-1.06 rad/s (0.0106 rad per step: lanes on both sides of 2^-6 at every sample) that swings the pitch between -0.5 and 0.56,
    away from the pole, so that the runs stay well conditioned; a yaw rate that wraps it; six roll bursts of +-25 rad/s
    (0.25 rad per step +- the noise: lanes on both sides of 0.25 within a wavefront).  ref_frame 0, runs offset beyond 2^32."""
    n, fs = 600, 100.0
    j = np.arange(n)
    gyro = np.stack([np.zeros(n), 1.06 * np.where((j // 100) % 2 == 0, 1.0, -1.0), np.full(n, 0.7)], axis=1)
    for k, sign in ((50, 1.0), (131, -1.0), (159, 1.0), (160, -1.0), (161, 1.0), (290, -1.0)):       # the roll stays within 0.25 rad of 0
        gyro[k, 0] = 25.0 * sign
    accel = np.stack([0.3 * np.sin(j / 30.0), 0.2 * np.cos(j / 17.0), -9.794 + 0.1 * np.sin(j / 9.0)], axis=1)
    ini = np.array([32.0 * D2R, 120.0 * D2R, 0.0, 5.0, 0.0, 0.0, 170.0 * D2R, -0.5, 0.0])
    gyr = {'b': np.zeros(3), 'b_drift': np.full(3, 2e-3), 'b_corr': np.full(3, 50.0), 'arw': np.full(3, 0.05)}
    acc = {'b': np.zeros(3), 'b_drift': np.full(3, 1e-3), 'b_corr': np.full(3, 50.0), 'vrw': np.full(3, 1e-2)}
    want = {'yaw_wrap_pos': 200, 'step_mid': 10000, 'step_big': 400, 'on_resync': 257, 'straddle_small': 300, 'straddle_big': 4}
    return Case('c_gyro_noise', 0, fs, gyro, accel, np.full(n, 5.0), ini, want, runs=257, off=2 ** 32 + 5, seed=5, gyr_err=gyr, acc_err=acc,
                strict=False, run_counts=RUN_COUNTS)


def _case_d(rf, fs, s, rows, want):
    """Attitude steps of 2 rad and more: rates of 2 .. 4 rad/s at 1 Hz (4 .. 6 at 2 Hz) on single rows of a slow motion, among them
    the rows around the resync at j + 1 = 32 and the row of a pitch fold and the one after it.  The series the device would rotate
    its cache with are off by 1.3e-6 (sin) and 1.9e-7 (cos) at 2 rad: the exact trig must be taken.  rows: {sample: (axis, step in
    rad)}; s: the direction of the fold.  Few rows: every step of 2 rad multiplies a perturbation of the body velocity by ~2.4
    (forward Euler of w x v), and the conditioning check allows ~100 in all."""
    n = 40
    dt = 1.0 / fs
    j = np.arange(n)
    gyro = np.stack([0.01 * np.sin(j / 5.0), 0.015 * np.cos(j / 9.0), 0.012 * np.sin(j / 7.0 + 1.0)], axis=1) / dt
    for k, (axis, step) in rows.items():
        gyro[k, axis] = step / dt
    accel = np.stack([0.2 * np.sin(j / 3.0), 0.1 * np.cos(j / 4.0), np.full(n, -9.8)], axis=1)
    ini = np.array([0.7, 0.3, 50.0, 0.3, 0.0, 0.0, 0.4, -0.2 * s, 0.1])
    return Case('d_big_steps_rf%d_%gHz' % (rf, fs), rf, fs, gyro, accel, np.full(n, 3.0), ini, want)


def _case_e(tag, fs, n, want, lat=-1.2):
    """Latitude steps in ref_frame 0: 7 km/s northwards at sampling rates far below 1 Hz, zero gyro, both algorithms."""
    ini = np.array([lat, 0.5, 1000.0, 7000.0, 0.0, 0.0, 0.1, 0.05, -0.03])
    accel = np.tile(np.array([0.0, 0.0, -9.8]), (n, 1))
    return Case('e_latitude_' + tag, 0, fs, np.zeros((n, 3)), accel, np.full(n, 7000.0), ini, want)


def _case_f_given():
    """Given data with one NaN and one Inf gyro sample: run 7 has NaN on all three axes at sample 40 (the step's size is NaN: it must
    take the exact branch), run 41 has +Inf on the roll axis at sample 41.  65 runs on the table of c_ini_table, 120 samples: the
    first fold of the neighbours falls on samples 17 .. 21, the bad samples among ordinary steps."""
    c = _case_c_ini()
    R, n = 65, 120
    gyro = np.tile(c.gyro[:n], (R, 1, 1))
    gyro[7, 40, :] = np.nan
    gyro[41, 41, 0] = np.inf
    want = {'fold_up': 32}
    return Case('f_given_nan_inf', 1, c.fs, c.gyro[:n], c.accel[:n], c.odo[:n], c.ini[:, :R], want, runs=R, strict=False, run_counts=(R,),
                given_gyro=gyro, generate=False, bad={7: 41, 41: 42})


def _case_f_ini():
    """A NaN initial attitude (all three angles) for run 33 of an ini table of 65 runs: its attitude and velocity are NaN from sample
    0, its position (the previous velocity times dt) from sample 1; its neighbours fold around sample 20."""
    c = _case_c_ini()
    R, n = 65, 120
    table = c.ini[:, :R].copy()
    clean = table.copy()
    table[6:9, 33] = np.nan
    want = {'fold_up': 32}
    return Case('f_ini_nan', 1, c.fs, c.gyro[:n], c.accel[:n], c.odo[:n], table, want, runs=R, strict=False, run_counts=(R,), bad={33: 0},
                clean_ini=clean)


@functools.lru_cache(maxsize=None)
def cases():
    out = [_case_a(), _case_b(0), _case_b(1), _case_c_ini(), _case_c_noise(), _case_d(1, 2.0, 1.0, {14: (1, 2.6), 30: (0, 0.4), 31: (0, -3.0), 32: (0, 2.3)},
                   {'step_huge': 3, 'step_big': 4, 'on_resync': 1, 'before_resync': 1, 'after_resync': 1, 'fold_up': 1, 'fold_next_to_huge': 1}),
           _case_d(0, 1.0, -1.0, {14: (1, -2.6), 15: (0, 2.4), 30: (0, 2.1), 31: (0, -3.0), 32: (0, 2.3), 33: (0, 2.6)},
                   {'step_huge': 6, 'step_big': 6, 'on_resync': 1, 'before_resync': 1, 'after_resync': 1, 'fold_down': 1, 'fold_next_to_huge': 2}),
           _case_e('small_mid', 2.0 ** -4, 40, {'lat_mid': 10, 'lat_small': 10}),
           _case_e('resync', 2.0 ** -6, 40, {'lat_mid': 20, 'free:lat_on_resync': 1, 'free:lat_before_resync': 1, 'free:lat_after_resync': 1}),
           _case_e('mid', 2.0 ** -6, 30, {'lat_mid': 15}),
           _case_e('big', 2.0 ** -8, 9, {'lat_mid': 1, 'lat_big': 1}),
           _case_e('huge', 2.0 ** -11, 3, {'lat_huge': 1, 'lat_big': 1}, lat=-1.1),      # the second step uses what the first left in the cache
           _case_f_given(), _case_f_ini()]
    return {c.name: c for c in out}


NAMES = ('a_pitch_thresholds', 'b_tumble_rf0', 'b_tumble_rf1', 'c_ini_table', 'c_gyro_noise', 'd_big_steps_rf1_2Hz', 'd_big_steps_rf0_1Hz',
         'e_latitude_small_mid', 'e_latitude_resync', 'e_latitude_mid', 'e_latitude_big', 'e_latitude_huge', 'f_given_nan_inf', 'f_ini_nan')
ALGOS = ('free', 'odo')


# ----------------------------------------------------------------------------------------------------------------- the oracle
@functools.lru_cache(maxsize=None)
def sensors(name):
    """(gyro, accel) as every run's kernel sees them, (runs, n, 3) each: the C oracle's own sensor series (the truth itself for a
    zero-error IMU), or the given per-run series"""
    from oracle import c_oracle
    c = cases()[name]
    if c.given_gyro is not None:
        gyro, accel = c.given_gyro, np.tile(c.accel, (c.runs, 1, 1))
    elif not c.noisy:
        gyro, accel = np.tile(c.gyro, (c.runs, 1, 1)), np.tile(c.accel, (c.runs, 1, 1))
    else:
        _, _, sens = c_oracle.mc_run(c.seed, c.off, c.runs, c.fs, c.rf, c.truth, c.acc_err, c.gyr_err, c.ini, odo_err=ODO_EXACT,
                                     earth_rot=c.earth_rot, keep=c.runs)
        gyro, accel = np.ascontiguousarray(sens[:, :, 3:6]), np.ascontiguousarray(sens[:, :, 0:3])
    gyro.setflags(write=False)
    accel.setflags(write=False)
    return gyro, accel


@functools.lru_cache(maxsize=None)
def oracle_given(name, algo, scale=1.0):
    """oracle_free_integration run by run on `sensors` (the gyro series times `scale`): (runs, n, 9) = att3, pos3, vel3"""
    from oracle import c_oracle
    c = cases()[name]
    gyro, accel = sensors(name)
    out = np.empty((c.runs, c.n, 9))
    for r in range(c.runs):
        att, pos, vel = c_oracle.free_integration(c.rf, c.fs, gyro[r] * scale, accel[r] if algo == 'free' else None, c.ini_of(r),
                                                  earth_rot=c.earth_rot, odo=c.odo if algo == 'odo' else None)
        out[r, :, 0:3], out[r, :, 3:6], out[r, :, 6:9] = att, pos, vel
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_mc(name, algo):
    """oracle_mc_run on the case as the generate-mode kernels get it: (end-point records (runs, 9), trajectories (runs, n, 9))"""
    from oracle import c_oracle
    c = cases()[name]
    end, traj, _ = c_oracle.mc_run(c.seed, c.off, c.runs, c.fs, c.rf, c.truth, c.acc_err, c.gyr_err, c.ini, algo=algo, odo_err=ODO_EXACT,
                                   earth_rot=c.earth_rot, keep=c.runs)
    end.setflags(write=False)
    traj.setflags(write=False)
    return end, traj


@functools.lru_cache(maxsize=None)
def oracle_numpy(name, algo):
    from oracle import ins_np
    c = cases()[name]
    gyro, accel = sensors(name)
    ini = c.ini if c.ini.ndim == 2 else np.repeat(c.ini[:, None], c.runs, axis=1)
    with np.errstate(all='ignore'):
        att, pos, vel = ins_np.free_integration(c.rf, c.fs, gyro, accel, ini, earth_rot=c.earth_rot,
                                                odo=np.tile(c.odo, (c.runs, 1)) if algo == 'odo' else None)
    return np.concatenate([att, pos, vel], axis=2)


def steps(c, traj, gyro):
    """The step from every sample j to j + 1 as attitude.euler_update_zyx (attitude.py:679-721) and the ref_frame 0 position update
    (free_integration.py:134-172) form it from the oracle's state at j: a dict of (runs, n - 1) arrays -- dy, dp, dr, the raw angles
    before the fold and the wraps, the fold / wrap decisions, the attitude after them, and dlat."""
    from oracle import ins_np
    dt = 1.0 / c.fs
    att, pos, vel = traj[:, :-1, 0:3], traj[:, :-1, 3:6], traj[:, :-1, 6:9]
    w = gyro[:, :-1]
    dlat = np.zeros(att.shape[:2])
    with np.errstate(all='ignore'):
        if c.rf == 0:
            rm, rn, _, sl, cl = ins_np.geo_param(pos[..., 0], pos[..., 2])
            rm_e, rn_e = rm + pos[..., 2], rn + pos[..., 2]
            w_en = np.stack([vel[..., 1] / rn_e, -vel[..., 0] / rm_e, -vel[..., 1] * sl / cl / rn_e], axis=-1)
            w_ie = np.zeros_like(w_en)
            if c.earth_rot:
                w_ie[..., 0], w_ie[..., 2] = ins_np.W_IE * cl, -ins_np.W_IE * sl
            w = w - np.einsum('rnij,rnj->rni', ins_np.dcm_zyx(att), w_en + w_ie)
            dlat = vel[..., 0] / rm_e * dt
        cr, sr = np.cos(att[..., 2]), np.sin(att[..., 2])
        q = w[..., 2] * cr + w[..., 1] * sr
        dy = q / np.cos(att[..., 1]) * dt
        dp = (w[..., 1] * cr - w[..., 2] * sr) * dt
        dr = (w[..., 0] + q * np.tan(att[..., 1])) * dt
        y, p, r = att[..., 0] + dy, att[..., 1] + dp, att[..., 2] + dr
        up, down = p > ins_np.HALF_PI, p < -ins_np.HALF_PI
        fold = up | down
        p2 = np.where(up, math.pi - p, np.where(down, -math.pi - p, p))
        y2, r2 = np.where(fold, y + math.pi, y), np.where(fold, r + math.pi, r)
        s = {'dy': dy, 'dp': dp, 'dr': dr, 'big': np.fmax(np.abs(dy), np.fmax(np.abs(dp), np.abs(dr))), 'dlat': dlat,
             'fold_up': up, 'fold_down': down, 'yaw_wrap_pos': y2 > math.pi, 'yaw_wrap_neg': y2 < -math.pi,
             'roll_wrap_pos': r2 > math.pi, 'roll_wrap_neg': r2 < -math.pi,
             'margin_pitch': np.abs(np.abs(p) - ins_np.HALF_PI), 'margin_yaw': np.abs(np.abs(y2) - math.pi),
             'margin_roll': np.abs(np.abs(r2) - math.pi)}
        s['next'] = np.stack([np.where(s['yaw_wrap_pos'], y2 - ins_np.TWO_PI, np.where(s['yaw_wrap_neg'], y2 + ins_np.TWO_PI, y2)), p2,
                              np.where(s['roll_wrap_pos'], r2 - ins_np.TWO_PI, np.where(s['roll_wrap_neg'], r2 + ins_np.TWO_PI, r2))], axis=-1)
    return s


DECISIONS = ('fold_up', 'fold_down', 'yaw_wrap_pos', 'yaw_wrap_neg', 'roll_wrap_pos', 'roll_wrap_neg')


def events(c, s, runs=None):
    """Counts of the branch events over the runs `runs` (a boolean mask; default all) of the steps `s`.  An event 'on / before /
    after resync' is a fold, a wrap or a step above 2^-6 rad whose j + 1 is 0 / 31 / 1 mod 32."""
    m = np.ones(s['big'].shape[0], dtype=bool) if runs is None else np.asarray(runs, dtype=bool)
    k = np.arange(1, s['big'].shape[1] + 1)[None, :]
    big, dlat = s['big'], np.abs(s['dlat'])
    ev = {name: s[name] for name in DECISIONS}
    ev['step_mid'] = (big > SMALL) & (big <= BIG)
    ev['step_big'] = big > BIG
    ev['step_huge'] = big >= HUGE
    ev['at_small'], ev['above_small'] = big == SMALL, big == UP(SMALL, 1.0)
    ev['at_big'], ev['above_big'] = big == BIG, big == UP(BIG, 1.0)
    rare = ev['fold_up'] | ev['fold_down'] | ev['yaw_wrap_pos'] | ev['yaw_wrap_neg'] | ev['roll_wrap_pos'] | ev['roll_wrap_neg'] | (big > SMALL)
    ev['on_resync'], ev['before_resync'], ev['after_resync'] = rare & (k % 32 == 0), rare & (k % 32 == 31), rare & (k % 32 == 1)
    ev['lat_small'] = (dlat > 0.0) & (dlat <= SMALL)
    ev['lat_mid'] = (dlat > SMALL) & (dlat <= BIG)
    ev['lat_big'] = dlat > BIG
    ev['lat_huge'] = dlat >= HUGE
    lat_rare = dlat > SMALL
    ev['lat_on_resync'], ev['lat_before_resync'], ev['lat_after_resync'] = lat_rare & (k % 32 == 0), lat_rare & (k % 32 == 31), lat_rare & (k % 32 == 1)
    fold = ev['fold_up'] | ev['fold_down']
    near = fold.copy()
    near[:, 1:] |= fold[:, :-1]
    near[:, :-1] |= fold[:, 1:]
    ev['fold_next_to_huge'] = near & ev['step_huge']
    # samples at which the runs counted lie on both sides of a threshold (a wavefront holds 64 neighbours of them)
    for key, thr in (('straddle_small', SMALL), ('straddle_big', BIG)):
        ev[key] = np.zeros(big.shape, dtype=bool)
        if m.any():             # counted once per sample: on the row of the first run counted
            ev[key][np.flatnonzero(m)[0]] = (big[m] <= thr).any(axis=0) & (big[m] > thr).any(axis=0)
    return {name: int(np.sum(v[m])) for name, v in ev.items()}


def ratio(got, ref, n):
    """error / tolerance of every run: (runs, n, 9) against (runs, n, 9) -> (runs,).  NaN where either side is not finite."""
    with np.errstate(all='ignore'):
        d_att = np.abs(np.mod(got[..., 0:3] - ref[..., 0:3] + np.pi, 2 * np.pi) - np.pi)
        d_pv = np.abs(got[..., 3:9] - ref[..., 3:9]) / np.maximum(1.0, np.abs(ref[..., 3:9]))
        worst = np.maximum(d_att.max(axis=(1, 2)), d_pv.max(axis=(1, 2)))
    return worst / tolerance(n)


@functools.lru_cache(maxsize=None)
def conditioning(name, algo):
    """The oracle alone, per run: (moved / tolerance under the 1 + 2^-40 gyro, the decisions all held, the smallest margin)"""
    c = cases()[name]
    gyro, _ = sensors(name)
    base, pert = oracle_given(name, algo), oracle_given(name, algo, PERTURB)
    s0, s1 = steps(c, base, gyro), steps(c, pert, gyro * PERTURB)
    on_pi = {'yaw': s0['margin_yaw'] <= ON_PI, 'roll': s0['margin_roll'] <= ON_PI}
    held = np.ones(c.runs, dtype=bool)
    for d in DECISIONS:
        same = s0[d] == s1[d]
        if not d.startswith('fold'):
            same = same | on_pi[d.split('_')[0]]
        held &= np.all(same, axis=1)
    with np.errstate(all='ignore'):
        margins = [s0['margin_pitch'], np.where(on_pi['yaw'], np.inf, s0['margin_yaw']), np.where(on_pi['roll'], np.inf, s0['margin_roll'])]
        margin = np.min([np.min(x, axis=1) for x in margins], axis=0)
    return ratio(pert, base, c.n), held, margin


@functools.lru_cache(maxsize=None)
def compared(name, algo):
    """The runs whose every sample is compared with the oracle.  The bad runs of (f) are never among them: they are held to the
    oracle's non-finite pattern instead."""
    c = cases()[name]
    moved, held, margin = conditioning(name, algo)
    ok = (moved <= 0.1) & held & (margin >= MARGIN)
    for r in c.bad:
        ok[r] = False
    ok.setflags(write=False)
    return ok
