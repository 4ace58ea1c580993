"""The reference's loosely coupled GPS/INS plugin on the GPU: ``InsLoose`` (demo_algorithms/ins_loose.py) with the same
``input`` / ``output`` / ``batch`` and ``run`` / ``get_results`` / ``reset``.

The reference declares the interface and leaves ``prediction`` and ``correction`` as ``pass``; this class fills them in with a
15-state closed-loop error-state Kalman filter (csrc/ins_loose.hip, ginsim.InsLooseJob; the equations are in DESIGN 4.11 and,
as NumPy, in tests/ins_loose_ref.py).  ``Sim`` runs an instance (``mc_algo`` 'loose') over all Monte-Carlo runs in one launch,
every lane making its own IMU samples and GPS fixes; ``run(set_of_input)`` on one logged series runs the same kernel on that series.
The checkout's own stub (demo_algorithms.ins_loose) stays hosted.  fp64 only.

    InsLoose(ini_pos_vel_att=None, earth_rot=True, ref_frame=None, imu=None, q_scale=1.0, p0=None,
             odo=False, nhc=False, odo_every=1, odo_std=None, nhc_std=0.05, odo_scale=None,
             mag=False, mag_every=1, mag_std=None, mag_si=None, mag_hi=None, geo_mag_n=None,
             odo_scale_state=False, odo_scale0=1.0, odo_scale_p0=0.02, odo_scale_q=0.0,
             zupt=False, zaru=False, still_every=1, still_speed=0.01, still_rate=2e-4, zupt_std=0.02, zaru_std=None,
             standstill=None, combined=False)

ini_pos_vel_att: the initial states FreeIntegration takes ((9|10,) or (9|10, k)); None under a Sim: the motion definition's.
imu: the IMU model the filter is tuned to (its accel_err, gyro_err, gps_err); None under a Sim: the Sim's own.  ref_frame is the
Sim's under a Sim and needed by ``run`` on a logged series.
q_scale multiplies the process noise; p0 = (sigma_r [m], sigma_v [m/s], sigma_psi [rad], sigma_bg [rad/s], sigma_ba [m/s^2]), the
initial 1 sigma; default (1e-3, 1e-3, 1e-5, 1e-7, 1e-5), the two bias terms raised to the sensor's largest constant bias.

The two aids of a land vehicle (csrc/ins_loose_aided.hip; as NumPy in tests/ins_loose_ref.py):
odo=True uses the odometer (``input`` gains a trailing 'odo'; the IMU model needs odo=True), nhc=True the non-holonomic constraints
(no sideways and no vertical body velocity), both every odo_every IMU samples.  odo_std [m/s]: 1 sigma of the scaled odometer
sample (default: the IMU model's odo_err['stdv'] / scale); nhc_std [m/s]: the constraints' pseudo-noise; odo_scale: the scale
factor the filter assumes (default: the IMU model's odo_err['scale']).

The magnetometer (csrc/ins_loose_mag.hip; as NumPy in tests/ins_loose_ref.py): mag=True observes the attitude
error with the three axes of the calibrated magnetometer sample every mag_every IMU samples (``input`` gains a trailing 'mag', after
'odo'; the IMU model needs axis=9).  mag_std [uT]: 1 sigma of the raw sample per axis; mag_si (3, 3), mag_hi (3,): the soft- and
hard-iron calibration the filter assumes (defaults: the IMU model's mag_err; MagCal's result can be passed).  geo_mag_n [uT, NED]:
the field the filter assumes; None under a Sim: the Sim's own.  ``run`` on a logged series needs it.

The odometer's scale factor as a state (csrc/ins_loose_scale.hip; as NumPy in tests/ins_loose_scale_ref.py):
odo_scale_state=True (needs odo=True) makes the scale factor the filter's 16th state instead of a number the user must know: the
estimate starts at odo_scale0 with the 1 sigma odo_scale_p0, is learnt while GPS is visible and used through an outage;
odo_scale_q [1/sqrt(s)] lets it wander (default 0: a constant).  ``output`` gains a trailing 'odo_scale', the estimate at every
sample.  odo_scale= belongs to the filter without the state and is an error with it; together with mag=True through combined=True (below).

Standstill (csrc/ins_loose_still.hip; as NumPy in tests/ins_loose_ref.py): zupt=True tells the filter that
the velocity is zero, zaru=True that the gyroscope reads its own bias (plus the earth rate the mechanisation assumes), at every
still_every-th IMU sample that the standstill signal marks.  The signal is standstill= (n,), one flag per IMU sample (a vehicle's
own signal), or, under a Sim, the Sim's truth: |velocity| <= still_speed [m/s] and |angular rate| <= still_rate [rad/s].  ``run`` on
a logged series has no truth and needs standstill=.  zupt_std [m/s], zaru_std [rad/s, per axis or one number]: the 1 sigma of the
two pseudo-measurements (zaru_std default: the per-sample gyro noise of the filter's own model).  ``input`` and ``output`` are
unchanged.  Together with mag=True or odo_scale_state=True through combined=True (below).

All of them together (csrc/ins_loose_all.hip; as NumPy in tests/ins_loose_all_ref.py): combined=True lifts the three
"not together" rules above.  A plugin with two or three of mag=True, odo_scale_state=True and zupt / zaru then runs one kernel
with every block, in the order GPS fix, odometer / constraints, magnetometer, standstill at a sample; ``input`` and ``output`` are
the union of what the options add ('odo', 'mag'; 'odo_scale').  With one of them or none, combined=True changes nothing.
odo_scale_state=True still needs odo=True; Sim.consistency_curve_any_family takes such a plugin.
"""
import numpy as np

VERSION = '1.0'


class InsLoose(object):
    '''
    Loosely coupled INS algorithm (ins_loose.py:20-36), run on the GPU.
    '''
    mc_algo = 'loose'

    def __init__(self, ini_pos_vel_att=None, earth_rot=True, ref_frame=None, imu=None, q_scale=1.0, p0=None,
                 odo=False, nhc=False, odo_every=1, odo_std=None, nhc_std=0.05, odo_scale=None,
                 mag=False, mag_every=1, mag_std=None, mag_si=None, mag_hi=None, geo_mag_n=None,
                 odo_scale_state=False, odo_scale0=1.0, odo_scale_p0=0.02, odo_scale_q=0.0,
                 zupt=False, zaru=False, still_every=1, still_speed=0.01, still_rate=2e-4, zupt_std=0.02, zaru_std=None, standstill=None,
                 combined=False):
        self.combined = bool(combined)
        self.odo, self.nhc, self.mag = bool(odo), bool(nhc), bool(mag)
        self.zupt, self.zaru = bool(zupt), bool(zaru)
        self.still = {'zupt': self.zupt, 'zaru': self.zaru, 'every': still_every, 'speed': still_speed, 'rate': still_rate,
                      'zupt_std': zupt_std, 'zaru_std': zaru_std}
        self.standstill = None if standstill is None else np.ascontiguousarray(np.asarray(standstill).reshape(-1) != 0, dtype=np.int32)
        if self.zupt or self.zaru:
            if self.mag and not self.combined:
                raise ValueError('zupt / zaru together with mag=True is not built')
            if odo_scale_state and not self.combined:
                raise ValueError('zupt / zaru together with odo_scale_state=True is not built')
            from ginsim.ins_loose import still_model
            still_model({'q_psi': np.ones(3)}, 1.0, self.still)         # the errors of the numbers
        self.odo_scale_state = bool(odo_scale_state)
        if self.odo_scale_state:
            if not self.odo:
                raise ValueError('odo_scale_state=True needs odo=True: a scale-factor state without the odometer is refused')
            if odo_scale is not None:
                raise ValueError('odo_scale= is the scale factor the filter WITHOUT the state assumes; with odo_scale_state=True the '
                                 'filter estimates it: give the starting value as odo_scale0=')
            if self.mag and not self.combined:
                raise ValueError('odo_scale_state=True together with mag=True is not built')
            from ginsim.ins_loose import scale_model
            scale_model(None, {'scale0': odo_scale0, 'p0': odo_scale_p0, 'q': odo_scale_q}, 1.0)        # the errors of the three numbers
        self.odo_scale0, self.odo_scale_p0, self.odo_scale_q = float(odo_scale0), float(odo_scale_p0), float(odo_scale_q)
        self.input = ['fs', 'gyro', 'accel', 'time', 'gps_time', 'gps'] + (['odo'] if self.odo else []) + (['mag'] if self.mag else [])
        self.output = ['pos', 'vel', 'att_euler', 'wb', 'ab'] + (['odo_scale'] if self.odo_scale_state else [])
        self.batch = True
        self.results = None
        self.ini = None if ini_pos_vel_att is None else np.array(ini_pos_vel_att, dtype=np.float64)
        self.earth_rot, self.ref_frame, self.imu = bool(earth_rot), ref_frame, imu
        self.q_scale = float(q_scale)
        if p0 is not None:
            p0 = tuple(float(x) for x in np.asarray(p0, dtype=np.float64).reshape(-1))
            if len(p0) != 5 or not all(x > 0.0 and np.isfinite(x) for x in p0):
                raise ValueError('p0 = (sigma_r, sigma_v, sigma_psi, sigma_bg, sigma_ba), five positive numbers')
        if not (self.q_scale > 0.0 and np.isfinite(self.q_scale)):
            raise ValueError('q_scale must be positive')
        self.p0 = p0
        if int(odo_every) != odo_every or int(odo_every) < 1:
            raise ValueError('odo_every must be an integer >= 1')
        for name, v, optional in (('odo_std', odo_std, True), ('nhc_std', nhc_std, False), ('odo_scale', odo_scale, True)):
            if not (optional and v is None) and not (float(v) > 0.0 and np.isfinite(float(v))):
                raise ValueError('%s must be positive' % name)
        self.odo_every, self.nhc_std = int(odo_every), float(nhc_std)
        self.odo_std = None if odo_std is None else float(odo_std)
        self.odo_scale = None if odo_scale is None else float(odo_scale)
        if int(mag_every) != mag_every or int(mag_every) < 1:
            raise ValueError('mag_every must be an integer >= 1')
        self.mag_every = int(mag_every)

        def numbers(name, v, size, positive=False):
            if v is None:
                return None
            v = np.asarray(v, dtype=np.float64)
            v = v * np.ones(3) if (positive and v.size == 1) else v
            if v.size != size or not np.all(np.isfinite(v)) or (positive and not np.all(v > 0.0)):
                raise ValueError('%s must be %d finite%s numbers' % (name, size, ', positive' if positive else ''))
            return v.copy()
        self.mag_std = numbers('mag_std', mag_std, 3, True)
        self.mag_si = numbers('mag_si', mag_si, 9)
        self.mag_si = None if self.mag_si is None else self.mag_si.reshape(3, 3)
        self.mag_hi = numbers('mag_hi', mag_hi, 3)
        self.geo_mag_n = numbers('geo_mag_n', geo_mag_n, 3)
        self.run_times = 0

    def aid(self):
        """The aiding options ginsim.InsLooseJob takes (ginsim.ins_loose.aiding_model), or None without aiding."""
        if not (self.odo or self.nhc):
            return None
        return {'odo': self.odo, 'nhc': self.nhc, 'every': self.odo_every, 'odo_std': self.odo_std, 'nhc_std': self.nhc_std,
                'scale': self.odo_scale}

    def mag_options(self):
        """The magnetometer options ginsim.InsLooseJob takes (ginsim.ins_loose.mag_model), or None without the magnetometer."""
        if not self.mag:
            return None
        return {'every': self.mag_every, 'std': self.mag_std, 'si': self.mag_si, 'hi': self.mag_hi}

    def scale_options(self):
        """The options of the scale-factor state ginsim.InsLooseJob takes (ginsim.ins_loose.scale_model), or None without it."""
        if not self.odo_scale_state:
            return None
        return {'scale0': self.odo_scale0, 'p0': self.odo_scale_p0, 'q': self.odo_scale_q}

    def still_options(self):
        """The standstill options ginsim.InsLooseJob takes (ginsim.ins_loose.still_model), or None without zupt and zaru; 'flags' is
        the plugin's standstill= (None: the job derives the signal from its truth)."""
        if not (self.zupt or self.zaru):
            return None
        return dict(self.still, flags=self.standstill)

    def finish(self, pos, vel, att, wb, ab, odo_scale=None):
        """State the plugin holds after a run: the last run's series, each (n, 3), in the order of `output`; with
        odo_scale_state the estimate's series (n,) the last."""
        self.results = [pos, vel, att, wb, ab] + ([odo_scale] if self.odo_scale_state else [])

    def run(self, set_of_input):
        '''
        set_of_input: [fs, gyro (n, 3), accel (n, 3), time (n,), gps_time (m,), gps (m, 6 | 7)], as the reference's run; a seventh
        gps column is the visibility; with InsLoose(odo=True) a seventh element, odo (n,); with InsLoose(mag=True) the next
        element, mag (n, 3), and geo_mag_n= on the plugin.  Needs InsLoose(ini_pos_vel_att=..., ref_frame=..., imu=...), and with
        zupt / zaru InsLoose(standstill=...) (n,).
        '''
        import ginsim
        from ginsim.ins_loose import InsLooseJob
        if self.ini is None or self.ref_frame not in (0, 1) or self.imu is None:
            raise ValueError('InsLoose.run on a logged series needs InsLoose(ini_pos_vel_att=..., ref_frame=0 | 1, imu=...): '
                             'there is no Sim to take them from')
        if (self.zupt or self.zaru) and self.standstill is None:
            raise ValueError('InsLoose(zupt / zaru).run on a logged series needs InsLoose(standstill=flags (n,)): there is no truth to '
                             'derive the standstill signal from')
        fs = float(np.asarray(set_of_input[0]).reshape(-1)[0])
        gyro = np.ascontiguousarray(np.asarray(set_of_input[1], dtype=np.float64))
        accel = np.ascontiguousarray(np.asarray(set_of_input[2], dtype=np.float64))
        time = np.asarray(set_of_input[3], dtype=np.float64).reshape(-1)
        gps_time = np.asarray(set_of_input[4], dtype=np.float64).reshape(-1)
        gps = np.asarray(set_of_input[5], dtype=np.float64).reshape(gps_time.shape[0], -1)
        n = gyro.shape[0]
        if gyro.shape != (n, 3) or accel.shape != (n, 3) or gps.shape[1] < 6:
            raise ValueError('gyro and accel must be (n, 3) arrays, gps (m, 6)')
        odo = None
        if self.odo:
            if len(set_of_input) < 7:
                raise ValueError("InsLoose(odo=True).run needs the odometer series as the seventh element ('odo')")
            odo = np.ascontiguousarray(np.asarray(set_of_input[6], dtype=np.float64).reshape(-1))
            if odo.shape[0] != n:
                raise ValueError('odo must be an (n,) array')
        mag = None
        if self.mag:
            at = 7 if self.odo else 6
            if len(set_of_input) <= at:
                raise ValueError("InsLoose(mag=True).run needs the magnetometer series as element %d ('mag')" % (at + 1))
            if self.geo_mag_n is None:
                raise ValueError('InsLoose(mag=True).run on a logged series needs InsLoose(geo_mag_n=[bx, by, bz] uT): there is no Sim '
                                 'to take the field from')
            mag = np.ascontiguousarray(np.asarray(set_of_input[at], dtype=np.float64))
            if mag.shape != (n, 3):
                raise ValueError('mag must be an (n, 3) array')
        t0 = time[0] if time.size else 0.0
        truth = {'ref_accel': accel, 'ref_gyro': gyro, 'ref_att': np.zeros((n, 3)), 'ref_pos': np.zeros((n, 3)), 'ref_vel': np.zeros((n, 3)),
                 'ref_gps': np.ascontiguousarray(gps[:, 0:6]), 'gps_time': gps_time - t0,
                 'gps_visibility': gps[:, 6] if gps.shape[1] > 6 else np.ones(gps.shape[0])}
        ctx = ginsim.default_context()
        bufs = {'accel': ctx.upload(np.ascontiguousarray(accel.T)), 'gyro': ctx.upload(np.ascontiguousarray(gyro.T)),       # [3][n][1]
                'gps': ctx.upload(np.ascontiguousarray(gps[:, 0:6].T))}
        if odo is not None:
            bufs['odo'] = ctx.upload(odo)                                                                                   # [n][1]
        if mag is not None:
            bufs['mag'] = ctx.upload(np.ascontiguousarray(mag.T))                                                           # [3][n][1]
        job = None
        try:
            job = InsLooseJob(ctx, fs, self.ref_frame, truth, self.imu.accel_err, self.imu.gyro_err, self.imu.gps_err, self.ini, 1,
                              ini_first=self.run_times, earth_rot=self.earth_rot, given=bufs, q_scale=self.q_scale, p0=self.p0,
                              keep_traj=True, odo_err=getattr(self.imu, 'odo_err', None), aid=self.aid(),
                              **self._mag_arguments(), **self._scale_arguments(), **self._still_arguments(),
                              **self.combined_arguments()).run()
            self.finish(*[job.series(k, [0])[0] for k in ('pos', 'vel', 'att', 'wb', 'ab') + (('odo_scale',) if self.odo_scale_state else ())])
        finally:
            if job is not None:
                job.release()
            for b in bufs.values():
                b.free()
        self.run_times += 1

    def combined_arguments(self):
        """The keyword of ginsim.InsLooseJob that lets it hold several of the magnetometer block, the scale-factor state and the
        standstill block; nothing for a plugin made without combined=True."""
        return {'combined': True} if self.combined else {}

    def _mag_arguments(self):
        return {} if not self.mag else {'mag_err': getattr(self.imu, 'mag_err', None), 'geo_mag_n': self.geo_mag_n, 'mag': self.mag_options()}

    def _still_arguments(self):
        return {} if not (self.zupt or self.zaru) else {'still': self.still_options()}

    def _scale_arguments(self):
        return {} if not self.odo_scale_state else {'odo_scale_state': self.scale_options(), 'keep_scale': True}

    def get_results(self):
        return self.results

    def reset(self):
        pass
