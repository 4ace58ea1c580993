"""BatchJob: what the device jobs (MonteCarloJob, AuxSensorJob, InsLooseJob, InclinometerJob, MagCalJob) do in the same way --
their named device buffers, the gather of selected runs, the placed decision, the run list of a partial launch, the truth's
navigation rows on the device and the results that are read from kept trajectories.  Not an extension point: a job class sets the
attributes named below in its constructor and calls what it needs.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib, check, dptr


class BatchJob(object):
    """ctx, runs and _bufs {name: DeviceBuffer | DeviceView} are set by every job; n, _ref_nav ((n, 9) host array: att3, pos3, vel3),
    _list (device pointer of a run list of `runs` entries), algos, keep_traj and the 'traj_<algo>' buffers by the jobs that use the
    methods that read them."""

    precision = 'f64'

    def buffer(self, name):
        """Device buffer of a materialised series ('accel', 'gyro', 'odo', 'traj_free', ...), e.g. to feed given=."""
        if name not in self._bufs:
            raise ValueError('%r was not kept by this job' % (name,))
        return self._bufs[name]

    def release(self):
        for b in self._bufs.values():
            b.free()
        self._bufs = {}

    def _gather(self, ptr, rows, ncomp, run_ids, fn=lib.ginsim_gather_runs):
        """(k, rows, ncomp): the selected runs of the [ncomp][rows][runs] series at ptr; fn: the gather entry point of the series'
        layout and precision."""
        ids = np.ascontiguousarray(np.asarray(run_ids, dtype=np.int64).reshape(-1))
        out = np.empty((ids.size, rows, ncomp))
        check(self.ctx.retry_oom(lambda: fn(self.ctx.handle, ptr, ncomp, rows, self.runs, ids.ctypes.data_as(C.POINTER(C.c_int64)),
                                            ids.size, dptr(out))))
        return out

    def _use_placed(self, placed, total):
        """Do the `total` bytes of planes a launch streams at once come from the device's placed arena?  placed: the constructor's
        argument (None: from Context.PLACED_MIN_JOB bytes on).  ONE reservation for all of them, so that the arena grows once."""
        use_placed = (total >= self.ctx.PLACED_MIN_JOB) if placed is None else bool(placed)
        use_placed = bool(use_placed and total > 0 and self.ctx.placed_reserve(total))
        return use_placed

    def _put_run_list(self, p, ids):
        """p.run_list / p.n_list of the next launch: every run (ids None) or the listed ones (lane i takes run ids[i]); returns their count."""
        if ids is None:
            p.run_list, p.n_list = None, self.runs
            return self.runs
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        check(lib.ginsim_memcpy_h2d(self.ctx.handle, self._list, ids.ctypes.data, ids.nbytes))
        p.run_list, p.n_list = self._list, ids.size
        return int(ids.size)

    def _nav(self):
        """Device pointer of the truth's navigation rows, uploaded when first asked for."""
        if 'ref_nav' not in self._bufs:
            self._bufs['ref_nav'] = self.ctx.upload(self._ref_nav)
        return self._bufs['ref_nav'].ptr

    def _fill_batch(self, m, fs, run_offset, seed):
        """The fields of ginsim_mc_params that say which runs a launch makes."""
        m.n, m.runs, m.run_offset, m.seed = self.n, self.runs, int(run_offset), int(seed) & (2 ** 64 - 1)
        m.fs = float(fs)

    def _sensor_source(self, m, fs, accel_err, gyro_err, vib_accel, vib_gyro, given, need, kernel):
        """Where the lanes of the inclinometer / filter kernel take their samples from.  given None: they make them again from the
        run's Philox streams (the two sensor models and vibration terms into m).  Otherwise given[key] holds components x length x
        runs doubles, [component][sample][run], for every (key, components, length) of need."""
        from .engine import sensor_model, vibration
        if given is None:
            m.accel = sensor_model(accel_err, 'vrw', fs)
            m.gyro = sensor_model(gyro_err, 'arw', fs)
            for v in (vib_accel, vib_gyro):
                if v is not None and str(v['type']).lower() == 'psd':
                    raise NotImplementedError("the 'psd' vibration is not a term of the %s kernel (random and sinusoidal are)" % kernel)
            m.vib_accel = vibration(vib_accel, float(fs), False)
            m.vib_gyro = vibration(vib_gyro, float(fs), True)
            return
        if vib_accel is not None or vib_gyro is not None:
            raise ValueError('given sensors: a vibration model cannot be added to sensor series that already exist')
        for k, c, length in need:
            if length and (k not in given or given[k].nbytes < c * length * self.runs * 8 or getattr(given[k], 'layout', 'runs') != 'runs'):
                raise ValueError('given sensors: %r missing, too small or not [component][sample][run]' % (k,))
        m.given_sensors, m.in_accel, m.in_gyro = 1, given['accel'].ptr, given['gyro'].ptr
        self._given = given         # keeps the buffers alive

    # ------------------------------------------------------------------ results from the kept trajectories
    def _origin(self):
        """Device table of the initial positions the fp32 displacement series are relative to ([n_ini][3]: ECEF for ref_frame 1,
        LLA for ref_frame 0; free_integration.py:96-98 / :127-128)."""
        if '_origin' not in self._bufs:
            from gnss_ins_sim.geoparams import geoparams
            lla = self._ini_table[:, 0:3]
            self._bufs['_origin'] = self.ctx.upload(np.ascontiguousarray(geoparams.lla2ecef(lla) if self._ref_frame == 1 else lla))
        return self._bufs['_origin']

    def _traj_call(self, fns, algo, what, mid, out):
        """fns = (fp64 entry point, its _f32 twin) on the kept trajectory of algo (None: the job's first algorithm):
        fn(handle, traj, ref_nav, n, runs, *mid[, origin, n_ini, ini_first], out); a tuple `out`: the arguments that end the call."""
        if not self.keep_traj:
            raise ValueError('%s the trajectories (keep_traj=True)' % what)
        args = (self.ctx.handle, self._bufs['traj_' + (algo or self.algos[0])].ptr, self._nav(), self.n, self.runs) + mid
        fn = fns[0]
        if self.precision == 'f32':     # float series, positions as displacement from the run's initial position
            fn, args = fns[1], args + (self._origin().ptr, self._ini_table.shape[0], self._ini_first)
        args += out if isinstance(out, tuple) else (out,)
        check(self.ctx.retry_oom(lambda: fn(*args)))

    def process_stats(self, algo=None, first_sample=0, pos_ned=False):
        """Per-run statistics of the error over time (samples >= first_sample): (runs, 3, 9) = max|e|, mean, std.
        Needs the trajectories (keep_traj=True) and truth['ref_att'/'ref_pos'/'ref_vel']."""
        out = np.empty((self.runs, 3, 9))
        self._traj_call((lib.ginsim_process_stats, lib.ginsim_process_stats_f32), algo, 'process-error statistics need',
                        (int(first_sample), int(bool(pos_ned))), dptr(out))
        return out

    def error_curve(self, algo=None, samples=None, pos_ned=False):
        """The error-growth curve of this batch: the across-run record (CurveResult) of the error at each of `samples` (sample
        indices in any order, repeats allowed; None: every sample).  Needs the trajectories (keep_traj=True)."""
        from .engine import CurveResult
        idx, m, _keep = self._sample_arg(samples)
        out = np.empty((max(m, 1), 9, 4))
        self._traj_call((lib.ginsim_error_curve, lib.ginsim_error_curve_f32), algo, 'an error-growth curve needs',
                        (idx, m, int(bool(pos_ned))), dptr(out))
        return CurveResult(out)

    def error_cov(self, algo=None, samples=None, which=0, pos_ned=False):
        """The error covariance of this batch: the across-run record (CovResult: count, mean vector, co-moment sums) of the position
        (which = 0; pos_ned: in local NED metres) or velocity (which = 1) error at each of `samples` (as error_curve takes them).
        A run with a non-finite component at a sample is left out of that sample's record.  Needs the trajectories
        (keep_traj=True)."""
        from .engine import CovResult
        idx, m, _keep = self._sample_arg(samples)
        out = np.empty((max(m, 1), 10))
        self._traj_call((lib.ginsim_error_cov, lib.ginsim_error_cov_f32), algo, 'an error covariance needs',
                        (idx, m, int(which), int(bool(pos_ned))), dptr(out))
        return CovResult(out)

    def _sample_arg(self, samples):
        """(POINTER(c_int64) | None, m, the array that owns the memory) of a sample list (None: every sample)."""
        if samples is None:
            return None, self.n, None
        ids = np.ascontiguousarray(np.asarray(samples, dtype=np.int64).reshape(-1))
        return ids.ctypes.data_as(C.POINTER(C.c_int64)), ids.size, ids

    def radial_keys(self, algo=None, samples=None, which=0, out=None, col0=0):
        """The radial error keys of this batch at `samples` (as error_curve takes them): per sample and run the horizontal
        sqrt(e0^2 + e1^2), vertical |e2| and 3-D sqrt(e0^2 + e1^2 + e2^2) error of the position (which = 0; ref_frame 0: always in
        local NED metres, ref_frame 1: the frame's own x, y are horizontal and z vertical) or the velocity (which = 1).  They stay
        on the device: a DeviceBuffer of [3][m][stride] doubles, this job's runs in columns col0 .. col0 + runs of every row.
        out: such a buffer of another call (stride = out.nbytes / (24 m) >= col0 + runs), so that several jobs fill one row; None: a
        new one of stride col0 + runs.  Needs the trajectories (keep_traj=True)."""
        idx, m, _keep = self._sample_arg(samples)
        col0, own = int(col0), out is None
        stride = col0 + self.runs if own else out.nbytes // (24 * max(m, 1))
        if own:                             # sizes the library refuses get a token buffer and its words
            out = self.ctx.malloc(24 * max(m, 1) * max(stride, 1))
        try:
            self._traj_call((lib.ginsim_radial_keys, lib.ginsim_radial_keys_f32), algo, 'the radial error keys need',
                            (idx, m, int(which), int(self._ref_frame == 0)), (out.ptr, stride, col0))
        except Exception:
            if own:
                out.free()
            raise
        return out

    def error_quantiles(self, algo=None, samples=None, which=0, probs=(0.5, 0.95)):
        """The quantiles `probs` across this batch's runs of the horizontal, vertical and 3-D error (radial_keys) at `samples`:
        a QuantileResult with values (3, m, q) and count (3, m).  CEP50 / CEP95 are values[0, :, i] of probs (0.5, 0.95)."""
        from .engine import quantile_rows, QuantileResult
        keys = self.radial_keys(algo, samples, which)
        try:
            m = keys.nbytes // (24 * self.runs)
            r = quantile_rows(self.ctx, keys, 3 * m, self.runs, self.runs, probs)
        finally:
            keys.free()
        return QuantileResult(r.values.reshape(3, m, -1), r.count.reshape(3, m))

    def stats_from_traj(self, algo=None, pos_ned=False):
        """End-point statistics recomputed on the device from the kept trajectories (used for extra_opt='ned')."""
        from .engine import StatsResult
        s = _lib.Stats()
        self._traj_call((lib.ginsim_end_stats_from_traj, lib.ginsim_end_stats_from_traj_f32), algo, 'needs', (int(bool(pos_ned)),), C.byref(s))
        return StatsResult(s)
