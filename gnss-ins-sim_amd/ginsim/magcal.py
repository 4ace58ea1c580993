"""MagCalJob: the soft / hard-iron magnetometer calibration (demo_algorithms/mag_calibrate.py::MagCal and the C library it calls,
mag_calibrate_src/src/MagCalibration.c) over a batch of Monte-Carlo runs on one device (csrc/magcal.hip, ginsim_magcal_run).

The reference calibrates one run per call, after six prompts for the three row ranges.  Here the ranges are an argument and every
run is a lane.  In the generated form the kernel makes run r's magnetometer sample j itself from the counter RNG -- the bits
AuxSensorJob writes for the same seed and run ids -- so no `mag` series exists on the device: 65 536 runs of 14 001 samples would
be 22 GB, the job holds ref_mag and 13 numbers per run.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib, check
from .job import BatchJob


def check_segments(segments, n):
    """((x0, xf), (y0, yf), (z0, zf)) as six ints; ValueError for anything but three non-empty ranges inside [0, n]."""
    try:
        seg = [(int(a), int(b)) for a, b in segments]
    except (TypeError, ValueError):
        raise ValueError('segments: three (start, end) row ranges ((x0, xf), (y0, yf), (z0, zf)), got %r' % (segments,))
    if len(seg) != 3:
        raise ValueError('segments: three (start, end) row ranges ((x0, xf), (y0, yf), (z0, zf)), got %d' % len(seg))
    for name, (a, b) in zip('xyz', seg):
        if a < 0 or b > int(n):
            raise ValueError('segments: range %s [%d, %d) is outside [0, %d]' % (name, a, b, n))
        if a >= b:
            raise ValueError('segments: range %s [%d, %d) is empty' % (name, a, b))
    return [v for ab in seg for v in ab]


class MagCalJob(BatchJob):
    """One batch of runs of the magnetometer calibration on one device.

    ref_mag: (n, 3) true magnetic field in the body frame [uT] (truth['ref_mag']); mag_err: {'si' (3, 3), 'hi', 'std'} as
    IMU.mag_err.  segments: ((x0, xf), (y0, yf), (z0, zf)), the rows of the rotations about x, y and z.
    given: None (the samples are generated inside the kernel: same seed and run ids as AuxSensorJob, same bits) or a device buffer
    of logged / materialised `mag` in the engine's [3][n][runs] layout (ref_mag and mag_err are then not read; n: its samples).
    keep: materialise mag_cal, [3][nx + ny + nz][runs].
    placed: as MonteCarloJob (a kept plane set of Context.PLACED_MIN_JOB bytes or more comes from the placed arena).
    """

    def __init__(self, ctx, ref_mag, mag_err, runs, segments, seed=0, run_offset=0, given=None, keep=False, placed=None, n=None):
        self.ctx, self.runs, self.keep = ctx, int(runs), bool(keep)
        if self.runs < 1:
            raise ValueError('runs must be >= 1')
        if given is None and ref_mag is None:
            raise ValueError('the generated form needs ref_mag, the given form a device buffer of mag')
        self.n = int(np.shape(ref_mag)[0] if n is None else n)
        seg = check_segments(segments, self.n)
        self.segments = tuple((seg[2 * a], seg[2 * a + 1]) for a in range(3))
        self.rows = sum(b - a for a, b in self.segments)
        self._bufs = {}
        p = self.params = _lib.MagCalParams()
        p.n, p.runs, p.run_offset, p.seed = self.n, self.runs, int(run_offset), int(seed) & (2 ** 64 - 1)
        p.seg[:] = seg
        if given is None:
            ref_mag = np.ascontiguousarray(ref_mag, dtype=np.float64)
            if ref_mag.shape != (self.n, 3):
                raise ValueError('ref_mag must be (n, 3)')
            p.mag_si[:] = [float(x) for x in np.asarray(mag_err['si'], dtype=np.float64).reshape(9)]
            p.mag_hi[:] = [float(x) for x in np.asarray(mag_err['hi'], dtype=np.float64) * np.ones(3)]
            p.mag_std[:] = [float(x) for x in np.asarray(mag_err['std'], dtype=np.float64) * np.ones(3)]
            self._bufs['ref_mag'] = ctx.upload(ref_mag)
            p.ref_mag = self._bufs['ref_mag'].ptr
        else:
            if given.nbytes < 3 * self.n * self.runs * 8 or getattr(given, 'layout', 'runs') != 'runs':
                raise ValueError('given mag: too small or not [axis][sample][run]')
            p.in_mag = given.ptr
            self._given = given
        R = self.runs
        self._bufs['results'] = ctx.malloc(13 * R * 8)              # soft_iron [9][R], hard_iron [4][R]
        p.out_si, p.out_hi = self._bufs['results'].ptr, self._bufs['results'].at(9 * R * 8)
        if keep:
            total = 3 * self.rows * R * 8
            self._bufs['mag_cal'] = ctx.malloc(total, placed=self._use_placed(placed, total))
            p.out_cal = self._bufs['mag_cal'].ptr

    @property
    def device_bytes(self):
        """Bytes of this job's own device buffers (ref_mag, the 13 x runs results, mag_cal when kept)."""
        return sum(b.nbytes for b in self._bufs.values())

    def run(self):
        """One launch; synchronises."""
        check(self.ctx.retry_oom(lambda: lib.ginsim_magcal_run(self.ctx.handle, C.byref(self.params))))
        self.ctx.sync()
        self._host = self._si = self._hi = None
        return self

    def _results(self):
        if getattr(self, '_host', None) is None:
            self._host = self.ctx.download(self._bufs['results'], (13, self.runs))
        return self._host

    def soft_iron(self):
        """(runs, 3, 3): MagCal's `soft_iron` of every run (read from the device once; the array is shared and read-only)."""
        if getattr(self, '_si', None) is None:
            self._si = np.ascontiguousarray(self._results()[0:9].T).reshape(self.runs, 3, 3)
            self._si.flags.writeable = False
        return self._si

    def hard_iron(self):
        """(runs, 4): MagCal's `hard_iron` (centre x, y, z and radius) of every run (shared and read-only, as soft_iron)."""
        if getattr(self, '_hi', None) is None:
            self._hi = np.ascontiguousarray(self._results()[9:13].T)
            self._hi.flags.writeable = False
        return self._hi

    def mag_cal(self, run_ids):
        """(k, nx + ny + nz, 3): the calibrated rows of selected runs, the three ranges stacked (kept jobs)."""
        if not self.keep:
            raise ValueError('mag_cal was not kept (keep=True)')
        return self._gather(self._bufs['mag_cal'].ptr, self.rows, 3, run_ids)

    def stats(self):
        """{'soft_iron': {'mean', 'std', 'min', 'max': (3, 3)}, 'hard_iron': {...: (4,)}} over the runs (std with ddof 0).  Host
        NumPy over 13 x runs doubles: not a hot path."""
        r = self._results()
        out = {}
        for name, rows, shape in (('soft_iron', slice(0, 9), (3, 3)), ('hard_iron', slice(9, 13), (4,))):
            a = r[rows]
            out[name] = {'mean': a.mean(axis=1).reshape(shape), 'std': a.std(axis=1).reshape(shape),
                         'min': a.min(axis=1).reshape(shape), 'max': a.max(axis=1).reshape(shape)}
        return out
