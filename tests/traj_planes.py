"""Constructed trajectory planes for the kernels that read kept trajectories ACROSS the runs (test infrastructure; no test in it,
imported by tests only): csrc/traj_error.hpp's readers -- error_curve.hip, error_cov.hip, error_quantile.hip's radial_keys_kernel
and stats.hip's process kernel.  Everything is built on the host from a seed; no Monte-Carlo launch is needed.

    planes(runs, n, rf, seed)              -> (series (runs, n, 9) float64, ref_nav (n, 9))
    split(series, rf, table_rows, first)   -> (disp32 (runs, n, 9) float32, origin (table_rows, 3), seen (runs, n, 9) float64)
    origin_row(r, table_rows, first)       -> the row of the origin table run r takes (the rule of the Monte-Carlo kernels)
    slices(runs, m, per_step, max_parts)   -> run_slices of csrc/traj_error.hpp, restated
    curve_slices / cov_slices / key_slices -> the slice count a launch of that family takes
    passes(runs, parts, per_step)          -> the trips of the run loop the busiest wavefront makes
    Planes(ctx, series, ref_nav, f32=..., origin=..., first=..., offset=...)
                                           -> the uploaded planes; .curve(), .cov(), .keys(), .process_stats(), .end_stats()
                                              call the raw entry points through ginsim.lib with ctx.handle

The columns of `series` (errors per sample unless stated):

    c0, c1   truth + 3.1 / truth - 3.1 rad with a 0.1 rad spread: a good third of the runs is beyond +-pi and wraps
    c2       1e-3 rad spread
    c3, c4   metres of error (ref_frame 0: 1e-6 rad of latitude and longitude)
    c5       a common offset of 1e3 m with a spread of 1e-3 m
    c6       the same error in every run (truth and error are eighths: every sum over the runs is exact)
    c7       unit normal
    c8       an offset of 1e6 with a spread of 1e-6 (truth in sixteenths: rounded to float every run holds the same number)

Sample EDGE_SAMPLE has truth 0 in c0 and c1 and carries EDGE_ERRORS in its first runs (as many as there are runs), so that the
differences are exact.  Sample BAD_SAMPLE is the one that is not finite (runs >= 3): run 0 has NaN in c3 and +inf in c7, run
runs - 1 has -inf in c7.  Every other sample is clean.
"""
import ctypes as C
import re

import numpy as np

import error_curve_ref

EDGE_SAMPLE = 1
BAD_SAMPLE = 4
PI = np.pi
EDGE_ERRORS = np.array([PI, -PI, 2 * PI, -2 * PI, np.nextafter(PI, 4.0), -np.nextafter(PI, 4.0), 7.0, -7.0])
LLA0 = np.array([0.56, 2.1, 100.0])


def planes(runs, n=6, rf=1, seed=0):
    """(series (runs, n, 9) float64, ref_nav (n, 9)): see the module docstring."""
    assert n > max(EDGE_SAMPLE, BAD_SAMPLE)
    rng = np.random.RandomState(seed)
    j = np.arange(n, dtype=np.float64)
    ref = np.empty((n, 9))
    ref[:, 0:3] = rng.uniform(-3.0, 3.0, (n, 3))
    ref[EDGE_SAMPLE, 0:2] = 0.0
    lla = LLA0[None] + np.stack([2e-6 * j, -3e-6 * j, 0.5 * j], axis=1)            # a few metres of motion per sample
    ref[:, 3:6] = lla if rf == 0 else error_curve_ref._lla2ecef(lla, np.float64)
    ref[:, 6:9] = rng.uniform(-10.0, 10.0, (n, 3))
    e = np.empty((runs, n, 9))
    e[..., 0] = 3.1 + 0.1 * rng.standard_normal((runs, n))
    e[..., 1] = -3.1 + 0.1 * rng.standard_normal((runs, n))
    e[..., 2] = 1e-3 * rng.standard_normal((runs, n))
    e[..., 3:5] = (1e-6 if rf == 0 else 5.0) * rng.standard_normal((runs, n, 2))
    e[..., 5] = 1e3 + 1e-3 * rng.standard_normal((runs, n))
    # c6: eighths, truth and error, so that the sums of the restatement are exact too: its std and co-moments are exactly 0, as
    # an accumulator about the first run's error gives them
    ref[:, 6] = np.round(ref[:, 6] * 8.0) / 8.0
    # c8's truth in sixteenths: rounded to float its 1e6 +- 1e-6 is ONE number (a float ulp there is 1/16), the error a multiple of
    # 1/16 again, and the two-pass sums of the covariance restatement over equal numbers stay exact (a zero bound asks for equality)
    ref[:, 8] = np.round(ref[:, 8] * 16.0) / 16.0
    e[..., 6] = (rng.randint(1, 17, n) * np.where(j % 2 == 0, 0.125, -0.125))[None]
    e[..., 7] = rng.standard_normal((runs, n))
    e[..., 8] = 1e6 + 1e-6 * rng.standard_normal((runs, n))
    k = min(runs, EDGE_ERRORS.size)
    e[:k, EDGE_SAMPLE, 0] = EDGE_ERRORS[:k]
    e[:k, EDGE_SAMPLE, 1] = -EDGE_ERRORS[:k]
    series = ref[None] + e
    if runs >= 3:
        series[0, BAD_SAMPLE, 3] = np.nan
        series[0, BAD_SAMPLE, 7] = np.inf
        series[runs - 1, BAD_SAMPLE, 7] = -np.inf
    return series, ref


def origin_row(r, table_rows, first):
    """Row `first + r` of the table while there is one, else row 0 (launch.hpp, ProcOrigin)."""
    r = np.asarray(r, dtype=np.int64) + int(first)
    return np.where(r < table_rows, r, 0)


def split(series, rf, table_rows, first, seed=1):
    """The float planes of `series` and their origin table: (disp32 (runs, n, 9) float32, origin (table_rows, 3), seen).  The rows of
    the table differ by kilometres (ref_frame 1) or by 1e-3 rad and 50 m (ref_frame 0); the position planes hold the displacement
    of each run from ITS row.  seen (runs, n, 9) float64 is what a reader must form: float64(origin[row(r)]) + float64(float32
    displacement), and the other six planes rounded to float."""
    runs = series.shape[0]
    rng = np.random.RandomState(seed)
    base = series[0, 0, 3:6]                                                        # sample 0 is clean in every run
    scale = np.array([1e-3, 1e-3, 50.0]) if rf == 0 else np.full(3, 2000.0)
    origin = np.ascontiguousarray(base[None] + scale[None] * rng.uniform(-1.0, 1.0, (int(table_rows), 3)))
    own = origin[origin_row(np.arange(runs), table_rows, first)]                    # (runs, 3)
    disp32 = series.astype(np.float32)
    with np.errstate(invalid='ignore'):
        disp32[:, :, 3:6] = (series[:, :, 3:6] - own[:, None, :]).astype(np.float32)
    seen = disp32.astype(np.float64)
    seen[:, :, 3:6] = own[:, None, :] + disp32[:, :, 3:6].astype(np.float64)
    return disp32, origin, seen


# ------------------------------------------------------------------------------------------ the cut of the run axis, restated
def _constant(path, name):
    return int(re.search(r'constexpr \w+ %s = (\d+);' % name, open(path).read()).group(1))


def kernel_constants(csrc):
    """kTargetWaves and the three caps, read from the sources, so that the restatement below follows a change of them and the
    tests that assert slice counts fail where a shape no longer reaches its path."""
    import os
    return {'target': _constant(os.path.join(csrc, 'traj_error.hpp'), 'kTargetWaves'),
            'curve': _constant(os.path.join(csrc, 'error_curve.hip'), 'kCurveMaxParts'),
            'cov': _constant(os.path.join(csrc, 'error_cov.hip'), 'kCovMaxParts'),
            'cov_batch': _constant(os.path.join(csrc, 'error_cov.hip'), 'kCovBatch'),
            'keys': _constant(os.path.join(csrc, 'error_quantile.hip'), 'kKeysMaxParts')}


def slices(runs, m, per_step, max_parts, target=8192):
    """run_slices (csrc/traj_error.hpp)."""
    most = (runs + per_step - 1) // per_step
    want = min((target + m - 1) // m, most, max_parts)
    return max(int(want), 1)


def curve_vec(runs, aligned=True):
    """Runs per lane and load of the curve kernel (curve_vec, csrc/error_curve.hip)."""
    return 2 if (runs % 2 == 0 and runs >= 128 and aligned) else 1


def curve_slices(runs, m, k, aligned=True):
    return slices(runs, m, 64 * curve_vec(runs, aligned), k['curve'], k['target'])


def cov_slices(runs, m, k):
    return slices(runs, m, 64, k['cov'], k['target'])


def key_slices(runs, m, k):
    return slices(runs, m, 64, k['keys'], k['target'])


def passes(runs, parts, per_step):
    """Trips of the run loop of slice 0, the busiest: its lane 0 starts at run 0 and advances by parts * per_step."""
    return (runs + parts * per_step - 1) // (parts * per_step)


# ------------------------------------------------------------------------------------------ on the device
def device_layout(series):
    """(runs, n, 9) -> [9][n][runs], as the kept-trajectory buffers hold them."""
    return np.ascontiguousarray(series.transpose(2, 1, 0))


class Planes(object):
    """`series` (runs, n, 9) on the device as [9][n][runs] and the truth rows next to it.  f32: float planes (series is then the
    float32 array of split()) with the origin table `origin` and first run `first`.  offset: the planes are uploaded into a
    region 16 bytes longer and start one element (8 bytes of doubles, 4 of floats) into it, so that no row is 16-byte aligned."""

    def __init__(self, ctx, series, ref_nav, f32=False, origin=None, first=0, offset=False):
        self.ctx, self.f32 = ctx, bool(f32)
        self.runs, self.n = int(series.shape[0]), int(series.shape[1])
        dtype = np.float32 if f32 else np.float64
        flat = device_layout(np.asarray(series, dtype=dtype)).reshape(-1)
        item = flat.itemsize
        pad = 16 // item
        host = np.zeros(flat.size + pad, dtype=dtype)
        lead = 1 if offset else 0
        host[lead:lead + flat.size] = flat
        self._buf = ctx.upload(host)
        self.traj = self._buf.ptr + lead * item
        assert self._buf.ptr % 16 == 0 and (self.traj % 16 == 0) == (not offset)
        self._ref = ctx.upload(np.ascontiguousarray(ref_nav, dtype=np.float64))
        self._origin = ctx.upload(np.ascontiguousarray(origin, dtype=np.float64)) if f32 else None
        self._tail = (self._origin.ptr, int(origin.shape[0]), int(first)) if f32 else ()

    def free(self):
        for b in (self._buf, self._ref, self._origin):
            if b is not None:
                b.free()

    def _ids(self, samples):
        if samples is None:
            return None, self.n, None
        ids = np.ascontiguousarray(np.asarray(samples, dtype=np.int64).reshape(-1))
        return ids.ctypes.data_as(C.POINTER(C.c_int64)), ids.size, ids

    def _call(self, fns, mid, out):
        from ginsim import _lib
        fn = fns[1] if self.f32 else fns[0]
        args = (self.ctx.handle, self.traj, self._ref.ptr, self.n, self.runs) + mid + self._tail + out
        _lib.check(fn(*args))

    def curve(self, samples=None, ned=False):
        """ginsim_error_curve[_f32] -> CurveResult."""
        import ginsim
        from ginsim import _lib
        idx, m, _keep = self._ids(samples)
        out = np.empty((m, 9, 4))
        self._call((_lib.lib.ginsim_error_curve, _lib.lib.ginsim_error_curve_f32), (idx, m, int(bool(ned))), (_lib.dptr(out),))
        return ginsim.CurveResult(out)

    def cov(self, samples=None, which=0, ned=False):
        """ginsim_error_cov[_f32] -> CovResult."""
        import ginsim
        from ginsim import _lib
        idx, m, _keep = self._ids(samples)
        out = np.empty((m, 10))
        self._call((_lib.lib.ginsim_error_cov, _lib.lib.ginsim_error_cov_f32), (idx, m, int(which), int(bool(ned))), (_lib.dptr(out),))
        return ginsim.CovResult(out)

    def keys(self, samples=None, which=0, ned=False, gap=(2, 1), fill=-7.0):
        """ginsim_radial_keys[_f32] into rows of gap[0] + runs + gap[1] doubles pre-filled with `fill`, this launch's runs from
        column gap[0]: (host copy (3, m, stride), the device buffer -- the caller frees it)."""
        from ginsim import _lib
        idx, m, _keep = self._ids(samples)
        col0, stride = int(gap[0]), int(gap[0] + self.runs + gap[1])
        buf = self.ctx.upload(np.full((3, m, stride), float(fill)))
        self._call((_lib.lib.ginsim_radial_keys, _lib.lib.ginsim_radial_keys_f32), (idx, m, int(which), int(bool(ned))),
                   (buf.ptr, stride, col0))
        return self.ctx.download(buf, (3, m, stride)), buf

    def process_stats(self, first_sample=0, ned=False):
        """ginsim_process_stats[_f32] -> (runs, 3, 9) = max|e|, mean, std over the samples >= first_sample."""
        from ginsim import _lib
        out = np.empty((self.runs, 3, 9))
        self._call((_lib.lib.ginsim_process_stats, _lib.lib.ginsim_process_stats_f32), (int(first_sample), int(bool(ned))),
                   (_lib.dptr(out),))
        return out

    def end_stats(self, ned=False):
        """ginsim_end_stats_from_traj[_f32] -> StatsResult."""
        import ginsim
        from ginsim import _lib
        s = _lib.Stats()
        self._call((_lib.lib.ginsim_end_stats_from_traj, _lib.lib.ginsim_end_stats_from_traj_f32), (int(bool(ned)),), (C.byref(s),))
        return ginsim.StatsResult(s)
