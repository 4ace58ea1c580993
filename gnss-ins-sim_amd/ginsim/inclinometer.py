"""InclinometerJob: MahonyFilter / TiltAcc (demo_algorithms/inclinometer_mahony.py, inclinometer_acc.py) over a batch of
Monte-Carlo runs on one device (csrc/inclinometer.hip, ginsim_incl_run).

The runs of one MahonyFilter object are CHAINED in the reference: InsAlgoMgr.run_algo calls reset() before each run
(ins_algo_manager.py:78), reset() clears `ini` only (inclinometer_mahony.py:159-163), so run r starts from the gyro_bias run
r-1 ended with.  The kernel takes every run's initial bias as an input; this job iterates whole-batch passes to the fixed point:

    pass k starts run 0 from bias0 and run r >= 1 from the final bias of run r-1 in pass k-1 (pass 1: from zero),
    and stops when the vector of initial biases of pass k+1 equals that of pass k bit for bit.

By induction over r that is the sequential answer exactly, after at most runs + 1 passes.  A pass after the first relaunches
only the runs whose initial bias changed (a compacted list of run ids); every launch writes all requested outputs, so each run's
outputs are those of its last launch -- the one with its converged initial bias -- and no extra output pass is needed.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib, check
from .engine import DeviceView, StatsResult
from .job import BatchJob

INCL_BITS = {'mahony': _lib.INCL_MAHONY, 'tilt': _lib.INCL_TILT}
INCL_SLOT = {'mahony': 0, 'tilt': 1}
MAHONY_DEFAULTS = dict(kp_high=1.0, kp_low=0.01, ki_high=0.5, ki_low=0.001, innovation_limit=0.1)   # inclinometer_mahony.py:35-40


class InclinometerJob(BatchJob):
    """One batch of runs of the inclinometer plugins on one device.

    truth: dict with 'ref_accel', 'ref_gyro' (n, 3) and, for statistics, 'ref_att' (n, 3); the other keys MonteCarloJob takes
    are accepted and ignored.  algos: subset of ('mahony', 'tilt'); both see one sensor realisation.
    gains: MahonyFilter's kp_acc_high, kp_acc_low, ki_acc_high, ki_acc_low, innovationLimit as MAHONY_DEFAULTS keys; dt: its
    sample period (1 / fs).  bias0: the MahonyFilter's gyro_bias before run 0.  start_bias: (runs, 3) initial biases to use as
    they are (one pass, no chain) -- e.g. the converged vector of another job over the same runs.
    given: None (sensors generated as MonteCarloJob generates them: same seed and run ids, same bits) or a dict of device
    buffers {'accel', 'gyro'} in the engine's [3][n][runs] layout.
    stats: accumulate the att_euler error statistics (end point; process window from proc_first).
    keep: materialise att_quat ([4][n][runs] per algorithm), wb / ab (Mahony) and att_euler ([3][n][runs] per algorithm).
    placed: as MonteCarloJob (kept planes of Context.PLACED_MIN_JOB bytes or more come from the placed arena).
    """

    keep_traj = False           # as a statistics job of Sim's _McResults: the statistics are the online ones
    proc_ned = False

    def __init__(self, ctx, fs, truth, accel_err, gyro_err, runs, algos=('mahony', 'tilt'), gains=None, dt=None, bias0=(0.0, 0.0, 0.0),
                 start_bias=None, seed=0, run_offset=0, given=None, stats=True, proc_first=0, keep=False,
                 vib_accel=None, vib_gyro=None, placed=None, block_threads=0):
        self.ctx = ctx
        self.algos = tuple(algos)
        if not self.algos or any(a not in INCL_BITS for a in self.algos):
            raise ValueError('algos: a non-empty subset of %s' % (tuple(INCL_BITS),))
        self.n, self.runs = int(truth['ref_accel'].shape[0]), int(runs)
        if self.runs < 1:
            raise ValueError('runs must be >= 1')
        self.keep, self.stats_on = bool(keep), bool(stats)
        self.proc_first = int(proc_first) if stats else None
        self.bias0 = np.array(bias0, dtype=np.float64).reshape(3)
        self.start_bias = None if start_bias is None else np.ascontiguousarray(np.asarray(start_bias, dtype=np.float64).reshape(self.runs, 3))
        self.passes = 0
        self.launched = []          # runs launched per pass
        self._bufs = {}
        m = self.mc = _lib.McParams()
        self._fill_batch(m, fs, run_offset, seed)
        m.block_threads = int(block_threads)
        self._sensor_source(m, fs, accel_err, gyro_err, vib_accel, vib_gyro, given, (('accel', 3, self.n), ('gyro', 3, self.n)), 'inclinometer')
        if given is None:
            self._bufs['inputs'] = ctx.upload(np.concatenate([np.asarray(truth['ref_accel'], dtype=np.float64).reshape(-1),
                                                              np.asarray(truth['ref_gyro'], dtype=np.float64).reshape(-1)]))
            m.ref_accel, m.ref_gyro = self._bufs['inputs'].ptr, self._bufs['inputs'].at(3 * self.n * 8)
        p = self.params = _lib.InclParams()
        p.algo_mask = sum(INCL_BITS[a] for a in self.algos)
        g = dict(MAHONY_DEFAULTS, **(gains or {}))
        p.dt = float(1.0 / fs if dt is None else dt)
        p.kp_high, p.kp_low, p.ki_high, p.ki_low = float(g['kp_high']), float(g['kp_low']), float(g['ki_high']), float(g['ki_low'])
        p.innovation_limit = float(g['innovation_limit'])
        R = self.runs
        self._bufs['bias'] = ctx.malloc(2 * 3 * R * 8 + R * 8)          # initial [3][R], final [3][R], run list [R]
        p.bias_in, p.bias_out, self._list = self._bufs['bias'].ptr, self._bufs['bias'].at(3 * R * 8), self._bufs['bias'].at(6 * R * 8)
        if stats:
            if 'ref_att' not in truth:
                raise ValueError("statistics need truth['ref_att']")
            nav = np.zeros((self.n, 9))
            nav[:, 0:3] = truth['ref_att']
            self._bufs['ref_nav'] = ctx.upload(nav)
            m.ref_nav, m.proc_first = self._bufs['ref_nav'].ptr, max(self.proc_first, 0)
            for a in self.algos:
                s = INCL_SLOT[a]
                self._bufs['end_' + a] = ctx.malloc(9 * R * 8)       # [9][R]: the end-point record ginsim_end_stats reduces
                ctx_memset(ctx, self._bufs['end_' + a], 9 * R * 8)
                self._bufs['proc_' + a] = ctx.malloc(9 * R * 8)
                p.out_end[s], p.out_proc[s] = self._bufs['end_' + a].ptr, self._bufs['proc_' + a].ptr
        if keep:
            plane = self.n * R * 8
            names = []
            for a in self.algos:
                names += [('quat_' + a, 4), ('euler_' + a, 3)]
            if 'mahony' in self.algos:
                names += [('wb', 3), ('ab', 3)]
            total = sum(c for _, c in names) * plane
            self._bufs['series'] = ctx.malloc(total, placed=self._use_placed(placed, total))
            off = 0
            for nm, c in names:
                self._bufs[nm] = DeviceView(self._bufs['series'], off, c * plane)
                off += c * plane
            for a in self.algos:
                s = INCL_SLOT[a]
                p.out_quat[s], p.out_euler[s] = self._bufs['quat_' + a].ptr, self._bufs['euler_' + a].ptr
            if 'mahony' in self.algos:
                p.out_wb, p.out_ab = self._bufs['wb'].ptr, self._bufs['ab'].ptr

    # ------------------------------------------------------------------ launches
    def kernel_name(self):
        buf = C.create_string_buffer(256)
        self.params.n_list = self.runs
        check(lib.ginsim_incl_kernel_name(C.byref(self.mc), C.byref(self.params), buf, 256))
        return buf.value.decode()

    def variant(self):
        v = C.c_int32(0)
        self.params.n_list = self.runs
        check(lib.ginsim_incl_variant(C.byref(self.mc), C.byref(self.params), C.byref(v)))
        return v.value

    def _launch(self, ids=None):
        p = self.params
        count = self._put_run_list(p, ids)
        check(self.ctx.retry_oom(lambda: lib.ginsim_incl_run(self.ctx.handle, C.byref(self.mc), C.byref(p))))
        self.passes += 1
        self.launched.append(count)

    def _put_start(self, start):
        a = np.ascontiguousarray(start.T)                           # (R, 3) -> [3][R]
        check(lib.ginsim_memcpy_h2d(self.ctx.handle, self.params.bias_in, a.ctypes.data, a.nbytes))

    def _finals(self):
        out = np.empty((3, self.runs))
        check(lib.ginsim_memcpy_d2h(self.ctx.handle, out.ctypes.data, self.params.bias_out, out.nbytes))
        return out.T.copy()

    def run(self):
        """All passes to the fixed point (one when there is no Mahony filter or start_bias is given); synchronises."""
        R = self.runs
        self.passes, self.launched = 0, []
        if self.start_bias is not None or 'mahony' not in self.algos:
            start = self.start_bias if self.start_bias is not None else np.zeros((R, 3))
            self._put_start(start)
            self._launch()
            self.ctx.sync()
            self._start = start.copy()
            return self
        start = np.zeros((R, 3))
        start[0] = self.bias0
        self._put_start(start)
        self._launch()
        while True:
            fin = self._finals()                                     # synchronous copy: waits for the pass
            nxt = np.empty_like(start)
            nxt[0] = self.bias0
            nxt[1:] = fin[:-1]
            changed = np.nonzero(np.any(nxt.view(np.uint64) != start.view(np.uint64), axis=1))[0]
            if changed.size == 0:
                break
            if self.passes > R:         # the induction bounds the chain by R + 1 passes
                raise RuntimeError('inclinometer chain: no fixed point after %d passes of %d runs' % (self.passes, R))
            start = nxt
            self._put_start(start)
            self._launch(changed)
        self.ctx.sync()
        self._start = start
        self._final = fin
        return self

    # ------------------------------------------------------------------ results
    def initial_biases(self):
        """(runs, 3): the gyro_bias each run started from (the converged chain)."""
        return self._start.copy()

    def final_biases(self):
        """(runs, 3): the gyro_bias each run ended with (Mahony)."""
        if 'mahony' not in self.algos:
            raise ValueError('no Mahony filter in this job')
        return self._final.copy() if hasattr(self, '_final') else self._finals()

    def stats(self, algo, ned=False):
        """End-point statistics of the att_euler error as a 9-component record (attitude in 0-2, the rest zero)."""
        if ned or not self.stats_on:
            raise ValueError('the inclinometer record holds the attitude error only' if ned else 'statistics were not requested')
        s = _lib.Stats()
        check(lib.ginsim_end_stats(self.ctx.handle, self._bufs['end_' + algo].ptr, self.runs, C.byref(s)))
        return StatsResult(s)

    def end_errors(self, algo, ned=False):
        """(runs, 3) att_euler error at the last sample, wrapped to [-pi, pi]."""
        return self.ctx.download(self._bufs['end_' + algo], (9, self.runs))[0:3].T.copy()

    def process_stats_online(self, algo):
        """(runs, 3, 9): max|e|, mean, std of the att_euler error over samples >= proc_first in components 0-2."""
        a = self.ctx.download(self._bufs['proc_' + algo], (3, 3, self.runs))
        out = np.zeros((self.runs, 3, 9))
        out[:, :, 0:3] = a.transpose(2, 0, 1)
        return out

    def series(self, name, run_ids):
        """Kept series of selected runs: 'quat_<algo>' (k, n, 4), 'euler_<algo>', 'wb', 'ab' (k, n, 3)."""
        if not self.keep:
            raise ValueError('the series were not kept (keep=True)')
        return self._gather(self._bufs[name].ptr, self.n, 4 if name.startswith('quat_') else 3, run_ids)


def ctx_memset(ctx, buf, nbytes):
    check(lib.ginsim_memset(ctx.handle, buf.ptr, 0, int(nbytes)))
