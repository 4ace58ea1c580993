"""INS simulation driver, interface-compatible with the reference's ``Sim``
(gnss_ins_sim/sim/ins_sim.py:27-832):

    Sim(fs, motion_def, ref_frame=0, imu=None, mode=None, env=None, algorithm=None)
    .run(num_times)  .results(data_dir, err_stats_start, gen_kml, extra_opt)  .get_data(names)
    .dmgr  .amgr  .sim_count  .sum

What differs is HOW ``run`` executes (ins_sim.py:164-192, 490-506 in the reference are two serial Python
loops over runs): here the truth comes from the native ``ginsim_pathgen``, and ALL Monte-Carlo runs go
through ONE launch of the fused HIP kernel (noise injection + mechanisation + end-point error) per GPU.
Sensor series and algorithm outputs stay in HBM; ``dmgr.<series>.data`` are mapping views that pull a run
to the host only when it is indexed.  With ``torch.distributed`` initialised (one process per GPU) the runs
are sharded across ranks and the end-point statistics are combined with one all-reduce.
``run`` is a sequence of steps (Sim._run_monte_carlo): every decision that needs no device is taken by plan_monte_carlo (a
_Plan), every device job is built by the run's _Jobs factory, and the steps pass both along.

Keyword-only extras (defaults keep the reference behaviour):
    seed               64-bit Philox key.  None: drawn from ``np.random`` (so ``np.random.seed(s)`` before
                       ``run`` makes a simulation repeatable, as it does for the reference).
    keep_trajectories  'auto' | True | False: materialise sensors + outputs in HBM ('auto': when they fit
                       ``max_device_bytes``), else keep only per-run end-point errors (stats-only).
    max_device_bytes   budget for materialised series on one GPU (default 64 GiB of the 288 GB).
    keep_runs          stats-only mode: still materialise sensors (incl. GPS / magnetometer), outputs and CSV files of the
                       first K runs of this rank (the counter RNG makes them the same runs wherever they are integrated: as the
                       first 256-run workgroup of the batch on a sibling stream when K <= 256 and this process integrates on one
                       GPU in fp64 -- no time of their own --, otherwise in a second, small launch).
    stats_start        stats-only mode: the ``err_stats_start`` that ``results()`` will be asked for (default 0 s, the
                       reference's default; -1 = end-point only).  The process-error statistics of that window are
                       accumulated inside the kernel; asking ``results()`` for another window integrates once more.
    device             GPU index (default LOCAL_RANK or 0).
    devices            'all' | [ids]: spread the runs of THIS process over several GPUs -- one context and one Python thread per
                       entry, contiguous run ranges, per-device records folded with the library's Chan merge (ginsim.multi;
                       no torch, no launcher).  The reference's loop being sharded is ins_sim.py:490-506.  An id may repeat
                       (``devices=[0, 0]``: two contexts on one GPU).  Not together with torch.distributed, where the
                       split is one process per GPU.  Default (None): $GINSIM_DEVICES if set (same values, comma separated;
                       'one' = never spread), else EVERY visible GPU when the batch is large enough to pay for it
                       (sim_count x samples >= 2^30, e.g. BASELINE configs 3 and 4) and nothing says this process owns one
                       GPU only (no device=, no $LOCAL_RANK, no initialised process group) -- so that an UNCHANGED
                       demo_free_integration.py uses the whole node.
    placed             None (default) | True | False: carve the materialised series from the device's PLACED arena (ginsim.Context
                       placed_*, ABI 7: a range whose 512 MiB stripes cycle through the three 96 GB classes of an MI355X's memory,
                       built once per device and process from physical chunks whose class was measured) -- C2's launch then takes
                       1.15-1.2 ms wherever the process stands instead of 1.21-1.40 ms by where hipMalloc put the planes.  Default:
                       on for batches that materialise 1 GiB or more; $GINSIM_PLACED=0 switches it off.  ``sim.placement`` says
                       what the last run() got.  (``spread_outputs=`` of round 5 is accepted as an alias.)
    geo_mag_n          geomagnetic field [uT] in the N frame at the initial position, needed for a 9-axis IMU.  The
                       reference evaluates the WMM model once per run for this vector (pathgen.py:164-168,
                       date = today); that model is outside the accelerated path: either the caller supplies the vector, or
                       a checkout of the reference is named in $GNSS_INS_SIM_REFERENCE and ITS geomag.py is
                       evaluated once on the host (geoparams.reference_geomag_n; geo_mag_date pins the date).
"""
import math
import os
import sys
import time
from collections import namedtuple

import numpy as np

from .ins_data_manager import InsDataMgr
from .ins_algo_manager import InsAlgoMgr
from . import sim_data
from .sim_data import McSeries, ChainSeries
from ..attitude import attitude

NAME = 'gnss-ins-sim'
VERSION = '3.0.0_alpha'
high_mobility = np.array([1.0, 0.5, 2.0])       # m/s/s, rad/s/s, rad/s  (ins_sim.py:25)


KEPT_BLOCK = 256        # runs of one workgroup of the lane-per-run kernels


class _BlockAndRest(object):
    """The statistics job of a statistics-only Sim with kept runs, in two launches that run AT THE SAME TIME: `block` integrates the
    first KEPT_BLOCK runs with everything materialised (the kept runs are its first ones) on a sibling context, `rest` every other
    run, statistics only -- together as many workgroups as the one launch over all runs, so the kept runs cost no time of their own
    (C3: the 2-run launch was a chain of 193 036 dependent steps, 0.27 s next to 0.99 s; tools/experiments/kept_block_overlap.py:
    block || rest 0.990 s against 0.991 s for the one launch).  Answers what _McResults asks of a statistics job; the per-run
    records are the block's followed by the rest's (run order), the end-point records are folded with the library's Chan merge."""

    keep_traj = False       # as a statistics job: the trajectories of the block are reached through Sim's kept jobs

    def __init__(self, block, rest):
        self.block, self.rest = block, rest
        self.precision, self.n, self.algos = rest.precision, rest.n, rest.algos
        self.runs = block.runs + rest.runs
        self.proc_first, self.proc_ned, self.end_ned = rest.proc_first, rest.proc_ned, rest.end_ned

    def stats(self, algo, ned=False):
        import ginsim
        return ginsim.StatsResult.merge([self.block.stats(algo, ned=ned).pack(), self.rest.stats(algo, ned=ned).pack()])

    def end_errors(self, algo, ned=False):
        return np.concatenate([self.block.end_errors(algo, ned=ned), self.rest.end_errors(algo, ned=ned)], axis=0)

    def process_stats_online(self, algo):
        return np.concatenate([self.block.process_stats_online(algo), self.rest.process_stats_online(algo)], axis=0)

    def release(self):
        self.rest.release()     # the block stays: it is also the kept job


class _McResults(object):
    """Device results of one Sim.run: per-algorithm jobs + cross-rank merge of the statistics.

    jobs[i] integrates ALL runs of this rank for fused algorithm i (statistics); kept[i] is the job whose series are
    materialised (the same object when everything is kept, a job over the first ``keep_runs`` runs otherwise, or None).
    """

    def __init__(self, jobs, kept, names, kinds, first_run, runs_local, total_runs, group, device, make_ps_job=None, ctx=None,
                 make_kept_job=None, block_runs=0, ned_from_traj=False, make_cons_job=None):
        self.jobs, self.kept, self.algo_names, self.kinds = jobs, kept, names, kinds
        # does the NED end-point record have to be recomputed from trajectories?  Decided by Sim from the CONFIGURATION
        # (identical on every rank), never from a rank's own jobs: a rank without runs has none, and the ranks must enter the
        # same collective
        self._ned_needs_traj = bool(ned_from_traj)
        self.first_run, self.runs_local, self.total_runs = first_run, runs_local, total_runs
        self._group, self._device, self._stats = group, device, {}
        self._make_ps_job, self._ctx = make_ps_job, ctx
        self._make_kept_job, self._block_runs = make_kept_job, int(block_runs)
        self._make_cons_job = make_cons_job
        self.exchange = None                # which exchange merged the records: 'abi', 'torch (...)', None = one process

    fused_names = None      # set by Sim when inclinometer plugins are present: only these produce 'pos' and 'vel'
    loose_names = ()        # the loosely coupled GPS/INS filters (InsLoose): their output holds 'pos' and 'vel' too
    nav_names = None        # fused_names + loose_names: every plugin whose output is a navigation solution

    def names_of(self, data_name):
        """The algorithms whose output holds `data_name`: every one for 'att_euler', the fused free integrations for 'pos' / 'vel'."""
        nav = self.nav_names if self.nav_names is not None else self.fused_names
        if nav is None or data_name == 'att_euler':
            return list(self.algo_names)
        return list(nav)

    def job_of(self, name):
        return self.jobs[self.algo_names.index(name)]

    def end_stats(self, name, ned=False):
        key = (name, bool(ned))
        if key not in self._stats:
            import ginsim
            from ginsim import distributed
            job, kind = self.job_of(name), self.kinds[self.algo_names.index(name)]
            # every rank takes the same branch: the flag comes from the Sim configuration, which is the same on every rank; a
            # rank without runs (world > sim_count) has job None and contributes the empty record to the SAME collective
            from_traj = ned and self._ned_needs_traj
            if from_traj:                           # NED record recomputed from trajectories (kept, or re-integrated block by block)
                part = ginsim.StatsResult.zero() if job is None else self._ned_from_traj(self.algo_names.index(name))
                self._stats[key] = part if self._group is None else distributed.allreduce_stats(part, self._group, self._device)
            elif self._group is None:
                self._stats[key] = job.stats(kind, ned=ned)
            else:
                # the record is on the device: the library's own RCCL all-gather behind the C ABI when the backend is nccl
                # (the exchange bench.py times), the torch.distributed all-reduce otherwise
                ex = distributed.StatsExchange.of(self._ctx, self._group, self._device)
                self._stats[key] = ex.merge(job, kind, ned=ned)
                self.exchange = ex.kind if ex.note is None else '%s (%s)' % (ex.kind, ex.note)
        return self._stats[key]

    def _blocks(self, idx):
        """Statistics that need trajectories a stats-only launch did not keep (the fp32 kernel has no online accumulator): the
        runs are integrated again in blocks that fit the device budget, trajectories kept, and each block is reduced on the
        device before the next one is launched -- the counter RNG reproduces exactly the same runs."""
        step = max(self._block_runs, 1)
        for off in range(0, self.runs_local, step):
            blk = self._make_kept_job(idx, off, min(step, self.runs_local - off))
            blk.run()
            try:
                yield blk
            finally:
                blk.release()

    def _ned_from_traj(self, idx):
        import ginsim
        job, kind = self.jobs[idx], self.kinds[idx]
        if job.keep_traj:
            return job.stats_from_traj(kind, pos_ned=True)
        return ginsim.StatsResult.merge([b.stats_from_traj(kind, pos_ned=True).pack() for b in self._blocks(idx)])

    def _process_array(self, idx, start_sample, ned):
        """(runs, 3, 9) process statistics of fused algorithm idx over this rank's runs."""
        job, kind = self.jobs[idx], self.kinds[idx]
        key = ('proc', idx, int(start_sample), bool(ned))
        if key not in self._stats:
            if job.precision != 'f64' and not job.keep_traj:       # fp32, statistics only: re-integrate block by block
                self._stats[key] = np.concatenate([b.process_stats(kind, start_sample, pos_ned=ned) for b in self._blocks(idx)])
            elif job.keep_traj:
                self._stats[key] = job.process_stats(kind, start_sample, pos_ned=ned)
            elif job.proc_first == int(start_sample) and job.proc_ned == bool(ned):
                self._stats[key] = job.process_stats_online(kind)
            else:       # another window than the one run() accumulated: integrate again with that window (same counter
                        # RNG, same runs, nothing kept) -- costs one more launch
                ps = self._make_ps_job(idx, int(start_sample), bool(ned))
                ps.run()
                self._stats[key] = ps.process_stats_online(kind)
                ps.release()
        return self._stats[key]

    def process_stats(self, data_name, start_sample, ned=False):
        """{'max'|'avg'|'std': {'<algo>_<run>': (3,)}} for data_name in att_euler/pos/vel (ins_data_manager.py:761-795)."""
        from .sim_data import RunStats
        sl = {'att_euler': slice(0, 3), 'pos': slice(3, 6), 'vel': slice(6, 9)}[data_name]
        parts = {'max': [], 'avg': [], 'std': []}
        wanted = self.names_of(data_name)
        for idx, name in enumerate(self.algo_names):
            if self.jobs[idx] is None or name not in wanted:
                continue
            arr = self._process_array(idx, start_sample, ned)
            for row, s in enumerate(('max', 'avg', 'std')):
                parts[s].append((name, self.first_run, arr[:, row, sl]))
        return {s: RunStats(parts[s]) for s in parts}

    def error_curve(self, name, samples, n, ned=False):
        """ginsim.CurveResult of fused algorithm `name` over ALL runs of the Sim: the across-run record of the error at each of
        `samples` (int64 sample indices; None: every one of the n samples).  Kept trajectories are reduced in one call;
        statistics-only runs (either precision) are integrated again through _blocks and folded block by block, so the device
        never holds more than the budget.  Merged over devices (JobSet) and ranks; every rank takes the same branches."""
        key = ('curve', name, None if samples is None else samples.tobytes(), bool(ned))
        if key not in self._stats:
            import ginsim
            from ginsim import distributed
            idx = self.algo_names.index(name)
            job, kind = self.jobs[idx], self.kinds[idx]
            if job is None:                 # a rank without runs: the empty curve, into the same collective
                part = ginsim.CurveResult.zero(n if samples is None else samples.size)
            elif job.keep_traj:
                part = job.error_curve(kind, samples, pos_ned=ned)
            else:
                part = ginsim.CurveResult.merge([b.error_curve(kind, samples, pos_ned=ned).pack() for b in self._blocks(idx)])
            self._stats[key] = distributed.allgather_curve(part, self._group, self._device)
        return self._stats[key]

    def error_covariance(self, name, samples, n, which, ned=False):
        """ginsim.CovResult of algorithm `name` over ALL runs of the Sim: the across-run count, mean vector and co-moment sums of
        the position (which = 0) or velocity (which = 1) error at each of `samples` (int64 sample indices; None: every one of the
        n samples).  Shaped like error_curve: kept trajectories in one call, statistics-only runs integrated again through _blocks
        and folded block by block, merged over devices (JobSet) and ranks; every rank takes the same branches."""
        key = ('cov', name, None if samples is None else samples.tobytes(), int(which))
        if key not in self._stats:
            import ginsim
            from ginsim import distributed
            idx = self.algo_names.index(name)
            job, kind = self.jobs[idx], self.kinds[idx]
            if job is None:                 # a rank without runs: the empty record, into the same collective
                part = ginsim.CovResult.zero(n if samples is None else samples.size)
            elif job.keep_traj:
                part = job.error_cov(kind, samples, which, pos_ned=ned)
            else:
                part = ginsim.CovResult.merge([b.error_cov(kind, samples, which, pos_ned=ned).pack() for b in self._blocks(idx)])
            self._stats[key] = distributed.allgather_cov(part, self._group, self._device)
        return self._stats[key]

    def error_quantiles(self, name, samples, n, which, probs, budget):
        """ginsim.QuantileResult (values (3, m, q), count (3, m): horizontal, vertical, 3-D) of algorithm `name` over ALL runs of
        the Sim at `samples`: one key buffer [3][m][runs] on the selecting device, then one select.  Kept trajectories fill it in
        one launch; statistics-only runs are integrated again through _blocks and every block writes its column range.  Over
        several devices every device's key columns come through the host into one buffer on the first device.  Quantiles are not
        mergeable records: nothing here crosses ranks (Sim.error_quantiles refuses a process group before it gets here)."""
        key = ('quantiles', name, None if samples is None else samples.tobytes(), int(which), probs.tobytes())
        if key not in self._stats:
            import ginsim
            idx = self.algo_names.index(name)
            job, kind = self.jobs[idx], self.kinds[idx]
            m, total = (n if samples is None else samples.size), self.runs_local
            if not job.keep_traj and 24 * m * total > budget:
                raise ValueError('error_quantiles: the keys of %d samples x %d runs are %d bytes (24 per sample and run) and must '
                                 'be on one device at once, more than max_device_bytes = %d: ask for fewer samples (every=, '
                                 'samples=)' % (m, total, 24 * m * total, budget))
            blocks = [job] if job.keep_traj else self._blocks(idx)
            if hasattr(self._ctx, 'contexts'):          # Sim(devices=...): a JobSet per block
                ctx = self._ctx.contexts[0]
                buf = ctx.upload(np.concatenate([b.radial_keys_host(kind, samples, which) for b in blocks], axis=1))
            else:
                ctx, col = self._ctx, 0
                buf = ctx.malloc(24 * m * total)
                for b in blocks:
                    b.radial_keys(kind, samples, which, out=buf, col0=col)
                    col += b.runs
            try:
                r = ginsim.quantile_rows(ctx, buf, 3 * m, total, total, probs)
            finally:
                buf.free()
            self._stats[key] = ginsim.QuantileResult(r.values.reshape(3, m, -1), r.count.reshape(3, m))
        return self._stats[key]

    def consistency(self, name, samples, any_family=False):
        """ginsim.ConsistencyResult of the InsLoose `name` over ALL runs of the Sim at `samples` (int64 sample indices): one more
        statistics-only launch of the filter with checkpoints (the counter RNG reproduces the same runs; nothing kept is needed),
        merged over ranks; every rank takes the same branches.  any_family: the launch goes through InsLooseJob(checkpoints=...),
        which serves a filter with any of its aiding blocks."""
        key = ('cons', name, samples.tobytes()) + (('any',) if any_family else ())
        if key not in self._stats:
            import ginsim
            from ginsim import distributed
            idx = self.algo_names.index(name)
            if self.jobs[idx] is None:      # a rank without runs: the empty record, into the same collective
                part = ginsim.ConsistencyResult.zero(samples.size)
            else:
                job = self._make_cons_job(idx, samples, True) if any_family else self._make_cons_job(idx, samples)
                job.run()
                part = job.consistency()
                job.release()
            self._stats[key] = distributed.allgather_consistency(part, self._group, self._device)
        return self._stats[key]

    def run_of_key(self, key):
        return int(str(key).rsplit('_', 1)[-1]) if isinstance(key, str) else int(key)


# Fused plugins that share one launch: the same initial states, earth_rot and call count (`first`), one plugin per kind
_FusedGroup = namedtuple('_FusedGroup', 'ini earth_rot first kinds idx')


class _InclGroup(object):
    """One MahonyFilter and / or one TiltAcc (the plugin objects, or None) in one InclinometerJob: `job` over all runs of this rank,
    `kept` the job whose series are materialised (the same object when everything is kept), `passes` the chain took."""
    __slots__ = ('kinds', 'idx', 'mahony', 'tilt', 'job', 'kept', 'passes')

    def __init__(self):
        self.kinds, self.idx, self.mahony, self.tilt, self.job, self.kept, self.passes = [], [], None, None, None, None, 0


class _Launched(object):
    """The fused jobs of one run(): by algorithm index the statistics job over all runs of this rank and the job whose series are
    materialised; `sensor_job` is the first job launched with keep_sensors (every launch draws the same noise: counter RNG)."""

    def __init__(self):
        self.stats, self.kept, self.sensor_job = {}, {}, None

    def launch(self, job, sensors=False):
        job.launch()
        if sensors:
            self.sensor_job = self.sensor_job or job
        return job


_Plan = namedtuple('_Plan', 'fused incl hosted groups first count spread ndev per_sample keep kcount online end_ned ride block_runs '
                            'proc_first magcal loose')


class _Roles(tuple):
    """(fused, incl, hosted) as _plugin_roles always returned them, and `magcal`: the indices of the magnetometer calibrations."""
    magcal = ()
    loose = ()          # the indices of the loosely coupled GPS/INS filters (InsLoose of demo_algorithms.ins_loose_device)


def _sample_of(t_axis, start_s):
    hit = np.where(t_axis >= max(float(start_s), 0.0))[0]
    return int(hit[0]) if hit.shape[0] else 0


def _plugin_roles(sim, kinds):
    """(fused, incl, hosted): the indices of the plugins inside the fused kernel, of the inclinometer plugins and of the others;
    the indices of the magnetometer calibrations (MagCal of demo_algorithms.mag_calibrate_device: their own kernel) are the
    result's `magcal`."""
    # which plugins are inside the fused kernel
    fused = [i for i, k in enumerate(kinds) if k in ('free', 'odo')]
    # the inclinometer plugins of demo_algorithms.inclinometer_device: their own kernel, same seed and run ids
    incl = [i for i, k in enumerate(kinds) if k in ('mahony', 'tilt')]
    magcal = [i for i, k in enumerate(kinds) if k == 'magcal']
    # the loosely coupled GPS/INS filters of demo_algorithms.ins_loose_device: their own kernel, same seed and run ids
    loose = [i for i, k in enumerate(kinds) if k == 'loose']
    hosted = [i for i in range(len(kinds)) if i not in fused and i not in incl and i not in magcal and i not in loose]
    if incl and sim.precision != 'f64':
        raise NotImplementedError("the inclinometer plugins (MahonyFilter, TiltAcc of demo_algorithms.inclinometer_device) run "
                                  "in fp64 only: use precision='f64'")
    for i in fused:
        if kinds[i] == 'odo' and not sim.imu.odo:
            raise ValueError("algorithm %d needs 'odo' but the IMU model has no odometer" % i)
    if magcal and not sim.imu.magnetometer:
        raise ValueError("algorithm %d needs 'mag' but the IMU model has no magnetometer (IMU(axis=9))" % magcal[0])
    if magcal and sim.precision != 'f64':
        raise NotImplementedError("the magnetometer calibration (MagCal of demo_algorithms.mag_calibrate_device) runs in fp64 only: "
                                  "use precision='f64'")
    if loose and not sim.imu.gps:
        raise ValueError("algorithm %d needs 'gps' but the IMU model has no GPS (IMU(gps=True))" % loose[0])
    for i in loose:
        if getattr(sim.amgr.algo[i], 'odo', False) and not sim.imu.odo:
            raise ValueError("algorithm %d needs 'odo' but the IMU model has no odometer" % i)
        if getattr(sim.amgr.algo[i], 'mag', False) and not sim.imu.magnetometer:
            raise ValueError("algorithm %d needs 'mag' but the IMU model has no magnetometer (IMU(axis=9))" % i)
    if loose and sim.precision != 'f64':
        raise NotImplementedError("the loosely coupled filter (InsLoose of demo_algorithms.ins_loose_device) runs in fp64 only: "
                                  "use precision='f64'")
    if loose and sim.env is not None and any(isinstance(sim.env.get(k), np.ndarray) for k in ('acc', 'gyro')):
        raise NotImplementedError("the 'psd' vibration (an (n, 4) env array) is not a term of the loosely coupled filter's kernel "
                                  "(InsLoose of demo_algorithms.ins_loose_device): 'random' and 'sinusoidal' are")
    roles = _Roles((fused, incl, hosted))
    roles.magcal = magcal
    roles.loose = loose
    return roles


def plan_monte_carlo(sim, algos, roles, t_axis, gps_rows, rank, world, in_group, place):
    """Every decision of one Sim.run() that needs no device, as a _Plan: which runs are this rank's (`first`, `count`), whether
    all of them are materialised (`keep`) or the first `kcount`, the launch groups of the fused plugins, what the statistics-only
    launches accumulate (`online`: the process window from sample `proc_first`; `end_ned`), whether the kept runs `ride` along as
    the first workgroup of the batch, and the runs per block of an fp32 re-integration.  `sim` is read for its configuration only;
    `roles` is _plugin_roles(); `t_axis` the time of every sample, `gps_rows` the length of the GPS series; `in_group`: a
    torch.distributed process group exists; `place(work, in_group)` says (spread over several devices?, how many) and is asked
    between the refusals as Sim._context always was (it may print the auto-spread notice and make a DeviceSet)."""
    from ginsim import distributed
    fused, incl, hosted = roles
    magcal = list(getattr(roles, 'magcal', ()))
    loose = list(getattr(roles, 'loose', ()))
    imu, n = sim.imu, t_axis.shape[0]
    kinds = [getattr(a, 'mc_algo', None) for a in algos]
    first, count = distributed.shard(sim.sim_count, world, rank)
    if incl and in_group:
        raise ValueError('the runs of a MahonyFilter are a chain (each starts from the gyro_bias the previous one ended with), '
                         'which does not cross torch.distributed ranks: run a Sim with inclinometer plugins in one process')
    if magcal and in_group:
        raise ValueError('a Sim with a MagCal runs on one device: spreading the magnetometer calibration over the ranks of a '
                         'torch.distributed process group is not built yet -- run it in one process')
    if loose and in_group:
        raise ValueError('a Sim with an InsLoose runs on one device: spreading the filter over the ranks of a torch.distributed '
                         'process group is not built yet (the runs are independent) -- run it in one process')
    # an inclinometer chain runs on one device: never spread it automatically; nor is a magnetometer calibration or a GPS/INS filter
    spread, ndev = place(0 if incl or magcal or loose else sim.sim_count * n, in_group)
    if loose and spread:
        raise ValueError('a Sim with an InsLoose runs on one device: spreading the filter over several GPUs is not built yet (the '
                         'runs are independent) -- give Sim(device=...) one GPU, not devices=... (or $GINSIM_DEVICES)')
    if magcal and spread:
        raise ValueError('a Sim with a MagCal runs on one device: spreading the magnetometer calibration over several GPUs is not '
                         'built yet -- give Sim(device=...) one GPU, not devices=... (or $GINSIM_DEVICES)')
    if incl and spread:
        raise ValueError('the runs of a MahonyFilter are a chain (each starts from the gyro_bias the previous one ended with), '
                         'which does not cross devices: give Sim(device=...) one GPU, not devices=... (or $GINSIM_DEVICES)')
    if spread and in_group:
        raise ValueError('Sim(devices=...) spreads the runs of ONE process over several GPUs; under torch.distributed the '
                         'split is one process per GPU (drop devices=, or do not initialise a process group)')
    per_sample = 48 + (8 if imu.odo else 0) + 72 * len(fused) + (24 if imu.magnetometer else 0) + \
        (48.0 * gps_rows / n if imu.gps else 0) + \
        sum(104 if kinds[i] == 'mahony' else 56 for i in incl) + 24 * len(magcal) + \
        120 * len(loose)                                                                  # mag_cal: at most n rows of 3
    keep = sim.keep_trajectories
    if keep == 'auto':
        # decided on the LARGEST share of any rank / device (rank 0's), so that every rank takes the same decision -- the
        # ranks enter collectives that depend on it
        largest = -(-distributed.shard(sim.sim_count, world, 0)[1] // ndev)
        keep = per_sample * n * max(largest, 1) <= sim.max_device_bytes
    if hosted and not keep:
        raise ValueError('plugins outside the fused kernel need the sensor series: use keep_trajectories=True')
    keep = bool(keep)
    # one launch per distinct (initial states, earth_rot); identical noise in every launch (counter RNG)
    groups = []
    for i in fused:
        a = algos[i]
        for g in groups:
            if np.array_equal(g.ini, a.ini) and g.earth_rot == a.earth_rot and kinds[i] not in g.kinds and g.first == a.run_times:
                break
        else:
            g = _FusedGroup(a.ini, a.earth_rot, a.run_times, [], [])
            groups.append(g)
        g.kinds.append(kinds[i])
        g.idx.append(i)
    # Which runs have their series materialised: all of this rank's runs (keep), or the first keep_runs of them next to
    # a stats-only launch over all runs (the counter RNG makes the small launch reproduce exactly those runs).
    kcount = count if keep else min(sim.keep_runs, count)
    f64 = sim.precision == 'f64'
    window = sim.stats_start not in (None, -1)
    online = (not keep) and f64 and window
    end_ned = (not keep) and f64 and sim.ref_frame == 0
    # The kept runs as the FIRST WORKGROUP of the batch (one process, one GPU, fp64): a block of KEPT_BLOCK runs with
    # everything materialised on a sibling context, at the same time as the statistics-only launch over the other runs
    # (_BlockAndRest).  Otherwise: one small launch for them in front of the launch over all runs.
    ride = (0 < kcount <= KEPT_BLOCK < count and f64 and not in_group and not spread and
            per_sample * n * KEPT_BLOCK <= sim.max_device_bytes)
    esize = 4 if sim.precision == 'f32' else 8
    block_runs = ndev * max(256, int(sim.max_device_bytes // (9 * esize * n)) // 256 * 256)
    proc_first = _sample_of(t_axis, sim.stats_start) if window and (online or incl) else 0
    return _Plan(fused, incl, hosted, groups, first, count, spread, ndev, per_sample, keep, kcount, online, end_ned, ride,
                 block_runs, proc_first, magcal, loose)


class _Jobs(object):
    """What every device job of one run() shares (sampling rate, frame, truth, the IMU error models, seed, this rank's first run,
    precision, placement, the two vibration definitions, one context or a DeviceSet), and the one place where a job is built from
    what differs."""

    def __init__(self, sim, ctx, spread, truth, vib, seed, first):
        import ginsim
        from ginsim import multi
        self.sim, self.ctx, self.truth, self.vib, self.seed, self.first = sim, ctx, truth, vib, seed, first
        self.fused_class = multi.JobSet if spread else ginsim.MonteCarloJob
        self.aux_class = multi.AuxJobSet if spread else ginsim.AuxSensorJob

    def fused(self, group, kinds, runs, off=0, ctx=None, keep_sensors=False, keep_traj=False, **kw):
        """A MonteCarloJob (JobSet) of `runs` runs from run `off` of this rank, for `kinds` of launch group `group`, on `ctx`
        (default: the run's own).  kw: proc_first / proc_ned / end_ned; and precision / placed / earth_rot / ini_first where a
        call site does not follow the Sim's and the group's (each such site says so)."""
        sim = self.sim
        kw = dict(dict(precision=sim.precision, placed=sim.placed, earth_rot=group.earth_rot,
                       ini_first=group.first + self.first + off), **kw)
        return self.fused_class(ctx or self.ctx, sim.fs[0], sim.ref_frame, self.truth, sim.imu.accel_err, sim.imu.gyro_err, group.ini,
                                runs=runs, algos=tuple(kinds), odo_err=sim.imu.odo_err, seed=self.seed,
                                run_offset=self.first + off, keep_sensors=keep_sensors, keep_traj=keep_traj, **self.vib, **kw)

    def magcal(self, segments, runs, keep, off=0):
        """A MagCalJob of `runs` runs from run `off` of this rank: the samples are made inside the kernel, as AuxSensorJob makes
        them for the same seed and run ids."""
        import ginsim
        sim = self.sim
        return ginsim.MagCalJob(self.ctx, sim.dmgr.ref_mag.data, sim.imu.mag_err, runs, segments, seed=self.seed,
                                run_offset=self.first + off, keep=keep, placed=sim.placed)

    def loose(self, algo, runs, keep, off=0, **kw):
        """An InsLooseJob of `runs` runs from run `off` of this rank for the plugin `algo`: the IMU samples and the fixes are made
        inside the kernel, as the fused job and AuxSensorJob make them for the same seed and run ids.  The SENSORS are the Sim's;
        the filter is tuned to the plugin's IMU model where it has one (else the Sim's).  kw: proc_first / proc_ned / end_ned /
        cons_samples, and ini_first where a launch of run() is made again."""
        from ginsim import workloads
        from ginsim.ins_loose import InsLooseJob, filter_model
        sim, d = self.sim, self.sim.dmgr
        tuned = algo.imu if algo.imu is not None else sim.imu
        truth = dict(self.truth, ref_gps=d.ref_gps.data, gps_time=d.gps_time.data, gps_visibility=d.gps_visibility.data)
        ini = algo.ini if algo.ini is not None else workloads.parse_motion(sim.data_src)[0]
        return InsLooseJob(self.ctx, sim.fs[0], sim.ref_frame, truth, sim.imu.accel_err, sim.imu.gyro_err, sim.imu.gps_err, ini, runs,
                           seed=self.seed, run_offset=self.first + off, ini_first=kw.pop('ini_first', algo.run_times + self.first + off),
                           earth_rot=algo.earth_rot, keep_traj=keep, placed=sim.placed,
                           model=filter_model(sim.fs[0], tuned.accel_err, tuned.gyro_err, tuned.gps_err, algo.q_scale, algo.p0),
                           **self._aiding(algo), **self._mag_aiding(algo, truth), **self._scale_state(algo, keep), **self._standstill(algo),
                           **(algo.combined_arguments() if hasattr(algo, 'combined_arguments') else {}), **self.vib, **kw)

    def _aiding(self, algo):
        """The aiding arguments of an InsLooseJob: none for a plugin without aiding.  The odometer SAMPLES are the Sim's
        (truth['ref_odo'] and the IMU's odo_err, as the fused job makes them); what the filter assumes of them is the plugin's."""
        aid = algo.aid() if hasattr(algo, 'aid') else None
        return {} if aid is None else {'odo_err': self.sim.imu.odo_err if self.sim.imu.odo else None, 'aid': aid}

    def _standstill(self, algo):
        """The standstill arguments of an InsLooseJob: none for a plugin without zupt and zaru.  The signal is the plugin's
        standstill= where it has one; else the job derives it from the Sim's truth."""
        opts = algo.still_options() if hasattr(algo, 'still_options') else None
        return {} if opts is None else {'still': opts}

    def _scale_state(self, algo, keep):
        """The scale-factor arguments of an InsLooseJob: none for a plugin without the state; the estimate's series is kept where the
        trajectories are."""
        opts = algo.scale_options() if hasattr(algo, 'scale_options') else None
        return {} if opts is None else {'odo_scale_state': opts, 'keep_scale': bool(keep)}

    def _mag_aiding(self, algo, truth):
        """The magnetometer arguments of an InsLooseJob: none for a plugin without the block.  The SAMPLES are the Sim's (ref_mag
        and the IMU's mag_err, as AuxSensorJob makes them); the field is the plugin's where it names one, else the Sim's; what the
        filter assumes of the calibration is the plugin's."""
        mag = algo.mag_options() if hasattr(algo, 'mag_options') else None
        if mag is None:
            return {}
        truth['ref_mag'] = self.sim.dmgr.ref_mag.data
        field = algo.geo_mag_n if getattr(algo, 'geo_mag_n', None) is not None else self.sim.geo_mag_n
        return {'mag_err': self.sim.imu.mag_err, 'geo_mag_n': field, 'mag': mag}

    def inclinometer(self, group, runs, keep, start_bias=None, stats=True, proc_first=0, off=0):
        """An InclinometerJob of `runs` runs from run `off` of this rank for the plugins of `group`; the MahonyFilter's gains and
        gyro_bias are read now."""
        import ginsim
        sim, mah = self.sim, group.mahony
        return ginsim.InclinometerJob(self.ctx, sim.fs[0], self.truth, sim.imu.accel_err, sim.imu.gyro_err, runs, algos=tuple(group.kinds),
                                      gains=mah.gains() if mah is not None else None, dt=1.0 / sim.fs[0],
                                      bias0=mah.gyro_bias if mah is not None else (0.0, 0.0, 0.0), start_bias=start_bias,
                                      seed=self.seed, run_offset=self.first + off, stats=stats, proc_first=proc_first, keep=keep,
                                      placed=sim.placed, **self.vib)


def _keyed_view(entries, first, count):
    """Mapping '<algo>_<run>' -> the series of that run over `entries` = [(algorithm name, fetch(positions in the kept job) ->
    (k, n, c))], for runs first .. first + count - 1."""
    def locate(key):
        if not isinstance(key, str) or '_' not in key:
            return None
        nm, _, r = key.rpartition('_')
        if not r.isdigit() or not (first <= int(r) < first + count):
            return None
        for a, (name, _) in enumerate(entries):
            if name == nm:
                return a * count + int(r) - first
        return None

    def fetch(positions):
        return np.stack([entries[a][1]([r])[0] for a, r in (divmod(p, count) for p in positions)])
    return McSeries(count * len(entries), fetch, key_of=lambda p: entries[p // count][0] + '_' + str(first + p % count),
                    pos_of=locate)


class Sim(object):
    def __init__(self, fs, motion_def, ref_frame=0, imu=None, mode=None, env=None, algorithm=None, *,
                 seed=None, keep_trajectories='auto', max_device_bytes=64 * 2 ** 30, device=None, geo_mag_n=None, precision='f64',
                 keep_runs=0, stats_start=0, geo_mag_date=None, devices=None, placed=None, spread_outputs=None):
        self.name, self.version = NAME, VERSION
        self.fs, self.imu, self.mode, self.env = fs, imu, mode, env
        self.ref_frame = ref_frame if ref_frame in (0, 1) else 0
        self.sim_count = 1
        self.sim_complete = False
        self.sim_results = False
        self.dmgr = InsDataMgr(fs, self.ref_frame)
        self.data_src = motion_def
        self.data_from_files = False
        self.amgr = InsAlgoMgr(algorithm)
        self.interested_error = {'att_euler': 'angle', 'pos': None, 'vel': None}
        self.sum = ''
        self.seed, self.keep_trajectories, self.max_device_bytes, self.device = seed, keep_trajectories, max_device_bytes, device
        self.geo_mag_n, self.geo_mag_date = geo_mag_n, geo_mag_date
        self.precision = precision      # 'f32': single-precision kernel (tolerances: tests/test_gpu_fp32.py)
        self.keep_runs, self.stats_start = max(int(keep_runs), 0), stats_start
        self.placed = placed if placed is not None else (None if spread_outputs is None else bool(spread_outputs))
        self.placement = None            # MonteCarloJob.placement() of the last materialising run
        self._auto_devices = False
        if devices is None and device is None:
            env = os.environ.get('GINSIM_DEVICES', '').strip()
            if env and env != 'one':
                devices = env if env == 'all' else [int(x) for x in env.split(',') if x.strip()]
            elif not env:
                self._auto_devices = True           # decided per run(), when the size of the batch is known
        self.devices = devices
        self._devset = None
        self._side_ctx = None
        self.mc = None

    # ------------------------------------------------------------------------------------ run
    def run(self, num_times=1):
        self.sim_count = max(int(num_times), 1)
        if isinstance(self.data_src, str) and os.path.isdir(self.data_src):
            self._run_from_files()
        else:
            self._psd_on_grid = []
            try:
                self._run_monte_carlo()
            finally:
                for v in self._psd_on_grid:
                    for k in 'xyz':
                        v[k][1:-1] *= 0.5 ** self.sim_count
        self.sim_complete = True

    AUTO_SPREAD_WORK = 2 ** 30      # sample x run products from which an un-configured Sim uses every visible GPU

    def _context(self, work=0, distributed=False):
        """Where this process integrates: a ginsim.Context (one GPU) or a ginsim.multi.DeviceSet (devices=..., or by default
        every visible GPU for a batch of at least AUTO_SPREAD_WORK sample x run products when this process is not one rank
        of a one-process-per-GPU job)."""
        import ginsim
        if self.devices is None and self._auto_devices and not distributed and not self._launcher_rank() \
                and work >= self.AUTO_SPREAD_WORK and ginsim.device_count() > 1:
            self.devices = 'all'
            if not Sim._AUTO_SPREAD_SAID:       # once per process: an unchanged script should not take a node silently
                Sim._AUTO_SPREAD_SAID = True
                print('gnss_ins_sim: %d sample x run products -> spreading the runs over all %d visible GPUs (GINSIM_DEVICES=one '
                      'keeps one GPU, GINSIM_DEVICES=0,1 names them; statistics merged across devices equal a one-GPU run to '
                      'rounding, not to the bit)' % (work, ginsim.device_count()), file=sys.stderr)
        if self.devices is not None:
            from ginsim import multi
            if self.device is not None:
                raise ValueError('Sim: give device (one GPU) or devices (several), not both')
            if self._devset is None or self._devset.devices != multi.parse_devices(self.devices):
                self._devset = multi.DeviceSet(self.devices)
            return self._devset
        if self.device is None:
            return ginsim.default_context()
        return ginsim.Context(self.device)

    _AUTO_SPREAD_SAID = False
    _RANK_ENV = ('LOCAL_RANK', 'OMPI_COMM_WORLD_LOCAL_RANK', 'SLURM_LOCALID', 'PMI_RANK', 'PMIX_RANK', 'MV2_COMM_WORLD_LOCAL_RANK')

    @staticmethod
    def _launcher_rank():
        """True when the environment says this process is ONE RANK of a multi-process job (torchrun, mpirun, srun ...): such a
        process owns one GPU and must not spread over the node by itself."""
        return any(k in os.environ for k in Sim._RANK_ENV)

    _SIBLINGS = {}          # device -> a second context (its own stream) for launches that run next to the main one

    def _block_and_rest_contexts(self, ctx, rest_workgroups):
        """(context of the one-workgroup launch of the kept runs, context of the statistics launch over the others): `ctx` and a
        sibling context of the same device, which way round decided by where their launches START.
        The dispatcher deals the workgroups of a launch to the eight XCDs of an MI355X in turn, starting at a die that belongs to the
        stream's hardware queue (ginsim_stream_first_xcc; consecutive for streams made one after the other, shifted by every stream
        any library of the process made in between -- the FFT plans of a PSD vibration, say).  A statistics launch of W workgroups on
        8 x 64 slots leaves a slot to spare on die (first + W) mod 8 when W is not a multiple of 8; the kept runs' workgroup on THAT
        die costs nothing (C3: 0.93 s for the pair), on any other die it costs its die a third round of workgroups (1.20 s;
        tools/experiments/c3_pair_matrix.py: 24 of 24 pairs as this rule says)."""
        import ginsim
        want = int(rest_workgroups) % 8
        hit = Sim._SIBLINGS.get(ctx.device)
        if hit is not None and hit['of'] == ctx.handle and hit['want'] == want and hit['side'].handle is not None:
            self._side_ctx = hit['side']
            return hit['pair']
        # Candidates first, questions afterwards: the dies move while the runtime is still making its hardware queues (four by
        # default: a fresh process answers 0 for every stream, then 0 / 7 / 6 / 5 ... as the queues come; with all of them there
        # the answers stay).  The candidates that are not taken stay alive -- closing streams could give queues back.
        spare = hit['spare'] + [hit['side']] if hit is not None and hit['of'] == ctx.handle else []
        spare = [c for c in spare if c.handle is not None and c is not ctx]
        try:                                # one more stream than the runtime has hardware queues: all of them exist afterwards
            want_spare = 1 + max(1, int(os.environ.get('GPU_MAX_HW_QUEUES', '4')))
        except ValueError:
            want_spare = 5
        while len(spare) < want_spare:
            spare.append(ginsim.Context(ctx.device))
        for c in spare:
            c.first_xcc()
        mine = ctx.first_xcc()
        pair = side = None
        for c in spare:
            theirs = c.first_xcc()
            if theirs == (mine + want) % 8:
                pair = (c, ctx)             # the kept runs on the sibling
            elif mine == (theirs + want) % 8:
                pair = (ctx, c)             # the kept runs here, the statistics launch on the sibling
            if pair is not None:
                side = c
                break
        if pair is None:                    # no such pair among the queues: a sibling on ANOTHER die at least (the same die = the same
            other = [c for c in spare if c.first_xcc() != mine]         # hardware queue: the two launches one after the other);
            side = (other or spare)[0]                                  # it costs one die one more round of workgroups
            pair = (side, ctx)
        spare = [c for c in spare if c is not side]
        Sim._SIBLINGS[ctx.device] = {'of': ctx.handle, 'want': want, 'side': side, 'pair': pair, 'spare': spare}
        self._side_ctx = side
        return pair

    @staticmethod
    def _dist():
        """(rank, world, group, exchange device) of the torch.distributed job, or a single-process stand-in."""
        # a process group can only exist if the caller imported torch.distributed already: do not pay the ~1 s
        # `import torch` of a single-GPU script for a question whose answer is then known to be "no"
        dist = sys.modules.get('torch.distributed')
        if dist is None or not (dist.is_available() and dist.is_initialized()):
            return 0, 1, None, None
        import torch
        dev = torch.device('cuda', int(os.environ.get('LOCAL_RANK', '0'))) if dist.get_backend() == 'nccl' \
            else torch.device('cpu')
        return dist.get_rank(), dist.get_world_size(), dist.group.WORLD, dev

    def _pick_seed(self, group, dev):
        seed = self.seed
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 62))
        if group is not None:                      # every rank must use rank 0's key
            import torch
            import torch.distributed as dist
            t = torch.tensor([seed], dtype=torch.int64, device=dev)
            dist.broadcast(t, src=0, group=group)
            seed = int(t.item())
        return seed

    def _run_monte_carlo(self):
        if self.imu is None:
            raise ValueError('an IMU model is required to generate sensor data from a motion definition')
        algos = self.amgr.algo or []
        kinds = [getattr(a, 'mc_algo', None) for a in algos]
        truth, t_axis, gps_rows = self._truth_to_dmgr()
        roles = _plugin_roles(self, kinds)
        vib = self._vibration(t_axis.shape[0])
        rank, world, group, xdev = self._dist()
        seed = self._pick_seed(group, xdev)
        plan = plan_monte_carlo(self, algos, roles, t_axis, gps_rows, rank, world, group is not None, self._place)
        self.kept = plan.keep
        jobs = _Jobs(self, self._ctx, plan.spread, truth, vib, seed, plan.first)
        run = self._launch_fused(plan, jobs)
        for i in plan.fused:                    # FreeIntegration.run_times accounting (free_integration.py:69)
            algos[i].run_times += self.sim_count
        loose_jobs = self._run_loose(plan, jobs)
        incl_groups = self._run_inclinometers(plan, jobs, kinds)
        self._sensor_views(plan, run.sensor_job)
        self._aux_views(plan, jobs)
        if self.amgr.algo is not None:
            self.dmgr.set_algo_output(self.amgr.output)
        name_of = self.amgr.get_algo_name
        self._output_views(plan, [(name_of(i), run.kept.get(i), kinds[i]) for i in plan.fused],
                           [(name_of(i), g.kept, kinds[i]) for i, g in incl_groups],
                           [(name_of(i), kept) for i, _, kept in loose_jobs])
        if plan.fused or plan.incl or plan.loose:
            self._publish_results(plan, jobs, run, incl_groups, kinds, group, xdev, loose_jobs)
        if plan.magcal:
            self._run_magcal(plan, jobs)
        if plan.hosted:
            self._run_hosted(plan, algos, run.sensor_job)

    def _truth_to_dmgr(self):
        """The motion definition through the native path generator into the data manager (ins_sim.py:467-480).  Returns (the truth
        dict every job takes, the time of every sample [s], the length of the GPS series)."""
        import ginsim
        from ginsim import workloads
        ini_pva, motion_def = workloads.parse_motion(self.data_src)
        mobility = self._parse_mode(self.mode)
        fs_imu = self.fs[0]
        if self.imu.magnetometer and self.geo_mag_n is None:
            # pathgen.py:164-168 evaluates the World Magnetic Model ONCE, on the host, at the initial position: done here with the
            # reference's own geomag.py when a reference checkout is reachable (unchanged 9-axis scripts then run unchanged)
            from ..geoparams import geoparams
            self.geo_mag_n = geoparams.reference_geomag_n(ini_pva[0], ini_pva[1], ini_pva[2], self.geo_mag_date)
            if self.geo_mag_n is None:
                raise NotImplementedError('a 9-axis IMU needs the local geomagnetic field: pass Sim(..., geo_mag_n=[bx,by,bz] uT), or '
                                          'name a checkout of the reference (its gnss_ins_sim/geoparams/geomag.py + WMM.COF) '
                                          'in $GNSS_INS_SIM_REFERENCE (the WMM evaluation of pathgen.py:164-168 is outside the '
                                          'accelerated path)')
        raw = ginsim.pathgen(ini_pva, motion_def, fs_imu, self.fs[1] if self.imu.gps else 0.0, mobility,
                             self.ref_frame, gps=self.imu.gps,
                             geo_mag_n=self.geo_mag_n if self.imu.magnetometer else None)
        d = self.dmgr
        nav, imu_t = raw['nav'], raw['imu']
        d.add_data(d.time.name, nav[:, 0] / fs_imu)                       # ins_sim.py:467-480
        d.add_data(d.ref_pos.name, np.ascontiguousarray(nav[:, 1:4]))
        d.add_data(d.ref_vel.name, np.ascontiguousarray(nav[:, 4:7]))
        d.add_data(d.ref_att_euler.name, np.ascontiguousarray(nav[:, 7:10]))
        d.add_data(d.ref_accel.name, np.ascontiguousarray(imu_t[:, 1:4]))
        d.add_data(d.ref_gyro.name, np.ascontiguousarray(imu_t[:, 4:7]))
        if self.imu.gps:
            d.add_data(d.gps_time.name, raw['gps'][:, 0] / fs_imu)
            d.add_data(d.ref_gps.name, np.ascontiguousarray(raw['gps'][:, 1:7]))
            d.add_data(d.gps_visibility.name, raw['gps'][:, 7].copy())
        if self.imu.magnetometer:
            d.add_data(d.ref_mag.name, np.ascontiguousarray(raw['mag'][:, 1:4]))
        if self.imu.odo:
            d.add_data(d.ref_odo.name, np.ascontiguousarray(raw['odo'][:, 2]))
        d.add_data(d.ref_att_quat.name, sim_data.Lazy(lambda e=d.ref_att_euler.data.copy(): attitude.euler2quat(e)))    # ins_sim.py:729-748, on first read
        truth = {'ref_accel': d.ref_accel.data, 'ref_gyro': d.ref_gyro.data, 'ref_pos': d.ref_pos.data,
                 'ref_vel': d.ref_vel.data, 'ref_att': d.ref_att_euler.data}
        if self.imu.odo:
            truth['ref_odo'] = d.ref_odo.data
        return truth, nav[:, 0] / fs_imu, raw['gps'].shape[0] if self.imu.gps else 0

    def _vibration(self, n):
        """environment --> vibration parameters (ins_sim.py:482-489): 'random' and 'sinusoidal' models are terms of the kernels, a
        'psd' model is a series per run and axis made on the device before the launch (ginsim_vib_psd_series).  Returns the two
        definitions as the keyword arguments of a job."""
        import ginsim
        fs_imu = self.fs[0]
        vib_acc = vib_gyro = None
        if self.env is not None:
            if 'acc' in self.env.keys():
                vib_acc = self._parse_env(self.env['acc'])
            if 'gyro' in self.env.keys():
                vib_gyro = self._parse_env(self.env['gyro'])
            for v in (vib_acc, vib_gyro):
                if v is not None and v['type'] != 'psd':
                    ginsim.vibration(v, fs_imu, False)       # raises for a definition the kernels do not know
                elif v is not None and self.precision != 'f64':
                    raise NotImplementedError("the 'psd' vibration (an (n, 4) env array) runs on the fp64 kernels only")
        # A PSD given on the series' own frequency grid is halved IN PLACE by the reference at every run and axis
        # (time_series_from_psd.py:44-49: no copy is made when no interpolation is needed; the arrays are views of the caller's
        # env).  The device applies run r's factor 0.5^(r + 1); the arrays are left as the reference leaves them, after the run.
        self._psd_on_grid = [v for v in (vib_acc, vib_gyro) if v is not None and v['type'] == 'psd' and
                             (ginsim.psd_amplitudes(v, fs_imu, n) or (0, 0, False))[2]]
        return dict(vib_accel=vib_acc, vib_gyro=vib_gyro)

    def _place(self, work, distributed):
        """plan_monte_carlo's question: (spread over several devices?, how many).  The context is kept in self._ctx."""
        from ginsim import multi
        self._ctx = self._context(work, distributed)        # one GPU (Context) or several (multi.DeviceSet)
        spread = isinstance(self._ctx, multi.DeviceSet)
        return spread, len(self._ctx) if spread else 1

    def _launch_fused(self, plan, jobs):
        """The launches of the fused plugins' groups, each in one of three shapes, or the sensor-only launch of a Sim without
        algorithm; then the wait for them.  Returns the _Launched record (empty for a rank without runs)."""
        run = _Launched()
        if plan.count <= 0:
            return run
        for g in plan.groups:
            if plan.keep:
                self._launch_all_kept(plan, jobs, g, run)
            elif plan.ride:
                self._launch_block_and_rest(plan, jobs, g, run)
            else:
                self._launch_kept_and_stats(plan, jobs, g, run)
        if not plan.groups and plan.kcount > 0:      # Sim without algorithm: sensor generation only (demo_no_algo.py)
            # kept from the parent on purpose and not yet judged: this job is built without the Sim's precision and placed, with
            # earth_rot and ini_first at the constructor's defaults (there is no table of initial states)
            run.launch(jobs.fused(_FusedGroup(None, True, 0, (), ()), (), plan.kcount, keep_sensors=True, precision='f64', placed=None,
                               earth_rot=True, ini_first=0), sensors=True)
        jobs.ctx.sync()
        if self._side_ctx is not None:
            self._side_ctx.sync()
        sj = run.sensor_job
        self.placement = sj.placement() if sj is not None and hasattr(sj, 'placement') else None
        return run

    def _launch_all_kept(self, plan, jobs, g, run):
        """Everything kept: one launch per group; it is the statistics job and the kept job of its plugins."""
        job = run.launch(jobs.fused(g, g.kinds, plan.count, keep_sensors=run.sensor_job is None, keep_traj=True), sensors=True)
        for i in g.idx:
            run.stats[i] = run.kept[i] = job

    def _launch_block_and_rest(self, plan, jobs, g, run):
        """Statistics only, the kept runs riding along as the first workgroup of the batch (_BlockAndRest)."""
        # which of the two contexts takes which launch: by where their launches start (_block_and_rest_contexts)
        c_block, c_rest = self._block_and_rest_contexts(jobs.ctx, -(-(plan.count - KEPT_BLOCK) // KEPT_BLOCK))
        kw = dict(proc_first=plan.proc_first) if plan.online else {}
        for kinds_ in ([[k] for k in g.kinds] if plan.online else [list(g.kinds)]):
            # placed=None is kept from the parent on purpose and not yet judged: the pair does not follow Sim(placed=)
            blk = jobs.fused(g, kinds_, KEPT_BLOCK, ctx=c_block, keep_sensors=run.sensor_job is None, keep_traj=True,
                             end_ned=plan.end_ned, placed=None, **kw)
            rest = jobs.fused(g, kinds_, plan.count - KEPT_BLOCK, off=KEPT_BLOCK, ctx=c_rest, end_ned=plan.end_ned, placed=None,
                              **kw)
            run.launch(blk, sensors=True)
            run.launch(rest)
            both = _BlockAndRest(blk, rest)
            for i, kind in zip(g.idx, g.kinds):
                if kind in kinds_:
                    run.stats[i], run.kept[i] = both, blk

    def _launch_kept_and_stats(self, plan, jobs, g, run):
        """Statistics only: one small launch for the kept runs (if any) in front of the launch(es) over all runs."""
        if plan.kcount > 0:  # the kept runs: one small launch
            kj = run.launch(jobs.fused(g, g.kinds, plan.kcount, keep_sensors=run.sensor_job is None, keep_traj=True), sensors=True)
            for i in g.idx:
                run.kept[i] = kj
        if plan.online:      # process-error statistics accumulated inside the kernel: one algorithm per launch
            for i, kind in zip(g.idx, g.kinds):
                run.stats[i] = run.launch(jobs.fused(g, [kind], plan.count, proc_first=plan.proc_first, end_ned=plan.end_ned))
        else:
            job = run.launch(jobs.fused(g, g.kinds, plan.count, end_ned=plan.end_ned))
            for i in g.idx:
                run.stats[i] = job

    def _run_inclinometers(self, plan, jobs, kinds):
        """The inclinometer plugins (kinds 'mahony' / 'tilt'): one InclinometerJob per pair of one MahonyFilter and one TiltAcc (both
        bits in one launch), the chain of the MahonyFilter's runs solved by its passes; the first kcount runs kept.  Leaves every
        plugin object as the reference's loop leaves it: gyro_bias, q, quat, wb, ab (Mahony), results and q (tilt) of the last run.
        Returns [(algorithm index, group)] in plugin order."""
        algos, count, kcount, pf = self.amgr.algo or [], plan.count, plan.kcount, plan.proc_first
        groups = []
        for i in plan.incl:
            g = next((g for g in groups if kinds[i] not in g.kinds), None)
            if g is None:
                g = _InclGroup()
                groups.append(g)
            g.kinds.append(kinds[i])
            g.idx.append(i)
            setattr(g, kinds[i], algos[i])
        for g in groups:
            if count <= 0:
                continue
            job = g.job = jobs.inclinometer(g, count, plan.keep, proc_first=pf).run()
            g.passes = job.passes
            if plan.keep:
                g.kept = job
            elif kcount > 0:
                g.kept = jobs.inclinometer(g, kcount, True, start_bias=job.initial_biases()[:kcount], stats=False, proc_first=pf).run()
            # the last run's series: the plugin objects hold them after the reference's loop
            last, pos = (g.kept, count - 1) if (plan.keep or kcount == count) else (None, 0)
            if last is None:
                last = jobs.inclinometer(g, 1, True, start_bias=job.initial_biases()[-1:], stats=False, proc_first=pf,
                                         off=count - 1).run()
            if g.mahony is not None:
                g.mahony.finish(last.series('quat_mahony', [pos])[0], last.series('wb', [pos])[0], last.series('ab', [pos])[0],
                                1.0 / self.fs[0])
            if g.tilt is not None:
                g.tilt.finish(last.series('quat_tilt', [pos])[0])
            if last is not g.kept:
                last.release()
        self.passes = [g.passes for g in groups]
        return sorted(((i, g) for g in groups for i in g.idx), key=lambda t: t[0])

    def _run_loose(self, plan, jobs):
        """The loosely coupled GPS/INS filters (kind 'loose'): one InsLooseJob over all runs of this rank per plugin -- with
        everything kept, or statistics only (the online process window, the NED end record) next to a job over the first kcount
        runs whose series are kept.  Leaves every plugin object with the last run's series as the reference's loop does.
        Returns [(algorithm index, statistics job, kept job or None)]."""
        algos, count, kcount = self.amgr.algo or [], plan.count, plan.kcount
        out = []
        for i in plan.loose:
            algo = algos[i]
            if count <= 0:
                out.append((i, None, None))
                continue
            if plan.keep:
                job = kept = jobs.loose(algo, count, True).run()
            else:
                kw = dict(proc_first=plan.proc_first) if plan.online else {}
                job = jobs.loose(algo, count, False, end_ned=plan.end_ned, **kw).run()
                kept = jobs.loose(algo, kcount, True).run() if kcount > 0 else None
            last, pos = (kept, count - 1) if (plan.keep or kcount == count) else (jobs.loose(algo, 1, True, off=count - 1).run(), 0)
            names = ('pos', 'vel', 'att', 'wb', 'ab') + (('odo_scale',) if getattr(algo, 'odo_scale_state', False) else ())
            algo.finish(*[last.series(k, [pos])[0] for k in names])
            if last is not kept:
                last.release()
            out.append((i, job, kept))
        for i in plan.loose:
            algos[i].run_times += self.sim_count
        self.loose_jobs = out
        return out

    def _run_magcal(self, plan, jobs):
        """The magnetometer calibrations (kind 'magcal'): one MagCalJob over all runs of this rank per plugin, nothing of `mag`
        materialised; mag_cal of the first kcount runs kept.  Fills soft_iron / hard_iron / mag_cal keyed '<algo>_<run>' in the
        reference's shapes ((3, 3), (1, 4), (nx + ny + nz, 3): mag_calibrate.py:77-89), read from the device when first indexed,
        and leaves every plugin object with the last run's results as the reference's loop does."""
        from demo_algorithms.mag_calibrate_device import segments_from_truth
        d, algos, first, count, kcount = self.dmgr, self.amgr.algo or [], plan.first, plan.count, plan.kcount
        self.magcal_jobs = []
        ents = {'soft_iron': [], 'hard_iron': [], 'mag_cal': []}
        for i in plan.magcal:
            algo, name = algos[i], self.amgr.get_algo_name(i)
            seg = algo.segments if algo.segments is not None else segments_from_truth(d.ref_gyro.data)
            if count <= 0:
                continue
            job = jobs.magcal(seg, count, plan.keep).run()
            kept = job if plan.keep else (jobs.magcal(seg, kcount, True).run() if kcount > 0 else None)
            self.magcal_jobs.append((name, job, kept))
            ents['soft_iron'].append((name, lambda pos, j=job: j.soft_iron()[list(pos)]))
            ents['hard_iron'].append((name, lambda pos, j=job: j.hard_iron()[list(pos)][:, None, :]))
            if kept is not None:
                ents['mag_cal'].append((name, lambda pos, j=kept: j.mag_cal(pos)))
            # the last run's results: the plugin object holds them after the reference's loop
            last, pos = (kept, count - 1) if (plan.keep or kcount == count) else (jobs.magcal(seg, 1, True, off=count - 1).run(), 0)
            algo.finish(job.soft_iron()[-1], job.hard_iron()[-1], last.mag_cal([pos])[0])
            if last is not kept:
                last.release()
        for out_name, n_runs in (('soft_iron', count), ('hard_iron', count), ('mag_cal', kcount)):
            d.add_data(out_name, _keyed_view(ents[out_name], first, n_runs) if ents[out_name] and n_runs > 0 else {})

    def _sensor_views(self, plan, sensor_job):
        """accel / gyro / odo of the kept runs: views of the sensor job's device series, keyed by run number."""
        d = self.dmgr
        if sensor_job is None:
            return
        def sens(name, squeeze=False, job=sensor_job):
            return self._run_view(plan, lambda pos, j=job, nm=name: j.sensors(nm, pos)[..., None] if nm == 'odo'
                                  else j.sensors(nm, pos), squeeze=squeeze)
        d.add_data(d.accel.name, sens('accel'))
        d.add_data(d.gyro.name, sens('gyro'))
        if self.imu.odo:
            d.add_data(d.odo.name, sens('odo', squeeze=True))

    @staticmethod
    def _run_view(plan, fetch, squeeze=False):
        """Mapping run number -> series of that run over the kept runs of this rank; fetch(positions in the kept job)."""
        first, kcount = plan.first, plan.kcount
        in_kept = lambda k: int(k) - first if isinstance(k, (int, np.integer)) and first <= int(k) < first + kcount else None
        return McSeries(kcount, fetch, key_of=lambda i: first + i, pos_of=in_kept, squeeze=squeeze)

    def _aux_views(self, plan, jobs):
        """GPS / magnetometer series of the kept runs (ins_sim.py:497-503): their own job, views keyed by run number."""
        d, kcount = self.dmgr, plan.kcount
        if not (kcount > 0 and (self.imu.gps or self.imu.magnetometer)):
            return
        aux = jobs.aux_class(
            jobs.ctx, kcount, seed=jobs.seed, run_offset=plan.first,
            ref_gps=d.ref_gps.data if self.imu.gps else None, gps_err=self.imu.gps_err, ref_frame=self.ref_frame,
            ref_mag=d.ref_mag.data if self.imu.magnetometer else None, mag_err=self.imu.mag_err).run()
        self._aux = aux
        view = lambda nm: self._run_view(plan, lambda pos, a=aux, nm=nm: a.series(nm, pos))
        if self.imu.gps:
            d.add_data(d.gps.name, view('gps'))
        if self.imu.magnetometer:
            d.add_data(d.mag.name, view('mag'))

    def _output_views(self, plan, fused, incl, loose=()):
        """att_euler / pos / vel / att_quat over the fused plugins and the GPS/INS filters, att_euler / att_quat over the
        inclinometer plugins, wb / ab over the MahonyFilters and the GPS/INS filters: device views keyed '<algo>_<run>' over the
        kept runs, or empty mappings when no run is kept (statistics only: names are known, series are not kept).
        fused, incl: [(algorithm name, kept job, kind)]; loose: [(algorithm name, kept job)]."""
        d, first, count = self.dmgr, plan.first, plan.kcount
        nav = list(fused) + [(nm, j, 'loose') for nm, j in loose]           # the navigation solutions: att, pos, vel
        with_bias = [(nm, j) for nm, j, k in incl if k == 'mahony'] + list(loose)
        if not (nav or incl):
            return
        if count <= 0:
            for out_name in ('att_euler',) + (('att_quat',) if incl else ()) + (('pos', 'vel') if nav else ()) + \
                    (('wb', 'ab') if with_bias else ()) + \
                    (('odo_scale',) if any(getattr(a, 'odo_scale_state', False) for a in self.amgr.algo or []) else ()):
                d.add_data(out_name, {})
            return

        def traj(job, kind, comp, quat):
            return lambda pos: (lambda x: np.stack([attitude.euler2quat(v) for v in x]) if quat else x)(job.trajectories(kind, pos)[comp])
        ser = lambda job, nm: (lambda pos, j=job: j.series(nm, pos))
        for out_name, comp in (('att_euler', 0), ('pos', 1), ('vel', 2)):
            ents = [(nm, traj(j, k, comp, False)) for nm, j, k in nav]
            if out_name == 'att_euler':
                ents += [(nm, ser(j, 'euler_' + k)) for nm, j, k in incl]
            if ents:
                d.add_data(out_name, _keyed_view(ents, first, count))
        d.add_data('att_quat', _keyed_view([(nm, traj(j, k, 0, True)) for nm, j, k in nav] +
                                           [(nm, ser(j, 'quat_' + k)) for nm, j, k in incl], first, count))
        for out_name in ('wb', 'ab') if with_bias else ():
            d.add_data(out_name, _keyed_view([(nm, ser(j, out_name)) for nm, j in with_bias], first, count))
        with_scale = [(nm, j) for nm, j in loose if getattr(j, 'keep_scale', False)]     # InsLoose(odo_scale_state=True)
        if with_scale:
            d.add_data('odo_scale', _keyed_view([(nm, ser(j, 'odo_scale')) for nm, j in with_scale], first, count))

    def _publish_results(self, plan, jobs, run, incl_groups, kinds, group, xdev, loose_jobs=()):
        """sim.mc: the statistics and kept jobs of every fused and inclinometer plugin, and how to build the jobs that statistics
        over another window (make_ps_job) or from trajectories that were not kept (make_kept_job) need."""
        algos = self.amgr.algo or []
        owners = [next(g for g in plan.groups if i in g.idx) for i in plan.fused] + [algos[i] for i, _, _ in loose_jobs] + \
            [g for _, g in incl_groups]
        order = plan.fused + [i for i, _, _ in loose_jobs] + [i for i, _ in incl_groups]
        n_loose = len(loose_jobs)

        def make_ps_job(idx, start_sample, ned):
            g = owners[idx]
            if isinstance(g, _InclGroup):           # an inclinometer: one pass from the converged initial biases
                return jobs.inclinometer(g, plan.count, False, start_bias=g.job.initial_biases(), proc_first=start_sample)
            if kinds[order[idx]] == 'loose':
                return jobs.loose(g, plan.count, False, proc_first=start_sample, proc_ned=ned)
            return jobs.fused(g, [kinds[order[idx]]], plan.count, proc_first=start_sample, proc_ned=ned, end_ned=False)

        def make_kept_job(idx, off, runs_):      # a block of this rank's runs, trajectories kept (fp32 statistics)
            if kinds[order[idx]] == 'loose':
                return jobs.loose(owners[idx], runs_, True, off=off)
            # placed=None is kept from the parent on purpose and not yet judged: these blocks do not follow Sim(placed=)
            return jobs.fused(owners[idx], (kinds[order[idx]],), runs_, off=off, keep_traj=True, placed=None)

        def make_cons_job(idx, samples, any_family=False):  # the filter over this rank's runs again, nothing kept, checkpoints at
            # `samples`; the initial states of the launch run() made (the plugin's call count has moved on since).  any_family: through
            # checkpoints=, the kernel family with every block; the truth of a scale-factor state is then the Sim's odometer scale
            first = next(j for i, j, _ in loose_jobs if i == order[idx]).mc.ini_first
            return jobs.loose(owners[idx], plan.count, False, ini_first=first, **{'checkpoints' if any_family else 'cons_samples': samples})
        names = [self.amgr.get_algo_name(i) for i in order]
        self.mc = _McResults([run.stats.get(i) for i in plan.fused] + [j for _, j, _ in loose_jobs] + [g.job for _, g in incl_groups],
                             [run.kept.get(i) for i in plan.fused] + [k for _, _, k in loose_jobs] + [g.kept for _, g in incl_groups], names,
                             [kinds[i] for i in order], plan.first, plan.count, self.sim_count, group,
                             xdev, make_ps_job, ctx=jobs.ctx, make_kept_job=make_kept_job, block_runs=plan.block_runs,
                             ned_from_traj=not plan.end_ned, make_cons_job=make_cons_job)
        self.mc.fused_names = names[:len(plan.fused)]
        self.mc.loose_names = names[len(plan.fused):len(plan.fused) + n_loose]
        self.mc.nav_names = names[:len(plan.fused) + n_loose]       # the plugins whose output holds 'pos' and 'vel'
        self.mc.devices = list(jobs.ctx.devices) if plan.spread else None
        self.mc.kept_block = any(isinstance(j, _BlockAndRest) for j in run.stats.values())    # the kept runs rode along
        self.dmgr.set_mc_results(self.mc)

    def _run_hosted(self, plan, algos, sensor_job):
        """plugins outside the fused kernel: the reference's per-run loop over host copies (user code)"""
        d, hosted, first = self.dmgr, plan.hosted, plan.first
        # plugins that take the device-resident sensor series of all runs at once (demo_algorithms.allan_analysis)
        on_device = [i for i in hosted if hasattr(algos[i], 'run_device') and sensor_job is not None and plan.count > 0]
        merged = [{} for _ in self.amgr.output]
        for i in on_device:
            name = self.amgr.get_algo_name(i)
            per_run = algos[i].run_device(sensor_job, self.fs[0])
            for k, res in enumerate(per_run):
                for j, slot in enumerate(self.amgr.output_alloc[i]):
                    merged[slot][name + '_' + str(first + k)] = res[j]
        rest = [i for i in hosted if i not in on_device]
        if rest:
            inputs = d.get_data(self.amgr.input)
            out = self.amgr.run_algo(inputs, list(range(first, first + plan.kcount)), only=rest)
            for j in range(len(merged)):
                merged[j].update(out[j])
        for j, oname in enumerate(self.amgr.output):
            if merged[j]:
                cur = d.get_data_all(oname).data if oname in d.available else None
                if isinstance(cur, McSeries):           # a fused plugin produced this output too: keep its device view
                    d.add_data(oname, ChainSeries(cur, merged[j]))
                else:
                    d.add_data(oname, merged[j])

    # ------------------------------------------------------------------------------------ logged data
    def _run_from_files(self):
        """Sim with a directory of logged CSV files (ins_sim.py:426-442): every plugin runs once per data key on
        the given-data entry point of the library."""
        self.data_src = os.path.abspath(self.data_src)
        self.data_from_files = True
        d = self.dmgr
        for fname in sorted(os.listdir(self.data_src)):
            low = fname.lower()
            if not low.endswith('.csv'):
                continue
            name, key = low[:-4], None
            cut = name.rfind('-')
            if cut != -1:
                key = name[cut + 1:]
                name = name[:cut]
                key = int(key) if key.isdigit() else key
            if not d.is_supported(name):
                continue
            full = os.path.join(self.data_src, fname)
            data = np.genfromtxt(full, delimiter=',', skip_header=1)
            with open(full) as f:
                cols = f.readline().split(',')
            units = [c[c.find('(') + 1:c.rfind(')')] for c in cols if '(' in c and c.rfind(')') > c.find('(')]
            units = units if len(units) == len(cols) else None
            if name in ('ref_pos', 'pos') and self.ref_frame == 1 and units in (['deg', 'deg', 'm'], ['rad', 'rad', 'm']):
                raise NotImplementedError('LLA -> local-frame conversion of logged positions is outside the hot path')
            d.add_data(name, data, key, units)
        if self.amgr.algo is not None:
            d.set_algo_output(self.amgr.output)
            inputs = d.get_data(self.amgr.input)
            out = self.amgr.run_algo(inputs, range(self.sim_count))
            for j, oname in enumerate(self.amgr.output):
                d.add_data(oname, out[j])

    # ------------------------------------------------------------------------------------ results
    def results(self, data_dir=None, err_stats_start=0, gen_kml=False, extra_opt='', *, max_saved_runs=16, max_summary_runs=None):
        """Sim.results (ins_sim.py:194-251).  CSV files are written for at most ``max_saved_runs`` Monte-Carlo runs.  The printed
        summary lists the per-run process statistics of EVERY run in the reference's order (ins_sim.py:387-392) unless there are
        more than ``max_summary_runs`` of them (default: 2048 entries, i.e. far beyond what the reference is ever run with);
        then the first ones by (algorithm, run number) are printed with a note -- ``sim.err_stats`` holds all of them."""
        if not self.sim_complete:
            print("Call Sim.run() to run the simulaltion first.")
            return None
        data_saved = []
        if data_dir is not None:
            data_dir = self._check_data_dir(data_dir)
            data_saved = self.dmgr.save_data(data_dir, max_runs=max_saved_runs)
        if gen_kml is True:
            self.dmgr.save_kml_files(data_dir)
        self._summary(data_dir, data_saved, err_stats_start, extra_opt, max_summary_runs)
        self.sim_results = True
        return self.dmgr.available

    def _summary(self, data_dir, data_saved, err_stats_start=0, extra_opt='', max_summary_runs=None):
        """Same text as Sim.__summary (ins_sim.py:339-413)."""
        d = self.dmgr
        line = '\n------------------------------------------------------------\n'
        s = line
        s += d.fs.description + ': [' + d.fs.name + '] = ' + str(d.fs.data) + ' ' + d.fs.units[0] + '\n'
        s += d.ref_frame.description + ': ' + str(d.ref_frame.data) + '\n'
        s += 'Simulation time duration: ' + str(len(d.time.data) / d.fs.data) + ' s' + '\n'
        s += 'Simulation runs: ' + str(self.sim_count) + '\n'
        if data_dir is not None:
            s += line + 'Simulation results are saved to ' + data_dir + '\n' + 'The following results are saved:\n'
            for i in data_saved:
                s += '\t' + i + ': ' + d.get_data_all(i).description + '\n'
        header = False
        self.err_stats = {}
        for data_name, kind in self.interested_error.items():
            if data_name not in d.available:
                continue
            st = d.get_error_stats(data_name, err_stats_start=err_stats_start, angle=(kind == 'angle'),
                                   use_output_units=True, extra_opt=extra_opt)
            if st is None:
                continue
            self.err_stats[data_name] = st
            if not header:
                header = True
                s += line + 'The following are error statistics.'
            s += '\n-----------statistics for ' + d.get_data_all(data_name).description + \
                 ' (in units of ' + st['units'] + ')\n'
            if hasattr(st['max'], 'keys'):
                limit = 2048 if max_summary_runs is None else int(max_summary_runs)
                total = len(st['max'])
                if total <= limit:
                    keys = sorted(st['max'].keys())      # the reference's (lexicographic) order
                elif hasattr(st['max'], 'first_keys'):   # truncating: first runs of every algorithm by run NUMBER,
                    keys = st['max'].first_keys(limit)   # made directly (10^5 keys are not built to print 2048 of them)
                else:
                    def run_order(k):
                        name, _, num = str(k).rpartition('_')
                        return (name, int(num)) if num.isdigit() else (str(k), -1)
                    keys = sorted(st['max'].keys(), key=run_order)[:limit]
                fast = sim_data.default_print_options()
                rows = []
                for k in keys:
                    rows.append('\tSimulation run ' + str(k) + ':\n'
                                '\t\t--Max error: ' + sim_data.vec_str(st['max'][k], fast) + '\n'
                                '\t\t--Avg error: ' + sim_data.vec_str(st['avg'][k], fast) + '\n'
                                '\t\t--Std of error: ' + sim_data.vec_str(st['std'][k], fast) + '\n')
                s += ''.join(rows)
                if total > limit:
                    s += '\t... %d more runs: sim.err_stats[%r]\n' % (total - limit, data_name)
            else:       # one vector per statistic (end-point mode): the same writer, a quarter of numpy's array printer
                fast = sim_data.default_print_options()
                s += '\t--Max error: ' + sim_data.vec_str(st['max'], fast) + '\n'
                s += '\t--Avg error: ' + sim_data.vec_str(st['avg'], fast) + '\n'
                s += '\t--Std of error: ' + sim_data.vec_str(st['std'], fast) + '\n'
        self.sum += s
        if self._dist()[0] == 0:
            print(self.sum)
            devs = getattr(self.mc, 'devices', None) if self.mc is not None else None
            if devs and len(devs) > 1:          # after the reference's text, never inside it (summary.txt stays the reference's)
                print('The runs were spread over %d devices of this process: %s' % (len(devs), ', '.join('cuda:%d' % k for k in devs)))
            if data_dir is not None:
                try:
                    with open(data_dir + '//summary.txt', 'w') as f:
                        f.write(self.sum + '\n')
                except Exception:
                    raise IOError('Unable to save summary to %s.' % data_dir)

    def _samples_of(self, who, every, samples, n):
        """The sample indices `every` (seconds between instants, from the first sample) or `samples` name, as contiguous int64, or
        None for every one of the n samples; refusals in the words of `who`."""
        if every is not None and samples is not None:
            raise ValueError('%s: give every (seconds) or samples (indices), not both' % who)
        if every is not None:
            step = int(round(float(every) * float(self.fs[0])))
            if step < 1:
                raise ValueError('%s: every=%r s is shorter than one sample at %g Hz' % (who, every, self.fs[0]))
            samples = np.arange(0, n, step, dtype=np.int64)
        if samples is not None:
            samples = np.ascontiguousarray(np.asarray(samples, dtype=np.int64).reshape(-1))
            if samples.size == 0 or samples.min() < 0 or samples.max() >= n:
                raise ValueError('%s: samples must be indices in [0, %d), at least one' % (who, n))
        return samples

    def error_curve(self, data_names=('att_euler', 'pos', 'vel'), *, every=None, samples=None, extra_opt=''):
        """How the error grows with time: the across-run max |e|, mean and std (ddof 0) of the attitude, position and velocity
        error at each instant -- at sample j what ``results(err_stats_start=-1)`` reports for the series cut after j
        (ins_data_manager.py:717-759, 797-808).  The reference draws one error line per run (``plot(..., opt={'pos': 'error'})``);
        this is the same information for any number of runs, reduced on the device.
          every     seconds between the instants (from the first sample); None and samples=None: every sample
          samples   or the sample indices themselves (any order, repeats allowed)
          extra_opt 'ned': position error in local NED metres (ref_frame 0), as in ``results``
        Returns {name: {'time': (m,), 'units': [...], 'max' | 'avg' | 'std': {algorithm name: (m, 3)}}} in the output units of
        ``get_error_stats(use_output_units=True)`` (attitude in degrees).  Only the fused free-integration plugins carry these
        curves.  Statistics-only Sims integrate their runs again in blocks that fit ``max_device_bytes``."""
        if not self.sim_complete:
            print("Call Sim.run() to run the simulaltion first.")
            return None
        d, mc = self.dmgr, self.mc
        names = list(getattr(mc, 'nav_names', None) or getattr(mc, 'fused_names', None) or []) \
            if mc is not None and not self.data_from_files else []
        if isinstance(data_names, str):
            data_names = (data_names,)
        slices = {'att_euler': slice(0, 3), 'pos': slice(3, 6), 'vel': slice(6, 9)}
        for nm in data_names:
            if nm not in slices:
                raise ValueError("error_curve: %r has no error curve (one of 'att_euler', 'pos', 'vel')" % (nm,))
        if not names:
            raise ValueError('error_curve: the curves of %s come from the fused free-integration plugins (FreeIntegration, '
                             'FreeIntegrationOdo), and this Sim has none -- inclinometer, MagCal and host plugins are not covered'
                             % (', '.join(data_names),))
        for a in getattr(mc, 'loose_names', ()):
            if not mc.job_of(a).keep_traj:
                raise ValueError('error_curve: %s (InsLoose) kept statistics only: its curve is read from the kept trajectory '
                                 'planes -- run the Sim with keep_trajectories=True' % a)
        t = np.asarray(d.time.data)
        n = t.shape[0]
        samples = self._samples_of('error_curve', every, samples, n)
        # one reduction serves every name: the NED form changes the position components only
        use_ned = self.ref_frame == 0 and extra_opt == 'ned' and 'pos' in data_names
        out = {}
        for nm in data_names:
            src = d.get_data_all(nm)
            units, out_units = list(src.units), list(src.output_units)
            if use_ned and nm == 'pos':
                units, out_units = ['m', 'm', 'm'], ['m', 'm', 'm']
            res = {'time': t.copy() if samples is None else t[samples], 'units': out_units, 'max': {}, 'avg': {}, 'std': {}}
            for a in names:
                c = mc.error_curve(a, samples, n, ned=use_ned)
                for stat, arr in (('max', c.maxabs), ('avg', c.mean), ('std', c.std)):
                    res[stat][a] = sim_data.convert_unit(np.ascontiguousarray(arr[:, slices[nm]]), units, out_units)
            out[nm] = res
        return out

    def error_quantiles(self, data_names=('pos',), probs=(0.5, 0.95), *, every=None, samples=None):
        """What share of the runs stays inside which radius: for each probability p of `probs` the horizontal, vertical and 3-D
        error that holds the share p of the runs at each instant -- CEP50 and CEP95 (R95) are the 'horizontal' columns of
        probs=(0.5, 0.95).  The across-run moments of ``error_curve`` do not give these numbers: the radial error is not Gaussian,
        and in ref_frame 0 the across-run mean is not zero.  Exact order statistics (nearest rank,
        ``np.quantile(method='inverted_cdf')``: the value is the error of one of the runs), selected on the device.
          data_names 'pos' and / or 'vel'.  The position error of ref_frame 0 is always taken in local NED metres (north and east
                     horizontal, down vertical); in ref_frame 1 the frame's own x, y are horizontal and z vertical
          probs      up to 8 probabilities in (0, 1]
          every      seconds between the instants (from the first sample); None and samples=None: every sample
          samples    or the sample indices themselves (any order, repeats allowed)
        Returns {name: {'time': (m,), 'units': ['m'] | ['m/s'], 'probs': (q,), 'count': {algorithm name: (m,) the runs whose
        error is finite, the others are left out}, 'horizontal' | 'vertical' | '3d': {algorithm name: (m, q)}}}.  Served: the fused
        free-integration plugins, kept or statistics only (their runs are integrated again in blocks that fit
        ``max_device_bytes``; the keys, 24 B per sample and run, must fit it at once), over one or several devices of this
        process, and InsLoose with kept trajectories."""
        if not self.sim_complete:
            print("Call Sim.run() to run the simulaltion first.")
            return None
        mc = self.mc
        names = list(getattr(mc, 'nav_names', None) or getattr(mc, 'fused_names', None) or []) \
            if mc is not None and not self.data_from_files else []
        if isinstance(data_names, str):
            data_names = (data_names,)
        which = {'pos': 0, 'vel': 1}
        for nm in data_names:
            if nm not in which:
                raise ValueError("error_quantiles: %r has no error quantiles (one of 'pos', 'vel')" % (nm,))
        if not names:
            raise ValueError('error_quantiles: the quantiles of %s come from the fused free-integration plugins (FreeIntegration, '
                             'FreeIntegrationOdo) and from InsLoose, and this Sim has none -- inclinometer, MagCal and host plugins '
                             'are not covered' % (', '.join(data_names),))
        if mc._group is not None:           # every rank, before any collective
            raise NotImplementedError('error_quantiles: quantiles are not mergeable records, and the keys of the ranks of a '
                                      'torch.distributed process group are not gathered yet -- run the Sim in one process '
                                      '(Sim(devices=...) spreads it over the GPUs of one)')
        for a in getattr(mc, 'loose_names', ()):
            if not mc.job_of(a).keep_traj:
                raise ValueError('error_quantiles: %s (InsLoose) kept statistics only: its keys are read from the kept trajectory '
                                 'planes -- run the Sim with keep_trajectories=True' % a)
        probs = np.ascontiguousarray(np.asarray(probs, dtype=np.float64).reshape(-1))
        t = np.asarray(self.dmgr.time.data)
        n = t.shape[0]
        samples = self._samples_of('error_quantiles', every, samples, n)
        out = {}
        for nm in data_names:
            res = {'time': t.copy() if samples is None else t[samples], 'units': ['m'] if nm == 'pos' else ['m/s'],
                   'probs': probs.copy(), 'count': {}, 'horizontal': {}, 'vertical': {}, '3d': {}}
            for a in names:
                r = mc.error_quantiles(a, samples, n, which[nm], probs, self.max_device_bytes)
                res['count'][a] = r.count[2].copy()         # the 3-D key is finite where all three components are
                for k, part in enumerate(('horizontal', 'vertical', '3d')):
                    res[part][a] = r.values[k].copy()
            out[nm] = res
        return out

    def error_covariance(self, data_names=('pos',), *, every=None, samples=None, frame='track'):
        """Which way the error points: the across-run mean vector and 3x3 covariance (ddof 0) of the position or velocity error at
        each instant, reduced on the device, and from it the correlation coefficients and the horizontal 1-sigma error ellipse.
        ``error_curve`` gives per-axis sigmas and ``error_quantiles`` one radius; an odometer-aided filter whose error is a narrow
        strip across the track looks unremarkable in both.
          data_names 'pos' and / or 'vel'.  The position error of ref_frame 0 is always taken in local NED metres
          every      seconds between the instants (from the first sample); None and samples=None: every sample
          samples    or the sample indices themselves (any order, repeats allowed)
          frame      'nav': the frame's own axes (north, east, down in ref_frame 0; x, y, z in ref_frame 1); 'track': rotated about
                     the vertical axis by the truth's yaw at each instant (ginsim.track_frame): along, cross, down
        Returns {name: {'time': (m,), 'units': ['m'] | ['m/s'], 'frame': frame, 'axes': (three names), 'count': {algorithm name:
        (m,) the runs that entered: a run with a non-finite component at an instant is left out there}, 'mean': {(m, 3)}, 'cov':
        {(m, 3, 3)}, 'corr': {(m, 3, 3) correlation coefficients, NaN where a variance is 0}, 'ellipse': {(m, 3): semi-major,
        semi-minor and azimuth of the major axis in degrees of the horizontal 1-sigma ellipse (ginsim.error_ellipse); the azimuth
        from north (axis 0) in 'nav', from the track in 'track'}}}.  Served: what ``error_curve`` serves -- the fused
        free-integration plugins, kept or statistics only (their runs are integrated again in blocks that fit
        ``max_device_bytes``), several devices, a process group -- and InsLoose with kept trajectories."""
        if not self.sim_complete:
            print("Call Sim.run() to run the simulaltion first.")
            return None
        import ginsim
        d, mc = self.dmgr, self.mc
        names = list(getattr(mc, 'nav_names', None) or getattr(mc, 'fused_names', None) or []) \
            if mc is not None and not self.data_from_files else []
        if isinstance(data_names, str):
            data_names = (data_names,)
        which = {'pos': 0, 'vel': 1}
        for nm in data_names:
            if nm not in which:
                raise ValueError("error_covariance: %r has no error covariance (one of 'pos', 'vel')" % (nm,))
        if frame not in ('nav', 'track'):
            raise ValueError("error_covariance: frame=%r is neither 'nav' nor 'track'" % (frame,))
        if not names:
            raise ValueError('error_covariance: the covariance of %s comes from the fused free-integration plugins (FreeIntegration, '
                             'FreeIntegrationOdo) and from InsLoose, and this Sim has none -- inclinometer, MagCal and host plugins '
                             'are not covered' % (', '.join(data_names),))
        for a in getattr(mc, 'loose_names', ()):
            if not mc.job_of(a).keep_traj:
                raise ValueError('error_covariance: %s (InsLoose) kept statistics only: its covariance is read from the kept '
                                 'trajectory planes -- run the Sim with keep_trajectories=True' % a)
        t = np.asarray(d.time.data)
        n = t.shape[0]
        samples = self._samples_of('error_covariance', every, samples, n)
        yaw = np.asarray(d.ref_att_euler.data, dtype=np.float64)[:, 0]
        yaw = yaw.copy() if samples is None else yaw[samples]
        axes = ('along', 'cross', 'down') if frame == 'track' else ('north', 'east', 'down') if self.ref_frame == 0 else ('x', 'y', 'z')
        out = {}
        for nm in data_names:
            res = {'time': t.copy() if samples is None else t[samples], 'units': ['m'] if nm == 'pos' else ['m/s'], 'frame': frame,
                   'axes': axes, 'count': {}, 'mean': {}, 'cov': {}, 'corr': {}, 'ellipse': {}}
            for a in names:
                r = mc.error_covariance(a, samples, n, which[nm], ned=self.ref_frame == 0)
                mean, cov = r.mean.copy(), r.cov
                if frame == 'track':
                    mean, cov = ginsim.track_frame(mean, cov, yaw)
                sd = np.sqrt(np.einsum('kaa->ka', cov))
                with np.errstate(invalid='ignore', divide='ignore'):
                    corr = cov / (sd[:, :, None] * sd[:, None, :])
                res['count'][a], res['mean'][a], res['cov'][a], res['corr'][a] = r.count.copy(), mean, cov, corr
                res['ellipse'][a] = np.stack(ginsim.error_ellipse(cov[:, :2, :2]), axis=1)
            out[nm] = res
        return out

    def consistency_curve_any_family(self, *, every=None, samples=None):
        """consistency_curve for EVERY InsLoose of the Sim: with the magnetometer block, the scale-factor state, the standstill block or
        several of them (combined=True) too, which consistency_curve refuses (InsLooseJob(checkpoints=...)).  The same
        arguments and the same dict; a plugin with the scale-factor state gains 'scale': {'sigma', 'rms', 'ratio'}, each (m,):
        sqrt(mean P[15][15]), the RMS of k_est - k against the Sim's odometer scale k, and their quotient.  (A method of its own and
        not a keyword: consistency_curve keeps its signature and every refusal it has.)"""
        return self._consistency_curve(every, samples, True)

    def consistency_curve(self, *, every=None, samples=None):
        """Is the covariance of the Sim's InsLoose filters honest along the run?  At each instant, across all runs: the filter's
        predicted 1 sigma next to the RMS of its actual error, state by state, and the normalised error of the position, velocity
        and attitude block -- before, during and after a GPS outage.  For every InsLoose of the Sim (aided ones included) the
        filter is launched once more over the Sim's runs, statistics only, with the same seed and run ids; the sums are taken
        inside the launch, so statistics-only Sims are served and no kept plane is read.
          every     seconds between the instants (from the first sample); None and samples=None: every sample
          samples   or the sample indices themselves (any order, repeats allowed)
        Returns {'time': (m,), 'states': ['dr_x', ..., 'dba_z'], algorithm name: {'count': (m,) runs included, 'sigma': (m, 15)
        sqrt(mean P_kk), 'rms': (m, 9) RMS error of dr, dv, psi, 'ratio': (m, 9) rms / sigma (1: consistent; above: overconfident),
        'nees': (m, 3) mean e^T P_bb^-1 e of the three blocks (3: consistent)}}.
        Units are the FILTER's, not the output units of ``results``: dr in m (NED metres in ref_frame 0), dv in m/s, psi in rad
        (a small rotation in the navigation frame, not Euler angles), dbg in rad/s, dba in m/s^2.  A run whose state or covariance
        is not finite, or whose P is not positive definite on a block, is left out and missing from 'count'."""
        return self._consistency_curve(every, samples, False)

    def _consistency_curve(self, every, samples, any_family):
        """consistency_curve (any_family False: the plugins with a magnetometer, scale-factor or standstill block are refused) and
        consistency_curve_any_family (True: they are served through InsLooseJob(checkpoints=...))."""
        if not self.sim_complete:
            print("Call Sim.run() to run the simulaltion first.")
            return None
        mc = self.mc
        names = list(getattr(mc, 'loose_names', ())) if mc is not None and not self.data_from_files else []
        if not names:
            raise ValueError('consistency_curve: the curves come from the loosely coupled GPS/INS filter plugins (InsLoose), and '
                             'this Sim has none -- free integration, inclinometer, MagCal and host plugins carry no covariance')
        t = np.asarray(self.dmgr.time.data)
        n = t.shape[0]
        samples = self._samples_of('consistency_curve', every, samples, n)
        if samples is None:
            samples = np.arange(n, dtype=np.int64)
        out = {'time': t[samples], 'states': ['%s_%s' % (b, a) for b in ('dr', 'dv', 'psi', 'dbg', 'dba') for a in 'xyz']}
        for a, (_, job, _) in zip(names, () if any_family else getattr(self, 'loose_jobs', ())):
            if getattr(job, 'allp', None) is not None:
                raise NotImplementedError('consistency_curve: %s runs several of the magnetometer block, the scale-factor state and the '
                                          'standstill block in one launch (InsLoose(combined=True)), and the consistency checkpoints of '
                                          'that filter are not built' % a)
            if getattr(job, 'mag', None) is not None:
                raise NotImplementedError('consistency_curve: %s is aided by the magnetometer (InsLoose(mag=True)), and the consistency '
                                          'checkpoints of that filter are not built' % a)
            if getattr(job, 'scale', None) is not None:
                raise NotImplementedError('consistency_curve: %s estimates the odometer\'s scale factor (InsLoose(odo_scale_state=True)), '
                                          'and the consistency checkpoints of that filter are not built' % a)
            if getattr(job, 'still', None) is not None:
                raise NotImplementedError('consistency_curve: %s is aided at standstill (InsLoose(zupt=True) / InsLoose(zaru=True)), and '
                                          'the consistency checkpoints of that filter are not built' % a)
        with_scale = {a for a, (_, job, _) in zip(names, getattr(self, 'loose_jobs', ())) if getattr(job, 'scale', None) is not None}
        for a in names:
            c = mc.consistency(a, samples, True) if any_family else mc.consistency(a, samples)
            out[a] = {'count': c.count, 'sigma': c.sigma, 'rms': c.rms, 'ratio': c.ratio, 'nees': c.nees}
            if any_family and a in with_scale:
                out[a]['scale'] = {'sigma': c.sigma_scale, 'rms': c.rms_scale, 'ratio': c.ratio_scale}
        return out

    def plot(self, what_to_plot, sim_idx=None, opt=None, extra_opt=''):
        """Plotting is outside the accelerated path; the call is accepted (the reference's demo scripts end with it) and
        says where the data are instead of drawing them."""
        print('plot(%s): not drawn by this package -- the series are in sim.dmgr.<name>.data (per-run views) and in the '
              'CSV files of results(data_dir).' % (what_to_plot,))

    def get_names_of_available_data(self):
        return self.dmgr.available

    def get_data(self, data_names):
        return self.dmgr.get_data(data_names).copy()

    def get_data_properties(self, data_name):
        return self.dmgr.get_data_properties(data_name)

    # ------------------------------------------------------------------------------------ helpers
    def _parse_env(self, env):
        """Sim.__parse_env (ins_sim.py:642-701): one entry of the env dict -> the vib_def dict acc_gen / gyro_gen take.
        '[x y z]<g|d|>-random' (1 sigma) or '[x y z]<g|d|>-<f>Hz-sinusoidal' (peak); 'g' = 9.8 m/s^2, 'd' = deg/s;
        an (n,4) array [freq, x, y, z] is a single-sided PSD, cut at fs/2."""
        if env is None:
            return None
        if isinstance(env, np.ndarray):
            if env.ndim == 2 and env.shape[1] == 4:
                rows, half_fs = env.shape[0], 0.5 * self.fs[0]
                if env[-1, 0] > half_fs:
                    rows = np.where(env[:, 0] > half_fs)[0][0]
                return {'type': 'psd', 'freq': env[:rows, 0], 'x': env[:rows, 1], 'y': env[:rows, 2], 'z': env[:rows, 3]}
            raise TypeError('env should be of size (n,2)')
        if not isinstance(env, str):
            raise TypeError('env should be a string or a numpy array of size (n,2)')
        text, vib = env.lower(), {}
        if 'random' in text:
            vib['type'] = 'random'
            text = text.replace('-random', '')
        elif 'sinusoidal' in text:
            vib['type'] = 'sinusoidal'
            text = text.replace('-sinusoidal', '')
            if text[-2:] != 'hz':
                raise ValueError('env = \'%s\' is not valid (No vib freq).' % text)
            try:
                mark = text.find('-')
                vib['freq'] = math.fabs(float(text[mark + 1:-2]))
                text = text[:mark]
            except Exception:
                raise ValueError('env = \'%s\' is not valid (invalid vib freq).' % text)
        else:
            raise ValueError('env = \'%s\' is not valid.' % text)
        unit = 1.0                              # 1 sigma (random) or peak (sinusoidal)
        if text[-1] == 'g':                     # accelerations in g
            unit, text = 9.8, text[:-1]
        elif text[-1] == 'd':                   # angular rates in deg/s
            unit, text = attitude.D2R, text[:-1]
        try:
            amp = unit * np.array(text[1:-1].split(' '), dtype='float64')
            vib['x'], vib['y'], vib['z'] = amp[0], amp[1], amp[2]
        except Exception:
            raise ValueError('Cannot convert \'%s\' to float' % text[1:-1].split(' '))
        return vib

    @staticmethod
    def _parse_mode(mode):
        """Sim.__parse_mode (ins_sim.py:612-640)."""
        if mode is None or isinstance(mode, str):
            return high_mobility
        if isinstance(mode, np.ndarray):
            if mode.shape != (3,):
                raise TypeError('mode should be of size (3,)')
            m = mode.astype(np.float64)
            m[1] *= attitude.D2R
            m[2] *= attitude.D2R
            return m
        raise TypeError('mode should be a string or a numpy array of size (3,)')

    @staticmethod
    def _check_data_dir(data_dir):
        """Sim.__check_data_dir (ins_sim.py:703-727)."""
        if data_dir == '':
            data_dir = os.path.join(os.path.abspath('.//demo_saved_data//'),
                                    time.strftime('%Y-%m-%d-%H-%M-%S', time.localtime()))
        data_dir = os.path.abspath(data_dir)
        if not os.path.exists(data_dir):
            try:
                os.makedirs(data_dir)
            except Exception:
                raise IOError('Cannot create dir: %s.' % data_dir)
        return data_dir
