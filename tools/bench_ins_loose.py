#!/usr/bin/env python3
"""Kernel time of the loosely coupled GPS/INS filter (csrc/ins_loose.hip) against its arithmetic floor.

    python tools/bench_ins_loose.py --isa                 # no GPU: fp64 instructions of the kernels' time loops, counted in the ISA
    python tools/bench_ins_loose.py [--runs 65536] [--reps 5] [--out profiles/ins_loose_timing.json]
    python tools/bench_ins_loose.py --aided [--reps 20] [--out profiles/ins_loose_aided_timing.json]
    python tools/bench_ins_loose.py --cons [--reps 20] [--out profiles/ins_loose_cons_timing.json]
    python tools/bench_ins_loose.py --mag [--reps 20] [--out profiles/ins_loose_mag_timing.json]
    python tools/bench_ins_loose.py --odo-scale [--reps 20] [--out profiles/ins_loose_scale_timing.json]
    python tools/bench_ins_loose.py --still [--reps 20] [--out profiles/ins_loose_still_timing.json]
    python tools/bench_ins_loose.py --combined [--reps 20] [--out profiles/ins_loose_all_timing.json]
    python tools/bench_ins_loose.py --combined-cons [--reps 20] [--out profiles/ins_loose_all_cons_timing.json]

Workload: 65 536 runs x the 1000 samples of the 90-degree turn at 100 Hz (BASELINE config C2's shape) with GPS at 10 Hz, ref_frame 1,
'mid-accuracy' IMU; statistics only (nothing but the per-run end records is written) and with everything kept (trajectory, wb, ab).
Times are HIP-event times of the launch alone (the job's buffers exist before the timer starts), the median of --reps launches
after one warm-up.

The arithmetic: the file is compiled to assembly with the build's flags and, for the instantiation each job launches
(InsLooseJob.kernel_name), the fp64 VALU instructions (v_fma_f64, v_mul_f64, v_add_f64, ...; a fused multiply-add is one
instruction) of the TIME LOOP are counted: the span of the kernel's longest backward branch, which leaves out the initialisation
of P and the epilogue.  The loop's text also holds the correction (six scalar updates), which one step in ten executes here, so
the count is an UPPER bound of a step's arithmetic and the time over the floor printed from it a LOWER bound.
Floor = instructions x runs x steps / (256 CUs x 4 SIMDs x 16 fp64 lanes per clock x 2.4 GHz).  --ops N overrides the count.
No threshold is set here.

--aided: the odometer / non-holonomic aiding of csrc/ins_loose_aided.hip on the same case, statistics only: the
unaided launch and aid_mask 7 at aid_every 1 and 10 (odometer scale 0.99, stdv 0.1, NHC sigma 0.05 m/s), launched in turn --reps
times after one warm-up each, so that a drift of the clocks falls on all three alike.  --unaided-only times the first leg alone
(a library without the aiding fields, named by $GINSIM_LIB, can run it: the comparison against an earlier build).

--cons: the consistency checkpoints of csrc/ins_loose_cons.hip on the same case, statistics only: the unaided launch
without checkpoints, with one every 100 samples and with one at every sample, launched in turn --reps times after one warm-up each.
The times with checkpoints include the kernel that adds the wavefronts' partial records.  A checkpoint's cost is printed in steps:
(time with m checkpoints - time without) / m over the time of one step of the launch without.

--mag: the magnetometer block of csrc/ins_loose_mag.hip on the same case, statistics only: the unaided launch, the
magnetometer block at mag_every 1 and 10, and aid_mask 7 together with the magnetometer (both at every sample), launched in turn
--reps times after one warm-up each (field (30, -3, 40) uT, no soft or hard iron, noise 0.01 uT).

--odo-scale: the odometer's scale factor as a 16th state (csrc/ins_loose_scale.hip) on the same case, statistics only:
the 15-state aided launch (aid_mask 7) and the 16-state launch, each at aid_every 1 and 10, launched in turn --reps times after one
warm-up each.  The price is the 16-state time over the 15-state time of the same library; the arithmetic on P grows by 136/120.

--still: the standstill block of csrc/ins_loose_still.hip, statistics only, on two profiles at 100 Hz with GPS at 10 Hz:
the 90-degree turn (no sample is flagged: the price of the compiled-in test alone) and the stops profile
(tests/golden/ins_loose/motion_def_stops.csv, 5500 samples).  On each: the unaided launch and the launch with both rows; on the stops
profile also each row alone; launched in turn --reps times after one warm-up each.

--combined: every aid in one launch (csrc/ins_loose_all.hip), statistics only, on the same two profiles: the unaided
launch, each single family (aid_mask 7; the magnetometer; aid_mask 7 with the scale-factor state; both standstill rows) and the
combined launch with 15 states (aid_mask 7, magnetometer, standstill) and with 16 (and the scale-factor state), every block at every
sample, launched in turn --reps times after one warm-up each.  Printed beside the ratios over the unaided launch: the combined
launch's excess over the unaided launch against the sum of the excesses of the single families it replaces.

--combined-cons: the consistency checkpoints of csrc/ins_loose_all_cons.hip on --cons' case, statistics only: the
combined 16-state launch (aid_mask 7, magnetometer, scale-factor state, standstill, every block at every sample) without checkpoints
(loose_all_kernel), and loose_all_cons_kernel with a checkpoint every 100 samples and with one at every sample, launched in turn
--reps times after one warm-up each.  A checkpoint's cost is printed in steps of the launch without, as --cons prints it."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PKG = os.path.join(REPO, 'gnss-ins-sim_amd')
sys.path.insert(0, PKG)
CLOCK_HZ = 2.4e9
FP64_LANES_PER_CLOCK = 256 * 4 * 16


def isa_counts():
    """{kernel name: (fp64 VALU instructions, of them fused multiply-adds)} from the assembly of csrc/ins_loose.hip."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('ginsim_build', os.path.join(PKG, 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    flags = dict(b.SOURCES)['ins_loose.hip']
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'ins_loose.s')
        subprocess.check_call([b.HIPCC] + b.COMMON + list(flags) + ['-S', '--cuda-device-only', os.path.join(b.CSRC, 'ins_loose.hip'), '-o', out],
                              stderr=subprocess.DEVNULL)
        text = open(out).read()
    return {k: count_loop(body) for k, body in kernel_bodies(text).items()}


def kernel_bodies(text):
    """{mangled kernel name: its instruction lines} of an AMDGPU assembly file."""
    res, cur = {}, None
    for line in text.splitlines():
        m = re.match(r'^(_ZN6ginsim12loose_kernel\w+):', line)
        if m:
            cur = m.group(1)
            res[cur] = []
        elif cur and '.end_amdhsa_kernel' in line:
            cur = None
        elif cur:
            res[cur].append(line)
    return res


def count_loop(lines):
    """(fp64 VALU instructions, of them fused multiply-adds, lines of the span) of the longest backward branch of a kernel."""
    labels = {}
    for i, line in enumerate(lines):
        m = re.match(r'^(\.?[A-Za-z_][\w.$]*):', line.strip())
        if m:
            labels[m.group(1)] = i
    lo, hi = 0, len(lines)
    best = 0
    for i, line in enumerate(lines):
        t = line.split()
        if len(t) >= 2 and (t[0].startswith('s_cbranch') or t[0] == 's_branch') and labels.get(t[1], i) < i and i - labels[t[1]] > best:
            best, lo, hi = i - labels[t[1]], labels[t[1]], i
    n = f = 0
    for line in lines[lo:hi]:
        op = line.split()[0] if line.split() else ''
        if re.match(r'^v_\w+_f64', op) and not op.startswith('v_cvt') and not op.startswith('v_cmp'):
            n += 1
            f += op.startswith('v_fma_f64')
    return n, f, hi - lo


def mangled_prefix(kernel_name):
    """'ginsim::loose_kernel<1, false, false, false>' -> '_ZN6ginsim12loose_kernelILi1ELb0ELb0ELb0EEE'."""
    args = [a.strip() for a in kernel_name[kernel_name.index('<') + 1:kernel_name.rindex('>')].split(',')]
    return '_ZN6ginsim12loose_kernelILi%sE' % args[0] + ''.join('Lb%dE' % (a == 'true') for a in args[1:]) + 'EE'


def time_launches(runs, reps):
    import numpy as np
    import ginsim
    from ginsim import workloads
    fs, rf = 100.0, 1
    ini, truth, _ = workloads.truth_from_profile('turn_90deg', fs, rf, fs_gps=10.0, gps=True)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    gps_err = {'stdp': np.array([5.0, 5.0, 7.0]), 'stdv': np.array([0.05, 0.05, 0.05])}
    ctx = ginsim.Context(0)
    out = {'device': ctx.name(), 'runs': runs, 'samples': int(truth['ref_accel'].shape[0]), 'fixes': int(truth['ref_gps'].shape[0])}
    for label, keep in (('statistics_only', False), ('everything_kept', True)):
        job = ginsim.InsLooseJob(ctx, fs, rf, truth, acc, gyr, gps_err, ini, runs, seed=1, keep_traj=keep)
        job.run()                                   # warm-up: code object, LDS attribute
        ms = []
        for _ in range(reps):
            ctx.timer_begin()
            job.launch()
            ms.append(ctx.timer_end())
        out[label] = {'kernel': job.kernel_name(), 'ms_median': float(np.median(ms)), 'ms_all': [float(x) for x in ms],
                      'bytes_written': (15 * out['samples'] * 8 if keep else 0) * runs + 30 * 8 * runs}
        job.release()
    ctx.close()
    return out


def time_aided(runs, reps, unaided_only=False):
    """{leg: {'kernel', 'ms_median', 'ms_min', 'ms_max', 'ms_all'}} of the unaided launch and the two aided ones, interleaved."""
    import numpy as np
    import ginsim
    from ginsim import workloads
    fs, rf = 100.0, 1
    ini, truth, _ = workloads.truth_from_profile('turn_90deg', fs, rf, fs_gps=10.0, gps=True)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    gps_err = {'stdp': np.array([5.0, 5.0, 7.0]), 'stdv': np.array([0.05, 0.05, 0.05])}
    odo_err = {'scale': 0.99, 'stdv': 0.1}
    ctx = ginsim.Context(0)
    out = {'device': ctx.name(), 'runs': runs, 'samples': int(truth['ref_accel'].shape[0]), 'fixes': int(truth['ref_gps'].shape[0]),
           'library': os.path.basename(ginsim.LIB_PATH)}
    legs = [('unaided', {})]
    if not unaided_only:
        legs += [('aided_mask7_every1', {'odo_err': odo_err, 'aid': {'odo': True, 'nhc': True, 'every': 1}}),
                 ('aided_mask7_every10', {'odo_err': odo_err, 'aid': {'odo': True, 'nhc': True, 'every': 10}})]
    jobs = [(label, ginsim.InsLooseJob(ctx, fs, rf, truth, acc, gyr, gps_err, ini, runs, seed=1, keep_traj=False, **kw)) for label, kw in legs]
    ms = {label: [] for label, _ in jobs}
    for _, job in jobs:
        job.run()                                       # warm-up: code object, LDS attribute
    for _ in range(reps):
        for label, job in jobs:
            ctx.timer_begin()
            job.launch()
            ms[label].append(ctx.timer_end())
    for label, job in jobs:
        t = ms[label]
        out[label] = {'kernel': job.kernel_name(), 'ms_median': float(np.median(t)), 'ms_min': float(np.min(t)), 'ms_max': float(np.max(t)),
                      'ms_all': [float(x) for x in t]}
        job.release()
    for label, _ in jobs[1:]:
        out[label]['over_unaided'] = out[label]['ms_median'] / out['unaided']['ms_median']
    ctx.close()
    return out


def time_mag(runs, reps):
    """{leg: {'kernel', 'ms_median', 'ms_min', 'ms_max', 'ms_all'}} of the unaided launch, the magnetometer block at mag_every 1 and
    10 and aid_mask 7 together with the magnetometer, interleaved."""
    import numpy as np
    import ginsim
    from ginsim import workloads
    fs, rf, geo = 100.0, 1, (30.0, -3.0, 40.0)
    ini, truth, _ = workloads.truth_from_profile('turn_90deg', fs, rf, fs_gps=10.0, gps=True)
    ini_m, seg = workloads.parse_motion(workloads.profile_path('turn_90deg'))
    raw = ginsim.pathgen(ini_m, seg, fs, 10.0, workloads.HIGH_MOBILITY, rf, gps=True, geo_mag_n=geo)
    n = int(truth['ref_accel'].shape[0])
    truth = dict(truth, ref_mag=np.ascontiguousarray(raw['mag'][:n, 1:4]))
    acc, gyr = workloads.imu_grade('mid-accuracy')
    gps_err = {'stdp': np.array([5.0, 5.0, 7.0]), 'stdv': np.array([0.05, 0.05, 0.05])}
    odo_err = {'scale': 0.99, 'stdv': 0.1}
    mag_err = {'si': np.eye(3), 'hi': np.zeros(3), 'std': np.array([0.01, 0.01, 0.01])}
    ctx = ginsim.Context(0)
    out = {'device': ctx.name(), 'runs': runs, 'samples': n, 'fixes': int(truth['ref_gps'].shape[0]), 'library': os.path.basename(ginsim.LIB_PATH)}
    mag = lambda every: {'mag_err': mag_err, 'geo_mag_n': geo, 'mag': {'every': every}}
    legs = [('unaided', {}), ('mag_every1', mag(1)), ('mag_every10', mag(10)),
            ('aided_mask7_mag_every1', dict(mag(1), odo_err=odo_err, aid={'odo': True, 'nhc': True, 'every': 1}))]
    jobs = [(label, ginsim.InsLooseJob(ctx, fs, rf, truth, acc, gyr, gps_err, ini, runs, seed=1, keep_traj=False, **kw)) for label, kw in legs]
    ms = {label: [] for label, _ in jobs}
    for _, job in jobs:
        job.run()                                       # warm-up: code object, LDS attribute
    for _ in range(reps):
        for label, job in jobs:
            ctx.timer_begin()
            job.launch()
            ms[label].append(ctx.timer_end())
    for label, job in jobs:
        t = ms[label]
        out[label] = {'kernel': job.kernel_name(), 'ms_median': float(np.median(t)), 'ms_min': float(np.min(t)), 'ms_max': float(np.max(t)),
                      'ms_all': [float(x) for x in t]}
        job.release()
    for label, _ in jobs[1:]:
        out[label]['over_unaided'] = out[label]['ms_median'] / out['unaided']['ms_median']
    ctx.close()
    return out


def time_scale(runs, reps):
    """{leg: {'kernel', 'ms_median', 'ms_min', 'ms_max', 'ms_all'}} of the 15-state aided launch and the 16-state launch at
    aid_every 1 and 10, interleaved; 'over_aided': the 16-state leg over the 15-state leg of the same period."""
    import numpy as np
    import ginsim
    from ginsim import workloads
    fs, rf = 100.0, 1
    ini, truth, _ = workloads.truth_from_profile('turn_90deg', fs, rf, fs_gps=10.0, gps=True)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    gps_err = {'stdp': np.array([5.0, 5.0, 7.0]), 'stdv': np.array([0.05, 0.05, 0.05])}
    odo_err = {'scale': 0.99, 'stdv': 0.1}
    ctx = ginsim.Context(0)
    out = {'device': ctx.name(), 'runs': runs, 'samples': int(truth['ref_accel'].shape[0]), 'fixes': int(truth['ref_gps'].shape[0]),
           'library': os.path.basename(ginsim.LIB_PATH)}
    aid = lambda every: {'odo_err': odo_err, 'aid': {'odo': True, 'nhc': True, 'every': every}}
    legs = [('aided_mask7_every1', aid(1)), ('scale_mask7_every1', dict(aid(1), odo_scale_state={})),
            ('aided_mask7_every10', aid(10)), ('scale_mask7_every10', dict(aid(10), odo_scale_state={}))]
    jobs = [(label, ginsim.InsLooseJob(ctx, fs, rf, truth, acc, gyr, gps_err, ini, runs, seed=1, keep_traj=False, **kw)) for label, kw in legs]
    ms = {label: [] for label, _ in jobs}
    for _, job in jobs:
        job.run()                                       # warm-up: code object, LDS attribute
    for _ in range(reps):
        for label, job in jobs:
            ctx.timer_begin()
            job.launch()
            ms[label].append(ctx.timer_end())
    for label, job in jobs:
        t = ms[label]
        out[label] = {'kernel': job.kernel_name(), 'ms_median': float(np.median(t)), 'ms_min': float(np.min(t)), 'ms_max': float(np.max(t)),
                      'ms_all': [float(x) for x in t]}
        job.release()
    for every in (1, 10):
        out['scale_mask7_every%d' % every]['over_aided'] = out['scale_mask7_every%d' % every]['ms_median'] / out['aided_mask7_every%d' % every]['ms_median']
    ctx.close()
    return out


def time_still(runs, reps):
    """{profile: {leg: {'kernel', 'ms_median', 'ms_min', 'ms_max', 'ms_all', 'over_unaided'}}} of the unaided launch and the launches
    with the standstill block on the 90-degree turn and on the stops profile, interleaved per profile."""
    import numpy as np
    import ginsim
    from ginsim import workloads
    fs, fs_gps, rf = 100.0, 10.0, 1
    acc, gyr = workloads.imu_grade('mid-accuracy')
    gps_err = {'stdp': np.array([5.0, 5.0, 7.0]), 'stdv': np.array([0.05, 0.05, 0.05])}
    ctx = ginsim.Context(0)
    out = {'device': ctx.name(), 'runs': runs, 'library': os.path.basename(ginsim.LIB_PATH)}

    def stops():
        ini, seg = workloads.parse_motion(os.path.join(REPO, 'tests', 'golden', 'ins_loose', 'motion_def_stops.csv'))
        raw = ginsim.pathgen(ini, seg, fs, fs_gps, workloads.HIGH_MOBILITY, rf, gps=True)
        return ini, {'ref_accel': np.ascontiguousarray(raw['imu'][:, 1:4]), 'ref_gyro': np.ascontiguousarray(raw['imu'][:, 4:7]),
                     'ref_pos': np.ascontiguousarray(raw['nav'][:, 1:4]), 'ref_vel': np.ascontiguousarray(raw['nav'][:, 4:7]),
                     'ref_att': np.ascontiguousarray(raw['nav'][:, 7:10]), 'ref_gps': np.ascontiguousarray(raw['gps'][:, 1:7]),
                     'gps_time': raw['gps'][:, 0] / fs, 'gps_visibility': raw['gps'][:, 7].copy()}
    both, zupt, zaru = {'still': {}}, {'still': {'zaru': False}}, {'still': {'zupt': False}}
    for profile, (ini, truth), legs in (('turn_90deg', workloads.truth_from_profile('turn_90deg', fs, rf, fs_gps=fs_gps, gps=True)[:2],
                                         [('unaided', {}), ('still', both)]),
                                        ('stops', stops(), [('unaided', {}), ('still', both), ('zupt_only', zupt), ('zaru_only', zaru)])):
        res = out[profile] = {'samples': int(truth['ref_accel'].shape[0]), 'fixes': int(truth['ref_gps'].shape[0])}
        jobs = [(label, ginsim.InsLooseJob(ctx, fs, rf, truth, acc, gyr, gps_err, ini, runs, seed=1, keep_traj=False, **kw)) for label, kw in legs]
        res['flagged_samples'] = int(np.count_nonzero(jobs[1][1].still_flags))
        ms = {label: [] for label, _ in jobs}
        for _, job in jobs:
            job.run()                                       # warm-up: code object, LDS attribute
        for _ in range(reps):
            for label, job in jobs:
                ctx.timer_begin()
                job.launch()
                ms[label].append(ctx.timer_end())
        for label, job in jobs:
            t = ms[label]
            res[label] = {'kernel': job.kernel_name(), 'ms_median': float(np.median(t)), 'ms_min': float(np.min(t)), 'ms_max': float(np.max(t)),
                          'ms_all': [float(x) for x in t]}
            job.release()
        for label, _ in jobs[1:]:
            res[label]['over_unaided'] = res[label]['ms_median'] / res['unaided']['ms_median']
    ctx.close()
    return out


def time_combined(runs, reps):
    """{profile: {leg: {'kernel', 'ms_median', 'ms_min', 'ms_max', 'ms_all', 'over_unaided'}}} of the unaided launch, the four single
    families and the two combined launches on the 90-degree turn and on the stops profile, interleaved per profile; per combined leg
    also 'excess_over_sum': (its time - unaided) over the sum of (time - unaided) of the single families whose blocks it holds."""
    import numpy as np
    import ginsim
    from ginsim import workloads
    fs, fs_gps, rf, geo = 100.0, 10.0, 1, (30.0, -3.0, 40.0)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    gps_err = {'stdp': np.array([5.0, 5.0, 7.0]), 'stdv': np.array([0.05, 0.05, 0.05])}
    odo_err = {'scale': 0.99, 'stdv': 0.1}
    mag_err = {'si': np.eye(3), 'hi': np.zeros(3), 'std': np.array([0.01, 0.01, 0.01])}
    ctx = ginsim.Context(0)
    out = {'device': ctx.name(), 'runs': runs, 'library': os.path.basename(ginsim.LIB_PATH)}

    def truth_of(path):
        ini, seg = workloads.parse_motion(path)
        raw = ginsim.pathgen(ini, seg, fs, fs_gps, workloads.HIGH_MOBILITY, rf, gps=True, geo_mag_n=geo)
        n = raw['imu'].shape[0]
        return ini, {'ref_accel': np.ascontiguousarray(raw['imu'][:, 1:4]), 'ref_gyro': np.ascontiguousarray(raw['imu'][:, 4:7]),
                     'ref_pos': np.ascontiguousarray(raw['nav'][:, 1:4]), 'ref_vel': np.ascontiguousarray(raw['nav'][:, 4:7]),
                     'ref_att': np.ascontiguousarray(raw['nav'][:, 7:10]), 'ref_gps': np.ascontiguousarray(raw['gps'][:, 1:7]),
                     'gps_time': raw['gps'][:, 0] / fs, 'gps_visibility': raw['gps'][:, 7].copy(),
                     'ref_odo': np.ascontiguousarray(raw['odo'][:n, 2]), 'ref_mag': np.ascontiguousarray(raw['mag'][:n, 1:4])}
    aid = {'odo_err': odo_err, 'aid': {'odo': True, 'nhc': True, 'every': 1}}
    mag = {'mag_err': mag_err, 'geo_mag_n': geo, 'mag': {'every': 1}}
    legs = [('unaided', {}), ('aided_mask7', aid), ('mag', mag), ('scale_mask7', dict(aid, odo_scale_state={})), ('still', {'still': {}}),
            ('combined_15', dict(aid, still={}, combined=True, **mag)), ('combined_16', dict(aid, odo_scale_state={}, still={}, combined=True, **mag))]
    replaced = {'combined_15': ('aided_mask7', 'mag', 'still'), 'combined_16': ('scale_mask7', 'mag', 'still')}
    for profile, path in (('turn_90deg', workloads.profile_path('turn_90deg')),
                          ('stops', os.path.join(REPO, 'tests', 'golden', 'ins_loose', 'motion_def_stops.csv'))):
        ini, truth = truth_of(path)
        res = out[profile] = {'samples': int(truth['ref_accel'].shape[0]), 'fixes': int(truth['ref_gps'].shape[0])}
        jobs = [(label, ginsim.InsLooseJob(ctx, fs, rf, truth, acc, gyr, gps_err, ini, runs, seed=1, keep_traj=False, **kw)) for label, kw in legs]
        res['flagged_samples'] = int(np.count_nonzero(dict(jobs)['still'].still_flags))
        ms = {label: [] for label, _ in jobs}
        for _, job in jobs:
            job.run()                                       # warm-up: code object, LDS attribute
        for _ in range(reps):
            for label, job in jobs:
                ctx.timer_begin()
                job.launch()
                ms[label].append(ctx.timer_end())
        for label, job in jobs:
            t = ms[label]
            res[label] = {'kernel': job.kernel_name(), 'ms_median': float(np.median(t)), 'ms_min': float(np.min(t)), 'ms_max': float(np.max(t)),
                          'ms_all': [float(x) for x in t]}
            job.release()
        base = res['unaided']['ms_median']
        for label, _ in jobs[1:]:
            res[label]['over_unaided'] = res[label]['ms_median'] / base
        for label, singles in replaced.items():
            res[label]['excess_over_sum'] = (res[label]['ms_median'] - base) / sum(res[k]['ms_median'] - base for k in singles)
    ctx.close()
    return out


def time_combined_cons(runs, reps):
    """{leg: {'kernel', 'checkpoints', 'ms_median', 'ms_min', 'ms_max', 'ms_all'}} of the combined 16-state launch without checkpoints,
    with one every 100 samples and with one at every sample, interleaved; and what one checkpoint costs, in steps of the first."""
    import numpy as np
    import ginsim
    from ginsim import workloads
    fs, fs_gps, rf, geo = 100.0, 10.0, 1, (30.0, -3.0, 40.0)
    ini, seg = workloads.parse_motion(workloads.profile_path('turn_90deg'))
    raw = ginsim.pathgen(ini, seg, fs, fs_gps, workloads.HIGH_MOBILITY, rf, gps=True, geo_mag_n=geo)
    n = int(raw['imu'].shape[0])
    truth = {'ref_accel': np.ascontiguousarray(raw['imu'][:, 1:4]), 'ref_gyro': np.ascontiguousarray(raw['imu'][:, 4:7]),
             'ref_pos': np.ascontiguousarray(raw['nav'][:, 1:4]), 'ref_vel': np.ascontiguousarray(raw['nav'][:, 4:7]),
             'ref_att': np.ascontiguousarray(raw['nav'][:, 7:10]), 'ref_gps': np.ascontiguousarray(raw['gps'][:, 1:7]),
             'gps_time': raw['gps'][:, 0] / fs, 'gps_visibility': raw['gps'][:, 7].copy(),
             'ref_odo': np.ascontiguousarray(raw['odo'][:n, 2]), 'ref_mag': np.ascontiguousarray(raw['mag'][:n, 1:4])}
    acc, gyr = workloads.imu_grade('mid-accuracy')
    gps_err = {'stdp': np.array([5.0, 5.0, 7.0]), 'stdv': np.array([0.05, 0.05, 0.05])}
    every = dict(odo_err={'scale': 0.99, 'stdv': 0.1}, aid={'odo': True, 'nhc': True, 'every': 1}, odo_scale_state={}, still={}, combined=True,
                 mag_err={'si': np.eye(3), 'hi': np.zeros(3), 'std': np.array([0.01, 0.01, 0.01])}, geo_mag_n=geo, mag={'every': 1})
    ctx = ginsim.Context(0)
    out = {'device': ctx.name(), 'runs': runs, 'samples': n, 'fixes': int(truth['ref_gps'].shape[0]), 'library': os.path.basename(ginsim.LIB_PATH)}
    legs = [('no_checkpoints', None), ('every_100_samples', np.arange(0, n, 100)), ('every_sample', np.arange(n))]
    jobs = [(label, ginsim.InsLooseJob(ctx, fs, rf, truth, acc, gyr, gps_err, ini, runs, seed=1, keep_traj=False, checkpoints=c, **every))
            for label, c in legs]
    ms = {label: [] for label, _ in jobs}
    for _, job in jobs:
        job.run()                                       # warm-up: code object, LDS attribute
    for _ in range(reps):
        for label, job in jobs:
            ctx.timer_begin()
            job.launch()
            ms[label].append(ctx.timer_end())
    for (label, job), (_, c) in zip(jobs, legs):
        t = ms[label]
        out[label] = {'kernel': job.kernel_name(), 'checkpoints': 0 if c is None else int(c.size), 'ms_median': float(np.median(t)),
                      'ms_min': float(np.min(t)), 'ms_max': float(np.max(t)), 'ms_all': [float(x) for x in t]}
        job.release()
    step_ms = out['no_checkpoints']['ms_median'] / (n - 1)
    for label, _ in jobs[1:]:
        r = out[label]
        r['over_no_checkpoints'] = r['ms_median'] / out['no_checkpoints']['ms_median']
        r['checkpoint_cost_in_steps'] = (r['ms_median'] - out['no_checkpoints']['ms_median']) / r['checkpoints'] / step_ms
    ctx.close()
    return out


def time_cons(runs, reps):
    """{leg: {'kernel', 'checkpoints', 'ms_median', 'ms_min', 'ms_max', 'ms_all'}} of the unaided launch without checkpoints, with one
    every 100 samples and with one at every sample, interleaved; and what one checkpoint costs, in steps."""
    import numpy as np
    import ginsim
    from ginsim import workloads
    fs, rf = 100.0, 1
    ini, truth, _ = workloads.truth_from_profile('turn_90deg', fs, rf, fs_gps=10.0, gps=True)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    gps_err = {'stdp': np.array([5.0, 5.0, 7.0]), 'stdv': np.array([0.05, 0.05, 0.05])}
    n = int(truth['ref_accel'].shape[0])
    ctx = ginsim.Context(0)
    out = {'device': ctx.name(), 'runs': runs, 'samples': n, 'fixes': int(truth['ref_gps'].shape[0]), 'library': os.path.basename(ginsim.LIB_PATH)}
    legs = [('no_checkpoints', None), ('every_100_samples', np.arange(0, n, 100)), ('every_sample', np.arange(n))]
    jobs = [(label, ginsim.InsLooseJob(ctx, fs, rf, truth, acc, gyr, gps_err, ini, runs, seed=1, keep_traj=False, cons_samples=c)) for label, c in legs]
    ms = {label: [] for label, _ in jobs}
    for _, job in jobs:
        job.run()                                       # warm-up: code object, LDS attribute
    for _ in range(reps):
        for label, job in jobs:
            ctx.timer_begin()
            job.launch()
            ms[label].append(ctx.timer_end())
    for (label, job), (_, c) in zip(jobs, legs):
        t = ms[label]
        out[label] = {'kernel': job.kernel_name(), 'checkpoints': 0 if c is None else int(c.size), 'ms_median': float(np.median(t)),
                      'ms_min': float(np.min(t)), 'ms_max': float(np.max(t)), 'ms_all': [float(x) for x in t]}
        job.release()
    step_ms = out['no_checkpoints']['ms_median'] / (n - 1)
    for label, _ in jobs[1:]:
        r = out[label]
        r['over_no_checkpoints'] = r['ms_median'] / out['no_checkpoints']['ms_median']
        r['checkpoint_cost_in_steps'] = (r['ms_median'] - out['no_checkpoints']['ms_median']) / r['checkpoints'] / step_ms
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--isa', action='store_true')
    ap.add_argument('--aided', action='store_true', help='the aided leg: unaided, aid_mask 7 at aid_every 1 and 10')
    ap.add_argument('--unaided-only', action='store_true', help='with --aided: the unaided launch alone')
    ap.add_argument('--cons', action='store_true', help='the checkpoint leg: none, one every 100 samples, one at every sample')
    ap.add_argument('--mag', action='store_true', help='the magnetometer leg: unaided, mag_every 1 and 10, aid_mask 7 with the magnetometer')
    ap.add_argument('--odo-scale', action='store_true', help='the scale-factor leg: aid_mask 7 with 15 and with 16 states, aid_every 1 and 10')
    ap.add_argument('--still', action='store_true', help='the standstill leg: unaided and ZUPT / ZARU on the 90-degree turn and on the stops profile')
    ap.add_argument('--combined', action='store_true', help='every aid in one launch, with 15 and with 16 states, beside the unaided launch and each single family, on the 90-degree turn and on the stops profile')
    ap.add_argument('--combined-cons', action='store_true', help='the checkpoints of the combined 16-state launch: none, one every 100 samples, one at every sample')
    ap.add_argument('--runs', type=int, default=65536)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--ops', type=int, default=0, help='fp64 instructions per step, instead of the count from the ISA')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.isa:
        for k, (n, f, span) in sorted(isa_counts().items()):
            print('%s: %d fp64 VALU instructions (%d fused multiply-adds) in a time loop of %d lines' % (k, n, f, span))
        return
    if a.aided or a.cons or a.mag or a.odo_scale or a.still or a.combined or a.combined_cons:
        res = time_combined_cons(a.runs, a.reps) if a.combined_cons else time_combined(a.runs, a.reps) if a.combined else time_still(a.runs, a.reps) if a.still else time_scale(a.runs, a.reps) if a.odo_scale else time_mag(a.runs, a.reps) if a.mag else time_cons(a.runs, a.reps) if a.cons else time_aided(a.runs, a.reps, a.unaided_only)
        print(json.dumps(res))
        if a.out:
            with open(a.out, 'w') as f:
                json.dump(res, f, indent=1)
                f.write('\n')
        return
    res = time_launches(a.runs, a.reps)
    counts = {} if a.ops else isa_counts()
    for label in ('statistics_only', 'everything_kept'):
        r = res[label]
        ops = a.ops or next(v[0] for k, v in counts.items() if k.startswith(mangled_prefix(r['kernel'])))
        r['fp64_instructions_per_step'] = int(ops)
        r['floor_ms'] = ops * res['runs'] * (res['samples'] - 1) / (FP64_LANES_PER_CLOCK * CLOCK_HZ) * 1e3
        r['time_over_floor'] = r['ms_median'] / r['floor_ms']
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
