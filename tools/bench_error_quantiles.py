#!/usr/bin/env python3
"""Error-quantile benchmark on BASELINE config 2 (65 536 runs x 1000 samples, fp64, trajectories kept, placed planes).

    python tools/bench_error_quantiles.py [OUT.json]       one JSON line: the median wall time of every call (synchronised)
    rocprofv3 --kernel-trace --stats -d DIR -o quant -- python tools/bench_error_quantiles.py
    python tools/bench_error_quantiles.py --summarize DIR OUT.csv   per kernel and grid: calls / avg / min / max of that trace

At every sample and at 1 Hz, CEP50 / CEP95 of the position error (probs 0.5, 0.95; three key rows per sample), in one process, one
after the other:
    keys        ginsim_radial_keys: 24 B read and 24 B written per sample*run
    select      ginsim_quantile_rows over the 3 m key rows (only 3 m x 2 results and 3 m counts come back)
    curve       ginsim_error_curve over the same samples: the moments a user gets today (72 B read per sample*run)
    host        what a user can do today for the same quantiles: bring the same keys to the host and np.partition every row at
                the same ranks -- timed WITHOUT the key launch, so it is compared with the select alone and with keys + select
The one condition of the feature: keys + select is faster than host at both sample sets ('device_beats_host')."""
import csv
import glob
import hashlib
import json
import os
import sqlite3
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, 'gnss-ins-sim_amd'), REPO]

PROBS = (0.5, 0.95)


def lib_hash():
    import ginsim
    return hashlib.sha256(open(ginsim.LIB_PATH, 'rb').read()).hexdigest()[:16]


def summarize(src, dst):
    hits = sorted(glob.glob(os.path.join(src, '**', '*.db'), recursive=True))
    con = sqlite3.connect(hits[0])
    rows = list(con.execute("select name, count(*), avg(end-start), min(end-start), max(end-start), max(vgpr_count), max(sgpr_count), "
                            "max(lds_size), grid_x, max(workgroup_x) from kernels group by name, grid_x order by sum(end-start) desc"))
    with open(dst, 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['# libginsim.so sha256[:16] = %s' % lib_hash()])
        w.writerow(['# rocprofv3 --kernel-trace --stats -- python tools/bench_error_quantiles.py  (C2 planes: 65 536 runs x 1000 samples, fp64, '
                    'placed; REPS calls of each after WARM)'])
        w.writerow(['kernel', 'calls', 'avg_ns', 'min_ns', 'max_ns', 'vgpr', 'sgpr', 'lds_bytes', 'grid_x', 'workgroup_x'])
        for r in rows:
            if any(k in r[0] for k in ('radial_keys_kernel', 'quantile_rows_kernel', 'curve_')):
                w.writerow([r[0], r[1], int(r[2]), int(r[3]), int(r[4])] + list(r[5:]))
    print(open(dst).read())


def main(dst=None):
    import numpy as np
    import ginsim
    from ginsim import workloads
    runs, fs, rf = int(os.environ.get('RUNS', 65536)), 100.0, int(os.environ.get('RF', 1))
    warm, reps, host_reps = int(os.environ.get('WARM', 5)), int(os.environ.get('REPS', 21)), int(os.environ.get('HOST_REPS', 3))
    ctx = ginsim.Context(0)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    ini, truth, _ = workloads.truth_from_profile('turn_90deg', fs, rf)
    job = ginsim.MonteCarloJob(ctx, fs, rf, truth, acc, gyr, ini, runs=runs, seed=1, keep_traj=True).run()
    n = job.n

    def timed(fn, warm=warm, reps=reps):
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {'ms_median': float(np.median(ts)), 'ms_min': min(ts), 'ms_max': max(ts), 'reps': reps}

    def host_quantiles(keys, m):
        rows = ctx.download(keys, (3 * m, runs))
        N = runs                                        # every key of this job is finite
        ks = sorted(set(int(min(max(np.ceil(p * N), 1), N)) - 1 for p in PROBS))
        return np.partition(rows, ks, axis=1)[:, ks]

    out = {'libginsim_sha256': lib_hash(), 'runs': runs, 'n': n, 'ref_frame': rf, 'placed': job.placement()['placed'], 'probs': PROBS,
           'method': 'time.perf_counter around calls that end in a stream synchronise; median of `reps` after `warm` warm-up calls'}
    for name, samples in (('every sample', None), ('1 Hz', np.arange(0, n, int(fs)))):
        m = n if samples is None else samples.size
        keys = job.radial_keys('free', samples, 0)
        leg = {'m': m, 'key_rows': 3 * m, 'key_bytes': 24 * m * runs}
        leg['keys'] = timed(lambda: job.radial_keys('free', samples, 0, out=keys))
        leg['select'] = timed(lambda: ginsim.quantile_rows(ctx, keys, 3 * m, runs, runs, PROBS))
        leg['curve'] = timed(lambda: job.error_curve('free', samples))
        leg['host'] = timed(lambda: host_quantiles(keys, m), warm=1, reps=host_reps)
        dev = ginsim.quantile_rows(ctx, keys, 3 * m, runs, runs, PROBS)
        assert np.array_equal(dev.values, host_quantiles(keys, m)) and np.all(dev.count == runs)     # the same numbers
        leg['device_ms'] = leg['keys']['ms_median'] + leg['select']['ms_median']
        leg['device_beats_host'] = bool(leg['device_ms'] < leg['host']['ms_median'])
        keys.free()
        out[name] = leg
    job.release()
    line = json.dumps(out)
    print(line)
    if dst:
        with open(dst, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    if len(sys.argv) > 3 and sys.argv[1] == '--summarize':
        summarize(sys.argv[2], sys.argv[3])
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else None)
