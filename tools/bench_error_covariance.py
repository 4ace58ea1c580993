#!/usr/bin/env python3
"""Error-covariance benchmark on BASELINE config 2 (65 536 runs x 1000 samples, fp64, trajectories kept, placed planes).

    python tools/bench_error_covariance.py [OUT.json]      one JSON line: the median wall time of every call (synchronised)
    rocprofv3 --kernel-trace --stats -d DIR -o cov -- python tools/bench_error_covariance.py
    python tools/bench_error_covariance.py --summarize DIR OUT.csv   per kernel and grid: calls / avg / min / max of that trace

At every sample and at 1 Hz, the covariance of the position error, in one process, the two device calls ALTERNATED (cov, curve, cov,
curve, ...) so that both see the same clocks and the same state of the caches:
    cov         ginsim_error_cov: 24 B read per sample*run, m records of 10 doubles come back
    curve       ginsim_error_curve over the same samples: the per-component moments a user gets today (72 B read per sample*run)
    host        what a user can do today for the same numbers: download the three position planes at those samples and take np.mean and
                np.cov(bias=True) per instant
The one condition of the feature: cov is faster than host at both sample sets ('device_beats_host').  The yardstick: cov should not
be slower than curve ('cov_not_slower_than_curve').  The tool asserts that cov and host give the same values: per entry
|dC_ab| / sqrt(C_aa C_bb) and |dmean_a| / max(|mean_a|, sigma_a) at most 16 x max(distance of np.cov from a long-double two-pass
evaluation, eps), at every instant of the 1 Hz set and at 50 instants spread over the every-sample set."""
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

UPPER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


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
        w.writerow(['# rocprofv3 --kernel-trace --stats -- python tools/bench_error_covariance.py  (C2 planes: 65 536 runs x 1000 samples, '
                    'fp64, placed; REPS alternated calls of each after WARM)'])
        w.writerow(['kernel', 'calls', 'avg_ns', 'min_ns', 'max_ns', 'vgpr', 'sgpr', 'lds_bytes', 'grid_x', 'workgroup_x'])
        for r in rows:
            if any(k in r[0] for k in ('cov_partial_kernel', 'cov_final_kernel', 'curve_')):
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
    base = job.buffer('traj_free').ptr
    ref_pos = np.asarray(truth['ref_pos'], dtype=np.float64)

    def stats(ts):
        return {'ms_median': float(np.median(ts)), 'ms_min': min(ts), 'ms_max': max(ts), 'reps': len(ts)}

    def timed(fn, warm=warm, reps=reps):
        return timed_alternated((fn,), warm, reps)[0]

    def timed_alternated(fns, warm=warm, reps=reps):
        for _ in range(warm):
            for fn in fns:
                fn()
        ts = [[] for _ in fns]
        for _ in range(reps):
            for k, fn in enumerate(fns):
                t0 = time.perf_counter()
                fn()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        return [stats(t) for t in ts]

    def host_errors(samples):
        """(m, runs, 3): the three position planes at `samples`, downloaded, minus the truth."""
        if samples is None:
            x = np.stack([ctx.download(base + (3 + c) * n * runs * 8, (n, runs)) for c in range(3)], axis=2)
            return x - ref_pos[:, None, :]
        x = np.stack([np.stack([ctx.download(base + ((3 + c) * n + int(j)) * runs * 8, (runs,)) for c in range(3)], axis=1) for j in samples])
        return x - ref_pos[samples][:, None, :]

    def host_cov(samples):
        e = host_errors(samples)
        return np.mean(e, axis=1), np.stack([np.cov(e[k].T, bias=True) for k in range(e.shape[0])]), e

    def over(d, scale):
        """max of d / scale; where the scale is 0 (every run has the same error) only d = 0 will do"""
        with np.errstate(invalid='ignore', divide='ignore'):
            return float(np.max(np.where(scale > 0.0, d / scale, np.where(d > 0.0, np.inf, 0.0))))

    def same_values(dev, samples, check):
        """The device record against np.mean / np.cov at the instants `check` of the sample set: the bound of the header."""
        mean, cov, e = host_cov(samples)
        worst, eps = 0.0, np.finfo(np.float64).eps
        for k in check:
            x = e[k].astype(np.longdouble)
            mu = x.mean(axis=0)
            d = x - mu
            ext = (d.T @ d) / np.longdouble(runs)
            sig = np.sqrt(np.diag(ext)).astype(np.float64)
            sm, sc = np.maximum(np.abs(mu.astype(np.float64)), sig), np.outer(sig, sig)
            E = max(over(np.abs(cov[k] - ext.astype(np.float64)), sc), over(np.abs(mean[k] - mu.astype(np.float64)), sm))
            bound = 16.0 * max(E, eps)
            got = max(over(np.abs(dev.cov[k] - cov[k]), sc), over(np.abs(dev.mean[k] - mean[k]), sm))
            assert dev.count[k] == runs and got <= bound, (k, got, bound)
            worst = max(worst, got / bound)
        return worst

    out = {'libginsim_sha256': lib_hash(), 'runs': runs, 'n': n, 'ref_frame': rf, 'placed': job.placement()['placed'],
           'method': 'time.perf_counter around calls that end in a stream synchronise; median of `reps` after `warm` warm-up calls; '
                     'cov and curve alternated call by call'}
    for name, samples in (('every sample', None), ('1 Hz', np.arange(0, n, int(fs)))):
        m = n if samples is None else samples.size
        leg = {'m': m, 'cov_bytes_read': 24 * m * runs, 'curve_bytes_read': 72 * m * runs}
        leg['cov'], leg['curve'] = timed_alternated((lambda: job.error_cov('free', samples, 0), lambda: job.error_curve('free', samples)))
        leg['cov_alone'] = timed(lambda: job.error_cov('free', samples, 0))
        leg['host'] = timed(lambda: host_cov(samples)[1], warm=1, reps=host_reps)
        check = range(m) if m <= 50 else np.linspace(0, m - 1, 50).astype(int)
        leg['largest_distance_over_bound'] = same_values(job.error_cov('free', samples, 0), samples, check)
        leg['cov_GBps'] = leg['cov_bytes_read'] / (leg['cov']['ms_median'] * 1e-3) / 1e9
        leg['curve_GBps'] = leg['curve_bytes_read'] / (leg['curve']['ms_median'] * 1e-3) / 1e9
        leg['device_beats_host'] = bool(leg['cov']['ms_median'] < leg['host']['ms_median'])
        leg['cov_not_slower_than_curve'] = bool(leg['cov']['ms_median'] <= leg['curve']['ms_median'])
        out[name] = leg
    job.release()
    line = json.dumps(out)
    print(line)
    if dst:
        with open(dst, 'w') as f:
            f.write(line + '\n')
    for name in ('every sample', '1 Hz'):
        assert out[name]['device_beats_host'], (name, out[name])


if __name__ == '__main__':
    if len(sys.argv) > 3 and sys.argv[1] == '--summarize':
        summarize(sys.argv[2], sys.argv[3])
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else None)
