#!/usr/bin/env python3
"""Error-growth curve benchmark on BASELINE config 2 (65 536 runs x 1000 samples, fp64, trajectories kept, placed planes).

    python tools/bench_error_curve.py                      one JSON line: wall time of every call (host copy included)
    rocprofv3 --kernel-trace --stats -d DIR -o curve -- python tools/bench_error_curve.py
    python tools/bench_error_curve.py --summarize DIR OUT.csv   per kernel and grid: calls / avg / min / max of that trace

The yardstick is process_stats_kernel<double>: it reads exactly the same 72 B per sample*run from the same planes.  In one
process, one after the other: the yardstick, the curve over every sample, the 1 Hz curve, the NED curve, and the curve of a
64-run job (latency-bound)."""
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
        w.writerow(['# rocprofv3 --kernel-trace --stats -- python tools/bench_error_curve.py  (C2 planes: 65 536 runs x 1000 samples, fp64, placed; '
                    'REPS calls of each after WARM)'])
        w.writerow(['kernel', 'calls', 'avg_ns', 'min_ns', 'max_ns', 'vgpr', 'sgpr', 'lds_bytes', 'grid_x', 'workgroup_x'])
        for r in rows:
            if any(k in r[0] for k in ('curve_', 'process_stats_kernel', 'stats_partial', 'stats_final')):
                w.writerow([r[0], r[1], int(r[2]), int(r[3]), int(r[4])] + list(r[5:]))
    print(open(dst).read())


def main():
    import numpy as np
    import ginsim
    from ginsim import workloads
    runs, fs, rf = int(os.environ.get('RUNS', 65536)), 100.0, int(os.environ.get('RF', 1))
    warm, reps = int(os.environ.get('WARM', 10)), int(os.environ.get('REPS', 20))
    ctx = ginsim.Context(0)
    acc, gyr = workloads.imu_grade('mid-accuracy')

    def job_of(frame, count):
        ini, truth, _ = workloads.truth_from_profile('turn_90deg', fs, frame)
        return ginsim.MonteCarloJob(ctx, fs, frame, truth, acc, gyr, ini, runs=count, seed=1, keep_traj=True).run()

    def timed(fn):
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {'ms_wall_min': min(ts), 'ms_wall_avg': sum(ts) / len(ts)}

    job = job_of(rf, runs)
    n = job.n
    one_hz = np.arange(0, n, int(fs))
    out = {'libginsim_sha256': lib_hash(), 'runs': runs, 'n': n, 'ref_frame': rf, 'placed': job.placement()['placed'],
           'algorithmic_bytes': 72.0 * runs * n}
    out['process_stats (yardstick, 14 MB copied back)'] = timed(lambda: job.process_stats('free', 0))
    out['error_curve every sample'] = timed(lambda: job.error_curve('free'))
    out['error_curve 1 Hz'] = timed(lambda: job.error_curve('free', one_hz))
    job.release()
    ned = job_of(0, runs)
    out['error_curve every sample, NED (ref_frame 0)'] = timed(lambda: ned.error_curve('free', pos_ned=True))
    ned.release()
    small = job_of(rf, 64)
    out['error_curve every sample, 64 runs'] = timed(lambda: small.error_curve('free'))
    small.release()
    f32 = ginsim.MonteCarloJob(ctx, fs, rf, workloads.truth_from_profile('turn_90deg', fs, rf)[1], acc, gyr,
                               workloads.truth_from_profile('turn_90deg', fs, rf)[0], runs=runs, seed=1, keep_traj=True, precision='f32').run()
    out['error_curve every sample, fp32 series'] = timed(lambda: f32.error_curve('free'))
    f32.release()
    print(json.dumps(out))


if __name__ == '__main__':
    if len(sys.argv) > 3 and sys.argv[1] == '--summarize':
        summarize(sys.argv[2], sys.argv[3])
    else:
        main()
