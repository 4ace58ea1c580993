#!/usr/bin/env python3
"""Overlapping Allan variance benchmark (BASELINE config 5's size: 192 series x 1 440 000 samples @ 400 Hz, 46 factors).

    python tools/bench_oallan.py [--launches 20] [--warmup 10] [--out profiles/oallan_timing.json] [--trace DIR]

HIP-event time of the call on one MI355X, `--launches` per leg after a warm-up, interleaved with ginsim_allan on the SAME buffer;
one leg with GINSIM_OALLAN_TILE=0 (every factor through the stream form); one leg at 6 x 1 440 000 against download + the
float64 NumPy restatement on the host.  Bytes are set against the cost model of DESIGN 4.3b.  Prints one JSON line and writes it to
--out.  --trace DIR measures nothing: it adds to the file at --out the time of each launch (scan, tile, stream, finish) from the
sqlite database that `rocprofv3 --kernel-trace -d DIR -- python tools/bench_oallan.py --no-host --out ''` left."""
import argparse
import glob
import json
import os
import re
import sqlite3
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, 'gnss-ins-sim_amd'), REPO]
import numpy as np      # noqa: E402


def restated(x, fs, mult):
    """The definition in float64 NumPy (tests/oallan_exact.py restated): a sequential cumsum of x - x[0], three taps per factor."""
    n = x.size
    th = np.concatenate([[0.0], np.cumsum(x - x[0])])
    return np.array([np.sum((th[2 * m:] - 2 * th[m:n + 1 - m] + th[:n + 1 - 2 * m]) ** 2) / (2.0 * float(m) * float(m) * (n - 2 * m + 1))
                     for m in mult])


def trace(d):
    hits = sorted(glob.glob(os.path.join(d, '**', '*.db'), recursive=True))
    if not hits:
        return None
    con = sqlite3.connect(hits[0])
    rows = con.execute("select name, grid_x, grid_y, grid_z, count(*), avg(end-start), min(end-start) from kernels "
                       "where name like '%allan%_kernel%' group by name, grid_x, grid_y, grid_z order by avg(end-start) desc")
    return [dict(kernel=re.search(r'(\w*allan\w*_kernel)', r[0]).group(1), grid_threads=[r[1], r[2], r[3]], launches=r[4], avg_us=r[5] / 1e3, min_us=r[6] / 1e3)
            for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--series', type=int, default=192)
    ap.add_argument('--n', type=int, default=1440000)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'oallan_timing.json'))
    ap.add_argument('--trace', default=None)
    ap.add_argument('--no-host', action='store_true', help='skip the NumPy leg (under a profiler)')
    a = ap.parse_args()
    if a.trace:
        with open(a.out) as f:
            res = json.load(f)
        res['kernel_trace'] = trace(a.trace)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res['kernel_trace']))
        return
    import ginsim
    S, n, fs = a.series, a.n, 400.0
    ctx = ginsim.Context(0)
    x = np.random.default_rng(0).normal(size=(S, n))
    buf = ctx.upload(x)
    os.environ.pop('GINSIM_OALLAN_TILE', None)
    factors, geo = ginsim.oallan_plan(buf, n, S, n, fs)

    def timed(fn):
        ctx.timer_begin()
        fn()
        return ctx.timer_end()

    o = lambda s=S: ginsim.oallan_var(ctx, buf, n, s, n, fs)        # noqa: E731
    al = lambda: ginsim.allan_var(ctx, buf, n, S, n, fs)            # noqa: E731
    for _ in range(a.warmup):
        o(), al()
    t_o, t_a = [], []
    for _ in range(a.launches):                                      # interleaved: both see the same clocks
        t_o.append(timed(o))
        t_a.append(timed(al))
    os.environ['GINSIM_OALLAN_TILE'] = '0'
    o()
    t_s = [timed(o) for _ in range(a.launches)]
    del os.environ['GINSIM_OALLAN_TILE']
    o(6)
    t_6 = [timed(lambda: o(6)) for _ in range(a.launches)]
    ov6, tau = o(6)
    mean = lambda v: sum(v) / len(v)                                 # noqa: E731
    C, H = geo['tile_payload'], geo['tile_halo']
    nt, ns = geo['tile_factors'], geo['stream_factors']
    # the model: the tile form reads x (C + H) / C times; the stream form reads x twice and writes theta for the scan, then three
    # 8-byte taps per shift and stream-form factor
    terms_stream = sum(f['terms'] for f in factors if f['form'] == 1)
    model = {'tile_read_bytes': 8.0 * S * n * (C + H) / C, 'scan_bytes': 24.0 * S * n, 'stream_tap_bytes': 24.0 * S * terms_stream,
             'lds_reads': 3.0 * S * sum(f['terms'] for f in factors if f['form'] == 0)}
    res = {'what': 'ginsim_oallan, HIP-event ms per call', 'series': S, 'n': n, 'ntau': int(tau.size), 'geometry': geo,
           'launches_per_leg': a.launches, 'oallan_ms': mean(t_o), 'oallan_ms_min': min(t_o), 'allan_ms_same_buffer': mean(t_a),
           'ratio_to_allan': mean(t_o) / mean(t_a), 'oallan_all_stream_ms': mean(t_s), 'oallan_6_series_ms': mean(t_6),
           'model': model, 'model_bytes_total': model['tile_read_bytes'] + model['scan_bytes'] + model['stream_tap_bytes'],
           'all_stream_tap_GBps': 24.0 * S * sum(f['terms'] for f in factors) / mean(t_s) / 1e6}
    if not a.no_host:
        t0 = time.perf_counter()
        host = ctx.download(buf, (6, n))
        mult = [f['m'] for f in factors]
        ref = np.array([restated(r, fs, mult) for r in host])
        dt = time.perf_counter() - t0
        res.update({'host_download_and_numpy_6_series_ms': dt * 1e3, 'ratio_host_to_device_6_series': dt * 1e3 / mean(t_6),
                    'worst_rel_difference_to_numpy': float(np.max(np.abs(ov6 / ref - 1.0)))})
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    buf.free()
    ctx.close()


if __name__ == '__main__':
    main()
