#!/usr/bin/env python3
"""Welch power-spectral-density benchmark (BASELINE config 5's size: 192 series x 1 440 000 samples @ 400 Hz).

    python tools/bench_psd.py [--launches 20] [--warmup 5] [--out profiles/psd_timing.json]

HIP-event time of ginsim_psd_welch on one MI355X, `--launches` per case after a warm-up, every launch interleaved with ginsim_allan
on the SAME buffer: nperseg 256, 1024 and 8192 at half overlap and 1024 without overlap (Hann, detrend), each on the 192 series and
on 6 of them (the plugin's size).  Per case: milliseconds, the algorithmic bytes 8 n S over that time as a fraction of 8 TB/s, and
the ratio to ginsim_allan.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, 'gnss-ins-sim_amd'), REPO]
import numpy as np      # noqa: E402

CASES = [(256, 128), (1024, 512), (8192, 4096), (1024, 1024)]       # (nperseg, step)
PEAK = 8e12                                                         # bytes per second of HBM3E on one MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--series', type=int, default=192)
    ap.add_argument('--n', type=int, default=1440000)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'psd_timing.json'))
    a = ap.parse_args()
    import ginsim
    S, n, fs = a.series, a.n, 400.0
    ctx = ginsim.Context(0)
    buf = ctx.upload(np.random.default_rng(0).normal(size=(S, n)))

    def timed(fn):
        ctx.timer_begin()
        fn()
        return ctx.timer_end()

    al = lambda: ginsim.allan_var(ctx, buf, n, S, n, fs)            # noqa: E731
    mean = lambda v: sum(v) / len(v)                                 # noqa: E731
    cases = []
    for L, D in CASES:
        p = lambda s=S: ginsim.welch_psd(ctx, buf, n, s, n, fs, L, D)        # noqa: E731
        for _ in range(a.warmup):
            p(), al(), p(6)
        t_p, t_a, t_6 = [], [], []
        for _ in range(a.launches):                                  # interleaved: all see the same clocks
            t_p.append(timed(p))
            t_a.append(timed(al))
            t_6.append(timed(lambda: p(6)))
        spec, freq = p(6)
        white = float(np.mean(spec[:, 2:-2]))                        # unit variance at fs: 2 / fs
        cases.append({'nperseg': L, 'step': D, 'geometry': ginsim.welch_plan(n, S, n, fs, L, D),
                      'psd_ms': mean(t_p), 'psd_ms_min': min(t_p), 'psd_ms_max': max(t_p), 'allan_ms_same_buffer': mean(t_a),
                      'ratio_to_allan': mean(t_p) / mean(t_a), 'fraction_of_8TBps': 8.0 * n * S / (mean(t_p) * 1e-3) / PEAK,
                      'psd_6_series_ms': mean(t_6), 'psd_6_series_ms_min': min(t_6), 'psd_6_series_ms_max': max(t_6),
                      'fraction_of_8TBps_6_series': 8.0 * n * 6 / (mean(t_6) * 1e-3) / PEAK,
                      'white_level_over_2_by_fs': white / (2.0 / fs)})
    res = {'what': 'ginsim_psd_welch (Hann, detrend), HIP-event ms per call, interleaved with ginsim_allan', 'series': S, 'n': n,
           'fs': fs, 'launches_per_case': a.launches, 'cases': cases}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    buf.free()
    ctx.close()


if __name__ == '__main__':
    main()
