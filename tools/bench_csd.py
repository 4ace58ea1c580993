#!/usr/bin/env python3
"""Welch cross-spectral-density benchmark on tools/bench_psd.py's buffer (192 series x 1 440 000 samples @ 400 Hz).

    python tools/bench_csd.py [--launches 20] [--warmup 5] [--out profiles/csd_timing.json]

HIP-event time of ginsim_csd_welch on one MI355X for the 96 pairs (2i, 2i + 1), `--launches` per case after a warm-up, every
launch interleaved with ginsim_psd_welch of the SAME 192 series: the cases of tools/bench_psd.py that the kernel takes, nperseg 256
and 1024 at half overlap and 1024 without overlap (Hann, detrend).  By transform count the two calls are equal -- a pair costs K
complex transforms, the PSD of its two series 2 (K / 2) -- so the ratio shows what the separation, the write-back of half the last
stage and four accumulators instead of one cost.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, 'gnss-ins-sim_amd'), REPO]
import numpy as np      # noqa: E402

CASES = [(256, 128), (1024, 512), (1024, 1024)]                     # (nperseg, step): bench_psd's, up to 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--series', type=int, default=192)
    ap.add_argument('--n', type=int, default=1440000)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'csd_timing.json'))
    a = ap.parse_args()
    import ginsim
    S, n, fs = a.series, a.n, 400.0
    ctx = ginsim.Context(0)
    buf = ctx.upload(np.random.default_rng(0).normal(size=(S, n)))
    pairs = [(2 * i, 2 * i + 1) for i in range(S // 2)]

    def timed(fn):
        ctx.timer_begin()
        fn()
        return ctx.timer_end()

    mean = lambda v: sum(v) / len(v)                                 # noqa: E731
    cases = []
    for L, D in CASES:
        c = lambda: ginsim.welch_csd(ctx, buf, n, S, n, fs, pairs, L, D)         # noqa: E731
        p = lambda: ginsim.welch_psd(ctx, buf, n, S, n, fs, L, D)                # noqa: E731
        for _ in range(a.warmup):
            c(), p()
        t_c, t_p = [], []
        for _ in range(a.launches):                                  # interleaved: both see the same clocks
            t_c.append(timed(c))
            t_p.append(timed(p))
        r, (spec, _) = c(), p()
        nb = r.pxx.shape[1]
        cases.append({'nperseg': L, 'step': D, 'geometry': ginsim.csd_plan(n, S, n, fs, len(pairs), L, D),
                      'csd_ms': mean(t_c), 'csd_ms_min': min(t_c), 'csd_ms_max': max(t_c), 'psd_ms_same_series': mean(t_p), 'psd_ms_min': min(t_p),
                      'ratio_to_psd': mean(t_c) / mean(t_p),
                      'pxx_against_psd_largest_relative_difference': float(np.max(np.abs(r.pxx / spec[0::2] - 1.0))),
                      'mean_coherence_of_independent_series': float(np.mean(r.coherence[:, 2:nb - 2])),
                      'one_over_segments': 1.0 / ginsim.csd_plan(n, S, n, fs, len(pairs), L, D)['segments']})
    res = {'what': 'ginsim_csd_welch of 96 pairs (Hann, detrend), HIP-event ms per call, interleaved with ginsim_psd_welch of the '
                   'same 192 series', 'series': S, 'pairs': len(pairs), 'n': n, 'fs': fs, 'launches_per_case': a.launches, 'cases': cases}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    buf.free()
    ctx.close()


if __name__ == '__main__':
    main()
