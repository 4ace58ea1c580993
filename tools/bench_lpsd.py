#!/usr/bin/env python3
"""Multi-resolution PSD benchmark on the buffer of tools/bench_psd.py (192 series x 1 440 000 samples @ 400 Hz).

    python tools/bench_lpsd.py [--launches 20] [--warmup 5] [--out profiles/lpsd_timing.json]

HIP-event times on one MI355X, `--launches` per leg after a warm-up, every launch interleaved with ginsim_psd_welch at the same
nperseg / step and with ginsim_allan on the SAME buffer.  Per case (nperseg, step; Hann, detrend, min_segments 1) three numbers:
  - the whole ginsim_lpsd call over the one-level ginsim_psd_welch call;
  - the level-0 ginsim_decimate2 launch alone, its 12 bytes per input sample over its time as a fraction of 8 TB/s (beside the
    fraction ginsim_allan reaches with its 8 bytes per sample in the same run);
  - the share of the call spent in decimation: the decimate2 launches of every level, timed one by one, over the call.
Beside them the ginsim_psd_welch call of every level past 0 on its own, timed the same way, and the workgroups it has: where the
call's time goes when it is more than twice the one-level call's.
Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, 'gnss-ins-sim_amd'), REPO]
import numpy as np      # noqa: E402

CASES = [(1024, 512), (8192, 4096)]                                 # (nperseg, step)
PEAK = 8e12                                                         # bytes per second of HBM3E on one MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--series', type=int, default=192)
    ap.add_argument('--n', type=int, default=1440000)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'lpsd_timing.json'))
    a = ap.parse_args()
    import ginsim
    S, n, fs = a.series, a.n, 400.0
    ctx = ginsim.Context(0)
    buf = ctx.upload(np.random.default_rng(0).normal(size=(S, n)))
    n1 = (n - 27) // 2 + 1
    n2 = (n1 - 27) // 2 + 1
    ping = [ctx.malloc(8 * S * n1), ctx.malloc(8 * S * max(n2, 1))]

    def timed(fn):
        ctx.timer_begin()
        fn()
        return ctx.timer_end()

    al = lambda: ginsim.allan_var(ctx, buf, n, S, n, fs)            # noqa: E731
    dec0 = lambda: ginsim.decimate2(ctx, buf, n, S, n, ping[0], n1)  # noqa: E731
    mean = lambda v: sum(v) / len(v)                                 # noqa: E731
    cases = []
    for L, D in CASES:
        plan = ginsim.lpsd_plan(n, S, n, fs, L, D)
        lengths = [lv['n'] for lv in plan['levels']]
        lp = lambda: ginsim.lpsd(ctx, buf, n, S, n, fs, L, D)        # noqa: E731
        ps = lambda: ginsim.welch_psd(ctx, buf, n, S, n, fs, L, D)   # noqa: E731

        def chain():
            """every level's decimate2 launch and its ginsim_psd_welch call, timed one by one: (level 0's decimation, all
            decimations, the Welch calls of the levels past 0)"""
            src, t, w = buf, [], []
            for j in range(len(lengths) - 1):
                dst = ping[j & 1]
                t.append(timed(lambda: ginsim.decimate2(ctx, src, lengths[j], S, lengths[j], dst, lengths[j + 1])))
                w.append(timed(lambda: ginsim.welch_psd(ctx, dst, lengths[j + 1], S, lengths[j + 1], fs / 2 ** (j + 1), L, D)))
                src = dst
            return (t[0] if t else 0.0), sum(t), w
        for _ in range(a.warmup):
            lp(), ps(), al(), dec0()
        t_l, t_p, t_a, t_d0, t_d, t_w = [], [], [], [], [], []
        for _ in range(a.launches):                                  # interleaved: all see the same clocks
            t_l.append(timed(lp))
            t_p.append(timed(ps))
            t_a.append(timed(al))
            d0, d, w = chain()
            t_d0.append(d0)
            t_d.append(d)
            t_w.append(w)
        spec, freq, lev = ginsim.lpsd(ctx, buf, n, 6, n, fs, L, D)
        white = [float(np.mean(spec[:, (lev == j) & (np.arange(freq.size) >= 2)])) / (2.0 / fs) for j in range(len(lengths))]
        cases.append({'nperseg': L, 'step': D, 'plan': plan,
                      'lpsd_ms': mean(t_l), 'lpsd_ms_min': min(t_l), 'lpsd_ms_max': max(t_l), 'psd_ms': mean(t_p), 'psd_ms_min': min(t_p),
                      'lpsd_over_psd': mean(t_l) / mean(t_p),
                      'samples_read_over_level_0': sum(lengths) / float(n),
                      'decimate2_level0_ms': mean(t_d0), 'decimate2_level0_ms_min': min(t_d0),
                      'decimate2_level0_fraction_of_8TBps': 12.0 * n * S / (mean(t_d0) * 1e-3) / PEAK,
                      'allan_ms_same_buffer': mean(t_a), 'allan_fraction_of_8TBps': 8.0 * n * S / (mean(t_a) * 1e-3) / PEAK,
                      'decimate2_all_levels_ms': mean(t_d), 'decimation_share_of_lpsd': mean(t_d) / mean(t_l),
                      'psd_ms_of_levels_past_0': [mean([w[j] for w in t_w]) for j in range(len(lengths) - 1)],
                      'workgroups_per_level': [S * lv['nparts'] for lv in plan['levels']],
                      'white_level_per_level_over_2_by_fs': white})
    res = {'what': 'ginsim_lpsd (Hann, detrend, min_segments 1), HIP-event ms per call, interleaved with ginsim_psd_welch and ginsim_allan',
           'series': S, 'n': n, 'fs': fs, 'launches_per_leg': a.launches, 'cases': cases}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    for b in ping:
        b.free()
    buf.free()
    ctx.close()


if __name__ == '__main__':
    main()
