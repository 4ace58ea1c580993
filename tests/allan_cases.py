"""The inputs and the expected level plans of the Allan edge tests, shared by test_allan_plan.py, test_allan_exact_oracle.py
(both without a device), test_gpu_allan_edges.py and the child process it starts (allan_forced_child.py).

A plan is one tuple of modes per decade level, in the numbering of ginsim_allan_level.mode: L register-staged
allan_level_kernel, P wave-pair LDS-DMA allan_pair_kernel, F0 / F1 allan_fused_kernel's two levels, T allan_tail_kernel.  The
expected plans are written out, not computed: the constants they follow from (csrc/allan.hip: kChunk 2520, kDmaStage 2560,
kFuseChunks 10; csrc/api_series.hip: 1024 workgroups in one round, at most 16 chunks each, else total / 4096 capped at 8) are
what the table pins."""
import numpy as np

L, P, F0, F1, T = 0, 1, 2, 3, 4

ALIGNED, ODD, OFF8 = 'aligned', 'odd', 'off8'


def fs_of(n):
    return 10.0 if n < 9000 else 100.0


def even_stride(n):
    return (n + 13) // 2 * 2


def placement(n, where):
    """(series stride, byte offset of the first series in the buffer) of a placement."""
    return {ALIGNED: (even_stride(n), 0), ODD: (even_stride(n) + 1, 0), OFF8: (even_stride(n), 8)}[where]


def series(seed, n):
    """White noise 0.3 plus a 1e-3 random walk (test_gpu_allan.py's _series)."""
    from oracle import philox
    j = np.arange(n, dtype=np.uint64)
    return 0.3 * philox.normal_pair(seed, 7, 5, j)[0] + 1e-3 * np.cumsum(philox.normal_pair(seed, 7, 4, j)[1])


def rows(seed, n, fs, count=4):
    """Row r is series(seed + r) as: r % 4 == 0 plain, 1 plus 1e6, 2 plus 1e6 and a ramp of 3e3 per second, 3 scaled by 1e-9."""
    t = np.arange(n) / fs
    out = []
    for r in range(count):
        x = series(seed + r, n)
        out.append((x, x + 1.0e6, x + 1.0e6 + 3.0e3 * t, x * 1.0e-9)[r % 4])
    return out


def pack(rws, stride, offset=0, repeat=1):
    """The rows (tiled `repeat` times) in one NaN-filled float64 buffer, series s at entry offset / 8 + s * stride."""
    S = len(rws) * repeat
    flat = np.full(offset // 8 + S * stride, np.nan)
    body = flat[offset // 8:].reshape(S, stride)
    for s in range(S):
        body[s, :rws[s % len(rws)].size] = rws[s % len(rws)]
    return flat


# ---- section a: the forms of level 0.  n -> plan on an aligned even-stride buffer; ODD and OFF8 put L at every chunked level 0
LEVEL0 = {2520: (T, T, T), 2521: (L, T, T), 2559: (L, T, T), 2560: (P, T, T), 2561: (P, T, T), 5039: (P, T, T), 5040: (P, T, T),
          5041: (P, T, T), 5079: (P, T, T), 5080: (P, T, T)}
LEVEL0_NTAU = {2520: 20, 2521: 20, 2559: 20, 2560: 20, 2561: 20, 5039: 23, 5040: 23, 5041: 23, 5079: 23, 5080: 23}


def level0_plan(n, where):
    p = LEVEL0[n]
    return p if where == ALIGNED or p[0] == T else (L,) + p[1:]


# ---- section b: the fuse boundary.  n -> (plan, plan with GINSIM_ALLAN_FUSE=0), aligned
FUSE = {25209: ((P, T, T, T), (P, T, T, T)), 25210: ((F0, F1, T, T), (P, L, T, T)), 25219: ((F0, F1, T, T), (P, L, T, T)),
        27720: ((F0, F1, T, T), (P, P, T, T)), 27760: ((F0, F1, T, T), (P, P, T, T)), 50400: ((F0, F1, T, T), (P, P, T, T)),
        50410: ((F0, F1, T, T), (P, L, T, T))}
FUSE_PARTS = {25209: 11, 25210: 2, 25219: 2, 27720: 2, 27760: 2, 50400: 2, 50410: 3}      # records per series of level 0

# ---- section c: deeper levels.  (n, S, placement) -> plan
DEEP = {(252090, 4, ALIGNED): (F0, F1, T, T, T), (252100, 4, ALIGNED): (F0, F1, L, T, T), (255900, 4, ALIGNED): (F0, F1, L, T, T),
        (256000, 4, ALIGNED): (F0, F1, P, T, T), (256100, 4, ALIGNED): (F0, F1, L, T, T),
        (360000, 4, ODD): (L, P, P, T, T), (360010, 4, ODD): (L, L, P, T, T),
        (2521000, 1, ALIGNED): (F0, F1, P, L, T, T), (2560000, 1, ALIGNED): (F0, F1, P, P, T, T)}

# ---- section d: powers of ten of floor(n / 9).  (n, fs) -> (ntau, plan), aligned
POWERS = {(90, 1.0): (9, (T,)), (98, 1.0): (9, (T,)), (99, 1.0): (10, (T, T)), (9000, 1.0): (27, (P, T, T)), (9008, 1.0): (27, (P, T, T)),
          (9009, 1.0): (28, (P, T, T, T)), (90000, 1.0): (36, (F0, F1, T, T)), (90009, 1.0): (37, (F0, F1, T, T, T)),
          (900, 100.0): (18, (T, T)), (899, 100.0): (0, ())}
# ntau alone (test_allan_plan.py): 89 and 90 seconds of samples, and the decades of floor(n / 9) up to 10^5
NTAU = {(89, 1.0): 9, (90, 1.0): 9, (8900, 100.0): 27, (9000, 100.0): 27, (9000, 1.0): 27, (9008, 1.0): 27, (9009, 1.0): 28,
        (90000, 1.0): 36, (90009, 1.0): 37, (900009, 1.0): 46}

# ---- section e: chunks per workgroup of the pair kernel.  (S, n) -> (plan with GINSIM_ALLAN_FUSE=0, chunks per workgroup and
# records per series of level 0); stride n, aligned
BATCH = {(512, 12650): ((P, T, T, T), 3, 2), (1024, 7570): ((P, T, T), 4, 1), (1025, 7570): ((P, T, T), 4, 1),
         (1024, 42890): ((P, L, T, T), 4, 5)}

# ---- section f: the register-staged form forced (GINSIM_ALLAN_DMA=0), S = 3.  n -> (plan, records per series of every chunked
# level with GINSIM_ALLAN_CPW=3, the same without)
FORCED_S = 3
FORCED = {2521: ((L, T, T), (2,), (2,)), 7561: ((L, T, T), (2,), (4,)), 15133: ((L, T, T, T), (4,), (8,)),
          100799: ((L, L, T, T, T), (14, 2), (40, 4)), 252110: ((L, L, L, T, T), (34, 4, 2), (102, 12, 2))}
FORCED_ENV = {'cpw3': {'GINSIM_ALLAN_DMA': '0', 'GINSIM_ALLAN_CPW': '3'}, 'cpw0': {'GINSIM_ALLAN_DMA': '0'}}

# ---- section g: non-finite samples, S = 7, aligned.  n -> plan
NONFINITE = {2000: (T, T, T), 10089: (P, T, T, T), 100799: (F0, F1, T, T, T), 256123: (F0, F1, L, T, T)}


def nonfinite_rows(n, fs):
    """Seven rows from one clean series: clean, NaN at n-1, NaN at n-7, NaN at 0, NaN at the first entry of the last chunk, +inf at
    n // 2, clean."""
    x = rows(70, n, fs, 1)[0]
    out = [x.copy() for _ in range(7)]
    out[1][n - 1] = np.nan
    out[2][n - 7] = np.nan
    out[3][0] = np.nan
    out[4][(n // 2520) * 2520] = np.nan
    out[5][n // 2] = np.inf
    return out
