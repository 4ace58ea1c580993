"""The PSD vibration series (ginsim_vib_psd_series, csrc/vib_psd.hip) stated exactly, and the shapes its tests run: shared by
test_vib_psd_oracle.py (this reference against itself and against oracle.ins_np.psd_series, without a device) and
test_gpu_vib_psd_edges.py (the device against it).

The operation.  For a period N, L = N/2 + 1 bins, amplitudes a[k] >= 0 and normals z[k] of one run and axis, the series is
real(ifft) of the Hermitian extension of a[k] exp(i pi z[k]) (time_series_from_psd.py:51-57).  Written out, the imaginary parts
of bins 0 and N/2 cancel and

    x[j] = ( a[0] cos(pi z[0]) + (-1)^j a[L-1] cos(pi z[L-1]) + 2 sum_{k=1..L-2} a[k] cos(2 pi ((j k) mod N) / N + pi z[k]) ) / N

``exact`` evaluates this sum in np.longdouble: the angle 2 pi m / N from the INTEGER m = (j k) mod N, pi a long-double constant,
z the exact floats of oracle.philox.vib_normals widened.  cos(2 pi m / N + pi z) is expanded into the long-double cosines and sines
of its two parts, so the sum over k is one long-double matrix product with a table of N angles; the two extra roundings per term
are 2^-64 relative, a two-thousandth of the unit below.  With `halve` the interior amplitudes a[1..L-2] of global run g are
multiplied by sqrt(0.5^(g + 1)), 0.5^(g + 1) formed first as the reference does (it halves its array once per call,
time_series_from_psd.py:49); bins 0 and L-1 are never scaled.

``restated`` is the plainest float64 implementation: np.fft.irfft of a exp(i pi z), what oracle.ins_np.psd_series does per axis
after its amplitude step (test_vib_psd_oracle.py holds the two together).

The unit.  A = (a[0] + a[L-1] + 2 sum interior a[k]) / N is the largest value any sample of the series can take (the amplitudes
as the run sees them: halved where the case halves).  Every error is stated in units of A 2^-53, per axis and run.

DEV[id]: the float64 restatement's largest deviation from the long-double sum over the positions the case is checked at
(``positions``, ``ref_runs``), in that unit, measured on the CPU (long double of 64 mantissa bits) and rounded up to two digits;
test_vib_psd_oracle.py::test_recorded_deviation_of_the_float64_restatement recomputes every figure and holds it under its record.
The device is allowed A 2^-53 (1 + MARGIN DEV[id]) per sample: the 1 is the result's own rounding, MARGIN = 16 times what
pocketfft and NumPy's sine and cosine are off by stands for an FFT and a sincos whose arithmetic differs from theirs.  In any event
the device stays under CEILING * A = 1e-12 A, the accelerometer tolerance of tests/test_gpu_edge_cases.py for a term of this size.

``exact`` takes a `fault`: one deliberate error of the kind a kernel could make.  The GPU tests assert, on the reference alone
and before the device is asked, that each fault moves a sample of the case by more than 1e3 bounds -- so a case that could not see
its fault, or a reference that had the fault built in, fails there."""
import collections
import zlib

import numpy as np

from oracle import philox

LD = np.longdouble
PI = 4 * np.arctan(LD(1))
UNIT = 2.0 ** -53
MARGIN = 16.0
CEILING = 1e-12
FS = 128.0                              # of the vib_def a case is restated as (a power of two: sxx * N * fs rounds twice, not thrice)

RUNS = (1, 63, 64, 65, 129)
CLASSES = {
    'tiny': (2, 4, 6),                                      # L = 2, 3, 4: no interior bin, one, two
    'tile': (62, 64, 66, 126, 128, 130),                    # a 64-sample transposition tile short by two, full, over by two; twice
    'block': (510, 512, 514),                               # L = 256, 257, 258 around the spectrum kernel's 256-lane block
    'composite': (1000, 4098, 16382),                       # the Sim tests' period; 2 3 683; 2 8191
    'capped': (16384,),                                     # time_series_from_psd.py:41-43
}
PERIODS = tuple(n for c in CLASSES.values() for n in c)
OFFSETS = (0, 37, 2 ** 32 + 5)
TABLES = ('rand', 'decades12', 'zero', 'edges')
FAULTS = ('swap_axes', 'no_alternation', 'local_run', 'block_local_run', 'halve_bin0', 'halve_last', 'skip_bin1', 'skip_last_interior')

Case = collections.namedtuple('Case', 'id N runs sensor off seed table halve rr base perm', defaults=(None, None, None))
S1, S2, S3 = 2 ** 33 + 7, 2 ** 63 + 9, 2 ** 40 + 12345         # seeds above 32 bits


def _c(N, runs, sensor, off, seed, table='rand', halve=0):
    name = 'N%d_R%d_%s_off%s_%s%s' % (N, runs, sensor, {0: '0', 37: '37'}.get(off, '2p32'), table, '_halved' if halve else '')
    return Case(name, N, runs, sensor, off, seed, table, halve)


# The square {run counts} x {period classes} with as few cases as it takes: five per class, six where the class has six
# periods.  The sensors, the offsets, the seeds and the tables are dealt over them; test_vib_psd_oracle.py asserts the pairs.
CASES = [
    _c(2, 1, 'gyr', 37, S1),
    _c(4, 63, 'acc', 0, S2, halve=1),
    _c(6, 64, 'gyr', 2 ** 32 + 5, S3),
    _c(4, 65, 'gyr', 37, S1, 'edges'),
    _c(6, 129, 'acc', 0, S2, halve=1),
    _c(62, 65, 'acc', 2 ** 32 + 5, S3),
    _c(64, 63, 'gyr', 0, S1),
    _c(66, 129, 'acc', 37, S2, halve=1),
    _c(126, 64, 'gyr', 0, S3, 'zero'),
    _c(128, 1, 'acc', 2 ** 32 + 5, S1),
    _c(130, 65, 'gyr', 37, S2, 'edges'),
    _c(510, 129, 'gyr', 0, S3),
    _c(512, 65, 'acc', 37, S1, 'decades12'),
    _c(514, 63, 'gyr', 2 ** 32 + 5, S2),
    _c(512, 1, 'gyr', 0, S3, halve=1),
    _c(510, 64, 'acc', 37, S1),
    _c(1000, 129, 'acc', 2 ** 32 + 5, S2),
    _c(4098, 65, 'gyr', 0, S3),
    _c(16382, 64, 'acc', 37, S1),
    _c(1000, 1, 'gyr', 37, S2, halve=1),
    _c(4098, 63, 'acc', 2 ** 32 + 5, S3),
    _c(16384, 1, 'acc', 0, S1),
    _c(16384, 63, 'gyr', 37, S2),
    _c(16384, 64, 'acc', 2 ** 32 + 5, S3),
    _c(16384, 65, 'gyr', 0, S1),
    _c(16384, 129, 'acc', 37, S2),
]
IDS = [c.id for c in CASES]

# halve_per_run at the global run ids 0, 1, 2 (one call), 9, 1000 and 2300 (0.5^2301 has underflowed: no interior bin is left),
# each reached through run_offset with three runs around it
HALVE_IDS = {0: (0, 1, 2), 8: (9,), 999: (1000,), 2299: (2300,)}
HALVING = [Case('halve_N%d_from%d' % (N, off), N, 3, ('acc', 'gyr')[i % 2], off, S1 + i, 'rand', 1)
           for i, (N, off) in enumerate((N, off) for N in (4, 6, 66, 512) for off in HALVE_IDS)]
# the 32768-run cap of a block of runs (the spectrum kernel's grid.y): two blocks, the second of 65 runs; three, the last of one
BLOCKS = [Case('blocks_N8_R32833', 8, 32768 + 65, 'acc', 37, S3, 'rand', 0, (0, 32767, 32768, 32832)),
          Case('blocks_N2_R65537', 2, 2 * 32768 + 1, 'gyr', 0, S2, 'rand', 0, (0, 32767, 32768, 65535, 65536))]


def derived(base, tag, **kw):
    """A case with the table of another and something else changed."""
    return BY_ID[base]._replace(id='%s_%s' % (base, tag), base=base, **kw)


BY_ID = {c.id: c for c in CASES + HALVING + BLOCKS}
# the same calls with another seed (other z[0] and z[L-1]: the imaginary parts of bins 0 and N/2), as the other sensor, and with two
# rows of the table swapped
RESEEDED = [derived('N64_R63_gyr_off0_rand', 'reseeded', seed=S2 + 1), derived('N4098_R65_gyr_off0_rand', 'reseeded', seed=S1 + 1)]
OTHER_SENSOR = [derived('N66_R129_acc_off37_rand_halved', 'as_gyr', sensor='gyr'), derived('N130_R65_gyr_off37_edges', 'as_acc', sensor='acc'),
                derived('N514_R63_gyr_off2p32_rand', 'as_acc', sensor='acc')]
SWAPPED = [derived('N62_R65_acc_off2p32_rand', 'rows%d%d%d' % p, perm=p) for p in ((1, 0, 2), (2, 1, 0), (0, 2, 1))]
EXTRA = HALVING + BLOCKS + RESEEDED + OTHER_SENSOR + SWAPPED
BY_ID.update({c.id: c for c in EXTRA})

DEV = {
    'N2_R1_gyr_off37_rand':             4.1,        # pi z rounds before the cosine: |pi z| 2^-53 |sin| per edge bin, |z| up to 4
    'N4_R63_acc_off0_rand_halved':      2.1,
    'N6_R64_gyr_off2p32_rand':          4.2,
    'N4_R65_gyr_off37_edges':           3.9,
    'N6_R129_acc_off0_rand_halved':     2.1,
    'N62_R65_acc_off2p32_rand':         2.1,
    'N64_R63_gyr_off0_rand':            2.4,
    'N66_R129_acc_off37_rand_halved':   4.1,
    'N126_R64_gyr_off0_zero':           0.0,
    'N128_R1_acc_off2p32_rand':         1.6,
    'N130_R65_gyr_off37_edges':         2.3,
    'N510_R129_gyr_off0_rand':          1.3,
    'N512_R65_acc_off37_decades12':     2.3,
    'N514_R63_gyr_off2p32_rand':        1.8,
    'N512_R1_gyr_off0_rand_halved':     0.9,
    'N510_R64_acc_off37_rand':          1.3,
    'N1000_R129_acc_off2p32_rand':      1.1,
    'N4098_R65_gyr_off0_rand':          0.53,
    'N16382_R64_acc_off37_rand':        0.33,
    'N1000_R1_gyr_off37_rand_halved':   6.4,        # run 37: the interior is 2^-19 of itself, bins 0 and N/2 carry the series
    'N4098_R63_acc_off2p32_rand':       0.57,
    'N16384_R1_acc_off0_rand':          0.18,
    'N16384_R63_gyr_off37_rand':        0.23,
    'N16384_R64_acc_off2p32_rand':      0.18,
    'N16384_R65_gyr_off0_rand':         0.21,
    'N16384_R129_acc_off37_rand':       0.25,
    # EXTRA
    'halve_N4_from0':                   2.1,
    'halve_N4_from8':                   3.9,
    'halve_N4_from999':                 1.8,
    'halve_N4_from2299':                1.2,
    'halve_N6_from0':                   2.0,
    'halve_N6_from8':                   2.5,
    'halve_N6_from999':                 3.4,
    'halve_N6_from2299':                2.5,
    'halve_N66_from0':                  3.5,
    'halve_N66_from8':                  3.2,
    'halve_N66_from999':                1.3,
    'halve_N66_from2299':               1.8,
    'halve_N512_from0':                 1.1,
    'halve_N512_from8':                 1.1,
    'halve_N512_from999':               4.4,
    'halve_N512_from2299':              2.0,
    'blocks_N8_R32833':                 2.6,
    'blocks_N2_R65537':                 3.0,
    'N64_R63_gyr_off0_rand_reseeded':   2.3,
    'N4098_R65_gyr_off0_rand_reseeded': 0.62,
    'N66_R129_acc_off37_rand_halved_as_gyr': 5.0,
    'N130_R65_gyr_off37_edges_as_acc':  4.6,
    'N514_R63_gyr_off2p32_rand_as_acc': 1.6,
    'N62_R65_acc_off2p32_rand_rows102': 2.5,
    'N62_R65_acc_off2p32_rand_rows210': 2.1,
    'N62_R65_acc_off2p32_rand_rows021': 2.5,
}


def period_class(N):
    return [k for k, v in CLASSES.items() if N in v][0]


def amplitudes(N, table='rand', key=0):
    """(3, L) float64: |normal| 10^uniform(-3, 0) per bin and axis ('rand'; 'decades12': twelve decades), all zero, or bins 0 and
    L-1 alone ('edges').  The three axes differ."""
    L = N // 2 + 1
    rng = np.random.default_rng([N, key, TABLES.index(table)])
    a = np.abs(rng.standard_normal((3, L))) * 10.0 ** rng.uniform(-12.0 if table == 'decades12' else -3.0, 0.0, (3, L))
    if table == 'zero':
        a[:] = 0.0
    elif table == 'edges':
        a[:, 1:L - 1] = 0.0
    return a


def case_amplitudes(case):
    """The table of a case: made from its id (or from the id of the case it is derived from), its rows permuted by `perm`."""
    a = amplitudes(case.N, case.table, zlib.crc32((case.base or case.id).encode()))
    return a[list(case.perm)] if case.perm else a


def normals(case, r):
    """(L, 3): the normals of run r of the case (global id off + r)."""
    return philox.vib_normals(case.seed, case.off + r, case.N // 2 + 1, case.sensor)


def halving(g, dtype=LD):
    """sqrt(0.5^(g + 1)) of global run g, 0.5^(g + 1) first: zero once that has underflowed."""
    with np.errstate(under='ignore'):
        return np.sqrt(dtype(0.5) ** dtype(g + 1))


def run_amplitudes(a, g, halve, dtype=LD, fault=None):
    """The amplitudes run g sees: the interior bins halved g + 1 times under `halve`."""
    a = np.array(a, dtype=dtype)
    if halve:
        L = a.shape[1]
        k = np.arange(L)
        scaled = (k >= 1) & (k <= L - 2)
        for name, bin_, to in (('halve_bin0', 0, True), ('halve_last', L - 1, True), ('skip_bin1', 1, False), ('skip_last_interior', L - 2, False)):
            if fault == name:
                scaled[bin_] = to
        a[:, scaled] *= halving(g, dtype)
    return a


def unit(a):
    """A (3,) of amplitudes (3, L): the largest value a sample can take."""
    a = np.asarray(a, dtype=np.float64)
    L = a.shape[1]
    return (a[:, 0] + a[:, L - 1] + 2.0 * a[:, 1:L - 1].sum(axis=1)) / (2 * (L - 1))


def positions(N):
    """The samples a case is checked at against the long-double sum: all of them up to N = 2048; above, the first, the last, the
    middle, a tile edge and a fixed random 246 more."""
    if N <= 2048:
        return np.arange(N)
    named = [0, 1, 63, 64, 65, N // 2 - 1, N // 2, N // 2 + 1, N - 2, N - 1]
    rest = np.setdiff1d(np.arange(N), named)
    more = np.random.default_rng(N).choice(rest, 246, replace=False)
    return np.sort(np.concatenate([named, more]))


def ref_runs(runs):
    """The runs a case is checked at against the long-double sum: the first two, the last, and both sides of every 64-run edge."""
    return np.array(sorted({r for r in (0, 1, 62, 63, 64, 65, 127, 128, runs - 1) if 0 <= r < runs}))


_tables = {}


def _angle_tables(N, js):
    """(cos, sin)(2 pi ((j k) mod N) / N) as (len(js), L) long-double arrays; the last one made is kept."""
    key = (N, np.asarray(js, dtype=np.int64).tobytes())
    if _tables.get('key') != key:
        L = N // 2 + 1
        m = (np.asarray(js, dtype=np.int64)[:, None] * np.arange(L, dtype=np.int64)[None, :]) % N
        t = 2 * PI * np.arange(N, dtype=LD) / LD(N)
        _tables.update(key=key, cos=np.cos(t)[m], sin=np.sin(t)[m])
    return _tables['cos'], _tables['sin']


def exact_sum(a, z, N, js, fault=None):
    """The direct sum in long double.  a (3, L) amplitudes as the run sees them, z (L, 3) normals -> (3, len(js)) long double."""
    L = N // 2 + 1
    a = np.asarray(a, dtype=LD)
    z = np.asarray(z, dtype=LD)
    if fault == 'swap_axes':
        z = z[:, [0, 2, 1]]
    assert a.shape == (3, L) and z.shape == (L, 3) and N % 2 == 0
    js = np.asarray(js, dtype=np.int64)
    c, s = a.T * np.cos(PI * z), a.T * np.sin(PI * z)                       # (L, 3)
    sign = np.ones(js.size, dtype=LD) if fault == 'no_alternation' else np.where(js % 2 == 0, LD(1), LD(-1))
    x = c[0][None, :] + sign[:, None] * c[L - 1][None, :]
    if L > 2:
        ct, st = _angle_tables(N, js)
        x = x + 2 * (ct[:, 1:L - 1] @ c[1:L - 1] - st[:, 1:L - 1] @ s[1:L - 1])
    return (x / LD(N)).T


def exact(case, rr, js, fault=None):
    """(3, len(js), len(rr)) long double: runs rr of the case at samples js.  fault: one of FAULTS, or None."""
    assert fault is None or fault in FAULTS
    a = case_amplitudes(case)
    out = np.empty((3, len(js), len(rr)), dtype=LD)
    for i, r in enumerate(rr):
        local = {'local_run': int(r), 'block_local_run': case.off + int(r) % 32768}.get(fault)
        g = case.off + int(r) if local is None else local
        z = philox.vib_normals(case.seed, g, case.N // 2 + 1, case.sensor)
        out[:, :, i] = exact_sum(run_amplitudes(a, g, case.halve, LD, fault), z, case.N, js, fault)
    return out


def restated_sum(a, z, N):
    """np.fft.irfft of a exp(i pi z) in float64: (3, N)."""
    return np.fft.irfft(np.asarray(a, dtype=np.float64) * np.exp(1j * (np.pi * np.asarray(z).T)), n=N, axis=1)


def restated(case, rr=None):
    """(3, N, len(rr)) float64, all the runs of the case by default."""
    a = case_amplitudes(case)
    rr = np.arange(case.runs) if rr is None else rr
    out = np.empty((3, case.N, len(rr)))
    for i, r in enumerate(rr):
        out[:, :, i] = restated_sum(run_amplitudes(a, case.off + int(r), case.halve, np.float64), normals(case, int(r)), case.N)
    return out


def units(case, rr=None):
    """A (3, len(rr)) of the runs of a case."""
    a = case_amplitudes(case)
    rr = np.arange(case.runs) if rr is None else rr
    return np.stack([unit(run_amplitudes(a, case.off + int(r), case.halve, np.float64)) for r in rr], axis=1)


def as_vib_def(case):
    """The case as the vib_def of oracle.ins_np.psd_series, at FS: a halved case GIVEN on the period's own grid (psd_series then takes
    calls_before = the global run id), every other one on the grid plus one frequency more, so that it is interpolated -- np.interp
    returns the value of a knot exactly at that knot."""
    a = case_amplitudes(case)
    N, L = case.N, case.N // 2 + 1
    f = np.linspace(0, FS / 2.0, L)
    sxx = a * a / N / FS
    if case.halve:
        return {'type': 'psd', 'freq': f, 'x': sxx[0], 'y': sxx[1], 'z': sxx[2]}
    sxx[:, 1:L - 1] *= 2.0
    f1 = np.insert(f, 1, 0.5 * (f[0] + f[1]))
    return dict({'type': 'psd', 'freq': f1}, **{k: np.insert(sxx[c], 1, 0.5 * (sxx[c, 0] + sxx[c, 1])) for c, k in enumerate('xyz')})


_reference = {}


def reference(case):
    """dict of a case, computed once per process and shared; callers leave it unchanged:
      a (3, L); js, rr: the samples and runs of the long-double sum, exact (3, len(js), len(rr)) long double;
      runs: the runs of the float64 restatement (all of them up to 1000 runs, rr above), f64 (3, N, len(runs)), A (3, len(runs));
      at: where rr lies in runs."""
    if case.id not in _reference:
        js = positions(case.N)
        rr = ref_runs(case.runs) if case.rr is None else np.array(case.rr)
        runs = np.arange(case.runs) if case.runs <= 1000 else rr
        _reference[case.id] = dict(a=case_amplitudes(case), js=js, rr=rr, exact=exact(case, rr, js), runs=runs, f64=restated(case, runs),
                                   A=units(case, runs), at=np.searchsorted(runs, rr))
    return _reference[case.id]


def _ratio(d, A):
    A = np.broadcast_to(A, d.shape)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(A > 0, d / (A * UNIT), np.where(d == 0, 0.0, np.inf))
    return float(np.max(np.where(np.isnan(r), np.inf, r)))


def deviation(got, ref):
    """Largest |got - exact| / (A 2^-53) of a (3, N, len(ref['runs'])) array at the positions of the long-double sum; where A is 0,
    0 if the two are equal and infinite if not."""
    d = np.abs(got[:, ref['js']][:, :, ref['at']].astype(LD) - ref['exact']).astype(np.float64)
    return _ratio(d, ref['A'][:, None, ref['at']])


def deviation_f64(got, ref):
    """Largest |got - restated| / (A 2^-53) of a (3, N, len(ref['runs'])) array over ALL its positions."""
    return _ratio(np.abs(got - ref['f64']), ref['A'][:, None, :])


def allowed(case, margin=MARGIN):
    """The device's bound per sample in units of A 2^-53, never above the ceiling."""
    return min(1.0 + margin * DEV[case.id], CEILING / UNIT)


def moved(case, fault):
    """By how many of the device's bounds the fault moves the long-double sum of the case, at the sample it moves most."""
    ref = reference(case)
    d = np.abs(exact(case, ref['rr'], ref['js'], fault) - ref['exact']).astype(np.float64)
    return _ratio(d, ref['A'][:, None, ref['at']]) / allowed(case)
