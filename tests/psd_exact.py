"""An exact Welch power spectral density and the tolerance that follows from it (used by test_psd_oracle.py and test_gpu_psd.py).

For a series x[0..n), a segment length L (a power of two), a step D, a window w and a sampling rate fs:

    K      = (n - L) // D + 1                      segments; samples past (K-1) D + L are not read
    seg_s  = x[sD .. sD+L)                          s = 0 .. K-1
    y_s[k] = (seg_s[k] - mean(seg_s)) * w[k]        detrend;  seg_s[k] * w[k] without
    X_s    = DFT_L(y_s)
    P[k]   = c_k * (1/K) * sum_s |X_s[k]|^2 / (fs * U),   k = 0 .. L/2,   U = sum_k w[k]^2
    c_k    = 2 for 0 < k < L/2,  1 for k = 0 and k = L/2
    f[k]   = k * fs / L

with w = 1 ('boxcar') or the periodic Hann window 0.5 - 0.5 cos(2 pi k / L) ('hann'): scipy.signal.welch(x, fs, window, nperseg=L,
noverlap=L-D, detrend='constant' | False, scaling='density').

``exact(x, fs, L, D, window, detrend)`` evaluates this in np.longdouble: the window from long-double cos, the mean, the
transform (np.fft.rfft keeps long double: its result is complex256, which exact asserts) and the sums.

``tol(x, fs, L, D, window, detrend, P)`` is the ABSOLUTE tolerance per bin:

    tol[k] = 1e-10 * P[k] + 2 * sqrt(P[k] * e[k]) + e[k]
    e[k]   = c_k * mean_s(d_s^2) / (fs * U)
    d_s[k] = 2^-53 * (4 log2(L) * ||y_s||_2 + (2 + log2(L)) * g[k] * max|seg_s|),    g[k] = max(sqrt(L), |W[k]|),  W = DFT_L(w)

d_s bounds the error of X_s: the norm-wise backward error of any fp64 power-of-two FFT (4 log2(L) roundings of the whole vector
is generous for radix 2), plus one rounding per level of a balanced mean and one of the subtraction, each at most
2^-53 max|seg_s| per sample.  An error d in X enters |X|^2 as 2 |X| d + d^2, hence the second and third term; the first is the
project's tolerance for the scaling.  A per-bin RELATIVE tolerance does not exist for a spectrum with dynamic range: next to a
tone of 100, a bin at the 1e-3 floor legitimately moves by far more than 1e-10 of itself.

g[k] is the one constant raised over the first form of this tolerance, which had sqrt(L) at every bin: independent errors of
2^-53 max|seg_s| per sample have norm sqrt(L) times that, but the error of the MEAN is the same number at every sample, so it
arrives in X as that number times the window's own transform W[k] -- L at bin 0 for the boxcar (L/2 at bin 0 and L/4 at bin 1
for Hann), where the exact value is 0 after detrending.  With sqrt(L) a mean that is CORRECTLY ROUNDED (half an ulp of 1e6) is
already outside at L = 4096: the float64 restatement below reached 5.6 of that form there (boxcar, detrend, the offset of 1e6,
bin 0; 4.1 and 2.8 with the random walk), and at most 2.4e-4 of it at every other bin.  At every bin where |W[k]| <= sqrt(L),
that is all but those named, the tolerance is the first form's.

Measured on the CPU (tests/test_psd_oracle.py prints every figure): the float64 restatement below -- np.fft.rfft and np.mean in
float64 -- over L = 8, 64, 1024, 4096, 8192 with D = L/4, L/2, L, both windows, detrend on and off, on white noise, an offset
of 1e6, white noise plus a random walk, a tone of 100 over noise of 1e-3 and a constant series; the largest ratio is 0.35
(L = 8192, D = L, boxcar, no detrend, the offset of 1e6)."""
import math

import numpy as np

LD = np.longdouble
WINDOWS = ('boxcar', 'hann')
KINDS = ('white', 'offset', 'walk', 'tone', 'constant')


def series(kind, n, seed):
    """The five kinds of input of the PSD tests."""
    rng = np.random.default_rng(seed)
    if kind == 'constant':
        return np.full(n, 3.25)
    x = rng.standard_normal(n)
    if kind == 'offset':
        x += 1e6
    elif kind == 'walk':
        x += np.cumsum(rng.standard_normal(n))
    elif kind == 'tone':
        x = 1e-3 * x + 100.0 * np.sin(2 * np.pi * 0.1234 * np.arange(n) + 0.3)
    return x


def window(L, kind, dtype=LD):
    assert kind in WINDOWS
    if kind == 'boxcar':
        return np.ones(L, dtype=dtype)
    k = np.arange(L, dtype=dtype)
    pi = 4 * np.arctan(LD(1)) if dtype is LD else np.pi
    return dtype(0.5) - dtype(0.5) * np.cos(2 * pi * k / L)


def segments(n, L, D):
    return (n - L) // D + 1


def _frames(x, L, D):
    K = segments(x.size, L, D)
    return np.lib.stride_tricks.sliding_window_view(x, L)[::D][:K]


def _ck(L):
    c = np.full(L // 2 + 1, 2.0)
    c[0] = c[-1] = 1.0
    return c


def _welch(x, fs, L, D, kind, detrend, dtype):
    seg = _frames(np.asarray(x, dtype=np.float64), L, D).astype(dtype)
    w = window(L, kind, dtype)
    if detrend:
        seg = seg - seg.mean(axis=1, keepdims=True)
    X = np.fft.rfft(seg * w, axis=1)
    if dtype is LD:
        assert X.dtype == np.complex256, 'np.fft.rfft did not keep long double'
    p = (X.real ** 2 + X.imag ** 2).mean(axis=0) * _ck(L).astype(dtype) / (dtype(fs) * (w * w).sum())
    return p


def freqs(fs, L):
    return np.arange(L // 2 + 1) * float(fs) / L


def exact(x, fs, L, D, kind='hann', detrend=True):
    """(P, f): the definition in long double, rounded to float64 at the end."""
    with np.errstate(invalid='ignore', over='ignore'):
        return _welch(x, fs, L, D, kind, detrend, LD).astype(np.float64), freqs(fs, L)


def restated(x, fs, L, D, kind='hann', detrend=True):
    """The definition in float64 NumPy: the plainest fp64 implementation."""
    return _welch(x, fs, L, D, kind, detrend, np.float64)


def tol(x, fs, L, D, kind, detrend, P):
    """Absolute tolerance per bin (derivation in the module's text) around the exact P."""
    seg = _frames(np.asarray(x, dtype=np.float64), L, D)
    w = window(L, kind, np.float64)
    y = (seg - seg.mean(axis=1, keepdims=True) if detrend else seg) * w
    lg = math.log2(L)
    a = 2.0 ** -53 * 4 * lg * np.sqrt((y * y).sum(axis=1))
    m = 2.0 ** -53 * (2 + lg) * np.abs(seg).max(axis=1)
    g = np.maximum(math.sqrt(L), np.abs(np.fft.rfft(w)))
    d2 = np.mean(a * a) + 2 * g * np.mean(a * m) + g * g * np.mean(m * m)        # mean over s of (a_s + g[k] m_s)^2
    e = _ck(L) * d2 / (float(fs) * float((w * w).sum()))
    P = np.asarray(P, dtype=np.float64)
    return 1e-10 * P + 2 * np.sqrt(P * e) + e


def ratio(got, want, tolerance):
    """Largest |got - want| / tol over the bins; a NaN in got counts as infinite."""
    got, want, tolerance = np.asarray(got), np.asarray(want), np.asarray(tolerance)
    assert got.shape == want.shape == tolerance.shape and np.all(tolerance > 0)
    r = np.abs(got - want) / tolerance
    return float(np.max(np.where(np.isnan(r), np.inf, r)))
