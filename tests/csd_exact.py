"""An exact Welch cross-spectral density and the tolerance that follows from it (used by test_csd_oracle.py and test_gpu_csd.py, and at the edges --
the shapes of csd_edge_cases.py -- by test_csd_edges_oracle.py and test_gpu_csd_edges.py).

With psd_exact's symbols, for series x and y of n samples, a segment length L (a power of two), a step D, a window w and a rate fs:

    K       = (n - L) // D + 1
    X_s     = DFT_L((segx_s - mean(segx_s)) * w)     likewise Y_s; without detrend no mean is removed
    Pxx[k]  = c_k / (K fs U) sum_s |X_s[k]|^2         Pyy likewise,  k = 0 .. L/2,  U = sum w^2,  c_k = 2 (1 at k = 0 and L/2)
    Pxy[k]  = c_k / (K fs U) sum_s conj(X_s[k]) Y_s[k]   complex

scipy.signal.csd(x, y, fs, window, nperseg=L, noverlap=L-D, detrend='constant' | False, scaling='density'); Pxx is
scipy.signal.welch of x.

``exact(x, y, fs, L, D, window, detrend)`` evaluates this in np.longdouble (np.fft.rfft keeps long double, which is asserted) and
returns (Pxx, Pyy, Pxy, f) rounded to float64 / complex128 at the end.

``tol(x, y, fs, L, D, window, detrend, Pxx, Pyy)`` is the ABSOLUTE tolerance per bin, (tol_xx, tol_yy, tol_xy):

    d_s[k] = 2^-53 (4 log2 L sqrt(||yx_s||^2 + ||yy_s||^2) + (2 + log2 L) g[k] max(max|segx_s|, max|segy_s|))
    e[k]   = c_k mean_s(d_s^2) / (fs U)
    tol_xx = 1e-10 Pxx + 2 sqrt(Pxx e) + e           (tol_yy likewise)
    tol_xy = 1e-10 sqrt(Pxx Pyy) + sqrt(Pxx e) + sqrt(Pyy e) + e         on |got - exact| as complex numbers

g[k] is psd_exact's.  The device transforms a segment of x and the same segment of y as ONE complex transform z = yx + i yy; the
backward error of Z scales with ||z||, so the smaller series inherits the larger one's rounding: d_s has the norm of both and the
larger of the two maxima.  An error d in X and in Y enters conj(X) Y as |X| d + |Y| d + d^2, hence tol_xy.

``packed(x, y, ...)`` restates the device's form in float64 NumPy: Z = fft(yx + i yy), A = Z[k], B = conj(Z[L-k]),
X = (A + B) / 2, Y = (A - B) / (2i), the four sums from the separated X and Y.  ``recombined(x, y, ...)`` is the form NOT to use:
it sums |A|^2, |B|^2 and A conj(B) and recombines at the end, Pyy = (sum AA + sum BB - 2 Re sum AB) / 4, which cancels when one
series is much smaller than the other; test_csd_oracle.py holds the first inside the tolerance and the second outside it."""
import math

import numpy as np

from psd_exact import LD, WINDOWS, window, segments, freqs, ratio, series, _frames, _ck       # noqa: F401

PAIR_KINDS = ('white/white', 'small/offset', 'offset/walk', 'tone/white', 'tone/smalltone', 'constant/white', 'small/large')
GRID_L = (8, 64, 1024, 4096, 8192)


def pair(kind, n, seed):
    """The seven kinds of input pairs of the CSD tests (psd_exact.series with two seeds, scaled)."""
    scaled = {'small': (1e-6, 'white'), 'large': (1e3, 'white'), 'smalltone': (1e-6, 'tone')}

    def one(k, s):
        f, base = scaled.get(k, (1.0, k))
        return f * series(base, n, s)
    a, b = kind.split('/')
    return one(a, seed), one(b, seed + 1)


def _spectra(x, y, L, D, kind, detrend, dtype):
    sx = _frames(np.asarray(x, dtype=np.float64), L, D).astype(dtype)
    sy = _frames(np.asarray(y, dtype=np.float64), L, D).astype(dtype)
    assert sx.shape == sy.shape
    w = window(L, kind, dtype)
    if detrend:
        sx = sx - sx.mean(axis=1, keepdims=True)
        sy = sy - sy.mean(axis=1, keepdims=True)
    return sx * w, sy * w, w


def _scale(L, fs, w, dtype):
    return _ck(L).astype(dtype) / (dtype(fs) * (w * w).sum())


def _csd(x, y, fs, L, D, kind, detrend, dtype):
    yx, yy, w = _spectra(x, y, L, D, kind, detrend, dtype)
    X, Y = np.fft.rfft(yx, axis=1), np.fft.rfft(yy, axis=1)
    if dtype is LD:
        assert X.dtype == np.complex256 and Y.dtype == np.complex256, 'np.fft.rfft did not keep long double'
    c = _scale(L, fs, w, dtype)
    pxx = (X.real ** 2 + X.imag ** 2).mean(axis=0) * c
    pyy = (Y.real ** 2 + Y.imag ** 2).mean(axis=0) * c
    pxy = (np.conj(X) * Y).mean(axis=0) * c
    return pxx, pyy, pxy


def exact(x, y, fs, L, D, kind='hann', detrend=True):
    """(Pxx, Pyy, Pxy, f): the definition in long double, rounded to float64 / complex128 at the end."""
    with np.errstate(invalid='ignore', over='ignore'):
        pxx, pyy, pxy = _csd(x, y, fs, L, D, kind, detrend, LD)
    return pxx.astype(np.float64), pyy.astype(np.float64), pxy.astype(np.complex128), freqs(fs, L)


def _packed_ab(x, y, L, D, kind, detrend):
    yx, yy, w = _spectra(x, y, L, D, kind, detrend, np.float64)
    Z = np.fft.fft(yx + 1j * yy, axis=1)
    k = np.arange(L // 2 + 1)
    return Z[:, k], np.conj(Z[:, (L - k) % L]), w


def packed(x, y, fs, L, D, kind='hann', detrend=True):
    """The device's form in float64: one complex transform per segment, separated per segment, four sums.  (Pxx, Pyy, Pxy)."""
    A, B, w = _packed_ab(x, y, L, D, kind, detrend)
    X, Y = (A + B) / 2, (A - B) / 2j
    c = _scale(L, fs, w, np.float64)
    return ((X.real ** 2 + X.imag ** 2).mean(axis=0) * c, (Y.real ** 2 + Y.imag ** 2).mean(axis=0) * c,
            (np.conj(X) * Y).mean(axis=0) * c)


def recombined(x, y, fs, L, D, kind='hann', detrend=True):
    """The form that cancels: sums of |A|^2, |B|^2 and A conj(B) recombined at the end.  (Pxx, Pyy, Pxy)."""
    A, B, w = _packed_ab(x, y, L, D, kind, detrend)
    aa, bb = (A.real ** 2 + A.imag ** 2).mean(axis=0), (B.real ** 2 + B.imag ** 2).mean(axis=0)
    ab = (A * np.conj(B)).mean(axis=0)
    c = _scale(L, fs, w, np.float64)
    # conj(X) Y = (conj(A) + conj(B)) (A - B) / 4i = (|A|^2 - |B|^2 + 2i Im(A conj(B))) / 4i
    return ((aa + bb + 2 * ab.real) / 4 * c, (aa + bb - 2 * ab.real) / 4 * c, (aa - bb + 2j * ab.imag) / 4j * c)


def tol(x, y, fs, L, D, kind, detrend, Pxx, Pyy):
    """Absolute tolerances per bin (tol_xx, tol_yy, tol_xy) around the exact spectra (derivation in the module's text)."""
    sx = _frames(np.asarray(x, dtype=np.float64), L, D)
    sy = _frames(np.asarray(y, dtype=np.float64), L, D)
    w = window(L, kind, np.float64)
    yx = (sx - sx.mean(axis=1, keepdims=True) if detrend else sx) * w
    yy = (sy - sy.mean(axis=1, keepdims=True) if detrend else sy) * w
    lg = math.log2(L)
    a = 2.0 ** -53 * 4 * lg * np.sqrt((yx * yx).sum(axis=1) + (yy * yy).sum(axis=1))
    m = 2.0 ** -53 * (2 + lg) * np.maximum(np.abs(sx).max(axis=1), np.abs(sy).max(axis=1))
    g = np.maximum(math.sqrt(L), np.abs(np.fft.rfft(w)))
    d2 = np.mean(a * a) + 2 * g * np.mean(a * m) + g * g * np.mean(m * m)        # mean over s of (a_s + g[k] m_s)^2
    e = _ck(L) * d2 / (float(fs) * float((w * w).sum()))
    Pxx, Pyy = np.asarray(Pxx, dtype=np.float64), np.asarray(Pyy, dtype=np.float64)
    return (1e-10 * Pxx + 2 * np.sqrt(Pxx * e) + e, 1e-10 * Pyy + 2 * np.sqrt(Pyy * e) + e,
            1e-10 * np.sqrt(Pxx * Pyy) + np.sqrt(Pxx * e) + np.sqrt(Pyy * e) + e)


def ratios(got, want, tolerance):
    """(r_xx, r_yy, r_xy): psd_exact.ratio of each output; got and want are (Pxx, Pyy, Pxy) with Pxy complex."""
    return tuple(ratio(g, w, t) if not np.iscomplexobj(w) else ratio(np.abs(np.asarray(g) - w), np.zeros(w.shape), t)
                 for g, w, t in zip(got, want, tolerance))
