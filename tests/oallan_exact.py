"""An exact overlapping Allan variance and the tolerance that follows from it (used by test_oallan_oracle.py and test_gpu_oallan.py).

For a series x[0..n) and an averaging factor m, with theta[k] = sum_{i<k} x[i] and theta[0] = 0:

    d_m[k]   = theta[k+2m] - 2 theta[k+m] + theta[k],      k = 0 .. n - 2m          (n - 2m + 1 terms)
    oavar(m) = sum_k d_m[k]**2 / (2 m**2 (n - 2m + 1)),    tau(m) = m * (1 / fs)

at the averaging factors of allan_exact.factors (the reference's own list).  d is unchanged when theta gains a + b k, so the
estimator does not see a constant offset of x.

``exact(x, fs)``: theta is the cumulative sum of x - x[0] in np.longdouble; differences, squares and sum in long double.  That path
is taken where allan_exact.WIDE holds (a long double of at least 63 mantissa bits).  Otherwise every d is ONE math.fsum over the 2 m
samples involved and the sum of squares an fsum too, on allan_exact.sampled_factors for series above allan_exact.FSUM_ALL samples
and NaN elsewhere, as allan_exact.exact does.

``bound(x, exact_oavar, m)`` is the relative tolerance per averaging factor, with n = x.size:

    1e-10 + 8 * log2(n) * 2**-53 * n * max|x - x[0]| / (m * sqrt(2 * exact))

The first term is the project's Allan tolerance.  The second is the worst case of ANY fp64 implementation that rounds a blocked
or pairwise prefix of the shifted samples: |theta| <= n max|w| with one rounding (2**-53 relative) per level of the scan, log2(n)
levels; d carries four such errors (theta[k+m] counts twice), hence 4 log2(n) 2**-53 n max|w|; rms(d) = m sqrt(2 oavar), and the
relative error of sum(d**2) is twice that of d over its rms.  Tile-local prefixes (csrc/oallan.hip, tile form) stay far below it.
A float64 NumPy restatement with a SEQUENTIAL global cumsum reaches at most 0.062 of it over n = 18, 30 000 and 1 440 000, each as
white noise, with an offset of 1e6 and as white noise plus a random walk; without the log2(n) factor that restatement would be
at 1.26 of the bound, so the factor stays."""
import math

import numpy as np

import allan_exact as ax


def factors(n, fs):
    """The averaging factors: exactly the list allan_var evaluates."""
    return ax.factors(n, fs)[0]


def exact_longdouble(x, fs):
    assert ax.WIDE
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    mult = factors(n, fs)
    out = np.empty(len(mult))
    with np.errstate(invalid='ignore', over='ignore'):
        th = np.concatenate([[np.longdouble(0)], np.cumsum(x.astype(np.longdouble) - np.longdouble(x[0]))])
        for i, m in enumerate(mult):
            d = th[2 * m:] - 2 * th[m:n + 1 - m] + th[:n + 1 - 2 * m]
            out[i] = float(np.sum(d * d) / (2 * np.longdouble(m) * np.longdouble(m) * (n - 2 * m + 1)))
    return out


def exact_fsum(x, fs, only=None):
    """Every factor (or the factors in `only`, NaN elsewhere) through math.fsum: d[k] = sum x[k+m .. k+2m) - sum x[k .. k+m)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    mult = factors(n, fs)
    pos, neg = x.tolist(), (-x).tolist()
    out = np.full(len(mult), np.nan)
    for i, m in enumerate(mult):
        if only is not None and m not in only:
            continue
        d = [ax._fsum(pos[k + m:k + 2 * m] + neg[k:k + m]) for k in range(n - 2 * m + 1)]
        out[i] = ax._fsum([v * v for v in d]) / (2.0 * (float(m) * float(m)) * (n - 2 * m + 1))
    return out


def exact(x, fs):
    """(oavar, tau): the exact overlapping Allan variance per averaging factor (NaN = not evaluated) and tau."""
    x = np.asarray(x, dtype=np.float64)
    mult = factors(x.size, fs)
    tau = np.array([m * (1.0 / fs) for m in mult])
    if ax.WIDE:
        return exact_longdouble(x, fs), tau
    return exact_fsum(x, fs, None if x.size <= ax.FSUM_ALL else ax.sampled_factors(x.size, fs)), tau


def restated(x, fs):
    """The definition in float64 NumPy with a sequential global cumsum of x - x[0]: the plainest fp64 implementation."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    th = np.concatenate([[0.0], np.cumsum(x - x[0])])
    out = []
    for m in factors(n, fs):
        d = th[2 * m:] - 2 * th[m:n + 1 - m] + th[:n + 1 - 2 * m]
        out.append(np.sum(d * d) / (2.0 * (float(m) * float(m)) * (n - 2 * m + 1)))
    return np.array(out)


def bound(x, exact_oavar, m):
    """Relative tolerance per averaging factor (derivation in the module's text); max|x - x[0]| over the finite samples."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    w = x - x[0]
    big = float(np.max(np.abs(w[np.isfinite(w)])))
    with np.errstate(invalid='ignore', divide='ignore'):
        return 1e-10 + 8.0 * math.log2(n) * 2.0 ** -53 * n * big / (np.asarray(m, dtype=np.float64)
                                                                    * np.sqrt(2.0 * np.asarray(exact_oavar, dtype=np.float64)))


def ratio(got, want, tol):
    """Largest |got / want - 1| / tol over the factors that were evaluated; an exact 0 must be met exactly."""
    got, want, tol = np.asarray(got), np.asarray(want), np.asarray(tol)
    k = ~np.isnan(want)
    assert k.any()
    got, want, tol = got[k], want[k], tol[k]
    zero = want == 0.0
    assert np.array_equal(got[zero], want[zero])
    if zero.all():
        return 0.0
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.abs(got[~zero] / want[~zero] - 1.0) / tol[~zero]
    return float(np.max(np.where(np.isnan(r), np.inf, r)))
