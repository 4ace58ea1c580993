"""An exact Allan variance and the tolerance that follows from it (used by test_allan_exact_oracle.py and test_gpu_allan_edges.py).

``exact(x, fs)`` evaluates allan.allan_var (gnss_ins_sim/allan/allan.py:18-59) with no rounding that matters: for an averaging
factor m with nb = n // m bins, every bin-sum difference d[b] = S[b+1] - S[b] is ONE math.fsum over the 2 m samples involved (the
correctly rounded value of the exact difference), and sum(d**2) is an fsum as well; avar = 0.5 / (nb - 1) * sum / m**2.  What is
left is the rounding of each d (2**-53 relative), of each square (2**-53) and of the two final operations: 1e-15.

A vectorised fast path does the same on x - x[0] in np.longdouble (bin sums by a reshape, their differences and squares in long
double).  It is taken only where long double has at least 63 mantissa bits: the rounding of a bin sum is then at most
2**-64 m max|x - x[0]|, 4096 times less than the term ``bound`` allows an fp64 implementation per level.
test_allan_exact_oracle.py holds the two paths together.  Without such a long double, series above ``FSUM_ALL`` samples are
evaluated at three factors per level (the first, the middle and the last one) through fsum and NaN elsewhere: the caller checks
the factors that are not NaN in ``checked``.

``bound(x, exact_avar, levels)`` is the relative tolerance per averaging factor,

    1e-10 + 4 * 2**-52 * levels * max|x| / sqrt(exact_avar)

The 1e-10 is the project's own Allan tolerance.  The second term is the worst case of what ANY fp64
implementation loses that rounds unshifted sums of m samples once per level: with eps = 2**-52, a sum of m samples of size
max|x| that is rounded once at each of `levels` decade levels is off by at most eps * levels * m * max|x| / 2, so a difference d
of two of them by at most eps * levels * m * max|x|.  The relative error of sum(d**2) is at most twice the error of d over
rms(d), and rms(d) = sqrt(2 * avar) * m, so it is at most 2 * eps * levels * max|x| / (sqrt(2) * sqrt(avar)); the factor 4
instead of sqrt(2) leaves room for the roundings inside one level.  An implementation that shifts every chunk by its first entry
(csrc/allan.hip) stays far below it; the float64 NumPy oracle, which forms means of unshifted samples, comes within 0.025 of it
on series with an offset of 1e6 (its worst relative error there: 3.8e-9)."""
import math

import numpy as np

WIDE = np.finfo(np.longdouble).nmant >= 63
FSUM_ALL = 300000


def factors(n, fs):
    """The averaging factors of allan.py:29-43 and the number of decade levels (oracle/ins_np.py allan_var, restated)."""
    mmax = int(math.floor(n / 9.0))
    if mmax * (1.0 / fs) < 1:
        return [], 0
    levels = math.ceil(math.log10(mmax))
    mult, scale = [], 0.1
    for _ in range(levels):
        scale *= 10
        for j in range(1, 10):
            m = int(j * scale)
            if m > mmax:
                break
            mult.append(m)
    return mult, levels


def _fsum(v):
    try:
        return math.fsum(v)
    except (ValueError, OverflowError):         # inf - inf inside the sum, or a sum beyond the range
        return float('nan')


def exact_fsum(x, fs, only=None):
    """Every factor (or the factors in `only`, NaN elsewhere) through math.fsum."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    mult, _ = factors(n, fs)
    pos, neg = x.tolist(), (-x).tolist()
    avar = np.full(len(mult), np.nan)
    for i, m in enumerate(mult):
        if only is not None and m not in only:
            continue
        nb = n // m
        if m == 1:                              # the correctly rounded difference of two doubles is their fp64 difference
            d = (x[1:nb] - x[:nb - 1]).tolist()
        else:
            d = [_fsum(pos[(b + 1) * m:(b + 2) * m] + neg[b * m:(b + 1) * m]) for b in range(nb - 1)]
        avar[i] = 0.5 / (nb - 1) * _fsum([v * v for v in d]) / (float(m) * float(m))
    return avar


def exact_longdouble(x, fs):
    assert WIDE
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    mult, _ = factors(n, fs)
    w = x.astype(np.longdouble) - np.longdouble(x[0])
    avar = np.empty(len(mult))
    with np.errstate(invalid='ignore', over='ignore'):
        for i, m in enumerate(mult):
            nb = n // m
            d = np.diff(w[:nb * m].reshape(nb, m).sum(axis=1))
            avar[i] = float(np.longdouble(0.5) / (nb - 1) * np.sum(d * d) / (np.longdouble(m) * np.longdouble(m)))
    return avar


def sampled_factors(n, fs):
    """Three factors per level: the first, the middle and the last one the level has."""
    mult, levels = factors(n, fs)
    keep = set()
    for k in range(levels):
        lv = [m for m in mult if 10 ** k <= m < 10 ** (k + 1)]
        keep.update((lv[0], lv[len(lv) // 2], lv[-1]))
    return keep


def exact(x, fs):
    """(avar, tau): the exact Allan variance per averaging factor (NaN = not evaluated, see the module's text) and the oracle's tau."""
    x = np.asarray(x, dtype=np.float64)
    mult, _ = factors(x.size, fs)
    tau = np.array([m * (1.0 / fs) for m in mult])
    if WIDE:
        return exact_longdouble(x, fs), tau
    return exact_fsum(x, fs, None if x.size <= FSUM_ALL else sampled_factors(x.size, fs)), tau


def bound(x, exact_avar, levels):
    """Relative tolerance per averaging factor (derivation in the module's text); max|x| over the finite samples."""
    x = np.asarray(x, dtype=np.float64)
    big = float(np.max(np.abs(x[np.isfinite(x)])))
    with np.errstate(invalid='ignore', divide='ignore'):
        return 1e-10 + 4.0 * 2.0 ** -52 * levels * big / np.sqrt(np.asarray(exact_avar, dtype=np.float64))


def ratio(got, want, tol):
    """Largest |got / want - 1| / tol over the factors that were evaluated (want not NaN)."""
    got, want, tol = np.asarray(got), np.asarray(want), np.asarray(tol)
    k = ~np.isnan(want)
    assert k.any()
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.abs(got[k] / want[k] - 1.0) / tol[k]
    return float(np.max(np.where(np.isnan(r), np.inf, r)))
