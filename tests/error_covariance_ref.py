"""NumPy restatement of the error covariance across runs (test infrastructure; no test in it, imported by tests only).

    errors3(traj, ref_nav, samples, which, ned)  -> (runs, m, 3): the position (which = 0) or velocity (which = 1) error, formed as
                                                    tests/error_curve_ref.py forms it
    record(e, dtype)                             -> (m, 10): count, mean[3], C[6] (00, 01, 02, 11, 12, 22), two passes in `dtype`;
                                                    a run with a non-finite component at a sample is left out of that sample
    merge(parts)                                 -> (m, 10): C = C_a + C_b + dd^T n_a n_b / n in the order given
    track_frame(mean, cov, yaw), error_ellipse(cov2), cov_of(rec)
    assert_record(got, b, what, slack)           -> the comparison every test makes, printed
    bounded(e, seed)                             -> dict(rec, tol_mean (m, 3), tol_c (m, 6), rel (m,)): the record and what a device
                                                    may differ from it by

The parity bound is the record's own (tests/error_curve_ref.py), measured on this side only:

    rel   = FACTOR * max(E, S, eps)
    E     = the float64 record's distance from its np.longdouble evaluation
    S     = the spread of the float64 record over PERMUTATIONS seeded permutations of the run order
            both per entry as |dC_ab| / (count sqrt(S_aa S_bb)) = |dC_ab| / sqrt(C_aa C_bb) and |dmean_a| / max(|mean_a|, sigma_a)
            of the long-double evaluation, the largest over the entries of the sample
    tol_c = rel * sqrt(C_aa C_bb),  tol_mean = rel * max(|mean_a|, sigma_a)

Where the inputs themselves may differ (NED metres, the fp32 origin) input_slack() adds what a change of every error component by
at most `a` moves the mean (a) and a co-moment (count (a sigma_a + a sigma_b + a^2)) by.  Nothing of it comes from a device.
"""
import numpy as np

import error_curve_ref

FACTOR = error_curve_ref.FACTOR
PERMUTATIONS = error_curve_ref.PERMUTATIONS
SEED = 20261019
UPPER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def errors3(traj, ref_nav, samples=None, which=0, ned=False, dtype=np.float64):
    with np.errstate(invalid='ignore', over='ignore'):
        e = error_curve_ref.errors(traj, ref_nav, samples, bool(ned) and not which, dtype=dtype)
    return e[..., 6:9] if which else e[..., 3:6]


def record(e, dtype=np.float64):
    """e (runs, m, 3) -> (m, 10) in `dtype`: two passes over the runs whose three components are finite at the sample."""
    e = np.ascontiguousarray(np.moveaxis(np.asarray(e), 0, 2))              # (m, 3, runs): NumPy sums the last axis pairwise
    ok = np.isfinite(e).all(axis=1)                                         # (m, runs)
    n = ok.sum(axis=1).astype(dtype)                                        # (m,)
    x = np.where(ok[:, None, :], e, 0).astype(dtype)
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = x.sum(axis=2) / n[:, None]
        d = np.where(ok[:, None, :], x - mean[:, :, None], dtype(0.0))
        c = np.stack([(d[:, a] * d[:, b]).sum(axis=1) for a, b in UPPER], axis=1)
    c[n == 0] = np.nan
    return np.concatenate([n[:, None], mean, c], axis=1)


def merge(parts):
    """Chan merge of (m, 10) records in the order given; a part with count 0 is a set without runs; no runs at all: NaN."""
    parts = [np.asarray(p) for p in parts]
    out = np.zeros_like(parts[0])
    for k in range(out.shape[0]):
        a = None
        for p in parts:
            b = p[k]
            if b[0] == 0:
                continue
            if a is None:
                a = b.copy()
                continue
            n = a[0] + b[0]
            d = b[1:4] - a[1:4]
            w = a[0] * b[0] / n
            a[4:10] = a[4:10] + b[4:10] + np.array([d[i] * d[j] for i, j in UPPER]) * w
            a[1:4] = a[1:4] + d * (b[0] / n)
            a[0] = n
        out[k] = a if a is not None else np.concatenate([[0.0], np.full(9, np.nan)])
    return out


def cov_of(rec):
    """(m, 3, 3) = C / count."""
    rec = np.asarray(rec)
    out = np.empty((rec.shape[0], 3, 3), dtype=rec.dtype)
    with np.errstate(invalid='ignore', divide='ignore'):
        for k, (a, b) in enumerate(UPPER):
            out[:, a, b] = out[:, b, a] = rec[:, 4 + k] / rec[:, 0]
    return out


def track_frame(mean, cov, yaw):
    """along = cos e0 + sin e1, cross = -sin e0 + cos e1, the vertical unchanged: (R mean, R cov R^T), one sample at a time."""
    mean, cov, yaw = np.asarray(mean, dtype=np.float64), np.asarray(cov, dtype=np.float64), np.asarray(yaw, dtype=np.float64)
    om, oc = np.empty_like(mean), np.empty_like(cov)
    for k in range(mean.shape[0]):
        c, s = np.cos(yaw[k]), np.sin(yaw[k])
        R = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
        om[k], oc[k] = R @ mean[k], R @ cov[k] @ R.T
    return om, oc


def error_ellipse(cov2):
    """(semi_major, semi_minor, azimuth in degrees in (-90, 90]) of one 2x2 block."""
    a, b, c = float(cov2[0][0]), float(cov2[0][1]), float(cov2[1][1])
    mid, rad = (a + c) / 2.0, np.hypot((a - c) / 2.0, b)
    az = np.degrees(0.5 * np.arctan2(2.0 * b, a - c))
    return np.sqrt(mid + rad), np.sqrt(max(mid - rad, 0.0)), az + 180.0 if az <= -90.0 else az


def _scales(ext):
    """(scale_mean (m, 3), scale_c (m, 6)) of a long-double record: max(|mean_a|, sigma_a) and sqrt(C_aa C_bb)."""
    n = ext[:, 0:1]
    with np.errstate(invalid='ignore', divide='ignore'):
        diag = np.stack([ext[:, 4], ext[:, 7], ext[:, 9]], axis=1)
        sigma = np.sqrt(diag / n)
        sm = np.maximum(np.abs(ext[:, 1:4]), sigma)
        sc = np.stack([np.sqrt(diag[:, a] * diag[:, b]) for a, b in UPPER], axis=1)
    return sm.astype(np.float64), sc.astype(np.float64)


def _rel(got, ext, sm, sc):
    """(m,) the largest normalised distance of a float64 record from the long-double one over its nine entries (0 / 0 counts 0)."""
    with np.errstate(invalid='ignore', divide='ignore'):
        dm = np.abs(got[:, 1:4].astype(np.longdouble) - ext[:, 1:4]).astype(np.float64) / sm
        dc = np.abs(got[:, 4:10].astype(np.longdouble) - ext[:, 4:10]).astype(np.float64) / sc
    r = np.concatenate([dm, dc], axis=1)
    return np.max(np.where(np.isfinite(r), r, 0.0), axis=1)


def bounded(e, seed=SEED):
    """The float64 record of e (runs, m, 3) and its bounds: dict(rec (m, 10), rel (m,), tol_mean (m, 3), tol_c (m, 6), E, S)."""
    e = np.asarray(e, dtype=np.float64)
    rec = record(e)
    ext = record(e, np.longdouble)
    sm, sc = _scales(ext)
    E = _rel(rec, ext, sm, sc)
    S = np.zeros_like(E)
    rng = np.random.RandomState(seed)
    for _ in range(PERMUTATIONS):
        S = np.maximum(S, _rel(record(e[rng.permutation(e.shape[0])]), rec.astype(np.longdouble), sm, sc))
    rel = FACTOR * np.maximum(np.maximum(E, S), np.finfo(np.float64).eps)
    with np.errstate(invalid='ignore'):
        return {'rec': rec, 'rel': rel, 'E': E, 'S': S, 'tol_mean': rel[:, None] * sm, 'tol_c': rel[:, None] * sc}


def input_slack(rec, a):
    """(slack_mean (m, 3), slack_c (m, 6)) for inputs that may differ by at most `a` per error component: the mean moves by at most
    a, a covariance entry by at most a sigma_a + a sigma_b + a^2, the co-moment by count times that."""
    rec = np.asarray(rec, dtype=np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        sigma = np.sqrt(np.stack([rec[:, 4], rec[:, 7], rec[:, 9]], axis=1) / rec[:, 0:1])
    sc = np.stack([rec[:, 0] * (a * sigma[:, i] + a * sigma[:, j] + a * a) for i, j in UPPER], axis=1)
    return np.full((rec.shape[0], 3), float(a)), sc


def component_tolerance(e, which, ned):
    """The section 4.10 component tolerance: 1e-9 max(1, |x|), 2e-8 m for NED positions."""
    if ned and which == 0:
        return 2e-8
    with np.errstate(invalid='ignore'):
        big = np.nanmax(np.where(np.isfinite(e), np.abs(e), 0.0)) if np.size(e) else 0.0
    return 1e-9 * max(1.0, float(big))


def assert_record(got, b, what, slack=None):
    """A (m, 10) record against bounded()'s: counts equal, NaN masks equal, mean and co-moments within the bound (an entry whose
    bound is 0 must be equal)."""
    want = b['rec']
    np.testing.assert_array_equal(got[:, 0], want[:, 0], err_msg=what + ': count')
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what + ': NaN mask')
    tm, tc = b['tol_mean'].copy(), b['tol_c'].copy()
    if slack is not None:
        tm, tc = tm + slack[0], tc + slack[1]
    fin = np.isfinite(want[:, 1:])
    d = np.where(fin, np.abs(np.where(fin, got[:, 1:], 0.0) - np.where(fin, want[:, 1:], 0.0)), 0.0)
    tol = np.where(fin, np.concatenate([tm, tc], axis=1), 0.0)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(d > 0.0, d / tol, 0.0)
    print('%s: largest |d| / bound = %.3g (bound %.3g x eps at its smallest)' % (what, ratio.max(), b['rel'].min() / np.finfo(np.float64).eps))
    worst = np.unravel_index(np.argmax(d - tol), d.shape)
    assert d[worst] <= tol[worst], '%s: entry %s is %.3e from the restatement, bound %.3e' % (what, worst, d[worst], tol[worst])
