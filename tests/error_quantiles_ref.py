"""NumPy restatement of the error quantiles across runs (test infrastructure; no test in it, imported by tests only).

    keys(traj, ref_nav, samples, which, ned)  -> (3, m, runs): horizontal sqrt(e0^2 + e1^2), vertical |e2|, 3-D sqrt(e0^2 + e1^2 + e2^2)
                                                 of the position (which = 0) or velocity (which = 1) error
    nearest_rank(row, probs)                  -> (values (q,), N): the k-th smallest finite key, k = min(max(ceil(p N), 1), N)
    quantile_rows(rows, probs)                -> (values (rows, q), count (rows,))
    key_tolerance(keys, which, ned)           -> what a key may differ by from a device's

The errors are tests/error_curve_ref.py's expression (errors()); nothing here comes from a device.
"""
import numpy as np

import error_curve_ref


def keys(traj, ref_nav, samples=None, which=0, ned=False):
    """traj (runs, n, 9), ref_nav (n, 9) -> (3, m, runs).  ned: the position error in local NED metres (ref_frame 0)."""
    with np.errstate(invalid='ignore', over='ignore'):
        e = error_curve_ref.errors(traj, ref_nav, samples, bool(ned) and not which)[..., slice(6, 9) if which else slice(3, 6)]
        e = np.moveaxis(e, 0, 1)                                    # (m, runs, 3)
        h2 = e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]
        return np.stack([np.sqrt(h2), np.abs(e[..., 2]), np.sqrt(h2 + e[..., 2] * e[..., 2])])


def nearest_rank(row, probs):
    """Nearest rank on the finite keys of one row: p * N is one float64 product; NaN when no key is finite."""
    row = np.asarray(row, dtype=np.float64).reshape(-1)
    kept = np.sort(row[np.isfinite(row)])
    N = kept.size
    out = np.full(len(probs), np.nan)
    for i, p in enumerate(probs):
        if N:
            k = int(min(max(np.ceil(np.float64(p) * np.float64(N)), 1.0), N))
            out[i] = kept[k - 1]
    return out, N


def quantile_rows(rows, probs):
    rows = np.asarray(rows, dtype=np.float64)
    got = [nearest_rank(r, probs) for r in rows]
    return np.array([g[0] for g in got]).reshape(rows.shape[0], len(probs)), np.array([float(g[1]) for g in got])


def key_tolerance(k, which, ned):
    """(3, ...) bound of |device key - restated key|.  The components carry the tolerance tests/test_gpu_error_curve.py uses on the
    same arithmetic (_atol: 1e-9, 2e-8 for NED metres); a change of every component by at most a moves the horizontal key by at
    most sqrt(2) a, the vertical by a and the 3-D key by sqrt(3) a (the norm is 1-Lipschitz in the 2-norm of its argument), and
    the square root and the contraction of the sum of squares add 4 units in the last place of the key."""
    a = 2e-8 if (ned and which == 0) else 1e-9
    scale = np.array([np.sqrt(2.0), 1.0, np.sqrt(3.0)]).reshape((3,) + (1,) * (np.ndim(k) - 1))
    with np.errstate(invalid='ignore'):
        return scale * a + 4.0 * np.spacing(np.abs(k))
