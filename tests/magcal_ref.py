"""NumPy restatement of the reference's soft / hard-iron magnetometer calibration, vectorised over runs.  TEST INFRASTRUCTURE only
(like tests/inclinometer_ref.py): the checker the device kernel (csrc/magcal.hip) is held to, itself held to the reference's own
library by tests/golden/magcal/*.npz (tests/test_magcal_oracle.py).

Restates demo_algorithms/mag_calibrate_src/src/MagCalibration.c step by step -- the rows themselves, not the moments the kernel
accumulates:
  1. per range v = (M^T M)^-1 M^T 1, sign so that its largest-magnitude component is positive, normalised: the rows of orthMtx;
  2. every row times orthMtx; sZ2Y, sZ2X, sY2X = (max - min) of two columns over the x, y, z range; sens; soft_iron = sens . orthMtx;
  3. rows scaled by sens; sphere fit over all three ranges (H = [2w, 1], B = |w|^2) -> hard_iron = [p, sqrt(p3 + p.p)];
  4. mag_cal = the scaled rows minus p, the three ranges stacked.
IEEE throughout, as the C code: the linear systems are eliminated without pivoting (a singular one gives the non-finite values its
divisions give, numpy.linalg would raise), the matrix products are full ones (0 * NaN reaches the sum), nothing is tested or clamped.
"""
import numpy as np


def solve(A, b, dtype=np.float64):
    """x of A x = b for stacks A (..., N, N), b (..., N): elimination without pivoting, IEEE (no exception for a singular A)."""
    A, b = np.array(A, dtype=dtype), np.array(b, dtype=dtype)
    N = A.shape[-1]
    for k in range(N):
        for i in range(k + 1, N):
            f = A[..., i, k] / A[..., k, k]
            A[..., i, k:] = A[..., i, k:] - f[..., None] * A[..., k, k:]
            b[..., i] = b[..., i] - f * b[..., k]
    x = np.zeros_like(b)
    for i in range(N - 1, -1, -1):
        s = b[..., i].copy()
        for j in range(i + 1, N):
            s = s - A[..., i, j] * x[..., j]
        x[..., i] = s / A[..., i, i]
    return x


def _vec_max(a):
    """vecMax's index over the columns of a (R, 3): the first largest; a NaN never wins a > comparison."""
    idx = np.zeros(a.shape[0], dtype=np.int64)
    best = a[:, 0].copy()
    for c in (1, 2):
        win = a[:, c] > best
        idx[win] = c
        best = np.where(win, a[:, c], best)
    return idx


def normal_choice(M, dtype=np.float64):
    """What decides the sign of a range's normal, M (R, k, 3) -> (the component vecMax selects, whether the normal is negated)."""
    M = np.asarray(M, dtype=dtype)
    with np.errstate(all='ignore'):
        v = solve(np.einsum('rki,rkj->rij', M, M), M.sum(axis=1), dtype)
    idx = _vec_max(np.abs(v))
    return idx, v[np.arange(v.shape[0]), idx] < 0.0


def points_normal(M, dtype=np.float64):
    """GetPointsNormal + the sign and norm MagCalibrate gives it: M (R, k, 3) -> (R, 3)."""
    mtm = np.einsum('rki,rkj->rij', M, M)
    mtb = M.sum(axis=1)
    v = solve(mtm, mtb, dtype)
    idx = _vec_max(np.abs(v))
    flip = v[np.arange(v.shape[0]), idx] < 0.0
    v = np.where(flip[:, None], -1.0 * v, v)
    return v / np.sqrt((v * v).sum(axis=1))[:, None]


def _span(col):
    return col.max(axis=1) - col.min(axis=1)


def calibrate(mx, my, mz, dtype=np.float64):
    """mx, my, mz: the rows of the rotations about x, y, z, (R, nx, 3), (R, ny, 3), (R, nz, 3) (or without the leading R).
    Returns soft_iron (R, 3, 3), hard_iron (R, 4), mag_cal (R, nx + ny + nz, 3).  dtype: the format everything is evaluated in
    (np.longdouble: the same steps in extended precision, what the float64 evaluation's own rounding is measured against)."""
    single = np.ndim(mx) == 2
    mx, my, mz = (np.asarray(m, dtype=dtype).reshape((-1,) + np.shape(m)[-2:]) for m in (mx, my, mz))
    with np.errstate(all='ignore'):
        orth = np.stack([points_normal(mx, dtype), points_normal(my, dtype), points_normal(mz, dtype)], axis=1)         # (R, 3, 3), rows vx vy vz
        ux, uy, uz = (np.einsum('rij,rkj->rki', orth, m) for m in (mx, my, mz))
        z2y = _span(ux[:, :, 2]) / _span(ux[:, :, 1])
        z2x = _span(uy[:, :, 2]) / _span(uy[:, :, 0])
        y2x = _span(uz[:, :, 1]) / _span(uz[:, :, 0])
        sens = np.zeros_like(orth)
        sens[:, 0, 0] = 1.0
        sens[:, 1, 1] = 1.0 / y2x
        sens[:, 2, 2] = (1.0 + y2x * y2x) / (y2x * y2x * z2x + y2x * z2y)
        si = np.einsum('rim,rmk->rik', sens, orth)
        w = np.concatenate([np.einsum('rij,rkj->rki', sens, u) for u in (ux, uy, uz)], axis=1)
        H = np.concatenate([2.0 * w, np.ones(w.shape[:2] + (1,), dtype=dtype)], axis=2)
        B = (w * w).sum(axis=2)
        p = solve(np.einsum('rki,rkj->rij', H, H), np.einsum('rki,rk->ri', H, B), dtype)
        hi = np.concatenate([p[:, 0:3], np.sqrt(p[:, 3] + (p[:, 0:3] * p[:, 0:3]).sum(axis=1))[:, None]], axis=1)
        cal = w - p[:, None, 0:3]
    return (si[0], hi[0], cal[0]) if single else (si, hi, cal)


def calibrate_series(mag, segments, dtype=np.float64):
    """mag (R, n, 3) or (n, 3) and ((x0, xf), (y0, yf), (z0, zf)): MagCal.run's slicing (mag_calibrate.py:81-88)."""
    (x0, xf), (y0, yf), (z0, zf) = segments
    mag = np.asarray(mag, dtype=dtype)
    return calibrate(mag[..., x0:xf, :], mag[..., y0:yf, :], mag[..., z0:zf, :], dtype)
