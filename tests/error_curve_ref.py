"""NumPy restatement of the error-growth curve (test infrastructure; no test in it, imported by tests only).

At sample j the curve is InsDataMgr.__end_point_error_stats applied to the series cut after j (ins_data_manager.py:717-759):
calc_data_err / array_error (:454-553: x - ref, the attitude through attitude.angle_range_pi, extra_opt='ned' through lla2ecef
and the NED rotation at the reference position), then __array_stats (:797-808) over the runs:

    {'max': np.max(np.abs(x), 0), 'avg': np.average(x, 0), 'std': np.std(x, 0)}

    errors(traj, ref_nav, samples, ned)   -> (runs, m, 9) errors [att3, pos3, vel3]
    curve(traj, ref_nav, samples, ned)    -> dict(max, avg, std, tol_max, tol_avg, tol_std, E, S), every array (m, 9)

The bound of a record is measured on this side only, in the idiom of tests/magcal_records.py:

    tol = FACTOR * max(E, S, eps * |q|)
    E   = |q in float64 - q by the same steps in np.longdouble|
    S   = max |delta q| of the float64 restatement over PERMUTATIONS seeded permutations of the run order

Nothing of it comes from a device.
"""
import numpy as np

from oracle import ins_np

assert np.finfo(np.longdouble).eps < 2e-19, 'the bound of a record is measured against 80-bit long doubles: this host has none'

FACTOR = 16.0
PERMUTATIONS = 8
SEED = 20261017
CHUNK = 1 << 22                 # elements of one slab of samples: bounds the long-double temporaries


def _angle_range_pi(x, two_pi, pi):
    """attitude.angle_range_pi (attitude.py:799-812)."""
    x = np.mod(x, two_pi)
    return np.where(x > pi, x - two_pi, x)


def _lla2ecef(lla, dtype):
    """geoparams.lla2ecef (geoparams.py:70-87)."""
    one = dtype(1.0)
    sl, cl = np.sin(lla[..., 0]), np.cos(lla[..., 0])
    r = dtype(ins_np.RE) / np.sqrt(one - dtype(ins_np.E_SQR) * sl * sl)
    rho = (r + lla[..., 2]) * cl
    return np.stack([rho * np.cos(lla[..., 1]), rho * np.sin(lla[..., 1]), (r * (one - dtype(ins_np.E_SQR)) + lla[..., 2]) * sl], axis=-1)


def errors(traj, ref_nav, samples=None, ned=False, dtype=np.float64):
    """array_error of every run at `samples` (None: every sample): traj (runs, n, 9), ref_nav (n, 9) -> (runs, m, 9)."""
    j = slice(None) if samples is None else np.asarray(samples, dtype=np.int64)
    x = np.asarray(traj)[:, j].astype(dtype)
    r = np.asarray(ref_nav)[j].astype(dtype)[None]
    pi = dtype(np.pi) if dtype is np.float64 else np.arctan(dtype(1.0)) * dtype(4.0)
    ea = _angle_range_pi(x[..., 0:3] - r[..., 0:3], dtype(2.0) * pi, pi)
    if ned:
        rp = np.broadcast_to(r[..., 3:6], x[..., 3:6].shape)
        d = _lla2ecef(x[..., 3:6], dtype) - _lla2ecef(rp, dtype)
        sl, cl, so, co = np.sin(rp[..., 0]), np.cos(rp[..., 0]), np.sin(rp[..., 1]), np.cos(rp[..., 1])
        ep = np.stack([-sl * co * d[..., 0] - sl * so * d[..., 1] + cl * d[..., 2],
                       -so * d[..., 0] + co * d[..., 1],
                       -cl * co * d[..., 0] - cl * so * d[..., 1] - sl * d[..., 2]], axis=-1)
    else:
        ep = x[..., 3:6] - r[..., 3:6]
    return np.concatenate([ea, ep, x[..., 6:9] - r[..., 6:9]], axis=-1)


def array_stats(e):
    """InsDataMgr.__array_stats (ins_data_manager.py:797-808) over the run axis."""
    return {'max': np.max(np.abs(e), 0), 'avg': np.average(e, 0), 'std': np.std(e, 0)}


def _slab(traj, ref_nav, samples, ned, rng):
    with np.errstate(invalid='ignore', over='ignore'):
        e = errors(traj, ref_nav, samples, ned)
        want = array_stats(e)
        ext = array_stats(errors(traj, ref_nav, samples, ned, dtype=np.longdouble))
        E = {k: np.abs(want[k].astype(np.longdouble) - ext[k]).astype(np.float64) for k in want}
        S = {k: np.zeros_like(want[k]) for k in want}
        for _ in range(PERMUTATIONS):
            got = array_stats(e[rng.permutation(e.shape[0])])
            for k in want:
                S[k] = np.maximum(S[k], np.abs(got[k] - want[k]))
        eps = np.finfo(np.float64).eps
        tol = {k: FACTOR * np.maximum(np.maximum(E[k], S[k]), eps * np.abs(want[k])) for k in want}
    return want, tol, E, S


def curve(traj, ref_nav, samples=None, ned=False, seed=SEED):
    """The curve and its per-record bounds: dict(max, avg, std, tol_max, tol_avg, tol_std, E_*, S_*), arrays (m, 9).  A record
    that holds a non-finite value has NaN bounds: such records are compared by their masks."""
    traj = np.asarray(traj)
    ids = np.arange(traj.shape[1], dtype=np.int64) if samples is None else np.asarray(samples, dtype=np.int64).reshape(-1)
    rng = np.random.RandomState(seed)
    step = max(1, CHUNK // (9 * traj.shape[0]))
    out = {}
    for a in range(0, ids.size, step):
        want, tol, E, S = _slab(traj, ref_nav, ids[a:a + step], ned, rng)
        for k in want:
            out.setdefault(k, []).append(want[k])
            out.setdefault('tol_' + k, []).append(tol[k])
            out.setdefault('E_' + k, []).append(E[k])
            out.setdefault('S_' + k, []).append(S[k])
    return {k: np.concatenate(v, axis=0) for k, v in out.items()}
