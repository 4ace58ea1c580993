"""NumPy restatement of the reference's inclinometer plugins, vectorised over runs (test infrastructure: the product never
imports it).

    mahony(gyro, accel, dt, bias0, gains)  -> quat (R, n, 4), wb (R, n, 3), ab (R, n, 3), final bias (R, 3)
    tilt(accel)                            -> quat (R, n, 4)
    quat2euler(q)                          -> (..., 3) yaw, pitch, roll
    chain(gyro, accel, dt, bias0)          -> the runs of ONE MahonyFilter object one after the other (run r starts from run
                                              r-1's final gyro_bias), as InsAlgoMgr.run_algo drives it

demo_algorithms/inclinometer_mahony.py:74-151, inclinometer_acc.py:37-56, attitude.py:22-107, 294-342, 605-609, 665-743.
Every run of `mahony` starts from ITS OWN initial bias (bias0 (R, 3)) with q = (1, 0, 0, 0) and err_int = 0; the branches of the
reference are taken per run with np.where, operation by operation as the reference writes them.
"""
import numpy as np

GAINS = dict(kp_high=1.0, kp_low=0.01, ki_high=0.5, ki_low=0.001, innovation_limit=0.1)


def _norm3(x):
    return np.sqrt(x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1] + x[..., 2] * x[..., 2])


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def acc_mag_quat(acc, mag, with_branch=False):
    """dcm2quat(get_cn2b_acc_mag_ned(acc, mag)) for (R, 3) arrays; with_branch: also the dcm2quat branch taken (0-3) per row.

    Both callers (tilt with mag = (1, 0, 0), mahony with its pseudo-magnetometer) build a DCM of zero yaw: c00 = cos(pitch) >= 0
    (it is a square root), c11 = cos(roll), c22 = cos(pitch) cos(roll), so tr = c00 + c11 (1 + c00) <= 0 needs c11 <= 0 and then
    c00 is the largest diagonal element: through these callers only the first and the LAST branch are reachable (the census of
    tests/test_inclinometer_oracle.py counts them).  The two middle branches restate the reference and stay."""
    with np.errstate(invalid='ignore', divide='ignore'):
        z = -acc / _norm3(acc)[:, None]
        c = _cross(z, mag)
        y = c / _norm3(c)[:, None]
        x = _cross(y, z)
        c00, c10, c20 = x[:, 0], x[:, 1], x[:, 2]
        c01, c11, c21 = y[:, 0], y[:, 1], y[:, 2]
        c02, c12, c22 = z[:, 0], z[:, 1], z[:, 2]
        tr = c00 + c11 + c22
        t = np.zeros((acc.shape[0], 4))
        b0 = tr > 0.0
        b1 = ~b0 & (c11 > c00) & (c11 > c22)
        b2 = ~b0 & ~b1 & (c22 > c00)
        b3 = ~b0 & ~b1 & ~b2
        h = 0.5 * np.sqrt(1.0 + tr)
        t0 = np.stack([h, 0.25 / h * (c12 - c21), 0.25 / h * (c20 - c02), 0.25 / h * (c01 - c10)], 1)
        s1 = np.sqrt(c11 - c00 - c22 + 1.0)
        f1 = np.where(s1 != 0.0, 0.5 / s1, s1)
        t1 = np.stack([(c20 - c02) * f1, (c01 + c10) * f1, 0.5 * s1, (c12 + c21) * f1], 1)
        s2 = np.sqrt(c22 - c00 - c11 + 1.0)
        f2 = np.where(s2 != 0.0, 0.5 / s2, s2)
        t2 = np.stack([(c01 - c10) * f2, (c20 + c02) * f2, (c12 + c21) * f2, 0.5 * s2], 1)
        s3 = np.sqrt(c00 - c11 - c22 + 1.0)
        f3 = np.where(s3 != 0.0, 0.5 / s3, s3)
        t3 = np.stack([(c12 - c21) * f3, 0.5 * s3, (c01 + c10) * f3, (c20 + c02) * f3], 1)
        for m, v in ((b0, t0), (b1, t1), (b2, t2), (b3, t3)):
            t[m] = v[m]
    out = np.where((t[:, 0] < 0)[:, None], -1.0 * t, t)
    if with_branch:
        return out, np.select([b0, b1, b2], [0, 1, 2], 3)
    return out


def quat2euler(q):
    q0, q1, q2, q3 = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    with np.errstate(invalid='ignore'):
        return np.stack([np.arctan2(2.0 * (q1 * q2 + q0 * q3), q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3),
                         np.arcsin(-2.0 * (q1 * q3 - q0 * q2)),
                         np.arctan2(2.0 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3)], axis=-1)


def tilt(accel, with_branch=False):
    accel = np.asarray(accel, dtype=np.float64)
    R, n, _ = accel.shape
    mag = np.array([1.0, 0.0, 0.0])
    out = [acc_mag_quat(accel[:, j], mag, True) for j in range(n)]
    q = np.stack([o[0] for o in out], axis=1)
    return (q, np.stack([o[1] for o in out], axis=1)) if with_branch else q


def mahony(gyro, accel, dt, bias0, gains=None, trace=None):
    """trace: a dict that receives, per run and sample, which way each branch went: 'low' (the low gains), 'limited' (the
    innovation was limited), 'cneg' (cos(theta / 2) < 0), 'theta0' (theta == 0), 'postponed' (no initialisation yet after this
    sample: a zero accelerometer so far), and per run 'ini_branch' (the dcm2quat branch of the initialisation, -1: never)."""
    g = dict(GAINS, **(gains or {}))
    gyro, accel = np.asarray(gyro, dtype=np.float64), np.asarray(accel, dtype=np.float64)
    R, n, _ = accel.shape
    q = np.tile([1.0, 0.0, 0.0, 0.0], (R, 1))
    ei = np.zeros((R, 3))
    b = np.array(bias0, dtype=np.float64).reshape(R, 3).copy()
    ini = np.zeros(R, dtype=bool)
    Q, WB, AB = np.empty((R, n, 4)), np.empty((R, n, 3)), np.empty((R, n, 3))
    k, k1 = 0.9, 1 - 0.9
    if trace is not None:
        trace.update({nm: np.zeros((R, n), dtype=bool) for nm in ('low', 'limited', 'cneg', 'theta0', 'postponed')})
        trace['ini_branch'] = np.full(R, -1)
    for j in range(n):
        a, w = accel[:, j].copy(), gyro[:, j]
        valid = np.any(a != 0.0, axis=1)
        an = _norm3(a)
        low = (np.abs(an - 9.8) > 0.2) | (_norm3(w) > 0.2)
        kp = np.where(low, g['kp_low'], g['kp_high'])[:, None]
        ki = np.where(low, g['ki_low'], g['ki_high'])[:, None]
        with np.errstate(invalid='ignore', divide='ignore'):
            a = np.where(valid[:, None], a / an[:, None], a)
        start = valid & ~ini
        if np.any(start):
            ini = ini | start
            ei[start] = 0.0
            s = a[start]
            with np.errstate(invalid='ignore', divide='ignore'):
                m0 = np.sqrt(1.0 - s[:, 0] * s[:, 0])
                pm = np.stack([m0, -s[:, 1] * s[:, 0] / m0, -s[:, 0] * s[:, 2] / m0], 1)
            pm[s[:, 0] >= 1.0] = [0.0, 0.0, 1.0]
            pm[(s[:, 0] < 1.0) & (s[:, 1] <= -1.0)] = [0.0, 0.0, -1.0]
            q[start], br = acc_mag_quat(s, pm, True)
            if trace is not None:
                trace['ini_branch'][start] = br
        v = np.stack([-2.0 * (q[:, 1] * q[:, 3] - q[:, 0] * q[:, 2]),
                      -2.0 * (q[:, 0] * q[:, 1] + q[:, 2] * q[:, 3]),
                      -q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] - q[:, 3] * q[:, 3]], 1)
        e = _cross(a, v)
        en = _norm3(e)
        lim = en > g['innovation_limit']
        with np.errstate(invalid='ignore', divide='ignore'):
            e = np.where(lim[:, None], e / en[:, None] * g['innovation_limit'], e)
        ei = ei + ki * e * dt
        b = k * b + k1 * (kp * e + ei)
        rv = (w + b) * dt
        th = _norm3(rv)
        h = 0.5 * th
        s, c = np.sin(h), np.cos(h)
        with np.errstate(invalid='ignore', divide='ignore'):
            tt = np.where(c >= 0, s / th, -s / th)
        r = np.stack([np.where(c >= 0, c, -c), tt * rv[:, 0], tt * rv[:, 1], tt * rv[:, 2]], 1)
        r[th == 0.0] = [1.0, 0.0, 0.0, 0.0]
        p = np.stack([q[:, 0] * r[:, 0] - q[:, 1] * r[:, 1] - q[:, 2] * r[:, 2] - q[:, 3] * r[:, 3],
                      q[:, 0] * r[:, 1] + q[:, 1] * r[:, 0] + q[:, 2] * r[:, 3] - q[:, 3] * r[:, 2],
                      q[:, 0] * r[:, 2] - q[:, 1] * r[:, 3] + q[:, 2] * r[:, 0] + q[:, 3] * r[:, 1],
                      q[:, 0] * r[:, 3] + q[:, 1] * r[:, 2] - q[:, 2] * r[:, 1] + q[:, 3] * r[:, 0]], 1)
        p = np.where((p[:, 0] < 0)[:, None], -p, p)
        q = p / np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2] + p[:, 3] * p[:, 3])[:, None]
        Q[:, j], WB[:, j], AB[:, j] = q, b, e
        if trace is not None:
            trace['low'][:, j], trace['limited'][:, j], trace['cneg'][:, j] = low, lim, c < 0
            trace['theta0'][:, j], trace['postponed'][:, j] = th == 0.0, ~ini
    return Q, WB, AB, b.copy()


def chain(gyro, accel, dt, bias0=(0.0, 0.0, 0.0), gains=None):
    """The runs of one object in sequence: (quat, wb, ab, initial biases (R, 3), final bias of the last run)."""
    R = np.asarray(accel).shape[0]
    outs, starts = [], []
    b = np.array(bias0, dtype=np.float64).reshape(1, 3)
    for r in range(R):
        starts.append(b[0].copy())
        o = mahony(gyro[r:r + 1], accel[r:r + 1], dt, b, gains)
        outs.append(o)
        b = o[3]
    return (np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs]), np.concatenate([o[2] for o in outs]),
            np.array(starts), b[0].copy())


def angle_range_pi(x):
    """attitude.angle_range_pi (attitude.py:799-812): x % 2 pi, minus 2 pi where that exceeds pi -- -pi, +pi, +-3 pi give +pi."""
    x = np.mod(x, 2.0 * np.pi)
    return np.where(x > np.pi, x - 2.0 * np.pi, x)


def angle_err(x, ref):
    return angle_range_pi(x - ref)


def stats(euler, ref_att, first=0):
    """end (R, 3) and process statistics (R, 3, 3) = max|e|, mean, std over samples >= first of the att_euler error."""
    e = angle_err(euler, ref_att[None])
    w = e[:, first:]
    return e[:, -1], np.stack([np.max(np.abs(w), 1), np.mean(w, 1), np.std(w, 1)], 1)
