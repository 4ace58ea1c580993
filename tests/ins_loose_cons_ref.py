"""NumPy restatement of InsLoose's consistency checkpoints (csrc/ins_loose_cons.hip) on top of tests/ins_loose_ref.py:
the specification by example of the record ginsim_loose_cons_run reduces, taken through the hook of ins_loose_ref.run.

A checkpoint is an IMU sample j of a list.  On the state that row j reports (after a GPS correction and an aiding block of the same
sample, before the row is stored) every run forms
  e[0:9]        the navigation part of ins_loose_ref.error_state against row j of ref_nav = (att3, pos3, vel3): dr in NED metres through
                the TRUTH's Rm + h and (Rn + h) cos(lat) in ref_frame 0, the plain difference in ref_frame 1; dv; psi from the
                antisymmetric part of I - C_est C^T
  the values    P_kk (15), e_k^2 (9), e_k^2 / P_kk (9), and for the blocks b = position, velocity, attitude e_b^T P_bb^-1 e_b by the
                explicit adjugate and determinant of the symmetric 3x3 block (np.linalg does not take np.longdouble)
  inclusion     a run with a non-finite value among them, a P_kk <= 0 or a block that is not positive definite (leading minors
                a, a d - b^2, det) contributes to nothing
and the record is the SUM over the included runs, RECORD = 43 numbers: [0] their count, [1:16] P_kk, [16:25] e_k^2, [25:34]
e_k^2 / P_kk, [34:37] the three block values, [37:43] reserved zeros.  The bias states carry P_kk only.
Every array carries `dtype` (np.float64 or np.longdouble)."""
import numpy as np

import ins_loose_ref as ref
from oracle import ins_np

NS = ref.NS
RECORD = 43
STATES = ['dr_x', 'dr_y', 'dr_z', 'dv_x', 'dv_y', 'dv_z', 'psi_x', 'psi_y', 'psi_z', 'dbg_x', 'dbg_y', 'dbg_z', 'dba_x', 'dba_y', 'dba_z']


def nav_error(f, t):
    """(R, 9) = dr, dv, psi of the filter state f (a LooseFilter) against the truth row t = (att3, pos3, vel3), in f's dtype."""
    dtype = f.dtype
    t = np.asarray(t).astype(dtype)
    e = np.zeros((f.R, 9), dtype=dtype)
    if f.rf == 0:
        rm, rn, _, _, cl = ins_np.geo_param(t[3:4], t[5:6])
        e[:, 0] = (f.pos[:, 0] - t[3]) * (rm[0] + t[5])
        e[:, 1] = (f.pos[:, 1] - t[4]) * (rn[0] + t[5]) * cl[0]
        e[:, 2] = -(f.pos[:, 2] - t[5])
    else:
        e[:, 0:3] = f.pos - t[3:6]
    e[:, 3:6] = f.vel - t[6:9]
    Ce = np.swapaxes(ref.dcm_zyx(f.att), 1, 2)                     # C_est, body -> navigation, of the reported angles
    Ct = ref.dcm_zyx(t[None, 0:3])[0].T
    M = np.einsum('rij,kj->rik', Ce, Ct)                            # C_est C^T; [psi x] = I - M
    e[:, 6] = (M[:, 1, 2] - M[:, 2, 1]) / 2
    e[:, 7] = (M[:, 2, 0] - M[:, 0, 2]) / 2
    e[:, 8] = (M[:, 0, 1] - M[:, 1, 0]) / 2
    return e


def block_nees(B, e):
    """e^T B^-1 e of symmetric 3x3 blocks B (R, 3, 3) by adjugate and determinant; NaN where B is not positive definite."""
    a, b, c, d, f, g = B[:, 0, 0], B[:, 0, 1], B[:, 0, 2], B[:, 1, 1], B[:, 1, 2], B[:, 2, 2]
    a00, a01, a02 = d * g - f * f, c * f - b * g, b * f - c * d
    a11, a12, a22 = a * g - c * c, b * c - a * f, a * d - b * b
    det = a * a00 + b * a01 + c * a02
    q = (e[:, 0] * e[:, 0] * a00 + e[:, 1] * e[:, 1] * a11 + e[:, 2] * e[:, 2] * a22) \
        + 2 * (e[:, 0] * e[:, 1] * a01 + e[:, 0] * e[:, 2] * a02 + e[:, 1] * e[:, 2] * a12)
    with np.errstate(all='ignore'):
        out = q / det
    out[~((a > 0) & (a22 > 0) & (det > 0))] = np.nan
    return out


def lane_values(f, t):
    """(R, 36): the values of every run at a checkpoint, in the record's order without the count."""
    e = nav_error(f, t)
    pd = f.P[:, np.arange(NS), np.arange(NS)]
    with np.errstate(all='ignore'):
        nes = e * e / pd[:, :9]
    nees = np.stack([block_nees(f.P[:, b:b + 3, b:b + 3], e[:, b:b + 3]) for b in (0, 3, 6)], axis=1)
    v = np.concatenate([pd, e * e, nes, nees], axis=1)
    v[~np.all(pd > 0, axis=1)] = np.nan
    return v


def record(f, t):
    """(RECORD,) of one checkpoint."""
    v = lane_values(f, t)
    keep = np.all(np.isfinite(v), axis=1)
    out = np.zeros(RECORD, dtype=f.dtype)
    out[0] = np.count_nonzero(keep)
    out[1:37] = v[keep].sum(axis=0)
    return out


class _Quiet(ref.LooseFilter):
    """Runs the checkpoints exclude (a non-finite value) are inputs here: propagate() does not warn about them."""

    def propagate(self, gyro, accel):
        with np.errstate(all='ignore'):
            super().propagate(gyro, accel)


def run(ref_frame, fs, gyro, accel, ini, model, ref_nav, cons_samples, gps=None, stamps=(), visible=None, earth_rot=True,
        dtype=np.float64, odo=None, aid=None):
    """ins_loose_ref.run, recording at the checkpoints and ending after the last one.  ref_nav (n, 9) = att3, pos3, vel3 of the truth;
    cons_samples in any order, repeats allowed.  Returns (len(cons_samples), RECORD) sums in `dtype`, in the caller's order."""
    asked = [int(s) for s in cons_samples]
    last = max(asked)
    got = {}

    def hook(f, j):
        if j in asked:
            got[j] = record(f, ref_nav[j])
        return j >= last

    ref.run(ref_frame, fs, gyro, accel, ini, model, gps, stamps, visible, earth_rot, dtype, odo, aid, hook=hook,
            filt=_Quiet(ref_frame, fs, ini, np.shape(gyro)[0], model, earth_rot, dtype))
    return np.stack([got[j] for j in asked])


def means(rec):
    """{'count' (m,), 'pbar' (m, 15), 'e2' (m, 9), 'nes' (m, 9), 'nees' (m, 3), 'ratio' (m, 9)} of (m, RECORD) sums."""
    rec = np.asarray(rec)
    m = rec / rec[:, 0:1]
    out = {'count': rec[:, 0], 'pbar': m[:, 1:16], 'e2': m[:, 16:25], 'nes': m[:, 25:34], 'nees': m[:, 34:37]}
    out['ratio'] = np.sqrt(out['e2']) / np.sqrt(out['pbar'][:, :9])
    return out


def deviation(a, b):
    """Per column of the record's used part [0:37], max over the checkpoints of |a - b| relative to the column's largest |b| over
    the case's checkpoints (0 where the column is zero in both)."""
    a, b = np.asarray(a, dtype=np.longdouble)[:, :37], np.asarray(b, dtype=np.longdouble)[:, :37]
    top = np.max(np.abs(b), axis=0)
    d = np.max(np.abs(a - b), axis=0)
    return np.array(np.where(top > 0, d / np.where(top > 0, top, 1), d), dtype=np.float64)
