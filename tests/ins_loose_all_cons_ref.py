"""NumPy restatement of the consistency checkpoints of InsLoose with any of its aids (csrc/ins_loose_all_cons.hip):
tests/ins_loose_cons_ref.py's record taken through the hook of tests/ins_loose_ref.py's run on the filter tests/ins_loose_all_ref.py
would choose: a ScaleFilter with a scale block, a LooseFilter without.  None of the three files is changed for it.

The checkpoint of sample j stands where ins_loose_ref.run calls its hook: after the fix, the odometer / constraint block, the
magnetometer block and the standstill block of that sample, before the row is stored.  The record keeps its 43 numbers and [0:37]
their meaning (ins_loose_cons_ref.lane_values on the 15 x 15 block P, which is exactly the 15-state filter's array).  With 16 states
  [37] the sum of P[15][15], [38] of (k_est - k_true)^2, [39] of (k_est - k_true)^2 / P[15][15], [40:43] zeros
k_true (R,) the true scale of every run, or None: [38] and [39] are then 0 and the scale error takes no part in a run's inclusion.
A run is included as ins_loose_cons_ref.record includes it and, with 16 states, only if P[15][15] > 0 and finite and, with a truth, both
quotients are finite.  With 15 states [37:43] are zeros: the record is ins_loose_cons_ref's.
Every array carries `dtype` (np.float64 or np.longdouble)."""
import numpy as np

import ins_loose_cons_ref as cref
import ins_loose_ref as ref
import ins_loose_scale_ref as sref

RECORD = cref.RECORD


def scale_values(f, k_true):
    """(R, 3) of a ScaleFilter at a checkpoint: P[15][15], (k_est - k_true)^2 and their quotient; the last two 0 without a truth.
    NaN in the first column where P[15][15] is not positive."""
    v = np.zeros((f.R, 3), dtype=f.dtype)
    v[:, 0] = f.pkk
    if k_true is not None:
        ek = f.k_est - np.asarray(k_true).astype(f.dtype)
        v[:, 1] = ek * ek
        with np.errstate(all='ignore'):
            v[:, 2] = v[:, 1] / f.pkk
    v[~(f.pkk > 0), 0] = np.nan
    return v


def record(f, t, k_true=None):
    """(RECORD,) of one checkpoint of the filter f (a LooseFilter or a ScaleFilter) against the truth row t."""
    v = cref.lane_values(f, t)
    if isinstance(f, sref.ScaleFilter):
        v = np.concatenate([v, scale_values(f, k_true)], axis=1)
    keep = np.all(np.isfinite(v), axis=1)
    out = np.zeros(RECORD, dtype=f.dtype)
    out[0] = np.count_nonzero(keep)
    out[1:1 + v.shape[1]] = v[keep].sum(axis=0)
    return out


def _quiet(base):
    class Quiet(base):
        """Runs the checkpoints exclude (a non-finite value) are inputs here: propagate() does not warn about them."""

        def propagate(self, gyro, accel):
            with np.errstate(all='ignore'):
                super().propagate(gyro, accel)
    return Quiet


def run(ref_frame, fs, gyro, accel, ini, model, ref_nav, checkpoints, gps=None, stamps=(), visible=None, earth_rot=True, dtype=np.float64,
        odo=None, aid=None, mag=None, mag_model=None, still=None, flags=None, scale=None, scale_truth=None, full=False):
    """ins_loose_ref.run with every block it takes, recording at the checkpoints and (unless full) ending after the last one.
    ref_nav (n, 9) = att3, pos3, vel3 of the truth; checkpoints in any order, repeats allowed; scale: {'scale0', 'p0_scale', 'q_k'} or
    None; scale_truth (R,), a scalar or None.  Returns (len(checkpoints), RECORD) sums in `dtype`, in the caller's order; with full
    (records, the dict of ins_loose_ref.run and the filter)."""
    asked = [int(s) for s in checkpoints]
    last = max(asked)
    got = {}
    R = np.shape(gyro)[0]
    if scale is None:
        f = _quiet(ref.LooseFilter)(ref_frame, fs, ini, R, model, earth_rot, dtype)
        assert scale_truth is None, 'a truth of the scale factor without the state'
    else:
        assert ref.aid_numbers(aid)[0] & 1, 'a scale-factor state without the odometer'
        f = _quiet(sref.ScaleFilter)(ref_frame, fs, ini, R, model, scale, earth_rot, dtype)
    k_true = None if scale_truth is None else np.broadcast_to(np.asarray(scale_truth, dtype=np.float64), (R,))

    def hook(f, j):
        if j in asked:
            got[j] = record(f, ref_nav[j], k_true)
        return j >= last and not full

    out = ref.run(ref_frame, fs, gyro, accel, ini, model, gps, stamps, visible, earth_rot, dtype, odo=odo, aid=aid, mag=mag,
                  mag_model=mag_model, still=still, flags=flags, hook=hook, filt=f)
    rec = np.stack([got[j] for j in asked])
    return (rec, out, f) if full else rec


def means(rec):
    """ins_loose_cons_ref.means and, of the scale state, 'pbar_scale', 'e2_scale', 'nes_scale' and 'ratio_scale' (m,) each."""
    rec = np.asarray(rec)
    out = cref.means(rec)
    m = rec / rec[:, 0:1]
    out['pbar_scale'], out['e2_scale'], out['nes_scale'] = m[:, 37], m[:, 38], m[:, 39]
    with np.errstate(all='ignore'):
        out['ratio_scale'] = np.sqrt(out['e2_scale']) / np.sqrt(out['pbar_scale'])
    return out


def deviation(a, b):
    """ins_loose_cons_ref.deviation over all 43 columns: per column, max over the checkpoints of |a - b| relative to the column's
    largest |b| over the case's checkpoints (the absolute difference where the column is zero in b)."""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    top = np.max(np.abs(b), axis=0)
    d = np.max(np.abs(a - b), axis=0)
    return np.array(np.where(top > 0, d / np.where(top > 0, top, 1), d), dtype=np.float64)
