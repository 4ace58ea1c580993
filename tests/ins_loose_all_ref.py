"""NumPy restatement of InsLoose with all its aids in one launch (csrc/ins_loose_all.hip): nothing of its own.
tests/ins_loose_ref.py's run already composes the blocks in the kernel's order (fix, aiding, magnetometer, standstill, row) on the
filter it is given, and tests/ins_loose_scale_ref.py's ScaleFilter overrides the two updates and the feedback that LooseFilter.mag
and LooseFilter.still call.  This file only chooses the filter: a ScaleFilter with `scale`, a LooseFilter without.  Neither of the
two files is changed for it.

With 16 states every block's feedback also does k_est -= x[15] (ScaleFilter.feedback); the magnetometer rows (update_row on the
columns 6:9 with hk None) and the standstill rows (update_state) have h[15] = 0 and move k_est through the cross-covariance."""
import numpy as np

import ins_loose_ref as ref
import ins_loose_scale_ref as sref


def run(ref_frame, fs, gyro, accel, ini, model, gps=None, stamps=(), visible=None, earth_rot=True, dtype=np.float64, odo=None, aid=None,
        mag=None, mag_model=None, still=None, flags=None, scale=None, keep_pdiag=False):
    """ins_loose_ref.run with every block it takes, on a ScaleFilter when scale = {'scale0', 'p0_scale', 'q_k'} is given (aid then
    has bit 0 in its mask).  Returns its dict; with scale also 'k_est' (R, n), 'scale_end' (R, 2) = k_est and P[15][15] at the last
    sample, 'pcross_end' (R, 15) = P[0:15, 15] and P_end (R, 16, 16), as ins_loose_scale_ref.run; keep_pdiag then has 16 columns."""
    blocks = dict(odo=odo, aid=aid, mag=mag, mag_model=mag_model, still=still, flags=flags, keep_pdiag=keep_pdiag)
    if scale is None:
        return ref.run(ref_frame, fs, gyro, accel, ini, model, gps, stamps, visible, earth_rot, dtype, **blocks)
    assert ref.aid_numbers(aid)[0] & 1, 'a scale-factor state without the odometer'
    R, n, _ = np.shape(gyro)
    f = sref.ScaleFilter(ref_frame, fs, ini, R, model, scale, earth_rot, dtype)
    k_est, pkk = np.zeros((R, n), dtype=dtype), np.zeros((R, n, 1), dtype=dtype)

    def hook(f, j):
        k_est[:, j], pkk[:, j, 0] = f.k_est, f.pkk

    out = ref.run(ref_frame, fs, gyro, accel, ini, model, gps, stamps, visible, earth_rot, dtype, hook=hook, filt=f, **blocks)
    out['k_est'] = k_est
    if keep_pdiag:
        out['pdiag'] = np.concatenate([out['pdiag'], pkk], axis=2)
    out['scale_end'] = np.stack([f.k_est, f.pkk], axis=1)
    out['pcross_end'] = f.c.copy()
    out['P_end'] = f.full_p()
    return out
