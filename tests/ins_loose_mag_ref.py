"""NumPy restatement of InsLoose's magnetometer aiding (csrc/ins_loose_mag.hip) on top of
tests/ins_loose_aided_ref.py (imported, not edited): the specification by example of the heading block, vectorised over runs.

Everything of ins_loose_ref's convention holds (state order dr dv psi dbg dba, x = estimate - truth, C_est = (I - [psi x]) C).
  measurements     D = C_est^T (navigation -> body) of the reported attitude, m_n the field the filter assumes in the navigation
                   frame, m_cal = cal_si . mag_j - cal_hi the calibrated sample; to first order D_est m_n = m_b - D [m_n x] psi.
                   For body axis i = 0, 1, 2:  z_i = D[i,:] . m_n - m_cal[i],  R_i = r_mag[i],
                   h_i = [0 0 0, 0 0 0, m_n x D[i,:], 0 0 0, 0 0 0]; D, z and every h_i from the state before the first row
  one block        x = 0; for the three rows in ascending order  Ph = P h (the three columns 6-8 of P), s = h.Ph + R,
                   g = (z - h.x) / s, x += Ph g, P -= Ph Ph^T / s;  then the feedback of a GPS fix, x = 0
  when             at every IMU sample j > 0 with j % every == 0, on the state row j reports: after a GPS correction and after an
                   odometer / non-holonomic block of the same sample, before the row is stored
Every array carries `dtype` (np.float64 or np.longdouble)."""
import numpy as np

import ins_loose_aided_ref as aref
import ins_loose_ref as ref
from oracle import ins_np

NS = ref.NS


def mag_rows(D, m_n):
    """(R, 3, 3): row i is the psi part of h_i, m_n x D[i,:]."""
    return np.cross(np.broadcast_to(m_n, D.shape), D)


class MagFilter(aref.AidedFilter):
    def mag(self, mag_j, m_n, cal_si, cal_hi, r_mag):
        """One magnetometer block.  mag_j (R, 3) the raw samples; returns the fed-back x (R, 15)."""
        R, dtype = self.R, self.dtype
        m_n, cal_si, cal_hi, r_mag = (np.asarray(v).astype(dtype) for v in (m_n, cal_si, cal_hi, r_mag))
        D = self.D
        m_cal = np.einsum('ik,rk->ri', cal_si.reshape(3, 3), np.asarray(mag_j).astype(dtype)) - cal_hi
        z = np.einsum('rij,j->ri', D, m_n) - m_cal
        H = mag_rows(D, m_n)
        if self.rf == 0:
            rm, rn, _, _, cl = ins_np.geo_param(self.pos[:, 0], self.pos[:, 2])
            mlat, mlon = rm + self.pos[:, 2], (rn + self.pos[:, 2]) * cl
        x = np.zeros((R, NS), dtype=dtype)
        P = self.P
        for i in range(3):
            h = H[:, i]
            ph = np.einsum('rkc,rc->rk', P[:, :, 6:9], h)
            inv = 1 / (np.einsum('rc,rc->r', h, ph[:, 6:9]) + r_mag[i])
            g = (z[:, i] - np.einsum('rc,rc->r', h, x[:, 6:9])) * inv
            x = x + ph * g[:, None]
            P = P - ph[:, :, None] * ph[:, None, :] * inv[:, None, None]
        self.P = P
        # the feedback of LooseFilter.correct
        if self.rf == 0:
            self.pos = np.stack([self.pos[:, 0] - x[:, 0] / mlat, self.pos[:, 1] - x[:, 1] / mlon, self.pos[:, 2] + x[:, 2]], axis=1)
        else:
            self.pos = self.pos - x[:, 0:3]
        self.vel = self.vel - x[:, 3:6]
        C = np.swapaxes(self.D, 1, 2)
        Cn = C + np.einsum('rij,rjk->rik', ref.skew(x[:, 6:9]), C)
        d00, d01, d02, d12, d22 = Cn[:, 0, 0], Cn[:, 1, 0], Cn[:, 2, 0], Cn[:, 2, 1], Cn[:, 2, 2]
        self.att = np.stack([np.arctan2(d01, d00), np.arctan2(-d02, np.sqrt(d00 * d00 + d01 * d01)), np.arctan2(d12, d22)], axis=1)
        self.D = ref.dcm_zyx(self.att)
        if self.rf == 1:
            self.vel_b = np.einsum('rij,rj->ri', self.D, self.vel)
        self.wb = self.wb - x[:, 9:12]
        self.ab = self.ab - x[:, 12:15]
        return x


def mag_numbers(model):
    """(every, m_n, cal_si, cal_hi, r_mag) of ginsim.ins_loose.mag_model's output (or the same keys)."""
    return (int(model['mag_every']), np.asarray(model['mag_n']), np.asarray(model['cal_si']), np.asarray(model['cal_hi']),
            np.asarray(model['r_mag']))


def run(ref_frame, fs, gyro, accel, ini, model, gps=None, stamps=(), visible=None, earth_rot=True, dtype=np.float64, odo=None, aid=None,
        mag=None, mag_model=None, keep_pdiag=False):
    """ins_loose_aided_ref.run with the magnetometer block.  mag (R, n, 3) the raw magnetometer series; mag_model:
    {'mag_every', 'mag_n', 'cal_si', 'cal_hi', 'r_mag'} (ginsim.ins_loose.mag_model makes it) or None: exactly
    ins_loose_aided_ref.run.  keep_pdiag: also 'pdiag' (R, n, 15), the diagonal of P at every stored row."""
    gyro, accel = np.asarray(gyro).astype(dtype), np.asarray(accel).astype(dtype)
    R, n, _ = gyro.shape
    mask, every, scale_f, r_odo, r_nhc = aref.aid_numbers(aid) if aid is not None else (0, 1, 1.0, 1.0, 1.0)
    if mask & 1:
        odo = np.asarray(odo).astype(dtype)
    mevery = 0
    if mag_model is not None:
        mevery, m_n, cal_si, cal_hi, r_mag = mag_numbers(mag_model)
        mag = np.asarray(mag).astype(dtype)
    f = MagFilter(ref_frame, fs, ini, R, model, earth_rot, dtype)
    out = {k: np.zeros((R, n, 3), dtype=dtype) for k in ('att', 'pos', 'vel', 'wb', 'ab')}
    if keep_pdiag:
        out['pdiag'] = np.zeros((R, n, NS), dtype=dtype)
    stamps = [int(s) for s in stamps]
    gps = None if gps is None else np.asarray(gps).astype(dtype)
    kf = 0
    for j in range(n):
        if kf < len(stamps) and stamps[kf] == j:
            if visible is None or visible[kf] != 0:
                f.correct(gps[:, kf])
            kf += 1
        if mask and j > 0 and j % every == 0:
            f.aid(odo[:, j] if mask & 1 else None, mask, scale_f, r_odo, r_nhc)
        if mevery and j > 0 and j % mevery == 0:
            f.mag(mag[:, j], m_n, cal_si, cal_hi, r_mag)
        out['att'][:, j], out['pos'][:, j], out['vel'][:, j], out['wb'][:, j], out['ab'][:, j] = f.att, f.pos, f.vel, f.wb, f.ab
        if keep_pdiag:
            out['pdiag'][:, j] = f.P[:, np.arange(NS), np.arange(NS)]
        if j == n - 1:
            break
        f.propagate(gyro[:, j], accel[:, j])
    out['pdiag_end'] = f.P[:, np.arange(NS), np.arange(NS)].copy()
    out['P_end'] = f.P
    return out


def sample_mag(rng, ref_mag, mag_err, runs):
    """(R, n, 3) magnetometer series drawn from pathgen.mag_gen's model: (ref_mag + hi) . si^T + std * N(0, 1)."""
    ref_mag = np.asarray(ref_mag, dtype=np.float64)
    si, hi = np.asarray(mag_err['si'], dtype=np.float64).reshape(3, 3), np.asarray(mag_err['hi'], dtype=np.float64).reshape(3)
    std = np.asarray(mag_err['std'], dtype=np.float64) * np.ones(3)
    return ((ref_mag + hi) @ si.T)[None] + std * rng.standard_normal((runs,) + ref_mag.shape)
