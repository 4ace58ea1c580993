"""NumPy restatement of InsLoose's odometer / non-holonomic aiding (csrc/ins_loose_aided.hip) on top of
tests/ins_loose_ref.py (imported, not edited): the specification by example of the aiding block, vectorised over runs.

Everything of ins_loose_ref's convention holds (state order dr dv psi dbg dba, x = estimate - truth, C_est = (I - [psi x]) C).
  measurements     D = C_est^T (navigation -> body) of the reported attitude, v the reported navigation-frame velocity, v_b = D v;
                   to first order v_b,est = v_b + D dv - D [v x] psi.  Row i of the mask:
                     i = 0     z0 = v_b[0] - odo_j / scale_f, R0 = odo_std^2           (the odometer)
                     i = 1, 2  z_i = v_b[i] - 0,              R_i = nhc_std^2           (the non-holonomic constraints)
                   h_i = [0 0 0, D[i,:], -(D [v x])[i,:], 0 0 0, 0 0 0]; D, v, v_b and every h_i from the state before the first row
  one block        x = 0; for every selected row in ascending order  Ph = P h, s = h.Ph + R, g = (z - h.x) / s, x += Ph g,
                   P -= Ph Ph^T / s;  then the feedback of a GPS fix (pos, vel, attitude by atan2, vb in ref_frame 1, biases), x = 0
  when             at every IMU sample j > 0 with j % every == 0, on the state row j reports: after a GPS correction of the same
                   sample, before the row is stored
Every array carries `dtype` (np.float64 or np.longdouble)."""
import numpy as np

import ins_loose_ref as ref
from oracle import ins_np

NS = ref.NS


class AidedFilter(ref.LooseFilter):
    def aid(self, odo_j, mask, scale_f=1.0, r_odo=1.0, r_nhc=1.0):
        """One aiding block.  odo_j (R,) the odometer samples (read for mask bit 0 only); returns the fed-back x (R, 15)."""
        R, dtype = self.R, self.dtype
        D, v = self.D, self.vel
        vb = np.einsum('rij,rj->ri', D, v)
        H = np.zeros((R, 3, NS), dtype=dtype)
        H[:, :, 3:6] = D
        H[:, :, 6:9] = -np.einsum('rij,rjk->rik', D, ref.skew(v))
        z = vb.copy()
        if mask & 1:
            z[:, 0] = vb[:, 0] - np.asarray(odo_j).astype(dtype) / dtype(scale_f)
        rv = (dtype(r_odo), dtype(r_nhc), dtype(r_nhc))
        if self.rf == 0:
            rm, rn, _, _, cl = ins_np.geo_param(self.pos[:, 0], self.pos[:, 2])
            mlat, mlon = rm + self.pos[:, 2], (rn + self.pos[:, 2]) * cl
        x = np.zeros((R, NS), dtype=dtype)
        P = self.P
        for i in range(3):
            if not (mask >> i) & 1:
                continue
            h = H[:, i]
            ph = np.einsum('rkc,rc->rk', P[:, :, 3:9], h[:, 3:9])
            inv = 1 / (np.einsum('rc,rc->r', h[:, 3:9], ph[:, 3:9]) + rv[i])
            g = (z[:, i] - np.einsum('rc,rc->r', h[:, 3:9], x[:, 3:9])) * inv
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


def aid_numbers(aid):
    """(mask, every, scale_f, r_odo, r_nhc) of an `aid` dict: either ginsim.ins_loose.aiding_model's output or the same keys."""
    return int(aid['aid_mask']), int(aid['aid_every']), float(aid['odo_scale_f']), float(aid['r_odo']), float(aid['r_nhc'])


def run(ref_frame, fs, gyro, accel, ini, model, gps=None, stamps=(), visible=None, earth_rot=True, dtype=np.float64, odo=None, aid=None,
        keep_pdiag=False):
    """ins_loose_ref.run with the aiding block.  odo (R, n) the odometer series; aid: {'aid_mask', 'aid_every', 'odo_scale_f',
    'r_odo', 'r_nhc'} (ginsim.ins_loose.aiding_model makes it) or None / mask 0: exactly ins_loose_ref.run.
    keep_pdiag: also 'pdiag' (R, n, 15), the diagonal of P at every stored row."""
    gyro, accel = np.asarray(gyro).astype(dtype), np.asarray(accel).astype(dtype)
    R, n, _ = gyro.shape
    mask, every, scale_f, r_odo, r_nhc = aid_numbers(aid) if aid is not None else (0, 1, 1.0, 1.0, 1.0)
    if mask & 1:
        odo = np.asarray(odo).astype(dtype)
    f = AidedFilter(ref_frame, fs, ini, R, model, earth_rot, dtype)
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
        out['att'][:, j], out['pos'][:, j], out['vel'][:, j], out['wb'][:, j], out['ab'][:, j] = f.att, f.pos, f.vel, f.wb, f.ab
        if keep_pdiag:
            out['pdiag'][:, j] = f.P[:, np.arange(NS), np.arange(NS)]
        if j == n - 1:
            break
        f.propagate(gyro[:, j], accel[:, j])
    out['pdiag_end'] = f.P[:, np.arange(NS), np.arange(NS)].copy()
    out['P_end'] = f.P
    return out


def sample_odo(rng, ref_odo, odo_err, runs):
    """(R, n) odometer series drawn from pathgen.odo_gen's model: scale * ref_odo + stdv * N(0, 1)."""
    ref_odo = np.asarray(ref_odo, dtype=np.float64)
    return float(odo_err['scale']) * ref_odo[None] + float(odo_err['stdv']) * rng.standard_normal((runs, ref_odo.shape[0]))
