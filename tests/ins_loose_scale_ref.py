"""NumPy restatement of InsLoose with the odometer's scale factor as a 16th state (csrc/ins_loose_scale.hip) on top of
tests/ins_loose_ref.py and tests/ins_loose_aided_ref.py (imported, not edited): the specification by example, vectorised over runs.

Everything of ins_loose_ref's convention holds for states 0-14.  State 15 is dk = k_est - k, k the true scale of the odometer,
odo_j = k v_b[0] + stdv z.  The 16 x 16 covariance is held as the 15 x 15 block P (exactly ins_loose_ref's array, so that every
operation on it is the 15-state filter's, bit for bit), the cross column c = P[0:15, 15] (R, 15) and pkk = P[15, 15] (R,).
  initial values   k_est = scale0, pkk = p0_scale^2, c = 0
  propagation      Phi is the identity on state 15 and couples it to nothing: P <- Phi15 P Phi15^T + Qd as ins_loose_ref,
                   c <- Phi15 c, pkk += q_k
  a GPS fix        six sequential scalar updates over 16 states (H = [I6 0]): col = column i of the 16 x 16 matrix
  the odometer     with D, v_b of the state before the first row:  z0 = v_b[0] - odo_j / k_est, the row of ins_loose_aided_ref on
                   states 3-8 and h[15] = v_b[0] / k_est; R0 = r_odo.  The constraint rows have h[15] = 0
  feedback         of states 0-14 as a GPS fix; k_est -= x[15]; at every block that ran a row
With p0_scale = 0 and q_k = 0, c and pkk stay 0, x[15] stays 0 and every output is the 15-state aided restatement's with
scale_f = scale0, exactly (tests/test_ins_loose_scale_oracle.py).
Every array carries `dtype` (np.float64 or np.longdouble)."""
import numpy as np

import ins_loose_aided_ref as aref
import ins_loose_ref as ref
from oracle import ins_np

NS = ref.NS             # the 15 states of the block P
NS16 = NS + 1


class ScaleFilter(aref.AidedFilter):
    def __init__(self, ref_frame, fs, ini, runs, model, scale, earth_rot=True, dtype=np.float64):
        """scale: {'scale0', 'p0_scale', 'q_k'} (ginsim.ins_loose.scale_model makes it)."""
        super().__init__(ref_frame, fs, ini, runs, model, earth_rot, dtype)
        self.k_est = np.full(self.R, dtype(scale['scale0']), dtype=dtype)
        self.c = np.zeros((self.R, NS), dtype=dtype)
        self.pkk = np.full(self.R, dtype(scale['p0_scale']) * dtype(scale['p0_scale']), dtype=dtype)
        self.q_k = dtype(scale['q_k'])

    def full_p(self):
        """(R, 16, 16)."""
        P = np.zeros((self.R, NS16, NS16), dtype=self.dtype)
        P[:, :NS, :NS] = self.P
        P[:, :NS, NS] = self.c
        P[:, NS, :NS] = self.c
        P[:, NS, NS] = self.pkk
        return P

    def propagate(self, gyro, accel):
        # c <- Phi15 c with ins_loose_ref's Phi of the state before the step, written out by blocks
        dt, c = self.dt, self.c
        C = np.swapaxes(self.D, 1, 2)
        fn = np.einsum('rij,rj->ri', C, accel - self.ab)
        n = c.copy()
        n[:, 0:3] = c[:, 0:3] + c[:, 3:6] * dt
        n[:, 3:6] = c[:, 3:6] + np.einsum('rij,rj->ri', ref.skew(fn) * dt, c[:, 6:9]) + np.einsum('rij,rj->ri', -C * dt, c[:, 12:15])
        n[:, 6:9] = c[:, 6:9] + np.einsum('rij,rj->ri', C * dt, c[:, 9:12])
        n[:, 9:12] = self.m['decay_g'] * c[:, 9:12]
        n[:, 12:15] = self.m['decay_a'] * c[:, 12:15]
        self.c = n
        self.pkk = self.pkk + self.q_k
        super().propagate(gyro, accel)

    def _feedback(self, x, mlat, mlon):
        """LooseFilter.correct's feedback of x[:, 0:15], and k_est -= x[:, 15]."""
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
        self.k_est = self.k_est - x[:, NS]

    def _metres(self):
        if self.rf != 0:
            return None, None
        rm, rn, _, _, cl = ins_np.geo_param(self.pos[:, 0], self.pos[:, 2])
        return rm + self.pos[:, 2], (rn + self.pos[:, 2]) * cl

    def correct(self, fix):
        R, dtype = self.R, self.dtype
        z = np.empty((R, 6), dtype=dtype)
        mlat, mlon = self._metres()
        if self.rf == 0:
            z[:, 0] = (self.pos[:, 0] - fix[:, 0]) * mlat
            z[:, 1] = (self.pos[:, 1] - fix[:, 1]) * mlon
            z[:, 2] = -(self.pos[:, 2] - fix[:, 2])
        else:
            z[:, 0:3] = self.pos - fix[:, 0:3]
        z[:, 3:6] = self.vel - fix[:, 3:6]
        x = np.zeros((R, NS), dtype=dtype)
        xk = np.zeros(R, dtype=dtype)
        P, c, pkk = self.P, self.c, self.pkk
        for i in range(6):
            col, ck = P[:, :, i].copy(), c[:, i].copy()
            inv = 1 / (col[:, i] + self.m['r_diag'][i])
            g = (z[:, i] - x[:, i]) * inv
            x = x + col * g[:, None]
            xk = xk + ck * g
            P = P - col[:, :, None] * col[:, None, :] * inv[:, None, None]
            c = c - col * (ck * inv)[:, None]
            pkk = pkk - ck * ck * inv
        self.P, self.c, self.pkk = P, c, pkk
        x = np.concatenate([x, xk[:, None]], axis=1)
        self._feedback(x, mlat, mlon)
        return x

    def aid(self, odo_j, mask, scale_f=None, r_odo=1.0, r_nhc=1.0):
        """One aiding block; scale_f is not read (the filter divides by k_est).  Returns the fed-back x (R, 16)."""
        R, dtype = self.R, self.dtype
        D, v = self.D, self.vel
        vb = np.einsum('rij,rj->ri', D, v)
        H = np.zeros((R, 3, NS), dtype=dtype)
        H[:, :, 3:6] = D
        H[:, :, 6:9] = -np.einsum('rij,rjk->rik', D, ref.skew(v))
        hk = np.zeros((R, 3), dtype=dtype)
        z = vb.copy()
        if mask & 1:
            z[:, 0] = vb[:, 0] - np.asarray(odo_j).astype(dtype) / self.k_est
            hk[:, 0] = vb[:, 0] / self.k_est
        rv = (dtype(r_odo), dtype(r_nhc), dtype(r_nhc))
        mlat, mlon = self._metres()
        x = np.zeros((R, NS), dtype=dtype)
        xk = np.zeros(R, dtype=dtype)
        P, c, pkk = self.P, self.c, self.pkk
        for i in range(3):
            if not (mask >> i) & 1:
                continue
            h, hl = H[:, i], hk[:, i]
            ph = np.einsum('rkc,rc->rk', P[:, :, 3:9], h[:, 3:9]) + c * hl[:, None]
            pk = np.einsum('rc,rc->r', c[:, 3:9], h[:, 3:9]) + pkk * hl
            inv = 1 / (np.einsum('rc,rc->r', h[:, 3:9], ph[:, 3:9]) + hl * pk + rv[i])
            g = (z[:, i] - (np.einsum('rc,rc->r', h[:, 3:9], x[:, 3:9]) + hl * xk)) * inv
            x = x + ph * g[:, None]
            xk = xk + pk * g
            P = P - ph[:, :, None] * ph[:, None, :] * inv[:, None, None]
            c = c - ph * (pk * inv)[:, None]
            pkk = pkk - pk * pk * inv
        self.P, self.c, self.pkk = P, c, pkk
        x = np.concatenate([x, xk[:, None]], axis=1)
        self._feedback(x, mlat, mlon)
        return x


def run(ref_frame, fs, gyro, accel, ini, model, gps=None, stamps=(), visible=None, earth_rot=True, dtype=np.float64, odo=None, aid=None,
        scale=None, keep_pdiag=False):
    """ins_loose_aided_ref.run with the scale-factor state.  aid: as there, with bit 0 in its mask (odo_scale_f is not read);
    scale: {'scale0', 'p0_scale', 'q_k'}.  Returns its dict (pdiag_end (R, 15), P_end (R, 16, 16)) and 'k_est' (R, n) of every
    stored row, 'scale_end' (R, 2) = k_est and P[15][15] at the last sample, 'pcross_end' (R, 15) = P[0:15, 15].
    keep_pdiag: also 'pdiag' (R, n, 16), the diagonal of P at every stored row."""
    gyro, accel = np.asarray(gyro).astype(dtype), np.asarray(accel).astype(dtype)
    R, n, _ = gyro.shape
    mask, every, _, r_odo, r_nhc = aref.aid_numbers(aid)
    assert mask & 1, 'a scale-factor state without the odometer'
    odo = np.asarray(odo).astype(dtype)
    f = ScaleFilter(ref_frame, fs, ini, R, model, scale, earth_rot, dtype)
    out = {k: np.zeros((R, n, 3), dtype=dtype) for k in ('att', 'pos', 'vel', 'wb', 'ab')}
    out['k_est'] = np.zeros((R, n), dtype=dtype)
    if keep_pdiag:
        out['pdiag'] = np.zeros((R, n, NS16), dtype=dtype)
    stamps = [int(s) for s in stamps]
    gps = None if gps is None else np.asarray(gps).astype(dtype)
    kf = 0
    for j in range(n):
        if kf < len(stamps) and stamps[kf] == j:
            if visible is None or visible[kf] != 0:
                f.correct(gps[:, kf])
            kf += 1
        if j > 0 and j % every == 0:
            f.aid(odo[:, j], mask, None, r_odo, r_nhc)
        out['att'][:, j], out['pos'][:, j], out['vel'][:, j], out['wb'][:, j], out['ab'][:, j] = f.att, f.pos, f.vel, f.wb, f.ab
        out['k_est'][:, j] = f.k_est
        if keep_pdiag:
            out['pdiag'][:, j, :NS], out['pdiag'][:, j, NS] = f.P[:, np.arange(NS), np.arange(NS)], f.pkk
        if j == n - 1:
            break
        f.propagate(gyro[:, j], accel[:, j])
    out['pdiag_end'] = f.P[:, np.arange(NS), np.arange(NS)].copy()
    out['scale_end'] = np.stack([f.k_est, f.pkk], axis=1)
    out['pcross_end'] = f.c.copy()
    out['P_end'] = f.full_p()
    return out


def sample_odo(rng, ref_odo, scales, stdv):
    """(R, n) odometer series with a true scale of its own per run: scales[r] * ref_odo + stdv * N(0, 1)."""
    ref_odo = np.asarray(ref_odo, dtype=np.float64)
    scales = np.asarray(scales, dtype=np.float64)
    return scales[:, None] * ref_odo[None] + float(stdv) * rng.standard_normal((scales.shape[0], ref_odo.shape[0]))
