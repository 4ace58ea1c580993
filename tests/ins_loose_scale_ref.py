"""NumPy restatement of InsLoose with the odometer's scale factor as a 16th state (csrc/ins_loose_scale.hip) on top of
tests/ins_loose_ref.py: the specification by example, vectorised over runs.  ScaleFilter carries the 16th state along LooseFilter's
two updates and its feedback, and forms the odometer's row; the blocks and the time loop are LooseFilter's and ins_loose_ref.run.

Everything of ins_loose_ref's convention holds for states 0-14.  State 15 is dk = k_est - k, k the true scale of the odometer,
odo_j = k v_b[0] + stdv z.  The 16 x 16 covariance is held as the 15 x 15 block P (exactly ins_loose_ref's array, so that every
operation on it is the 15-state filter's, bit for bit), the cross column c = P[0:15, 15] (R, 15) and pkk = P[15, 15] (R,).
  initial values   k_est = scale0, pkk = p0_scale^2, c = 0
  propagation      Phi is the identity on state 15 and couples it to nothing: P <- Phi15 P Phi15^T + Qd as ins_loose_ref,
                   c <- Phi15 c, pkk += q_k
  a GPS fix        six sequential scalar updates over 16 states (H = [I6 0]): col = column i of the 16 x 16 matrix
  the odometer     with D, v_b of the state before the first row:  z0 = v_b[0] - odo_j / k_est, the row of ins_loose_ref's aid on
                   states 3-8 and h[15] = v_b[0] / k_est; R0 = r_odo.  The constraint rows have h[15] = 0
  feedback         of states 0-14 as a GPS fix; k_est -= x[15]; at every block that ran a row
With p0_scale = 0 and q_k = 0, c and pkk stay 0, x[15] stays 0 and every output is the 15-state restatement's with
scale_f = scale0, exactly (tests/test_ins_loose_scale_oracle.py).
Every array carries `dtype` (np.float64 or np.longdouble)."""
import numpy as np

import ins_loose_ref as ref

NS = ref.NS             # the 15 states of the block P
NS16 = NS + 1


class ScaleFilter(ref.LooseFilter):
    def __init__(self, ref_frame, fs, ini, runs, model, scale, earth_rot=True, dtype=np.float64):
        """scale: {'scale0', 'p0_scale', 'q_k'} (ginsim.ins_loose.scale_model makes it)."""
        super().__init__(ref_frame, fs, ini, runs, model, earth_rot, dtype)
        self.k_est = np.full(self.R, dtype(scale['scale0']), dtype=dtype)
        self.c = np.zeros((self.R, NS), dtype=dtype)
        self.pkk = np.full(self.R, dtype(scale['p0_scale']) * dtype(scale['p0_scale']), dtype=dtype)
        self.q_k = dtype(scale['q_k'])
        self.xk = np.zeros(self.R, dtype=dtype)                     # x[15] of the block under way

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

    def update_state(self, i, z, rv):
        ck = self.c[:, i].copy()
        col, inv, g = super().update_state(i, z, rv)
        self.xk = self.xk + ck * g
        self.c = self.c - col * (ck * inv)[:, None]
        self.pkk = self.pkk - ck * ck * inv

    def update_row(self, lo, hi, h, z, rv, hk=None):
        P, c, pkk = self.P, self.c, self.pkk
        hl = np.zeros(self.R, dtype=self.dtype) if hk is None else hk
        ph = np.einsum('rkc,rc->rk', P[:, :, lo:hi], h) + c * hl[:, None]
        pk = np.einsum('rc,rc->r', c[:, lo:hi], h) + pkk * hl
        inv = 1 / (np.einsum('rc,rc->r', h, ph[:, lo:hi]) + hl * pk + rv)
        g = (z - (np.einsum('rc,rc->r', h, self.x[:, lo:hi]) + hl * self.xk)) * inv
        self.x = self.x + ph * g[:, None]
        self.xk = self.xk + pk * g
        self.P = P - ph[:, :, None] * ph[:, None, :] * inv[:, None, None]
        self.c = c - ph * (pk * inv)[:, None]
        self.pkk = pkk - pk * pk * inv

    def feedback(self):
        """LooseFilter's feedback of x[:, 0:15], and k_est -= x[:, 15].  Returns the fed-back x (R, 16)."""
        x, xk = super().feedback(), self.xk
        self.k_est = self.k_est - xk
        self.xk = np.zeros_like(xk)
        return np.concatenate([x, xk[:, None]], axis=1)

    def odo_row(self, vb0, odo_j, scale_f):
        """scale_f is not read: the filter divides by k_est, and h[15] = v_b[0] / k_est."""
        return vb0 - odo_j / self.k_est, vb0 / self.k_est


def run(ref_frame, fs, gyro, accel, ini, model, gps=None, stamps=(), visible=None, earth_rot=True, dtype=np.float64, odo=None, aid=None,
        scale=None, keep_pdiag=False):
    """ins_loose_ref.run on a ScaleFilter.  aid: as there, with bit 0 in its mask (odo_scale_f is not read); scale: {'scale0',
    'p0_scale', 'q_k'}.  Returns its dict (pdiag_end (R, 15), P_end (R, 16, 16)) and 'k_est' (R, n) of every stored row,
    'scale_end' (R, 2) = k_est and P[15][15] at the last sample, 'pcross_end' (R, 15) = P[0:15, 15].
    keep_pdiag: also 'pdiag' (R, n, 16), the diagonal of P at every stored row."""
    assert ref.aid_numbers(aid)[0] & 1, 'a scale-factor state without the odometer'
    R, n, _ = np.shape(gyro)
    f = ScaleFilter(ref_frame, fs, ini, R, model, scale, earth_rot, dtype)
    k_est, pkk = np.zeros((R, n), dtype=dtype), np.zeros((R, n, 1), dtype=dtype)

    def hook(f, j):
        k_est[:, j], pkk[:, j, 0] = f.k_est, f.pkk

    out = ref.run(ref_frame, fs, gyro, accel, ini, model, gps, stamps, visible, earth_rot, dtype, odo, aid, keep_pdiag=keep_pdiag, hook=hook,
                  filt=f)
    out['k_est'] = k_est
    if keep_pdiag:
        out['pdiag'] = np.concatenate([out['pdiag'], pkk], axis=2)
    out['scale_end'] = np.stack([f.k_est, f.pkk], axis=1)
    out['pcross_end'] = f.c.copy()
    out['P_end'] = f.full_p()
    return out
