"""NumPy restatement of InsLoose's standstill aiding, the zero-velocity update (ZUPT) and the zero-angular-rate update (ZARU)
(csrc/ins_loose_still.hip), on top of tests/ins_loose_aided_ref.py (imported, not edited): the specification by
example of the standstill block, vectorised over runs.

Everything of ins_loose_ref's convention holds (state order dr dv psi dbg dba, x = estimate - truth, C_est = (I - [psi x]) C).
  measurements     every row observes one state, H = e_I:
                     ZUPT (bit 0), I = 3, 4, 5:    z_i = vel_i, the reported navigation-frame velocity (the truth is 0); R = r_zupt
                     ZARU (bit 1), I = 9, 10, 11:  z_i = wb_i + w_rest_i - gyro_i, R = r_zaru[i]; gyro the RAW sample j - 1 (the last
                                                   one propagate() integrated), w_rest = D (W cos lat, 0, -W sin lat) with D = C_est^T
                                                   of the reported attitude and the reported latitude in ref_frame 0 with
                                                   earth_rot, zero otherwise; its dependence on psi is neglected in H
                   every z from the state before the first row
  one block        x = 0; for the selected rows in ascending state order  col = P[:, I], g = (z - x_I) / (P_II + R), x += col g,
                   P -= col col^T / (P_II + R) (the scalar update of a GPS fix);  then the feedback of a GPS fix, x = 0
  when             at every IMU sample j > 0 with j % every == 0 and flags[j] != 0, on the state row j reports: after a GPS
                   correction and after an odometer / non-holonomic block of the same sample, before the row is stored
Every array carries `dtype` (np.float64 or np.longdouble)."""
import numpy as np

import ins_loose_aided_ref as aref
import ins_loose_ref as ref
from oracle import ins_np

NS = ref.NS


class StillFilter(aref.AidedFilter):
    def rest_rate(self):
        """(R, 3): the body rate the mechanisation assumes of a body at rest (propagate() with v = 0)."""
        w = np.zeros((self.R, 3), dtype=self.dtype)
        if self.rf == 0 and self.earth_rot:
            _, _, _, sl, cl = ins_np.geo_param(self.pos[:, 0], self.pos[:, 2])
            w_ie = np.zeros((self.R, 3), dtype=self.dtype)
            w_ie[:, 0] = ins_np.W_IE * cl
            w_ie[:, 2] = -ins_np.W_IE * sl
            w = np.einsum('rij,rj->ri', self.D, w_ie)
        return w

    def still(self, gyro_prev, mask, r_zupt, r_zaru):
        """One standstill block.  gyro_prev (R, 3) the raw gyro samples j - 1; returns the fed-back x (R, 15)."""
        R, dtype = self.R, self.dtype
        r_zaru = np.asarray(r_zaru).astype(dtype)
        rows = []
        if mask & 1:
            rows += [(3 + i, self.vel[:, i], dtype(r_zupt)) for i in range(3)]
        if mask & 2:
            zg = self.wb + self.rest_rate() - np.asarray(gyro_prev).astype(dtype)
            rows += [(9 + i, zg[:, i], r_zaru[i]) for i in range(3)]
        if self.rf == 0:
            rm, rn, _, _, cl = ins_np.geo_param(self.pos[:, 0], self.pos[:, 2])
            mlat, mlon = rm + self.pos[:, 2], (rn + self.pos[:, 2]) * cl
        x = np.zeros((R, NS), dtype=dtype)
        P = self.P
        for i, z, rv in rows:
            col = P[:, :, i].copy()
            inv = 1 / (col[:, i] + rv)
            g = (z - x[:, i]) * inv
            x = x + col * g[:, None]
            P = P - col[:, :, None] * col[:, None, :] * inv[:, None, None]
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


def still_numbers(model):
    """(mask, every, r_zupt, r_zaru) of ginsim.ins_loose.still_model's output (or the same keys)."""
    return int(model['still_mask']), int(model['still_every']), float(model['r_zupt']), np.asarray(model['r_zaru'], dtype=np.float64)


def run(ref_frame, fs, gyro, accel, ini, model, gps=None, stamps=(), visible=None, earth_rot=True, dtype=np.float64, odo=None, aid=None,
        still=None, flags=None, keep_pdiag=False):
    """ins_loose_aided_ref.run with the standstill block.  still: {'still_mask', 'still_every', 'r_zupt', 'r_zaru'}
    (ginsim.ins_loose.still_model makes it) or None / mask 0: exactly ins_loose_aided_ref.run.  flags (n,): the standstill signal.
    keep_pdiag: also 'pdiag' (R, n, 15), the diagonal of P at every stored row."""
    gyro, accel = np.asarray(gyro).astype(dtype), np.asarray(accel).astype(dtype)
    R, n, _ = gyro.shape
    mask, every, scale_f, r_odo, r_nhc = aref.aid_numbers(aid) if aid is not None else (0, 1, 1.0, 1.0, 1.0)
    if mask & 1:
        odo = np.asarray(odo).astype(dtype)
    smask = 0
    if still is not None:
        smask, severy, r_zupt, r_zaru = still_numbers(still)
        flags = np.asarray(flags).reshape(n)
    f = StillFilter(ref_frame, fs, ini, R, model, earth_rot, dtype)
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
        if smask and j > 0 and j % severy == 0 and flags[j] != 0:
            f.still(gyro[:, j - 1], smask, r_zupt, r_zaru)
        out['att'][:, j], out['pos'][:, j], out['vel'][:, j], out['wb'][:, j], out['ab'][:, j] = f.att, f.pos, f.vel, f.wb, f.ab
        if keep_pdiag:
            out['pdiag'][:, j] = f.P[:, np.arange(NS), np.arange(NS)]
        if j == n - 1:
            break
        f.propagate(gyro[:, j], accel[:, j])
    out['pdiag_end'] = f.P[:, np.arange(NS), np.arange(NS)].copy()
    out['P_end'] = f.P
    return out
