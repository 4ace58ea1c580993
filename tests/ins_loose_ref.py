"""NumPy restatement of the loosely coupled GPS/INS filter and of its optional blocks (csrc/ins_loose.hpp and the family files
ins_loose.hip, ins_loose_aided.hip, ins_loose_mag.hip, ins_loose_still.hip), vectorised over
runs: batched einsum, one Python loop over time.  The reference declares InsLoose's interface only (demo_algorithms/ins_loose.py:
prediction and correction are `pass`), so this file IS the specification by example; the device kernels are held to it and it is
held to oracle/ins_np.py's free integration (a filter without a usable fix is free integration) and to the statistics of its own
covariance.  tests/ins_loose_scale_ref.py adds the 16th state, tests/ins_loose_cons_ref.py the consistency checkpoints.

Convention (one consistent set):
  error state x = estimate - truth, order dr(0-2) dv(3-5) psi(6-8) dbg(9-11) dba(12-14)
  dr: NED metres (ref_frame 0) or the virtual-inertial axes (ref_frame 1); psi: C_est = (I - [psi x]) C, C = body -> navigation
  per IMU sample   P <- Phi P Phi^T + Qd,  Phi = I + F dt,  F blocks (r,v) = I, (v,psi) = [f^n x], (v,ba) = -C, (psi,bg) = C,
                   (bg,bg) = -1/tau_g, (ba,ba) = -1/tau_a  [decay = 1 - dt/tau on the diagonal of Phi]; f^n = C (accel - ab)
                   Qd = blockdiag(0, C diag(q_v) C^T, C diag(q_psi) C^T, diag(q_bg), diag(q_ba))
  mechanisation    oracle/ins_np.free_integration's step on accel - ab, gyro - wb
Every block works on the state that IMU sample j's row reports, before the row is stored, in this order; each forms all its z, h
and R from the state before its first row, runs its rows as sequential scalar updates on x (0 at the block's start), and ends in
the feedback (pos, vel -= dr, dv; C <- (I + [psi x]) C_est, Euler angles from its rows by atan2; vel_b in ref_frame 1; wb, ab
-= dbg, dba) and x = 0.  The two updates (the names mirror CovT::update and CovT::update_row on the device):
  update_state     a row that observes state I, H = e_I:  col = P[:, I], g = (z - x_I) / (P_II + R), x += col g, P -= col col^T / (P_II + R)
  update_row       a row h on the columns lo:hi:  Ph = P h, s = h.Ph + R, g = (z - h.x) / s, x += Ph g, P -= Ph Ph^T / s
  correct          fix k at sample stamp[k], when visible[k] != 0: z = ins - gps (LLA difference -> NED metres with (Rm + h),
                   (Rn + h) cos(lat) in ref_frame 0), H = [I6 0], R = r_diag: update_state of the states 0-5
  aid              at j > 0 with j % every == 0.  D = C_est^T (navigation -> body) of the reported attitude, v the reported
                   navigation-frame velocity, v_b = D v; to first order v_b,est = v_b + D dv - D [v x] psi.  Row i of the mask:
                     i = 0     z0 = v_b[0] - odo_j / scale_f, R0 = odo_std^2           (the odometer)
                     i = 1, 2  z_i = v_b[i] - 0,              R_i = nhc_std^2           (the non-holonomic constraints)
                   h_i = [0 0 0, D[i,:], -(D [v x])[i,:], 0 0 0, 0 0 0]: update_row on the columns 3:9, ascending
  mag              at j > 0 with j % every == 0.  m_n the field the filter assumes in the navigation frame, m_cal = cal_si . mag_j
                   - cal_hi the calibrated sample; to first order D_est m_n = m_b - D [m_n x] psi.  For body axis i = 0, 1, 2:
                   z_i = D[i,:] . m_n - m_cal[i], R_i = r_mag[i], h_i = m_n x D[i,:] on psi: update_row on the columns 6:9
  still            at j > 0 with j % every == 0 and flags[j] != 0: update_state of
                     ZUPT (bit 0), I = 3, 4, 5:    z_i = vel_i, the reported navigation-frame velocity (the truth is 0); R = r_zupt
                     ZARU (bit 1), I = 9, 10, 11:  z_i = wb_i + w_rest_i - gyro_i, R = r_zaru[i]; gyro the RAW sample j - 1 (the last
                                                   one propagate() integrated), w_rest = D (W cos lat, 0, -W sin lat) of the reported
                                                   attitude and latitude in ref_frame 0 with earth_rot, zero otherwise; its
                                                   dependence on psi is neglected in H
Every array carries `dtype` (np.float64 or np.longdouble)."""
import math

import numpy as np

from oracle import ins_np

NS = 15


def dcm_zyx(att):
    """ins_np.dcm_zyx (n -> b) keeping the dtype of att (R, 3) -> (R, 3, 3)."""
    c, s = np.cos(att), np.sin(att)
    cy, cp, cr = c[..., 0], c[..., 1], c[..., 2]
    sy, sp, sr = s[..., 0], s[..., 1], s[..., 2]
    m = np.empty(att.shape[:-1] + (3, 3), dtype=att.dtype)
    m[..., 0, 0] = cp * cy
    m[..., 0, 1] = cp * sy
    m[..., 0, 2] = -sp
    m[..., 1, 0] = sr * sp * cy - cr * sy
    m[..., 1, 1] = sr * sp * sy + cr * cy
    m[..., 1, 2] = cp * sr
    m[..., 2, 0] = sp * cr * cy + sy * sr
    m[..., 2, 1] = sp * cr * sy - cy * sr
    m[..., 2, 2] = cp * cr
    return m


def skew(v):
    """[v x] of (R, 3) -> (R, 3, 3)."""
    z = np.zeros(v.shape[0], dtype=v.dtype)
    return np.stack([np.stack([z, -v[:, 2], v[:, 1]], 1), np.stack([v[:, 2], z, -v[:, 0]], 1), np.stack([-v[:, 1], v[:, 0], z], 1)], 1)


class LooseFilter(object):
    """State of R runs; step-by-step so that tests can look inside.  ini: (9|10,) or (9|10, R) as FreeIntegration takes it."""

    def __init__(self, ref_frame, fs, ini, runs, model, earth_rot=True, dtype=np.float64):
        self.rf, self.dt, self.R, self.dtype, self.earth_rot = int(ref_frame), dtype(1.0) / dtype(fs), int(runs), dtype, bool(earth_rot)
        ini = np.asarray(ini, dtype=np.float64)
        if ini.ndim == 1:
            ini = np.repeat(ini[:, None], runs, axis=1)
        ini = ini.astype(dtype)
        R = self.R
        self.att = ini[6:9].T.copy()
        self.vel_b = ini[3:6].T.copy()
        self.D = dcm_zyx(self.att)                                  # n -> b
        self.vel = np.einsum('rji,rj->ri', self.D, self.vel_b)
        r0 = ini[0:3].T.copy()
        self.g_ext = ini[9].copy() if ini.shape[0] > 9 else None
        if self.rf == 1:
            self.pos = ins_np.lla2ecef(r0.astype(np.float64)).astype(dtype) if dtype is np.float64 else _lla2ecef(r0)
            self.g = ins_np.geo_param(r0[:, 0], r0[:, 2])[2] if self.g_ext is None else self.g_ext
        else:
            self.pos = r0
        self.wb = np.zeros((R, 3), dtype=dtype)
        self.ab = np.zeros((R, 3), dtype=dtype)
        self.m = {k: np.asarray(v, dtype=np.float64).astype(dtype) for k, v in model.items()}
        self.P = np.zeros((R, NS, NS), dtype=dtype)
        p0 = np.repeat(self.m['p0'], 3)
        self.P[:, np.arange(NS), np.arange(NS)] = p0 * p0
        self.x = np.zeros((R, NS), dtype=dtype)                     # the error state a block accumulates; feedback() zeroes it

    # ------------------------------------------------------------------ one IMU sample
    def propagate(self, gyro, accel):
        """Sample j -> j + 1 with the raw sensor samples (R, 3): covariance first (from the attitude before the step), then the
        mechanisation of ins_np.free_integration on the bias-corrected samples."""
        dt, R, dtype = self.dt, self.R, self.dtype
        w = gyro - self.wb
        f = accel - self.ab
        C = np.swapaxes(self.D, 1, 2)                               # b -> n
        fn = np.einsum('rij,rj->ri', C, f)
        Phi = np.zeros((R, NS, NS), dtype=dtype)
        Phi[:] = np.eye(NS, dtype=dtype)
        Phi[:, 0:3, 3:6] += np.eye(3, dtype=dtype) * dt
        Phi[:, 3:6, 6:9] += skew(fn) * dt
        Phi[:, 3:6, 12:15] += -C * dt
        Phi[:, 6:9, 9:12] += C * dt
        Phi[:, np.arange(9, 12), np.arange(9, 12)] = self.m['decay_g']
        Phi[:, np.arange(12, 15), np.arange(12, 15)] = self.m['decay_a']
        Q = np.zeros((R, NS, NS), dtype=dtype)
        Q[:, 3:6, 3:6] = np.einsum('rij,j,rkj->rik', C, self.m['q_v'], C)
        Q[:, 6:9, 6:9] = np.einsum('rij,j,rkj->rik', C, self.m['q_psi'], C)
        Q[:, np.arange(9, 12), np.arange(9, 12)] = self.m['q_bg']
        Q[:, np.arange(12, 15), np.arange(12, 15)] = self.m['q_ba']
        self.P = np.matmul(np.matmul(Phi, self.P), np.swapaxes(Phi, 1, 2)) + Q
        # mechanisation: ins_np.free_integration's loop body
        if self.rf == 1:
            att = ins_np.euler_step_zyx(self.att, w, dt)
            cg = self.D[:, :, 2] * self.g[:, None]
            self.vel_b = self.vel_b + (f + cg) * dt - ins_np.cross(w, self.vel_b) * dt
            self.D = dcm_zyx(att)
            vel = np.einsum('rji,rj->ri', self.D, self.vel_b)
            self.pos = self.pos + self.vel * dt
            self.att, self.vel = att, vel
        else:
            p, v = self.pos, self.vel
            rm, rn, g, sl, cl = ins_np.geo_param(p[:, 0], p[:, 2])
            rm_e, rn_e = rm + p[:, 2], rn + p[:, 2]
            if self.g_ext is not None:
                g = self.g_ext
            w_en = np.stack([v[:, 1] / rn_e, -v[:, 0] / rm_e, -v[:, 1] * sl / cl / rn_e], axis=1)
            w_ie = np.zeros((R, 3), dtype=dtype)
            if self.earth_rot:
                w_ie[:, 0] = ins_np.W_IE * cl
                w_ie[:, 2] = -ins_np.W_IE * sl
            w_nb_b = w - np.einsum('rij,rj->ri', self.D, w_en + w_ie)
            att = ins_np.euler_step_zyx(self.att, w_nb_b, dt)
            gn = np.zeros((R, 3), dtype=dtype)
            gn[:, 2] = g
            vdot = np.einsum('rji,rj->ri', self.D, f) + gn - ins_np.cross(2 * w_ie + w_en, v)
            pos = np.stack([p[:, 0] + v[:, 0] / rm_e * dt, p[:, 1] + v[:, 1] / rn_e / cl * dt, p[:, 2] + (-v[:, 2]) * dt], axis=1)
            self.vel = v + vdot * dt
            self.pos, self.att = pos, att
            self.D = dcm_zyx(att)

    # ------------------------------------------------------------------ the two updates and the feedback
    def metres(self):
        """Metres per radian of latitude and of longitude at the reported position; (None, None) in ref_frame 1."""
        if self.rf != 0:
            return None, None
        rm, rn, _, _, cl = ins_np.geo_param(self.pos[:, 0], self.pos[:, 2])
        return rm + self.pos[:, 2], (rn + self.pos[:, 2]) * cl

    def update_state(self, i, z, rv):
        """The row that observes state i.  Returns (col, inv, g): column i of P before the update, 1 / s and the gain's factor."""
        col = self.P[:, :, i].copy()
        inv = 1 / (col[:, i] + rv)
        g = (z - self.x[:, i]) * inv
        self.x = self.x + col * g[:, None]
        self.P = self.P - col[:, :, None] * col[:, None, :] * inv[:, None, None]
        return col, inv, g

    def update_row(self, lo, hi, h, z, rv, hk=None):
        """The row h (R, hi - lo) on the columns lo:hi.  hk: the row's entry on a 16th state, which ScaleFilter alone has."""
        assert hk is None
        ph = np.einsum('rkc,rc->rk', self.P[:, :, lo:hi], h)
        inv = 1 / (np.einsum('rc,rc->r', h, ph[:, lo:hi]) + rv)
        g = (z - np.einsum('rc,rc->r', h, self.x[:, lo:hi])) * inv
        self.x = self.x + ph * g[:, None]
        self.P = self.P - ph[:, :, None] * ph[:, None, :] * inv[:, None, None]

    def feedback(self):
        """Applies x to the navigation state and the biases, zeroes it and returns what it was (R, 15)."""
        x, self.x = self.x, np.zeros_like(self.x)
        mlat, mlon = self.metres()
        if self.rf == 0:
            self.pos = np.stack([self.pos[:, 0] - x[:, 0] / mlat, self.pos[:, 1] - x[:, 1] / mlon, self.pos[:, 2] + x[:, 2]], axis=1)
        else:
            self.pos = self.pos - x[:, 0:3]
        self.vel = self.vel - x[:, 3:6]
        C = np.swapaxes(self.D, 1, 2)
        Cn = C + np.einsum('rij,rjk->rik', skew(x[:, 6:9]), C)      # (I + [psi x]) C_est
        d00, d01, d02, d12, d22 = Cn[:, 0, 0], Cn[:, 1, 0], Cn[:, 2, 0], Cn[:, 2, 1], Cn[:, 2, 2]
        self.att = np.stack([np.arctan2(d01, d00), np.arctan2(-d02, np.sqrt(d00 * d00 + d01 * d01)), np.arctan2(d12, d22)], axis=1)
        self.D = dcm_zyx(self.att)
        if self.rf == 1:
            self.vel_b = np.einsum('rij,rj->ri', self.D, self.vel)
        self.wb = self.wb - x[:, 9:12]
        self.ab = self.ab - x[:, 12:15]
        return x

    # ------------------------------------------------------------------ the blocks; each returns the fed-back x
    def correct(self, fix):
        """fix (R, 6) = pos3, vel3 in the units of the state."""
        z = np.empty((self.R, 6), dtype=self.dtype)
        if self.rf == 0:
            mlat, mlon = self.metres()
            z[:, 0] = (self.pos[:, 0] - fix[:, 0]) * mlat
            z[:, 1] = (self.pos[:, 1] - fix[:, 1]) * mlon
            z[:, 2] = -(self.pos[:, 2] - fix[:, 2])
        else:
            z[:, 0:3] = self.pos - fix[:, 0:3]
        z[:, 3:6] = self.vel - fix[:, 3:6]
        for i in range(6):
            self.update_state(i, z[:, i], self.m['r_diag'][i])
        return self.feedback()

    def odo_row(self, vb0, odo_j, scale_f):
        """(z, hk) of the odometer's row: its innovation and its entry on a 16th state (None: there is none)."""
        return vb0 - odo_j / self.dtype(scale_f), None

    def aid(self, odo_j, mask, scale_f=1.0, r_odo=1.0, r_nhc=1.0):
        """One aiding block.  odo_j (R,) the odometer samples (read for mask bit 0 only)."""
        R, dtype = self.R, self.dtype
        D, v = self.D, self.vel
        vb = np.einsum('rij,rj->ri', D, v)
        H = np.zeros((R, 3, NS), dtype=dtype)
        H[:, :, 3:6] = D
        H[:, :, 6:9] = -np.einsum('rij,rjk->rik', D, skew(v))
        z, hk = vb.copy(), None
        if mask & 1:
            z[:, 0], hk = self.odo_row(vb[:, 0], np.asarray(odo_j).astype(dtype), scale_f)
        rv = (dtype(r_odo), dtype(r_nhc), dtype(r_nhc))
        for i in range(3):
            if (mask >> i) & 1:
                self.update_row(3, 9, H[:, i, 3:9], z[:, i], rv[i], hk if i == 0 else None)
        return self.feedback()

    def mag(self, mag_j, m_n, cal_si, cal_hi, r_mag):
        """One magnetometer block.  mag_j (R, 3) the raw samples."""
        dtype = self.dtype
        m_n, cal_si, cal_hi, r_mag = (np.asarray(v).astype(dtype) for v in (m_n, cal_si, cal_hi, r_mag))
        D = self.D
        m_cal = np.einsum('ik,rk->ri', cal_si.reshape(3, 3), np.asarray(mag_j).astype(dtype)) - cal_hi
        z = np.einsum('rij,j->ri', D, m_n) - m_cal
        H = mag_rows(D, m_n)
        for i in range(3):
            self.update_row(6, 9, H[:, i], z[:, i], r_mag[i])
        return self.feedback()

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
        """One standstill block.  gyro_prev (R, 3) the raw gyro samples j - 1."""
        dtype = self.dtype
        r_zaru = np.asarray(r_zaru).astype(dtype)
        rows = []
        if mask & 1:
            rows += [(3 + i, self.vel[:, i], dtype(r_zupt)) for i in range(3)]
        if mask & 2:
            zg = self.wb + self.rest_rate() - np.asarray(gyro_prev).astype(dtype)
            rows += [(9 + i, zg[:, i], r_zaru[i]) for i in range(3)]
        for i, z, rv in rows:
            self.update_state(i, z, rv)
        return self.feedback()


def mag_rows(D, m_n):
    """(R, 3, 3): row i is the psi part of the magnetometer's h_i, m_n x D[i,:]."""
    return np.cross(np.broadcast_to(m_n, D.shape), D)


def _lla2ecef(lla):
    sl, cl = np.sin(lla[:, 0]), np.cos(lla[:, 0])
    r = ins_np.RE / np.sqrt(1.0 - ins_np.E_SQR * sl * sl)
    rho = (r + lla[:, 2]) * cl
    return np.stack([rho * np.cos(lla[:, 1]), rho * np.sin(lla[:, 1]), (r * (1.0 - ins_np.E_SQR) + lla[:, 2]) * sl], axis=-1)


def aid_numbers(aid):
    """(mask, every, scale_f, r_odo, r_nhc) of an `aid` dict: either ginsim.ins_loose.aiding_model's output or the same keys."""
    return int(aid['aid_mask']), int(aid['aid_every']), float(aid['odo_scale_f']), float(aid['r_odo']), float(aid['r_nhc'])


def mag_numbers(model):
    """(every, m_n, cal_si, cal_hi, r_mag) of ginsim.ins_loose.mag_model's output (or the same keys)."""
    return (int(model['mag_every']), np.asarray(model['mag_n']), np.asarray(model['cal_si']), np.asarray(model['cal_hi']),
            np.asarray(model['r_mag']))


def still_numbers(model):
    """(mask, every, r_zupt, r_zaru) of ginsim.ins_loose.still_model's output (or the same keys)."""
    return int(model['still_mask']), int(model['still_every']), float(model['r_zupt']), np.asarray(model['r_zaru'], dtype=np.float64)


def run(ref_frame, fs, gyro, accel, ini, model, gps=None, stamps=(), visible=None, earth_rot=True, dtype=np.float64, odo=None, aid=None,
        mag=None, mag_model=None, still=None, flags=None, keep_pdiag=False, hook=None, filt=None):
    """gyro, accel (R, n, 3); gps (R, m, 6); stamps (m,) IMU sample indices, strictly increasing; visible (m,) or None.
    model: dict r_diag(6) p0(5) q_v q_psi q_bg q_ba decay_g decay_a (3 each) -- ginsim.ins_loose.filter_model makes it.
    The optional blocks, each off when its numbers are None (or its mask 0) and then without any effect on the result:
      odo (R, n), aid         {'aid_mask', 'aid_every', 'odo_scale_f', 'r_odo', 'r_nhc'} (ginsim.ins_loose.aiding_model)
      mag (R, n, 3), mag_model {'mag_every', 'mag_n', 'cal_si', 'cal_hi', 'r_mag'} (ginsim.ins_loose.mag_model)
      still, flags (n,)       {'still_mask', 'still_every', 'r_zupt', 'r_zaru'} (ginsim.ins_loose.still_model), the standstill signal
    At sample j: the fix, the blocks in that order, hook(f, j) (a true return ends the loop), the row, propagate().
    filt: the filter to step, a LooseFilter of R runs made by the caller (None: a new LooseFilter).
    Returns dict att, pos, vel, wb, ab (R, n, 3), pdiag_end (R, 15), P_end (R, 15, 15); keep_pdiag: also 'pdiag' (R, n, 15), the
    diagonal of P at every stored row."""
    gyro, accel = np.asarray(gyro).astype(dtype), np.asarray(accel).astype(dtype)
    R, n, _ = gyro.shape
    f = LooseFilter(ref_frame, fs, ini, R, model, earth_rot, dtype) if filt is None else filt
    blocks = []                                                     # (period, gate (n,) or None, what fires at sample j)
    if aid is not None and aid_numbers(aid)[0]:
        mask, every, scale_f, r_odo, r_nhc = aid_numbers(aid)
        if mask & 1:
            odo = np.asarray(odo).astype(dtype)
        blocks.append((every, None, lambda j: f.aid(odo[:, j] if mask & 1 else None, mask, scale_f, r_odo, r_nhc)))
    if mag_model is not None:
        mevery, m_n, cal_si, cal_hi, r_mag = mag_numbers(mag_model)
        mag = np.asarray(mag).astype(dtype)
        blocks.append((mevery, None, lambda j: f.mag(mag[:, j], m_n, cal_si, cal_hi, r_mag)))
    if still is not None and still_numbers(still)[0]:
        smask, severy, r_zupt, r_zaru = still_numbers(still)
        blocks.append((severy, np.asarray(flags).reshape(n), lambda j: f.still(gyro[:, j - 1], smask, r_zupt, r_zaru)))
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
        for period, gate, fire in blocks:
            if period and j > 0 and j % period == 0 and (gate is None or gate[j] != 0):
                fire(j)
        stop = hook is not None and hook(f, j)
        out['att'][:, j], out['pos'][:, j], out['vel'][:, j], out['wb'][:, j], out['ab'][:, j] = f.att, f.pos, f.vel, f.wb, f.ab
        if keep_pdiag:
            out['pdiag'][:, j] = f.P[:, np.arange(NS), np.arange(NS)]
        if j == n - 1 or stop:
            break
        f.propagate(gyro[:, j], accel[:, j])
    out['pdiag_end'] = f.P[:, np.arange(NS), np.arange(NS)].copy()
    out['P_end'] = f.P
    return out


def error_state(ref_frame, att, pos, vel, wb, ab, t_att, t_pos, t_vel, t_bg, t_ba):
    """The 15 error states (estimate - truth) of R runs at one sample, in the filter's own coordinates: what pdiag describes.
    att, pos, vel, wb, ab (R, 3); truth t_att, t_pos, t_vel (3,) and t_bg, t_ba (R, 3) (constant bias + drift at that sample)."""
    R = att.shape[0]
    e = np.zeros((R, NS))
    if ref_frame == 0:
        rm, rn, _, _, cl = ins_np.geo_param(t_pos[0], t_pos[2])
        e[:, 0] = (pos[:, 0] - t_pos[0]) * (rm + t_pos[2])
        e[:, 1] = (pos[:, 1] - t_pos[1]) * (rn + t_pos[2]) * cl
        e[:, 2] = -(pos[:, 2] - t_pos[2])
    else:
        e[:, 0:3] = pos - t_pos
    e[:, 3:6] = vel - t_vel
    Ce = np.swapaxes(ins_np.dcm_zyx(np.asarray(att, dtype=np.float64)), 1, 2)
    Ct = ins_np.dcm_zyx(np.asarray(t_att, dtype=np.float64)[None])[0].T
    Psi = np.eye(3)[None] - np.einsum('rij,kj->rik', Ce, Ct)           # I - C_est C^T = [psi x]
    e[:, 6] = 0.5 * (Psi[:, 2, 1] - Psi[:, 1, 2])
    e[:, 7] = 0.5 * (Psi[:, 0, 2] - Psi[:, 2, 0])
    e[:, 8] = 0.5 * (Psi[:, 1, 0] - Psi[:, 0, 1])
    e[:, 9:12] = wb - t_bg
    e[:, 12:15] = ab - t_ba
    return e


def sample_sensors(rng, fs, ref_accel, ref_gyro, accel_err, gyro_err, runs):
    """Sensor series of `runs` runs drawn from the model itself with a NumPy generator (pathgen.acc_gen / gyro_gen / bias_drift as
    ins_np.sensor_errors restates them), and the bias truth b + drift[j] of every sample: (accel, gyro, t_ba, t_bg), each (R, n, 3)."""
    n = ref_accel.shape[0]
    out = []
    for ref, err, key in ((ref_accel, accel_err, 'vrw'), (ref_gyro, gyro_err, 'arw')):
        nd, nw = rng.standard_normal((runs, n, 3)), rng.standard_normal((runs, n, 3))
        meas = ins_np.sensor_errors(fs, ref, err, key, nd, nw)
        white = np.asarray(err[key], dtype=np.float64) * np.ones(3) / math.sqrt(1.0 / fs) * nw
        out.append((meas, meas - ref[None] - white))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def sample_odo(rng, ref_odo, odo_err, runs):
    """(R, n) odometer series drawn from pathgen.odo_gen's model: scale * ref_odo + stdv * N(0, 1)."""
    ref_odo = np.asarray(ref_odo, dtype=np.float64)
    return float(odo_err['scale']) * ref_odo[None] + float(odo_err['stdv']) * rng.standard_normal((runs, ref_odo.shape[0]))


def sample_mag(rng, ref_mag, mag_err, runs):
    """(R, n, 3) magnetometer series drawn from pathgen.mag_gen's model: (ref_mag + hi) . si^T + std * N(0, 1)."""
    ref_mag = np.asarray(ref_mag, dtype=np.float64)
    si, hi = np.asarray(mag_err['si'], dtype=np.float64).reshape(3, 3), np.asarray(mag_err['hi'], dtype=np.float64).reshape(3)
    std = np.asarray(mag_err['std'], dtype=np.float64) * np.ones(3)
    return ((ref_mag + hi) @ si.T)[None] + std * rng.standard_normal((runs,) + ref_mag.shape)
