"""NumPy restatement of the loosely coupled GPS/INS filter (csrc/ins_loose.hip, ginsim_loose_run), vectorised over runs: batched
einsum, one Python loop over time.  The reference declares InsLoose's interface only (demo_algorithms/ins_loose.py: prediction
and correction are `pass`), so this file IS the specification by example; the device kernel is held to it and it is held to
oracle/ins_np.py's free integration (a filter without a usable fix is free integration) and to the statistics of its own covariance.

Convention (one consistent set):
  error state x = estimate - truth, order dr(0-2) dv(3-5) psi(6-8) dbg(9-11) dba(12-14)
  dr: NED metres (ref_frame 0) or the virtual-inertial axes (ref_frame 1); psi: C_est = (I - [psi x]) C, C = body -> navigation
  per IMU sample   P <- Phi P Phi^T + Qd,  Phi = I + F dt,  F blocks (r,v) = I, (v,psi) = [f^n x], (v,ba) = -C, (psi,bg) = C,
                   (bg,bg) = -1/tau_g, (ba,ba) = -1/tau_a  [decay = 1 - dt/tau on the diagonal of Phi]; f^n = C (accel - ab)
                   Qd = blockdiag(0, C diag(q_v) C^T, C diag(q_psi) C^T, diag(q_bg), diag(q_ba))
  fix k at IMU sample stamp[k], when visible[k] != 0, on the state that sample's row reports, before the row is stored:
                   z = ins - gps (LLA difference -> NED metres with (Rm + h), (Rn + h) cos(lat) in ref_frame 0), H = [I6 0],
                   six sequential scalar updates, then feedback (pos, vel -= dr, dv; C <- (I + [psi x]) C_est, Euler angles from
                   its rows by atan2; wb, ab -= dbg, dba) and x = 0
  mechanisation    oracle/ins_np.free_integration's step on accel - ab, gyro - wb
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

    # ------------------------------------------------------------------ one fix
    def correct(self, fix):
        """fix (R, 6) = pos3, vel3 in the units of the state."""
        R, dtype = self.R, self.dtype
        z = np.empty((R, 6), dtype=dtype)
        if self.rf == 0:
            rm, rn, _, _, cl = ins_np.geo_param(self.pos[:, 0], self.pos[:, 2])
            mlat, mlon = rm + self.pos[:, 2], (rn + self.pos[:, 2]) * cl
            z[:, 0] = (self.pos[:, 0] - fix[:, 0]) * mlat
            z[:, 1] = (self.pos[:, 1] - fix[:, 1]) * mlon
            z[:, 2] = -(self.pos[:, 2] - fix[:, 2])
        else:
            z[:, 0:3] = self.pos - fix[:, 0:3]
        z[:, 3:6] = self.vel - fix[:, 3:6]
        x = np.zeros((R, NS), dtype=dtype)
        P = self.P
        for i in range(6):
            col = P[:, :, i].copy()
            inv = 1 / (col[:, i] + self.m['r_diag'][i])
            g = (z[:, i] - x[:, i]) * inv
            x = x + col * g[:, None]
            P = P - col[:, :, None] * col[:, None, :] * inv[:, None, None]
        self.P = P
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


def _lla2ecef(lla):
    sl, cl = np.sin(lla[:, 0]), np.cos(lla[:, 0])
    r = ins_np.RE / np.sqrt(1.0 - ins_np.E_SQR * sl * sl)
    rho = (r + lla[:, 2]) * cl
    return np.stack([rho * np.cos(lla[:, 1]), rho * np.sin(lla[:, 1]), (r * (1.0 - ins_np.E_SQR) + lla[:, 2]) * sl], axis=-1)


def run(ref_frame, fs, gyro, accel, ini, model, gps=None, stamps=(), visible=None, earth_rot=True, dtype=np.float64):
    """gyro, accel (R, n, 3); gps (R, m, 6); stamps (m,) IMU sample indices, strictly increasing; visible (m,) or None.
    model: dict r_diag(6) p0(5) q_v q_psi q_bg q_ba decay_g decay_a (3 each) -- ginsim.ins_loose.filter_model makes it.
    Returns dict att, pos, vel, wb, ab (R, n, 3), pdiag_end (R, 15), P_end (R, 15, 15)."""
    gyro, accel = np.asarray(gyro).astype(dtype), np.asarray(accel).astype(dtype)
    R, n, _ = gyro.shape
    f = LooseFilter(ref_frame, fs, ini, R, model, earth_rot, dtype)
    out = {k: np.zeros((R, n, 3), dtype=dtype) for k in ('att', 'pos', 'vel', 'wb', 'ab')}
    stamps = [int(s) for s in stamps]
    gps = None if gps is None else np.asarray(gps).astype(dtype)
    kf = 0
    for j in range(n):
        if kf < len(stamps) and stamps[kf] == j:
            if visible is None or visible[kf] != 0:
                f.correct(gps[:, kf])
            kf += 1
        out['att'][:, j], out['pos'][:, j], out['vel'][:, j], out['wb'][:, j], out['ab'][:, j] = f.att, f.pos, f.vel, f.wb, f.ab
        if j == n - 1:
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
