"""CPU: the InsLoose restatements (tests/ins_loose_ref.py with its aiding, magnetometer and standstill blocks,
tests/ins_loose_scale_ref.py, tests/ins_loose_cons_ref.py) against
the nonlinear model they linearise, at 200 random attitudes (yaw over +-pi, pitch over +-80 deg, roll over +-pi) with fully
three-dimensional velocities, specific forces and fields, in np.longdouble where the platform has it.  The rotation the tests hold
the restatements to (rot_nb: Rx(roll) Ry(pitch) Rz(yaw) from elementary rotations, Rodrigues' formula for the error rotation) is
written here and shares nothing with them.

Every other InsLoose test runs tests/golden/ins_loose/motion_def_outage.csv: pitch 0, roll 0, no vertical velocity, 32 N 120 E.
There five of the nine entries of body_to_nav collapse, and a wrong sign or index in a term that sp, sr, a vertical velocity or a
horizontal specific force multiplies passes.  Each of B1-B4 therefore also applies a list of MUTATIONS to a copy of the restatement
(the module's source with one expression replaced, family()) and asserts that the residual grows beyond 100 x the allowance on the
random attitudes.  The same mutants run on LEVEL attitudes (yaw 30-120 deg, pitch 0, roll 0, horizontal velocity, 32 N 120 E, the
northern field) with the same general psi, specific force and calibration: LEVEL_BLIND, asserted below, names per test the mutants
whose residual stays within the allowance there -- what level attitudes cannot see whatever else a test varies:
    feedback (B1)            none
    measurement rows (B2)    dcm_sp, dcm_sr (aiding rows and magnetometer rows alike: the residual is the original's to three digits)
    magnetometer block (B2)  none
    transition blocks (B3)   none
    checkpoint (B4)          none
    rest rate (B5')          dcm_sp, dcm_sr (the residual is exactly the original's)
    odometer row, 16 states (B6')  dcm_sp, cross_order (a level vehicle moves along D[0,:]: v x D[0,:], the row's whole psi part, is zero)
    all rows, 16 states (B6')      dcm_sp, dcm_sr
B5'-B7' are the blocks of the two newest kernel families (the ZARU rest rate of ins_loose_ref.LooseFilter.still, the rows of
ins_loose_scale_ref.ScaleFilter.aid; the primes keep them apart from the consistency tests B5, B6 at the end of this file):
    B5'  rest_rate() in ref_frame 0 against rot_nb(att) (W cos lat, 0, -W sin lat): no linearisation, the allowance is rounding,
         8 eps W_IE (measured 0: both sides round alike); zero in ref_frame 1 and without earth_rot.
    B6'  the rows read back from what one block does to P = I, against central differences of the nonlinear innovation
         (D_est (v + dv))[0] - odo / (k + dk): measured 3.3e-9, B2's truncation.  The odometer's row reads D[0,:] only, so dcm_sr
         cannot move it (asserted); it is held to the 100 x on all three rows of the block.
    B7'  zero, +W sin lat, D^T for D, pitch and roll ignored as the rest rate move the restatement's wb on
         tests/golden/ins_loose/motion_def_tilted_stops.csv (4 runs, ref_frame 0, ZUPT and ZARU) by 5.5e7-1.0e9 x the parity bound
         tests/test_gpu_ins_loose_tilted_aids.py allows the device there (>= 100 x asserted); on the level stops profile 'pitch and roll
         ignored' moves it by 6e4 x only (printed).
B1, B3 and B4 see dcm_sp and dcm_sr on level attitudes only because their psi is general: the mutant then shows at 2 |psi| = 2e-4 rad,
not at 1 rad as on the random attitudes.  The level PROFILE has no such reference at all -- its tests compare kernel and restatement
with each other, and in a term that sp or sr multiplies both may carry the same mistake; that, and the rows above, is the gap.

Allowances.  Not taken from the issue: each is 10 x the residual of the unmodified restatement measured here (BASE, in the units
the test states), which is the truncation of the linearisation and nothing else:
    B1  |psi| = 1e-4: the feedback C <- (I + [psi x]) C_est leaves |psi|^2 = 1e-8, times 1 / cos(pitch) in yaw and roll where the
        angles are taken from the matrix that is orthogonal to first order only: measured 2.6e-8 rad, and the same when the fed-back
        x is the one error_state measures.  Rounding (1e-19) is eleven orders below.
    B2  central differences with a step of 1e-4 rad in psi through the exact rotation: step^2 / 6 = 1.7e-9 of |v| or |m|; the
        rows are exact in dv.  Measured 1.7e-9 for the magnetometer rows, 3.3e-9 for the aiding rows (compared as h h^T relative to
        |h|^2, which doubles it), 2.5e-9 rad for the block's estimate of a psi of 1e-4 (second order in psi).
    B3  F = (Phi - I) / dt at dt = 1e-6 s against central differences of two propagate() calls.  The mechanisation carries what
        Phi omits on purpose: the rotation during the step, |w| dt = 1e-6 of a block; the Coriolis and transport terms,
        (2 w_ie + w_en) dt = 1.5e-10; in ref_frame 0 the curvature, v dt / R = 1e-12.  Measured, relative to the largest entry of
        the block: 7.0e-6 in ref_frame 0 ((psi,bg): |w| dt / cos(pitch)^2 from the Euler-angle step) and 1.7e-4 in ref_frame 1
        ((v,psi): the body-frame velocity update rotates |v| = 14 m/s by w dt, |v| |w| dt / |f| / cos(pitch)^2).  Both halve with dt.
    B4  the checkpoint's psi is the antisymmetric part of I - C_est C^T = sin(|psi|) / |psi| psi: third order, |psi|^3 / 6 = 1.7e-13
        at |psi| = 1e-4 (measured 1.7e-13 rad); dr and dv are differences and exact to rounding (allowance: three half ulps of an
        angle of pi, in metres on the earth's radius: 3e-12 m in np.longdouble).  block_nees against np.linalg.solve in float64: 64 eps cond(B).
"""
import inspect
import sys
import types

import numpy as np
import pytest

import ins_loose_cases as cs
import ins_loose_cons_ref as cref
import ins_loose_mag_cases as mc
import ins_loose_ref                # noqa: F401  (family() copies the restatements from sys.modules)
import ins_loose_scale_ref          # noqa: F401
import ins_loose_still_cases as stc
from oracle import ins_np

LD = np.longdouble
N_ATT, PSI_NORM = 200, 1e-4
ORDER = ['ins_loose_ref', 'ins_loose_cons_ref', 'ins_loose_scale_ref']
TRANSPOSE = ('C = np.swapaxes(self.D, 1, 2)', 'C = self.D')
REST_RATE = "w_ie[:, 2] = -ins_np.W_IE * sl\n            w = np.einsum('rij,rj->ri', self.D, w_ie)"       # the two lines of rest_rate()
# name -> {module: [(expression, replacement), ...]}; every expression must occur in its module
MUTATIONS = {
    'dcm_sp': {'ins_loose_ref': [('m[..., 0, 2] = -sp', 'm[..., 0, 2] = sp')]},
    'dcm_sr': {'ins_loose_ref': [('m[..., 1, 2] = cp * sr', 'm[..., 1, 2] = -cp * sr')]},
    'transpose_C': {'ins_loose_ref': [TRANSPOSE, ('D, v = self.D, self.vel', 'D, v = np.swapaxes(self.D, 1, 2), self.vel'),
                                      ('        D = self.D\n', '        D = np.swapaxes(self.D, 1, 2)\n'),
                                      (REST_RATE, REST_RATE.replace('rij,rj->ri', 'rji,rj->ri'))],
                    'ins_loose_cons_ref': [('Ce = np.swapaxes(ref.dcm_zyx(f.att), 1, 2)', 'Ce = ref.dcm_zyx(f.att)'),
                                           ('Ct = ref.dcm_zyx(t[None, 0:3])[0].T', 'Ct = ref.dcm_zyx(t[None, 0:3])[0]')]},
    'negate_skew': {'ins_loose_ref': [('return np.stack([np.stack([z, -v[:, 2], v[:, 1]], 1)', 'return -np.stack([np.stack([z, -v[:, 2], v[:, 1]], 1)')]},
    'swap_d12_d22': {'ins_loose_ref': [('np.arctan2(d12, d22)', 'np.arctan2(d22, d12)')]},
    'cross_order': {'ins_loose_ref': [("H[:, :, 6:9] = -np.einsum('rij,rjk->rik', D, skew(v))", "H[:, :, 6:9] = np.einsum('rij,rjk->rik', D, skew(v))"),
                                      ('np.cross(np.broadcast_to(m_n, D.shape), D)', 'np.cross(D, np.broadcast_to(m_n, D.shape))')],
                    'ins_loose_cons_ref': [('e[:, 6] = (M[:, 1, 2] - M[:, 2, 1]) / 2', 'e[:, 6] = (M[:, 2, 1] - M[:, 1, 2]) / 2')]},
    'cal_si_T': {'ins_loose_ref': [("np.einsum('ik,rk->ri', cal_si.reshape(3, 3)", "np.einsum('ki,rk->ri', cal_si.reshape(3, 3)")]},
    'rest_hemisphere': {'ins_loose_ref': [(REST_RATE, REST_RATE.replace('-ins_np.W_IE * sl', 'ins_np.W_IE * sl'))]},
    'scale_entry_sign': {'ins_loose_scale_ref': [('return vb0 - odo_j / self.k_est, vb0 / self.k_est', 'return vb0 - odo_j / self.k_est, -vb0 / self.k_est')]},
}
# measured residuals of the unmodified restatement (module docstring); the allowance is 10 x
BASE = {'feedback': 2.6e-8, 'feedback_reverse': 2.6e-8, 'aid_rows': 3.3e-9, 'mag_rows': 1.7e-9, 'mag_block': 2.5e-9,
        'phi': {0: 7.0e-6, 1: 1.7e-4}, 'cons_psi': 1.7e-13, 'scale_row': 3.3e-9, 'scale_rows': 3.3e-9,
        # not measured: rounding of a three-term dot product of entries not above 1 (the allowance, 10 x, is 8 eps W_IE)
        'rest': 0.8 * float(np.finfo(LD).eps) * ins_np.W_IE}
LEVEL_BLIND = {'feedback': [], 'rows': ['dcm_sp', 'dcm_sr'], 'phi': [], 'cons': [], 'rest': ['dcm_sp', 'dcm_sr'], 'scale_row': ['dcm_sp', 'cross_order'], 'scale_rows': ['dcm_sp', 'dcm_sr']}


def family(name=None):
    """The two restatement modules, compiled again from their source with the mutation `name` applied (None: unchanged copies),
    each importing the copies before it: {module name: module}."""
    edits = MUTATIONS[name] if name else {}
    saved = {n: sys.modules[n] for n in ORDER}
    out = {}
    try:
        for n in ORDER:
            src = inspect.getsource(saved[n])
            for old, new in edits.get(n, ()):
                assert old in src, (name, n, old)
                src = src.replace(old, new)
            m = types.ModuleType(n)
            m.__file__ = saved[n].__file__
            exec(compile(src, saved[n].__file__, 'exec'), m.__dict__)
            sys.modules[n] = out[n] = m
    finally:
        sys.modules.update(saved)
    return out


@pytest.fixture(scope='module')
def families():
    return {name: family(name) for name in [None] + sorted(MUTATIONS)}


# ------------------------------------------------------------------------------------------------- the independent model
def rot_nb(att):
    """Navigation -> body of ZYX Euler angles (..., 3) as Rx(roll) Ry(pitch) Rz(yaw), in att's dtype."""
    att = np.asarray(att)
    out = None
    for axis, a in ((0, att[..., 2]), (1, att[..., 1]), (2, att[..., 0])):
        c, s = np.cos(a), np.sin(a)
        m = np.zeros(att.shape[:-1] + (3, 3), dtype=att.dtype)
        i, j = (axis + 1) % 3, (axis + 2) % 3
        m[..., axis, axis] = 1
        m[..., i, i], m[..., j, j], m[..., i, j], m[..., j, i] = c, c, s, -s
        out = m if out is None else np.matmul(out, m)
    return out


def euler_of(C):
    """ZYX Euler angles of a body -> navigation rotation (..., 3, 3)."""
    return np.stack([np.arctan2(C[..., 1, 0], C[..., 0, 0]), -np.arcsin(np.clip(C[..., 2, 0], -1, 1)), np.arctan2(C[..., 2, 1], C[..., 2, 2])], axis=-1)


def cross_matrix(v):
    m = np.zeros(v.shape[:-1] + (3, 3), dtype=v.dtype)
    m[..., 0, 1], m[..., 0, 2], m[..., 1, 0], m[..., 1, 2], m[..., 2, 0], m[..., 2, 1] = -v[..., 2], v[..., 1], v[..., 2], -v[..., 0], -v[..., 1], v[..., 0]
    return m


def error_rotation(psi):
    """exp(-[psi x]) by Rodrigues' formula: C_est = error_rotation(psi) C is the rotation whose first order is (I - [psi x]) C."""
    th = np.sqrt(np.sum(psi * psi, axis=-1))[..., None, None]
    K = -cross_matrix(psi)
    safe = np.where(th > 0, th, 1)
    a = np.where(th > 0, np.sin(safe) / safe, 1)
    b = np.where(th > 0, (1 - np.cos(safe)) / (safe * safe), 0.5)
    return np.eye(3, dtype=psi.dtype) + a * K + b * np.matmul(K, K)


def psi_between(C_est, C):
    """The psi of C_est = exp(-[psi x]) C to second order: the antisymmetric part of I - C_est C^T."""
    A = np.eye(3, dtype=C.dtype) - np.matmul(C_est, np.swapaxes(C, -1, -2))
    return 0.5 * np.stack([A[..., 2, 1] - A[..., 1, 2], A[..., 0, 2] - A[..., 2, 0], A[..., 1, 0] - A[..., 0, 1]], axis=-1)


def radii(lat, h):
    """(Rm + h, (Rn + h) cos(lat)) of WGS-84."""
    s = np.sin(lat)
    w = 1 - LD(ins_np.E_SQR) * s * s
    return LD(ins_np.RE) * (1 - LD(ins_np.E_SQR)) / (w * np.sqrt(w)) + h, (LD(ins_np.RE) / np.sqrt(w) + h) * np.cos(lat)


def test_the_independent_rotation_is_the_projects():
    att = draw('tilted')['att']
    assert np.max(np.abs(rot_nb(att).astype(np.float64) - ins_np.dcm_zyx(att.astype(np.float64)))) < 1e-15
    C = np.swapaxes(rot_nb(att), 1, 2)
    assert np.max(np.abs(np.mod(euler_of(C) - att + np.pi, 2 * np.pi) - np.pi)) < 1e-15
    psi = draw('tilted')['psi']
    assert np.max(np.abs(psi_between(np.matmul(error_rotation(psi), C), C) - psi)) < PSI_NORM ** 3


# ------------------------------------------------------------------------------------------------- the cases
_DRAWN = {}


def draw(kind):
    """The 200 cases of one kind, in np.longdouble: 'tilted' (random attitudes, three-dimensional velocity and field, both
    hemispheres) or 'level' (what the outage profile has: yaw 30-120 deg, pitch = roll = 0, horizontal velocity, 32 N 120 E, GEO)."""
    if kind in _DRAWN:
        return _DRAWN[kind]
    rng = np.random.default_rng(20260118 + (kind == 'level'))
    n = N_ATT
    u = lambda lo, hi, *shape: rng.uniform(lo, hi, (n,) + shape)
    d = {}
    if kind == 'tilted':
        att = np.stack([u(-np.pi, np.pi), np.deg2rad(u(-80, 80)), u(-np.pi, np.pi)], axis=1)
        att[:20, 0] = np.pi * np.where(np.arange(20) % 2, 1, -1) * (1 - 1e-7 * rng.uniform(0, 1, 20))      # at the yaw wrap
        d['vel'] = rng.normal(0, 8, (n, 3))
        d['field'] = rng.normal(0, 30, (n, 3))
        d['lla'] = np.stack([np.deg2rad(u(-80, 80)), np.deg2rad(u(-179.9, 179.9)), u(-100, 10000)], axis=1)
    else:
        att = np.stack([np.deg2rad(u(30, 120)), np.zeros(n), np.zeros(n)], axis=1)
        speed = u(5, 15)
        d['vel'] = np.stack([speed * np.cos(att[:, 0]), speed * np.sin(att[:, 0]), np.zeros(n)], axis=1)
        d['field'] = np.tile(np.array(mc.GEO), (n, 1))
        d['lla'] = np.tile(np.array([np.deg2rad(32.0), np.deg2rad(120.0), 10.0]), (n, 1))
    d['att'] = att
    psi = rng.normal(0, 1, (n, 3))
    d['psi'] = psi / np.linalg.norm(psi, axis=1, keepdims=True) * PSI_NORM
    d['gyro'], d['accel'] = rng.normal(0, 0.5, (n, 3)), rng.normal(0, 3, (n, 3))
    d['dr'], d['dv'] = rng.normal(0, 3, (n, 3)), rng.normal(0, 0.3, (n, 3))
    d['k'] = u(0.95, 1.05)                                                        # the odometer's scale factor (B6); drawn last
    _DRAWN[kind] = d = {k: v.astype(LD) for k, v in d.items()}
    return d


def model(fs):
    from ginsim.ins_loose import filter_model
    acc_e, gyr_e = cs.imu_errors()
    return filter_model(fs, acc_e, gyr_e, cs.GPS_ERR)


def make_filter(fam, rf, d, att=None, fs=20.0, scale=False):
    """A filter of N_ATT runs, one per case, at the case's position and navigation-frame velocity with the attitude att.
    scale: the 16-state filter (ins_loose_scale_ref.ScaleFilter) whose estimate of the scale factor is the case's k."""
    att = d['att'] if att is None else att
    vel_b = np.einsum('rij,rj->ri', rot_nb(att), d['vel'])
    ini = np.concatenate([d['lla'], vel_b, att], axis=1).T
    if scale:
        f = fam['ins_loose_scale_ref'].ScaleFilter(rf, fs, np.asarray(ini, dtype=np.float64), N_ATT, model(fs),
                                                   {'scale0': 1.0, 'p0_scale': 1.0, 'q_k': 0.0}, dtype=LD)
        f.k_est = d['k'].copy()
    else:
        f = fam['ins_loose_ref'].LooseFilter(rf, fs, np.asarray(ini, dtype=np.float64), N_ATT, model(fs), dtype=LD)
    # the constructor takes float64: put the long double values in, through the module's own dcm_zyx
    f.att, f.D = att.copy(), fam['ins_loose_ref'].dcm_zyx(att)
    f.vel = d['vel'].copy()
    f.vel_b = np.einsum('rij,rj->ri', f.D, f.vel)
    return f


def check(what, measure, families, names, base):
    """measure(family, kind) -> residual.  The unmodified restatement stays within 10 x base on the random attitudes, every mutant
    exceeds 100 x that allowance there, and the mutants the level attitudes cannot tell from the original are LEVEL_BLIND's."""
    allow = 10.0 * base
    got = float(measure(families[None], 'tilted'))
    level = float(measure(families[None], 'level'))
    print('%s: residual %.2e tilted, %.2e level (allowance %.2e)' % (what, got, level, allow))
    assert got <= allow and level <= allow, (what, got, level, allow)
    blind = []
    for name in names:
        t, l = float(measure(families[name], 'tilted')), float(measure(families[name], 'level'))
        print('  mutant %-13s residual %.2e tilted (x %.1e of the allowance), %.2e level%s' % (name, t, t / allow, l, '' if l > allow else '   <-- not seen'))
        assert t >= 100.0 * allow, (what, name, t, allow)
        if not l > allow:
            blind.append(name)
    return blind


# ------------------------------------------------------------------------------------------------- B1 feedback
def feedback_residual(fam, kind, reverse=False):
    """Truth C, estimate C_est = exp(-[psi x]) C; LooseFilter.correct, whose feedback is every block's,
    is driven so that its x[6:9] is psi exactly: P = I with P[0, 6:9] = P[6:9, 0] = psi and a fix whose only innovation is
    z0 = P00 + R0, so the first scalar update has gain 1 on that column and the other five have innovation 0.  Returns the largest
    |psi| left between the fed-back attitude and the truth [rad].  reverse: x[6:9] is what error_state measures on the estimate."""
    d = draw(kind)
    mod = fam['ins_loose_ref']
    C = np.swapaxes(rot_nb(d['att']), 1, 2)
    att_est = euler_of(np.matmul(error_rotation(d['psi']), C))
    f = make_filter(fam, 1, d, att_est)
    x_in = d['psi']
    if reverse:
        z3 = np.zeros((N_ATT, 3))
        # error_state takes ONE truth attitude: row by row
        e = np.stack([mod.error_state(1, att_est[i:i + 1].astype(np.float64), z3[:1], z3[:1], z3[:1], z3[:1], d['att'][i].astype(np.float64),
                                      z3[0], z3[0], z3[:1], z3[:1])[0] for i in range(N_ATT)])
        x_in = e[:, 6:9].astype(LD)
    f.P = np.zeros((N_ATT, 15, 15), dtype=LD)
    f.P[:] = np.eye(15, dtype=LD)
    f.P[:, 0, 6:9] = f.P[:, 6:9, 0] = x_in
    fix = np.concatenate([f.pos, f.vel], axis=1)
    fix[:, 0] -= 1 + f.m['r_diag'][0]
    x = f.correct(fix)
    assert np.max(np.abs(x[:, 6:9] - x_in)) < 1e-15 * PSI_NORM * 1e4
    return np.max(np.linalg.norm(psi_between(np.swapaxes(rot_nb(f.att), 1, 2), C).astype(np.float64), axis=1))


def test_feedback_removes_the_attitude_error_to_second_order(families):
    names = ['dcm_sp', 'dcm_sr', 'transpose_C', 'negate_skew', 'swap_d12_d22']
    blind = check('B1 feedback', feedback_residual, families, names, BASE['feedback'])
    assert blind == LEVEL_BLIND['feedback']
    check('B1 feedback of the measured error state', lambda fam, kind: feedback_residual(fam, kind, reverse=True), families,
          names, BASE['feedback_reverse'])


# ------------------------------------------------------------------------------------------------- B2 measurement rows
STEP = LD(1e-4)


def measurement_jacobian(C, vec, with_dv):
    """Central differences of h(dv, psi) = D_est (vec + dv), D_est = (exp(-[psi x]) C)^T, at dv = psi = 0: (R, 3, 6) = [dh/ddv, dh/dpsi]
    (the dv part is the exact D: h is linear in dv)."""
    J = np.zeros(C.shape[:1] + (3, 6), dtype=LD)
    J[:, :, 0:3] = np.swapaxes(C, 1, 2) if with_dv else 0
    for k in range(3):
        e = np.zeros(C.shape[:1] + (3,), dtype=LD)
        e[:, k] = STEP
        hp = np.einsum('rji,rj->ri', np.matmul(error_rotation(e), C), vec)
        hm = np.einsum('rji,rj->ri', np.matmul(error_rotation(-e), C), vec)
        J[:, :, 3 + k] = (hp - hm) / (2 * STEP)
    return J


def aid_rows_residual(fam, kind):
    """LooseFilter.aid builds its rows inside the block; they are read back from what the block does to P = I with R = 1, one row
    at a time: I - P' = h h^T / (|h|^2 + 1).  Compared, as h h^T / |h|^2, with the finite differences' (a row's overall sign is the
    innovation's; the sign of its psi part against its dv part is in the outer product)."""
    d = draw(kind)
    C = np.swapaxes(rot_nb(d['att']), 1, 2)
    J = measurement_jacobian(C, d['vel'], True)
    worst = 0.0
    for i in range(3):
        f = make_filter(fam, 1, d)
        f.P = np.zeros((N_ATT, 15, 15), dtype=LD)
        f.P[:] = np.eye(15, dtype=LD)
        f.aid(np.zeros(N_ATT), 1 << i, 1.0, 1.0, 1.0)
        M = (np.eye(15, dtype=LD) - f.P)
        outside = M.copy()
        outside[:, 3:9, 3:9] = 0
        assert np.max(np.abs(outside)) < 1e-15                                     # the rows touch dv and psi only
        M = M[:, 3:9, 3:9]
        hh = M / (1 - np.trace(M, axis1=1, axis2=2))[:, None, None]
        want = J[:, i, :, None] * J[:, i, None, :]
        worst = max(worst, float(np.max(np.abs(hh - want) / np.trace(want, axis1=1, axis2=2)[:, None, None])))
    return worst


def mag_rows_residual(fam, kind):
    d = draw(kind)
    C = np.swapaxes(rot_nb(d['att']), 1, 2)
    J = measurement_jacobian(C, d['field'], False)[:, :, 3:6]
    D = fam['ins_loose_ref'].dcm_zyx(d['att'])
    got = np.stack([fam['ins_loose_ref'].mag_rows(D[i:i + 1], d['field'][i])[0] for i in range(N_ATT)])
    return float(np.max(np.abs(got - J) / np.linalg.norm(d['field'], axis=1)[:, None, None]))


def mag_block_residual(fam, kind):
    """LooseFilter.mag on the estimate C_est = exp(-[psi x]) C with the error-free sample of the TRUE attitude, generated by a general
    magnetometer (MAG_ERR_SKEW) and calibrated by the block: with P = I on psi and R -> 0 the block returns the part of psi the
    field makes observable, psi minus its component along m_n.  [rad], relative to nothing: |psi| = 1e-4."""
    d = draw(kind)
    C = np.swapaxes(rot_nb(d['att']), 1, 2)
    att_est = euler_of(np.matmul(error_rotation(d['psi']), C))
    f = make_filter(fam, 1, d, att_est)
    f.P = np.zeros((N_ATT, 15, 15), dtype=LD)
    f.P[:, np.arange(6, 9), np.arange(6, 9)] = 1
    si, hi = mc.MAG_ERR_SKEW['si'].astype(LD), mc.MAG_ERR_SKEW['hi'].astype(LD)
    m_b = np.einsum('rji,rj->ri', C, d['field'])
    raw = np.einsum('ik,rk->ri', si, m_b + hi)
    cal_si = np.linalg.inv(mc.MAG_ERR_SKEW['si']).astype(LD)
    cal_si = cal_si + np.matmul(cal_si, np.eye(3, dtype=LD) - np.matmul(si, cal_si))        # one Newton step: the inverse in long double
    x = np.zeros((N_ATT, 15), dtype=LD)
    for i in range(N_ATT):                                                        # the block takes ONE field: row by row
        g = fam['ins_loose_ref'].LooseFilter.__new__(fam['ins_loose_ref'].LooseFilter)
        g.__dict__.update({k: (v[i:i + 1] if isinstance(v, np.ndarray) and v.shape[:1] == (N_ATT,) else v) for k, v in f.__dict__.items()})
        g.R = 1
        x[i] = g.mag(raw[i:i + 1], d['field'][i], cal_si, hi, np.full(3, 1e-12))[0]
    unit = d['field'] / np.linalg.norm(d['field'], axis=1, keepdims=True)
    want = d['psi'] - unit * np.sum(unit * d['psi'], axis=1, keepdims=True)
    return float(np.max(np.linalg.norm((x[:, 6:9] - want).astype(np.float64), axis=1)))


def test_measurement_rows_are_the_jacobian_of_the_nonlinear_measurement(families):
    blind = check('B2 aiding rows', aid_rows_residual, families, ['dcm_sp', 'dcm_sr', 'transpose_C', 'negate_skew', 'cross_order'], BASE['aid_rows'])
    blind_m = check('B2 magnetometer rows', mag_rows_residual, families, ['dcm_sp', 'dcm_sr', 'cross_order'], BASE['mag_rows'])
    assert blind == LEVEL_BLIND['rows'] and blind_m == LEVEL_BLIND['rows']
    check('B2 magnetometer block', mag_block_residual, families, ['dcm_sp', 'dcm_sr', 'transpose_C', 'cross_order', 'cal_si_T'],
          BASE['mag_block'])


# ------------------------------------------------------------------------------------------------- B5' the rest rate (standstill block)
def rest_residual(fam, kind):
    """LooseFilter.rest_rate() in ref_frame 0 against rot_nb(att) (W cos lat, 0, -W sin lat): the largest entry's deviation [rad/s]."""
    d = draw(kind)
    f = make_filter(fam, 0, d)
    lat = d['lla'][:, 0]
    w_n = LD(ins_np.W_IE) * np.stack([np.cos(lat), np.zeros_like(lat), -np.sin(lat)], axis=1)
    want = np.einsum('rij,rj->ri', rot_nb(d['att']), w_n)
    got = f.rest_rate()
    assert got.dtype == LD
    return float(np.max(np.abs(got - want)))


def test_rest_rate_is_the_earth_rate_in_the_body_axes(families):
    """No linearisation: the allowance is rounding, 8 eps W_IE (check() takes 10 x BASE['rest'] = 0.8 eps W_IE)."""
    blind = check("B5' rest rate", rest_residual, families, ['dcm_sp', 'dcm_sr', 'transpose_C', 'rest_hemisphere'], BASE['rest'])
    assert blind == LEVEL_BLIND['rest']
    for kind in ('tilted', 'level'):
        d = draw(kind)
        assert not make_filter(families[None], 1, d).rest_rate().any()
        f = make_filter(families[None], 0, d)
        assert f.rest_rate().any()
        f.earth_rot = False
        assert not f.rest_rate().any()


# ------------------------------------------------------------------------------------------------- B6' the odometer row of the 16 states
DK_STEP = LD(1e-6)
SCALE_STATES = [3, 4, 5, 6, 7, 8, 15]


def scale_row_residual(fam, kind, rows=(0,)):
    """ScaleFilter.aid's rows, read back one at a time from what one block (mask 1 << i, P = I, R = 1) does to P:
    I - P' = h h^T / (|h|^2 + 1) on the states 3-8 and 15.  Compared, as h h^T / |h|^2, with central differences of the nonlinear
    innovation: the odometer's z_0(dv, psi, dk) = (D_est (v + dv))[0] - odo / (k + dk) at odo = k v_b[0], the constraints'
    z_i = (D_est (v + dv))[i], which do not depend on dk.  Exact in dv, a step of 1e-4 rad in psi through the exact rotation, a step
    of 1e-6 in dk (truncation step^2 / k^2 = 1e-12 of the entry).  The largest deviation over `rows`."""
    d = draw(kind)
    C = np.swapaxes(rot_nb(d['att']), 1, 2)
    k = d['k']
    odo = k * np.einsum('rj,rj->r', C[:, :, 0], d['vel'])
    J = np.zeros((N_ATT, 3, 7), dtype=LD)
    J[:, :, 0:6] = measurement_jacobian(C, d['vel'], True)
    J[:, 0, 6] = (-odo / (k + DK_STEP) + odo / (k - DK_STEP)) / (2 * DK_STEP)
    pick = np.ix_(np.arange(N_ATT), SCALE_STATES, SCALE_STATES)
    worst = 0.0
    for i in rows:
        f = make_filter(fam, 1, d, scale=True)
        f.P = np.zeros((N_ATT, 15, 15), dtype=LD)
        f.P[:] = np.eye(15, dtype=LD)
        f.c, f.pkk = np.zeros((N_ATT, 15), dtype=LD), np.ones(N_ATT, dtype=LD)
        f.aid(odo, 1 << i, 1.0, 1.0, 1.0)
        M = np.eye(16, dtype=LD) - f.full_p()
        outside = M.copy()
        outside[pick] = 0
        assert np.max(np.abs(outside)) < 1e-15                                    # the rows touch dv, psi and dk only
        M = M[pick]
        hh = M / (1 - np.trace(M, axis1=1, axis2=2))[:, None, None]
        want = J[:, i, :, None] * J[:, i, None, :]
        worst = max(worst, float(np.max(np.abs(hh - want) / np.trace(want, axis1=1, axis2=2)[:, None, None])))
    return worst


def test_scale_row_is_the_jacobian_of_the_nonlinear_odometer_innovation(families):
    """The odometer's row reads D[0, :] = (cp cy, cp sy, -sp) and nothing else of D, so the mutant dcm_sr (the sign of D[1, 2]) cannot
    move it: that is asserted, and dcm_sr is held to the 100 x with the two constraint rows of the same block next to the odometer's
    (their entry on state 15 is zero), where every one of the five mutants shows."""
    blind = check("B6' odometer row, 16 states", scale_row_residual, families, ['dcm_sp', 'transpose_C', 'cross_order', 'scale_entry_sign'],
                  BASE['scale_row'])
    assert blind == LEVEL_BLIND['scale_row']
    assert scale_row_residual(families['dcm_sr'], 'tilted') == scale_row_residual(families[None], 'tilted')
    blind = check("B6' all three rows, 16 states", lambda fam, kind: scale_row_residual(fam, kind, (0, 1, 2)), families,
                  ['dcm_sp', 'dcm_sr', 'transpose_C', 'cross_order', 'scale_entry_sign'], BASE['scale_rows'])
    assert blind == LEVEL_BLIND['scale_rows']


# ------------------------------------------------------------------------------------------------- B7' the parity bound sees the rest rate
def _rest_zero(f):
    return np.zeros((f.R, 3), dtype=f.dtype)


def _rest_with(f, hemisphere=1.0, transposed=False, level=False):
    _, _, _, sl, cl = ins_np.geo_param(f.pos[:, 0], f.pos[:, 2])
    w_ie = np.zeros((f.R, 3), dtype=f.dtype)
    w_ie[:, 0], w_ie[:, 2] = ins_np.W_IE * cl, -hemisphere * ins_np.W_IE * sl
    D = ins_loose_ref.dcm_zyx(f.att * np.array([1.0, 0.0, 0.0], dtype=f.dtype)) if level else f.D
    return np.einsum('rji,rj->ri' if transposed else 'rij,rj->ri', D, w_ie)


WRONG_REST_RATES = {'zero': _rest_zero, '+W sin lat': lambda f: _rest_with(f, hemisphere=-1.0), 'D^T for D': lambda f: _rest_with(f, transposed=True),
                    'pitch and roll ignored': lambda f: _rest_with(f, level=True)}


def rest_rate_ratios(profile, runs=4):
    """{wrong version: deviation of the restatement with it from the unmodified one in wb, over the parity bound of the case}: 4 runs
    drawn from the model on `profile`, ref_frame 0, ZUPT and ZARU at every flagged sample."""
    rf, fs = 0, 20.0
    ini, truth, stamps = stc.stops_truth(fs, rf, 2.0, None, profile)
    acc_e, gyr_e = cs.imu_errors()
    rng = np.random.default_rng(20260118)
    accel, gyro, _, _ = ins_loose_ref.sample_sensors(rng, fs, truth['ref_accel'], truth['ref_gyro'], acc_e, gyr_e, runs)
    gps = cs.sample_gps(rng, truth, rf, runs)
    m = model(fs)
    args = (rf, fs, gyro, accel, ini, m, gps, stamps, truth['gps_visibility'])
    kw = dict(still=stc.model(m, fs, 3), flags=stc.flags_of(truth))
    assert _rest_with(ins_loose_ref.LooseFilter(rf, fs, ini, runs, m)).tobytes() == ins_loose_ref.LooseFilter(rf, fs, ini, runs, m).rest_rate().tobytes()
    good = ins_loose_ref.run(*args, **kw)
    bound = cs.parity_bound(*args, **kw)
    out = {}
    for name, fn in WRONG_REST_RATES.items():
        wrong = type('WrongRestRate', (ins_loose_ref.LooseFilter,), {'rest_rate': fn})
        o = ins_loose_ref.run(*args, filt=wrong(rf, fs, ini, runs, m), **kw)
        dev = cs.deviation(o, good)
        out[name] = {k: dev[k] / bound[k] for k in dev}
    return out


def test_the_parity_bound_sees_a_wrong_rest_rate_on_the_tilted_stops_profile():
    """What tests/test_gpu_ins_loose_tilted_aids.py would do to a kernel whose w_rest is wrong: each of four wrong rest rates moves the
    restatement's wb on the tilted stops profile by at least 100 x the parity bound the device is allowed there.  The level stops
    profile's ratios are printed for information."""
    for label, profile in (('tilted stops', stc.TILTED_STOPS_CSV), ('level stops', stc.STOPS_CSV)):
        ratios = rest_rate_ratios(profile)
        for name, r in ratios.items():
            print("B7' %s, rest rate '%s': deviation over the parity bound: " % (label, name) + ', '.join('%s %.1e' % kv for kv in r.items()))
        if profile == stc.TILTED_STOPS_CSV:
            for name, r in ratios.items():
                assert r['wb'] >= 100.0, (name, r)


# ------------------------------------------------------------------------------------------------- B3 transition blocks
PHI_FS = 1e6
BLOCKS = {'v,psi': (slice(3, 6), slice(6, 9)), 'v,ba': (slice(3, 6), slice(12, 15)), 'psi,bg': (slice(6, 9), slice(9, 12)), 'r,v': (slice(0, 3), slice(3, 6))}


def _perturbed(fam, rf, d, k, eps):
    mod = fam['ins_loose_ref']
    f = make_filter(fam, rf, d, fs=PHI_FS)
    if k < 3:
        raise AssertionError('no block of the list has a position column')
    if k < 6:
        f.vel[:, k - 3] += eps
    elif k < 9:
        e = np.zeros((N_ATT, 3), dtype=LD)
        e[:, k - 6] = eps
        f.att = euler_of(np.matmul(error_rotation(e), np.swapaxes(rot_nb(d['att']), 1, 2)))
        f.D = mod.dcm_zyx(f.att)
    elif k < 12:
        f.wb[:, k - 9] += eps
    else:
        f.ab[:, k - 12] += eps
    f.vel_b = np.einsum('rij,rj->ri', f.D, f.vel)
    return f


def _difference(rf, a, b):
    """The error state a - b of two filters (R, 15), position in the filter's own coordinates."""
    e = np.zeros((N_ATT, 15), dtype=LD)
    if rf == 0:
        mlat, mlon = radii(b.pos[:, 0], b.pos[:, 2])
        e[:, 0], e[:, 1], e[:, 2] = (a.pos[:, 0] - b.pos[:, 0]) * mlat, (a.pos[:, 1] - b.pos[:, 1]) * mlon, -(a.pos[:, 2] - b.pos[:, 2])
    else:
        e[:, 0:3] = a.pos - b.pos
    e[:, 3:6] = a.vel - b.vel
    e[:, 6:9] = psi_between(np.swapaxes(rot_nb(a.att), 1, 2), np.swapaxes(rot_nb(b.att), 1, 2))
    e[:, 9:12], e[:, 12:15] = a.wb - b.wb, a.ab - b.ab
    return e


def phi_residual(fam, kind, rf):
    """Phi as propagate() builds it is read from what it does to P: with P = E(k, 0) (one entry; column 0 of Phi is e_0, nothing
    depends on the position) column 0 of P' is column k of Phi.  F = (Phi - I) / dt of the four blocks against central differences
    of the mechanisation over one step; the largest deviation relative to the block's largest entry."""
    d = draw(kind)
    dt = LD(1) / LD(PHI_FS)
    F = np.zeros((N_ATT, 15, 15), dtype=LD)
    G = np.zeros((N_ATT, 15, 15), dtype=LD)
    for k in range(3, 15):
        f = make_filter(fam, rf, d, fs=PHI_FS)
        f.P = np.zeros((N_ATT, 15, 15), dtype=LD)
        f.P[:, k, 0] = 1
        f.propagate(d['gyro'], d['accel'])
        F[:, :, k] = f.P[:, :, 0]
        eps = LD(1.0) if k < 6 else LD(1e-5) if k < 9 else LD(1e-3)                # the velocity column is exactly linear
        a, b = _perturbed(fam, rf, d, k, eps), _perturbed(fam, rf, d, k, -eps)
        e0 = _difference(rf, a, b)
        a.propagate(d['gyro'], d['accel'])
        b.propagate(d['gyro'], d['accel'])
        G[:, :, k] = (_difference(rf, a, b) - e0) / (2 * eps) / dt
    F[:, np.arange(15), np.arange(15)] -= 1
    F /= dt
    worst = 0.0
    for rows, cols in BLOCKS.values():
        scale = np.max(np.abs(G[:, rows, cols]), axis=(1, 2))
        worst = max(worst, float(np.max(np.abs(F[:, rows, cols] - G[:, rows, cols]) / scale[:, None, None])))
    return worst


@pytest.mark.parametrize('rf', [0, 1])
def test_transition_blocks_are_the_jacobian_of_the_mechanisation(families, rf):
    blind = check('B3 Phi rf%d' % rf, lambda fam, kind: phi_residual(fam, kind, rf), families, ['transpose_C', 'negate_skew'], BASE['phi'][rf])
    assert blind == LEVEL_BLIND['phi']


# ------------------------------------------------------------------------------------------------- B4 checkpoint
def cons_residual(fam, kind, rf=0):
    """ins_loose_cons_ref.nav_error of an estimate displaced by (dr, dv, psi) from the truth row: [worst |psi - psi_in| in rad,
    worst deviation of dr and dv in m, m/s]."""
    d = draw(kind)
    C = np.swapaxes(rot_nb(d['att']), 1, 2)
    att_est = euler_of(np.matmul(error_rotation(d['psi']), C))
    out_psi, out_lin = 0.0, 0.0
    for i in range(N_ATT):
        lla = d['lla'][i]
        if rf == 0:
            mlat, mlon = radii(lla[0], lla[2])
            pos = lla + np.stack([d['dr'][i, 0] / mlat, d['dr'][i, 1] / mlon, -d['dr'][i, 2]])
        else:
            pos = lla + d['dr'][i]
        f = types.SimpleNamespace(dtype=LD, R=1, rf=rf, pos=pos[None], vel=(d['vel'][i] + d['dv'][i])[None], att=att_est[i:i + 1])
        e = fam['ins_loose_cons_ref'].nav_error(f, np.concatenate([d['att'][i], lla, d['vel'][i]]))[0]
        out_psi = max(out_psi, float(np.linalg.norm((e[6:9] - d['psi'][i]).astype(np.float64))))
        want = np.concatenate([d['dr'][i], d['dv'][i]])
        out_lin = max(out_lin, float(np.max(np.abs(e[0:6] - want))))
    return out_psi, out_lin


def test_checkpoint_error_state(families):
    names = ['dcm_sp', 'dcm_sr', 'transpose_C', 'cross_order']
    blind = check('B4 checkpoint psi', lambda fam, kind: cons_residual(fam, kind)[0], families, names, BASE['cons_psi'])
    assert blind == LEVEL_BLIND['cons']
    for rf in (0, 1):
        lin = cons_residual(families[None], 'tilted', rf)[1]
        print('B4 checkpoint dr, dv rf%d: %.2e m' % (rf, lin))
        # a latitude or longitude of up to pi rad carries half an ulp, times 6.4e6 m; estimate, truth and their difference: 3 of them
        assert lin <= 3 * 0.5 * np.finfo(LD).eps * np.pi * 6.4e6, lin
    d = draw('tilted')
    wrapped = np.abs(euler_of(np.matmul(error_rotation(d['psi']), np.swapaxes(rot_nb(d['att']), 1, 2)))[:, 0] - d['att'][:, 0]) > 6.0
    assert wrapped.any()                                                          # an estimate across the yaw wrap from its truth is among the cases


def test_block_nees_is_the_solve():
    rng = np.random.default_rng(5)
    A = rng.normal(0, 1, (N_ATT, 3, 3)) * 10.0 ** rng.uniform(-4, 1, (N_ATT, 1, 1))
    B = np.matmul(A, np.swapaxes(A, 1, 2)) + 1e-3 * np.eye(3) * np.max(np.abs(A), axis=(1, 2))[:, None, None] ** 2
    e = rng.normal(0, 1, (N_ATT, 3))
    got = cref.block_nees(B.astype(LD), e.astype(LD)).astype(np.float64)
    want = np.einsum('ri,ri->r', e, np.linalg.solve(B, e[:, :, None])[:, :, 0])
    bound = 64 * np.finfo(np.float64).eps * np.linalg.cond(B)
    assert np.all(np.abs(got - want) <= bound * want), np.max(np.abs(got - want) / want / bound)
    bad = B.copy()
    bad[0] = -bad[0]
    bad[1, 0, 1] = bad[1, 1, 0] = 10 * np.sqrt(bad[1, 0, 0] * bad[1, 1, 1])        # second leading minor negative
    out = cref.block_nees(bad, e)
    assert np.isnan(out[0]) and np.isnan(out[1]) and np.all(np.isfinite(out[2:]))


# ------------------------------------------------------------------------------------------------- B5, B6 consistency
def end_stats(c, name):
    o = mc.restate_filter(c, name)
    e = mc.end_error(c, o['att'][:, -1], o['pos'][:, -1], o['vel'][:, -1], o['wb'][:, -1], o['ab'][:, -1])
    return e, mc.end_statistics(e, o['pdiag_end'])


@pytest.fixture(scope='module')
def tilted_draw():
    return mc.consistency_draw('tilted', 1, cs.CONSISTENCY_FS, cs.CONSISTENCY_RUNS)


@pytest.mark.parametrize('name', list(mc.FILTERS))
def test_consistency_on_the_tilted_profile(tilted_draw, name):
    """B5.  ref_frame 1, 1024 runs at 20 Hz with 2 Hz GPS: RMS end error over sqrt(mean pdiag_end) lies in [0.7, 1.4] for GPS only, the
    odometer (mask 1) and the magnetometer (MAG_ERR_SKEW, GEO_SOUTH); with the magnetometer and mask 7 it is bounded above only, as
    mask 7 is on the level profile (the pseudo-noise of the non-holonomic rows is an allowance, not a noise that is drawn).  The
    ratios are the ones recorded in ins_loose_mag_cases.CONSISTENCY_BY_PROFILE, which the device is held to."""
    _, s = end_stats(tilted_draw, name)
    print("tilted, ref_frame 1, '%s': " % name + ', '.join('%.3f' % x for x in s['ratio']))
    assert np.all(s['ratio'] <= 1.4) and (name == 'mag7' or np.all(s['ratio'] >= 0.7)), s['ratio']
    np.testing.assert_allclose(s['ratio'], mc.CONSISTENCY_BY_PROFILE['tilted'][name], rtol=0, atol=2e-3)


@pytest.fixture(scope='module', params=['level', 'tilted'])
def error_free(request):
    """{(rf, fs, filter): e0 / sigma (15,)} of one run with error-free sensors, fixes and magnetometer."""
    out = {}
    for rf, fs in ((0, 20.0), (0, 100.0), (1, 20.0)):
        c = mc.consistency_draw(request.param, rf, fs, 1, error_free=True)
        for name in ('gps', 'mag'):
            e, s = end_stats(c, name)
            out[rf, fs, name] = e[0] / s['sigma']
    return request.param, out


def test_error_free_offset(error_free):
    """B6.  With error-free inputs the ref_frame 1 estimate ends on the truth (|e0| < 1e-3 sigma in every state): the mechanisation
    reproduces the path generator.  In ref_frame 0 it does not: the mechanisation and the path generator's truth differ by a term of
    first order in dt, the filter takes the drift for sensor error, and the estimate ends e0 away from the truth -- the same e0 in
    every run, which no covariance describes.  e0 / sigma is the table ins_loose_mag_cases.E0_OVER_SIGMA; it scales with dt."""
    profile, out = error_free
    for name in ('gps', 'mag'):
        assert np.max(np.abs(out[1, 20.0, name])) < 1e-3, (profile, name, out[1, 20.0, name])
        for fs in (20.0, 100.0):
            print("e0 / sigma, ref_frame 0, %s, '%s', %g Hz: " % (profile, name, fs) + ', '.join('%.3f' % x for x in out[0, fs, name]))
            np.testing.assert_allclose(out[0, fs, name], mc.E0_OVER_SIGMA[profile, name, int(fs)], rtol=0, atol=2e-3)
        big = np.abs(out[0, 20.0, name]) > 0.3
        assert big.any()                                                          # the offset is there, and it shrinks with dt
        assert np.all(np.abs(out[0, 100.0, name][big]) < 0.5 * np.abs(out[0, 20.0, name][big]))


B6_FS, B6_RUNS = 100.0, 256


@pytest.mark.parametrize('profile', ['level', 'tilted'])
def test_ref_frame_0_spread_and_mean(profile):
    """B6.  ref_frame 0, 256 runs at 100 Hz: the across-run spread of the end error is what the covariance says (std over
    sqrt(mean pdiag_end) in [0.7, 1.4] for all 15 states), and the across-run mean is the error-free offset e0 and nothing else
    (within 4 sigma / sqrt(R) per state)."""
    c = mc.consistency_draw(profile, 0, B6_FS, B6_RUNS)
    for name in ('gps', 'mag'):
        e, s = end_stats(c, name)
        e0 = np.array(mc.E0_OVER_SIGMA[profile, name, int(B6_FS)])
        excess = (s['mean'] - e0) * np.sqrt(B6_RUNS)
        print("ref_frame 0, %s, '%s': spread %s\n    (mean - e0) in sigma / sqrt(R): %s" % (profile, name, ', '.join('%.3f' % x for x in s['spread']),
                                                                                         ', '.join('%.2f' % x for x in excess)))
        assert np.all(s['spread'] >= 0.7) and np.all(s['spread'] <= 1.4), (name, s['spread'])
        assert np.all(np.abs(excess) <= 4.0), (name, excess)
