"""CPU: what check_mc_params, check_incl_params, check_loose_params, check_loose_cons, check_loose_mag and check_loose_scale
(csrc/api_mc.hip) refuse, in which order, and the dispatch table of the loose family -- through the name queries
ginsim_mc_kernel_name, ginsim_incl_kernel_name, ginsim_loose_kernel_name, ginsim_loose_cons_kernel_name,
ginsim_loose_mag_kernel_name and ginsim_loose_scale_kernel_name, which run the same checks as the launches and need no device.

Every case starts from one valid block per entry point (dummy non-NULL pointers: a name query reads host memory only) and breaks
one field per REQUIRE of those functions; 'a + b' breaks two, which pins the ORDER of the checks where the functions share
helpers: sizes before the sensor source, the sensor source before the vibration, the vibration before what follows it.

tests/golden/api_refusals.json holds (return code, full message) of every case, recorded from commit 89d973d (each function with
its own copy of every check) by this file run with GINSIM_RECORD_REFUSALS=1; the 'mag' and 'scale' entries were added to it from
commit 20487e3 (the last one in which every entry point of the loose family orders its checks itself).  It is the definition of
"the same refusals" for any later shape of those functions and is not regenerated from changed code."""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, 'api_refusals.json')
NAN, INF = float('nan'), float('inf')
N, RUNS = 30, 4
TOO_MANY_RUNS = 0x7FFFFFFF * 64 + 1


class Blocks(object):
    """The valid parameter blocks of one entry point: mc (ginsim_mc_params), p (the kernel's own block), q (the family's block:
    checkpoints, magnetometer or scale-factor state)."""

    def __init__(self, entry, given):
        from ginsim import _lib as L
        self.entry = entry
        self.dummy = np.zeros(64)
        self.stamps = np.array([0, 10, 20], dtype=np.int64)
        self.samples = np.array([5, 10, 29], dtype=np.int64)
        d = self.d = self.dummy.ctypes.data
        m = self.mc = L.McParams()
        m.n, m.runs, m.fs, m.n_ini, m.ini = N, RUNS, 100.0, 1, d
        if given:
            m.given_sensors, m.in_accel, m.in_gyro, m.in_odo = 1, d, d, d
        else:
            m.ref_accel, m.ref_gyro, m.ref_odo = d, d, d
        self.p = self.q = None
        if entry == 'mc':
            m.algo_mask = 1
        elif entry == 'incl':
            p = self.p = L.InclParams()
            p.algo_mask, p.dt, p.n_list, p.bias_in = 3, 0.01, RUNS, d
        else:
            p = self.p = L.LooseParams()
            p.m, p.gps_stamp, p.n_list = 3, self.stamps.ctypes.data, RUNS
            p.in_gps, p.ref_gps = (d, None) if given else (None, d)
            p.r_diag[:], p.p0[:] = [1.0] * 6, [1.0] * 5
            p.decay_g[:], p.decay_a[:] = [1.0] * 3, [1.0] * 3
            if entry == 'cons':
                q = self.q = L.LooseConsParams()
                q.cons_sample, q.cons_m, q.out_cons, q.cons_work = self.samples.ctypes.data, 3, d, d
                m.ref_nav = d
            elif entry == 'mag':
                q = self.q = L.LooseMagParams()
                q.mag_every, q.in_mag, q.ref_mag = 1, (d if given else None), (None if given else d)
                q.mag_si[:], q.cal_si[:] = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
                q.mag_std[:], q.mag_n[:], q.r_mag[:] = [0.01] * 3, [30.0, -3.0, 40.0], [1e-4] * 3
            elif entry == 'scale':
                q = self.q = L.LooseScaleParams()
                q.scale0, q.p0_scale, q.q_k = 1.0, 0.02, 0.0
                p.aid_mask, p.aid_every, p.r_odo, p.odo_scale_f = 1, 1, 0.01, 1.0

    def name(self):
        """(return code, kernel name or the refusal's message)"""
        from ginsim import _lib as L
        buf = ctypes.create_string_buffer(256)
        ref = lambda s: None if s is None else ctypes.byref(s)
        if self.entry == 'mc':
            rc = L.lib.ginsim_mc_kernel_name(ref(self.mc), buf, 256)
        elif self.entry == 'incl':
            rc = L.lib.ginsim_incl_kernel_name(ref(self.mc), ref(self.p), buf, 256)
        elif self.entry == 'loose':
            rc = L.lib.ginsim_loose_kernel_name(ref(self.mc), ref(self.p), buf, 256)
        else:
            fn = {'cons': L.lib.ginsim_loose_cons_kernel_name, 'mag': L.lib.ginsim_loose_mag_kernel_name,
                  'scale': L.lib.ginsim_loose_scale_kernel_name}[self.entry]
            rc = fn(ref(self.mc), ref(self.p), ref(self.q), buf, 256)
        return [rc, (buf.value if rc == L.OK else L.lib.ginsim_last_error()).decode()]


def _set(path, value, index=None):
    """A violation: b.<path> = value (or b.<path>[index] = value)."""
    def apply(b):
        obj, names = b, path.split('.')
        for k in names[:-1]:
            obj = getattr(obj, k)
        if index is None:
            setattr(obj, names[-1], value)
        else:
            getattr(obj, names[-1])[index] = value
    return apply


def _all(*fns):
    def apply(b):
        for f in fns:
            f(b)
    return apply


def _stamp(attr, k, value):
    def apply(b):
        getattr(b, attr)[k] = value
    return apply


def _drop(attr):
    def apply(b):
        setattr(b, attr, None)
    return apply


def _ptr(path, index=None):
    def apply(b):
        _set(path, b.d, index)(b)
    return apply


# sizes, the first checks of all three parameter checks
SIZES = {'n=0': _set('mc.n', 0), 'runs=0': _set('mc.runs', 0), 'n=2^32': _set('mc.n', 2 ** 32), 'runs too many': _set('mc.runs', TOO_MANY_RUNS)}
# the vibration block of the kernels without psd
VIB = {'vib_accel psd': _set('mc.vib_accel.type', 3), 'vib_gyro type 9': _set('mc.vib_gyro.type', 9),
       'vib_accel amp nan': _all(_set('mc.vib_accel.type', 1), _set('mc.vib_accel.amp', NAN, 1)),
       'vib_gyro omega_dt inf': _all(_set('mc.vib_gyro.type', 2), _set('mc.vib_gyro.omega_dt', INF))}
MODELS = {'accel.bias nan': _set('mc.accel.bias', NAN, 0), 'accel.gm_a inf': _set('mc.accel.gm_a', INF, 1),
          'gyro.gm_b nan': _set('mc.gyro.gm_b', NAN, 2), 'gyro.white -inf': _set('mc.gyro.white', -INF, 0)}

# {entry: {form ('gen' | 'given'): {violation: function of the blocks}}}
SINGLE = {
    'mc': {
        'gen': dict(SIZES, **dict(MODELS, **{
            'mc NULL': _drop('mc'), 'fs=0': _set('mc.fs', 0.0), 'fs nan': _set('mc.fs', NAN), 'fs inf is legal': _set('mc.fs', INF), 'fs<0': _set('mc.fs', -1.0),
            'ref_frame=2': _set('mc.ref_frame', 2), 'proc_plain_sums=2': _set('mc.proc_plain_sums', 2), 'algo_mask=4': _set('mc.algo_mask', 4),
            'algo_mask=-1': _set('mc.algo_mask', -1), 'algo_mask=0 no outputs': _set('mc.algo_mask', 0),
            'n_ini=0': _set('mc.n_ini', 0), 'ini NULL': _set('mc.ini', None), 'block_threads=32': _set('mc.block_threads', 32),
            'ref_gyro NULL': _set('mc.ref_gyro', None), 'ref_accel NULL': _set('mc.ref_accel', None),
            'odo without ref_odo': _all(_set('mc.algo_mask', 2), _set('mc.ref_odo', None)),
            'out_odo without ref_odo': _all(_ptr('mc.out_odo'), _set('mc.ref_odo', None)),
            'vib_accel type 4': _set('mc.vib_accel.type', 4), 'vib_gyro type -1': _set('mc.vib_gyro.type', -1),
            'psd without series': _all(_set('mc.vib_accel.type', 3), _set('mc.vib_accel.period', 16)),
            'psd period 1': _all(_set('mc.vib_gyro.type', 3), _ptr('mc.vib_gyro.series'), _set('mc.vib_gyro.period', 1)),
            'psd period 16385': _all(_set('mc.vib_gyro.type', 3), _ptr('mc.vib_gyro.series'), _set('mc.vib_gyro.period', 16385)),
            'psd fp32': _all(_set('mc.vib_accel.type', 3), _ptr('mc.vib_accel.series'), _set('mc.vib_accel.period', 16), _set('mc.precision', 1)),
            'psd sensor_layout 1': _all(_set('mc.vib_accel.type', 3), _ptr('mc.vib_accel.series'), _set('mc.vib_accel.period', 16),
                                        _set('mc.sensor_layout', 1)),
            'vib_accel amp nan': VIB['vib_accel amp nan'], 'vib_gyro omega_dt inf': VIB['vib_gyro omega_dt inf'],
            'precision=2': _set('mc.precision', 2), 'sensor_layout=2': _set('mc.sensor_layout', 2), 'sensor_layout=1 off the series path': _set('mc.sensor_layout', 1),
            'out_proc fp32': _all(_ptr('mc.out_proc', 0), _ptr('mc.ref_nav'), _set('mc.precision', 1)),
            'out_proc two algorithms': _all(_ptr('mc.out_proc', 0), _ptr('mc.ref_nav'), _set('mc.algo_mask', 3)),
            'out_proc of the other algorithm': _all(_ptr('mc.out_proc', 1), _ptr('mc.ref_nav')),
            'out_proc without ref_nav': _ptr('mc.out_proc', 0),
            'proc_first=-1': _all(_ptr('mc.out_proc', 0), _ptr('mc.ref_nav'), _set('mc.proc_first', -1)),
            'proc_first=n': _all(_ptr('mc.out_proc', 0), _ptr('mc.ref_nav'), _set('mc.proc_first', N)),
            'proc_pos_ned ref_frame 1': _all(_ptr('mc.out_proc', 0), _ptr('mc.ref_nav'), _set('mc.proc_pos_ned', 1), _set('mc.ref_frame', 1)),
            'out_end_ned ref_frame 1': _all(_ptr('mc.out_end_ned', 0), _set('mc.ref_frame', 1)),
            'out_end_ned fp32': _all(_ptr('mc.out_end_ned', 1), _set('mc.precision', 1)),
            'fp32 sensors only': _all(_set('mc.precision', 1), _set('mc.algo_mask', 0), _ptr('mc.out_accel')),
            'fp32 wave_trace': _all(_set('mc.precision', 1), _ptr('mc.wave_trace')),
            'fp32 block_threads=128': _all(_set('mc.precision', 1), _set('mc.block_threads', 128)),
        })),
        'given': {
            'in_gyro NULL': _set('mc.in_gyro', None), 'free without in_accel': _set('mc.in_accel', None),
            'odo without in_odo': _all(_set('mc.algo_mask', 2), _set('mc.in_odo', None)),
            'in_accel NULL is legal for odo': _all(_set('mc.algo_mask', 2), _set('mc.in_accel', None)),
            'algo_mask=0': _all(_set('mc.algo_mask', 0), _ptr('mc.out_accel')), 'vib_accel random': _set('mc.vib_accel.type', 1),
            'out_proc': _all(_ptr('mc.out_proc', 0), _ptr('mc.ref_nav')), 'out_end_ned': _ptr('mc.out_end_ned', 0),
            'accel.bias nan is not read': _set('mc.accel.bias', NAN, 0),
        },
    },
    'incl': {
        'gen': dict(SIZES, **dict(VIB, **dict(MODELS, **{
            'mc NULL': _drop('mc'), 'p NULL': _drop('p'), 'algo_mask=0': _set('p.algo_mask', 0), 'algo_mask=4': _set('p.algo_mask', 4),
            'n_list=-1': _set('p.n_list', -1), 'n_list=runs+1': _set('p.n_list', RUNS + 1), 'mahony without bias_in': _set('p.bias_in', None),
            'tilt without bias_in is legal': _all(_set('p.algo_mask', 2), _set('p.bias_in', None)),
            'dt=0': _set('p.dt', 0.0), 'dt nan': _set('p.dt', NAN), 'dt inf': _set('p.dt', INF), 'block_threads=32': _set('mc.block_threads', 32),
            'precision=1': _set('mc.precision', 1), 'ref_gyro NULL': _set('mc.ref_gyro', None), 'ref_accel NULL': _set('mc.ref_accel', None),
            'out_end without ref_nav': _ptr('p.out_end', 0), 'out_proc without ref_nav': _ptr('p.out_proc', 1),
            'proc_first=-1': _all(_ptr('p.out_end', 0), _ptr('mc.ref_nav'), _set('mc.proc_first', -1)),
            'proc_first=-1 without statistics is legal': _set('mc.proc_first', -1),
            'out_wb without mahony': _all(_set('p.algo_mask', 2), _ptr('p.out_wb')),
            'out_end[0] without mahony': _all(_set('p.algo_mask', 2), _ptr('p.out_end', 0), _ptr('mc.ref_nav')),
            'out_quat[1] without tilt': _all(_set('p.algo_mask', 1), _ptr('p.out_quat', 1)),
            'out_proc[1] without tilt': _all(_set('p.algo_mask', 1), _ptr('p.out_proc', 1), _ptr('mc.ref_nav')),
            'fs is not read': _set('mc.fs', NAN),
        }))),
        'given': {
            'in_accel NULL': _set('mc.in_accel', None), 'in_gyro NULL': _set('mc.in_gyro', None), 'vib_accel random': _set('mc.vib_accel.type', 1),
            'vib_gyro psd': _set('mc.vib_gyro.type', 3), 'accel.bias nan is not read': _set('mc.accel.bias', NAN, 0),
        },
    },
    'loose': {
        'gen': dict(SIZES, **dict(VIB, **dict(MODELS, **{
            'mc NULL': _drop('mc'), 'p NULL': _drop('p'), 'fs=0': _set('mc.fs', 0.0), 'fs nan': _set('mc.fs', NAN), 'fs inf': _set('mc.fs', INF),
            'ref_frame=2': _set('mc.ref_frame', 2), 'precision=1': _set('mc.precision', 1), 'n_ini=0': _set('mc.n_ini', 0), 'ini NULL': _set('mc.ini', None),
            'block_threads=128': _set('mc.block_threads', 128), 'block_threads=64 is legal': _set('mc.block_threads', 64),
            'n_list=-1': _set('p.n_list', -1), 'n_list=runs+1': _set('p.n_list', RUNS + 1), 'm=-1': _set('p.m', -1), 'm=n+1': _set('p.m', N + 1),
            'gps_stamp NULL': _set('p.gps_stamp', None), 'stamp -1': _stamp('stamps', 0, -1), 'stamp n': _stamp('stamps', 2, N),
            'stamps repeat': _stamp('stamps', 1, 0), 'stamps fall': _stamp('stamps', 2, 5),
            'ref_gyro NULL': _set('mc.ref_gyro', None), 'ref_accel NULL': _set('mc.ref_accel', None), 'ref_gps NULL': _set('p.ref_gps', None),
            'ref_gps NULL without fixes is legal': _all(_set('p.ref_gps', None), _set('p.m', 0)),
            'gps_sigma nan': _set('p.gps_sigma', NAN, 3), 'gps_sigma inf': _set('p.gps_sigma', INF, 0),
            'r_diag=0': _set('p.r_diag', 0.0, 2), 'r_diag nan': _set('p.r_diag', NAN, 5), 'p0=0': _set('p.p0', 0.0, 4), 'p0 inf': _set('p.p0', INF, 0),
            'q_v<0': _set('p.q_v', -1.0, 0), 'q_psi nan': _set('p.q_psi', NAN, 1), 'q_bg inf': _set('p.q_bg', INF, 2), 'q_ba<0': _set('p.q_ba', -1e-300, 1),
            'decay_g nan': _set('p.decay_g', NAN, 0), 'decay_a inf': _set('p.decay_a', INF, 2),
            'out_proc without ref_nav': _ptr('p.out_proc'), 'proc_first=-1': _all(_ptr('p.out_proc'), _ptr('mc.ref_nav'), _set('mc.proc_first', -1)),
            'proc_first=n': _all(_ptr('p.out_proc'), _ptr('mc.ref_nav'), _set('mc.proc_first', N)),
            'proc_pos_ned ref_frame 1': _all(_set('mc.proc_pos_ned', 1), _set('mc.ref_frame', 1)),
            'out_end_ned ref_frame 1': _all(_ptr('p.out_end_ned'), _set('mc.ref_frame', 1)),
            'aid_mask=-1': _set('p.aid_mask', -1), 'aid_mask=8': _set('p.aid_mask', 8), 'aid_every=0': _all(_set('p.aid_mask', 6), _set('p.r_nhc', 0.01)),
            'r_nhc=0': _all(_set('p.aid_mask', 6), _set('p.aid_every', 1)),
            'r_odo=0': _all(_set('p.aid_mask', 1), _set('p.aid_every', 1), _set('p.odo_scale_f', 1.0)),
            'odo_scale_f nan': _all(_set('p.aid_mask', 1), _set('p.aid_every', 1), _set('p.r_odo', 0.01), _set('p.odo_scale_f', NAN)),
            'odo without ref_odo': _all(_set('p.aid_mask', 1), _set('p.aid_every', 1), _set('p.r_odo', 0.01), _set('p.odo_scale_f', 1.0), _set('mc.ref_odo', None)),
            'odo_scale nan': _all(_set('p.aid_mask', 1), _set('p.aid_every', 1), _set('p.r_odo', 0.01), _set('p.odo_scale_f', 1.0), _set('mc.odo_scale', NAN)),
            'odo_stdv inf': _all(_set('p.aid_mask', 1), _set('p.aid_every', 1), _set('p.r_odo', 0.01), _set('p.odo_scale_f', 1.0), _set('mc.odo_stdv', INF)),
        }))),
        'given': {
            'in_accel NULL': _set('mc.in_accel', None), 'in_gyro NULL': _set('mc.in_gyro', None), 'in_gps NULL': _set('p.in_gps', None),
            'in_gps NULL without fixes is legal': _all(_set('p.in_gps', None), _set('p.m', 0)), 'vib_gyro sinusoidal': _set('mc.vib_gyro.type', 2),
            'vib_accel psd': _set('mc.vib_accel.type', 3), 'gps_sigma nan is not read': _set('p.gps_sigma', NAN, 0),
            'gyro.white nan is not read': _set('mc.gyro.white', NAN, 1),
            'odo without in_odo': _all(_set('p.aid_mask', 1), _set('p.aid_every', 1), _set('p.r_odo', 0.01), _set('p.odo_scale_f', 1.0), _set('mc.in_odo', None)),
            'odo_scale nan is not read': _all(_set('p.aid_mask', 1), _set('p.aid_every', 1), _set('p.r_odo', 0.01), _set('p.odo_scale_f', 1.0), _set('mc.odo_scale', NAN)),
        },
    },
    'cons': {
        'gen': {
            'q NULL': _drop('q'), 'cons_m=-1': _set('q.cons_m', -1), 'cons_m=n+1': _set('q.cons_m', N + 1), 'cons_m=0 is the plain launch': _set('q.cons_m', 0),
            'cons_m=0 reads nothing else': _all(_set('q.cons_m', 0), _set('q.cons_sample', None), _set('mc.ref_nav', None)),
            'cons_sample NULL': _set('q.cons_sample', None), 'out_cons NULL': _set('q.out_cons', None), 'cons_work NULL': _set('q.cons_work', None),
            'ref_nav NULL': _set('mc.ref_nav', None), 'out_proc': _ptr('p.out_proc'), 'checkpoint -1': _stamp('samples', 0, -1),
            'checkpoint n': _stamp('samples', 2, N), 'checkpoints repeat': _stamp('samples', 1, 5), 'checkpoints fall': _stamp('samples', 2, 7),
            'runs=0': SIZES['runs=0'], 'ref_gps NULL': _set('p.ref_gps', None), 'vib_accel psd': VIB['vib_accel psd'], 'aid_mask=8': _set('p.aid_mask', 8),
        },
        'given': {'in_gps NULL': _set('p.in_gps', None), 'checkpoint n': _stamp('samples', 2, N)},
    },
    'mag': {
        'gen': {
            'q NULL': _drop('q'), 'mag_every=-1': _set('q.mag_every', -1), 'mag_every=0 is legal: the plain launch': _set('q.mag_every', 0),
            'mag_every=0 is legal: the aided launch': _all(_set('q.mag_every', 0), _set('p.aid_mask', 6), _set('p.aid_every', 1), _set('p.r_nhc', 0.0025)),
            'mag_every=0 is legal and reads nothing else': _all(_set('q.mag_every', 0), _set('q.ref_mag', None), _set('q.r_mag', 0.0, 0), _set('q.mag_n', NAN, 1)),
            'ref_mag NULL': _set('q.ref_mag', None), 'mag_si nan': _set('q.mag_si', NAN, 4), 'mag_hi inf': _set('q.mag_hi', INF, 2),
            'mag_std nan': _set('q.mag_std', NAN, 0), 'cal_si inf': _set('q.cal_si', INF, 8), 'mag_n nan': _set('q.mag_n', NAN, 1),
            'cal_hi -inf': _set('q.cal_hi', -INF, 0), 'r_mag=0': _set('q.r_mag', 0.0, 1), 'r_mag nan': _set('q.r_mag', NAN, 2),
            'mag_n zero': _all(_set('q.mag_n', 0.0, 0), _set('q.mag_n', 0.0, 1), _set('q.mag_n', 0.0, 2)),
            'runs=0': SIZES['runs=0'], 'ref_gps NULL': _set('p.ref_gps', None), 'vib_accel psd': VIB['vib_accel psd'], 'aid_mask=8': _set('p.aid_mask', 8),
        },
        'given': {
            'in_mag NULL': _set('q.in_mag', None), 'ref_mag NULL is legal': _set('q.ref_mag', None), 'mag_si nan is not read': _set('q.mag_si', NAN, 0),
            'mag_std inf is not read': _set('q.mag_std', INF, 1), 'cal_si nan': _set('q.cal_si', NAN, 0), 'r_mag=0': _set('q.r_mag', 0.0, 0),
            'in_gps NULL': _set('p.in_gps', None),
        },
    },
    'scale': {
        'gen': {
            'q NULL': _drop('q'), 'aid_mask without bit 0': _all(_set('p.aid_mask', 6), _set('p.r_nhc', 0.0025)), 'aid_mask=0': _set('p.aid_mask', 0),
            'scale0=0': _set('q.scale0', 0.0), 'scale0 nan': _set('q.scale0', NAN), 'scale0 inf': _set('q.scale0', INF),
            'p0_scale<0': _set('q.p0_scale', -1e-300), 'p0_scale inf': _set('q.p0_scale', INF), 'p0_scale=0 is legal': _set('q.p0_scale', 0.0),
            'q_k<0': _set('q.q_k', -1.0), 'q_k nan': _set('q.q_k', NAN), 'q_k>0 is legal': _set('q.q_k', 1e-8),
            'runs=0': SIZES['runs=0'], 'vib_accel psd': VIB['vib_accel psd'], 'aid_mask=8': _set('p.aid_mask', 8), 'r_odo=0': _set('p.r_odo', 0.0),
            'odo without ref_odo': _set('mc.ref_odo', None), 'precision=1': _set('mc.precision', 1),
        },
        'given': {'odo without in_odo': _set('mc.in_odo', None), 'scale0 nan': _set('q.scale0', NAN), 'in_gps NULL': _set('p.in_gps', None)},
    },
}

# two violations at once: the message is that of the check that comes first
PAIRS = [
    # inside the sizes, and the sizes before what follows them
    ('mc', 'gen', 'n=2^32', 'runs too many'), ('mc', 'gen', 'runs too many', 'fs=0'), ('mc', 'gen', 'n=0', 'ref_gyro NULL'),
    ('incl', 'gen', 'n=2^32', 'runs too many'), ('incl', 'gen', 'runs too many', 'algo_mask=0'), ('incl', 'gen', 'runs=0', 'ref_gyro NULL'),
    ('incl', 'given', 'in_accel NULL', 'vib_accel random'),
    ('loose', 'gen', 'n=2^32', 'runs too many'), ('loose', 'gen', 'runs too many', 'fs nan'), ('loose', 'gen', 'n=0', 'ref_gps NULL'),
    # what precedes the sensor source, before it
    ('mc', 'gen', 'block_threads=32', 'ref_gyro NULL'), ('incl', 'gen', 'precision=1', 'ref_accel NULL'), ('loose', 'gen', 'stamps fall', 'ref_gyro NULL'),
    # inside the sensor source
    ('incl', 'gen', 'ref_gyro NULL', 'accel.bias nan'), ('incl', 'gen', 'accel.gm_a inf', 'gyro.gm_b nan'),
    ('loose', 'gen', 'ref_accel NULL', 'ref_gps NULL'), ('loose', 'gen', 'ref_gps NULL', 'accel.bias nan'), ('loose', 'gen', 'accel.gm_a inf', 'gyro.gm_b nan'),
    ('loose', 'gen', 'gyro.white -inf', 'gps_sigma nan'), ('loose', 'given', 'in_gyro NULL', 'in_gps NULL'),
    ('mc', 'gen', 'ref_accel NULL', 'odo without ref_odo'), ('mc', 'gen', 'out_odo without ref_odo', 'accel.bias nan'),
    # the sensor source before the vibration
    ('mc', 'gen', 'gyro.gm_b nan', 'vib_accel type 4'), ('incl', 'gen', 'gyro.white -inf', 'vib_accel psd'), ('incl', 'gen', 'ref_accel NULL', 'vib_gyro type 9'),
    ('loose', 'gen', 'gps_sigma inf', 'vib_accel psd'), ('loose', 'gen', 'ref_gps NULL', 'vib_accel amp nan'), ('loose', 'given', 'in_gps NULL', 'vib_gyro sinusoidal'),
    ('loose', 'given', 'in_accel NULL', 'vib_accel psd'),
    # inside the vibration block: the accelerometer's term before the gyroscope's, the type before the values
    ('incl', 'gen', 'vib_accel amp nan', 'vib_gyro type 9'), ('loose', 'gen', 'vib_accel amp nan', 'vib_gyro type 9'),
    ('incl', 'given', 'vib_gyro psd', 'vib_accel random'), ('loose', 'given', 'vib_accel psd', 'vib_gyro sinusoidal'),
    # the vibration before what follows it
    ('mc', 'gen', 'vib_gyro omega_dt inf', 'precision=2'), ('incl', 'gen', 'vib_gyro omega_dt inf', 'out_end without ref_nav'),
    ('incl', 'gen', 'vib_accel psd', 'out_wb without mahony'), ('loose', 'gen', 'vib_gyro omega_dt inf', 'r_diag=0'), ('loose', 'gen', 'vib_gyro type 9', 'aid_mask=8'),
    ('loose', 'given', 'vib_gyro sinusoidal', 'odo without in_odo'),
    # the filter's block before the magnetometer's, and the order inside the magnetometer's
    ('mag', 'gen', 'aid_mask=8', 'mag_every=-1'), ('mag', 'gen', 'vib_accel psd', 'q NULL'), ('mag', 'gen', 'runs=0', 'ref_mag NULL'),
    ('mag', 'gen', 'ref_gps NULL', 'r_mag=0'), ('mag', 'given', 'in_gps NULL', 'in_mag NULL'), ('mag', 'gen', 'ref_mag NULL', 'mag_si nan'),
    ('mag', 'gen', 'mag_hi inf', 'cal_si inf'), ('mag', 'gen', 'cal_si inf', 'mag_n nan'), ('mag', 'gen', 'r_mag=0', 'mag_n zero'),
    ('mag', 'given', 'in_mag NULL', 'cal_si nan'),
    # the filter's block before the scale-factor state's, and the order inside the state's
    ('scale', 'gen', 'aid_mask=8', 'scale0=0'), ('scale', 'gen', 'vib_accel psd', 'q NULL'), ('scale', 'gen', 'r_odo=0', 'q_k<0'),
    ('scale', 'gen', 'precision=1', 'p0_scale inf'), ('scale', 'given', 'odo without in_odo', 'scale0 nan'),
    ('scale', 'gen', 'aid_mask without bit 0', 'scale0 nan'), ('scale', 'gen', 'scale0=0', 'p0_scale<0'), ('scale', 'gen', 'p0_scale inf', 'q_k nan'),
    # the filter's block before the checkpoints'
    ('cons', 'gen', 'aid_mask=8', 'cons_m=-1'), ('cons', 'gen', 'vib_accel psd', 'q NULL'), ('cons', 'gen', 'ref_nav NULL', 'out_proc'),
    ('cons', 'gen', 'cons_work NULL', 'ref_nav NULL'), ('cons', 'given', 'in_gps NULL', 'checkpoint n'),
]


def _cases():
    out = {}
    for entry, forms in SINGLE.items():
        for form, table in forms.items():
            out['%s %s: valid' % (entry, form)] = (entry, form, [])
            for what, fn in table.items():
                out['%s %s: %s' % (entry, form, what)] = (entry, form, [fn])
    for entry, form, a, b in PAIRS:
        out['%s %s: %s + %s' % (entry, form, a, b)] = (entry, form, [SINGLE[entry][form][a], SINGLE[entry][form][b]])
    return out


CASES = _cases()


def outcome(name):
    entry, form, fns = CASES[name]
    b = Blocks(entry, form == 'given')
    for f in fns:
        f(b)
    return b.name()


def test_fixture_lists_every_case():
    """GINSIM_RECORD_REFUSALS=1: write the fixture (at the commit it characterises, once); otherwise only check it is complete."""
    if os.environ.get('GINSIM_RECORD_REFUSALS') == '1':
        with open(FIXTURE, 'w') as f:
            f.write('{\n' + ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(outcome(k))) for k in CASES) + '\n}\n')
    with open(FIXTURE) as f:
        assert sorted(json.load(f)) == sorted(CASES)


@pytest.fixture(scope='module')
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize('name', list(CASES))
def test_refusal_is_the_recorded_one(name, recorded):
    assert outcome(name) == recorded[name]


def test_every_refusal_is_an_argument_error_with_its_entry_point_s_prefix(recorded):
    """What the fixture itself must look like: a legal block names a kernel, a refused one returns GINSIM_ERR_ARG and says who."""
    from ginsim import _lib as L
    refused = 0
    for name, (rc, text) in recorded.items():
        if name.endswith('valid') or 'legal' in name or 'not read' in name or 'cons_m=0' in name:
            assert rc == L.OK and text.startswith('ginsim::'), name
        else:
            assert rc == L.ERR_ARG and text.split(':')[0] in ('mc_kernel_name', 'mc_run', 'incl_run', 'loose_run', 'loose_cons_run', 'loose_mag_run',
                                                               'loose_scale_run'), name
            refused += 1
    assert refused >= 150


# ------------------------------------------------------------------------------------------------- the loose family's dispatch
TF = {False: 'false', True: 'true'}


@pytest.mark.parametrize('rf, source, flag, kind', list(itertools.product((0, 1), ('gen', 'vib', 'given'), (False, True),
                                                                          ('plain', 'aided', 'cons', 'mag', 'scale'))))
def test_loose_family_dispatch(rf, source, flag, kind):
    """60 names: <RF, GIVEN, VIB, F> with F = online process statistics (out_proc) for loose_kernel, loose_aided_kernel (aid_mask
    != 0), loose_mag_kernel (mag_every > 0) and loose_scale_kernel, F = aiding for loose_cons_kernel (cons_m > 0)."""
    b = Blocks(kind if kind in ('cons', 'mag', 'scale') else 'loose', source == 'given')
    b.mc.ref_frame = rf
    if source == 'vib':
        b.mc.vib_gyro.type = 1
    aided = kind == 'aided' or (kind == 'cons' and flag)
    if aided:
        b.p.aid_mask, b.p.aid_every, b.p.r_nhc = 6, 3, 0.0025
    if kind != 'cons' and flag:
        b.p.out_proc, b.mc.ref_nav = b.d, b.d
    kernel = {'plain': 'loose_kernel', 'aided': 'loose_aided_kernel', 'cons': 'loose_cons_kernel', 'mag': 'loose_mag_kernel',
              'scale': 'loose_scale_kernel'}[kind]
    want = 'ginsim::%s<%d, %s, %s, %s>' % (kernel, rf, TF[source == 'given'], TF[source == 'vib'], TF[flag])
    assert b.name() == [0, want]
