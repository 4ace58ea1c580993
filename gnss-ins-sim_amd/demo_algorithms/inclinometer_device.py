"""The reference's inclinometer plugins on the GPU: ``MahonyFilter`` (demo_algorithms/inclinometer_mahony.py) and ``TiltAcc``
(demo_algorithms/inclinometer_acc.py) with the same constructor, attributes, ``input`` / ``output`` / ``batch`` and
``run`` / ``get_results`` / ``reset``.

``Sim`` runs instances of these classes (``mc_algo`` 'mahony' / 'tilt') in the inclinometer kernel over all runs at once
(csrc/inclinometer.hip, ginsim.InclinometerJob), with the same seed and run ids as the free-integration kernel, so both see
the same sensors; the chain of a MahonyFilter's runs (run r starts from the gyro_bias run r-1 ended with, because reset()
clears ``ini`` only) is solved exactly by fixed-point passes.  ``run(set_of_input)`` on one record runs the same kernel on the
given sensors.  The checkout's own classes (demo_algorithms.inclinometer_mahony / inclinometer_acc) stay hosted.

Differences from the reference a caller may notice: every ``run`` starts as after ``reset()`` (q and err_int are rebuilt at the
first sample with a non-zero accelerometer); ``err_int`` is not brought back from the device; fp64 only.
"""
import numpy as np

VERSION = '1.0'


def _given_job(fs, gyro, accel, algos, bias, gains=None, dt=None):
    import ginsim
    from ginsim.inclinometer import InclinometerJob
    gyro = np.ascontiguousarray(np.asarray(gyro, dtype=np.float64))
    accel = np.ascontiguousarray(np.asarray(accel, dtype=np.float64))
    if gyro.ndim != 2 or gyro.shape[1] != 3 or accel.shape != gyro.shape:
        raise ValueError('gyro and accel must be (n, 3) arrays of the same length')
    ctx = ginsim.default_context()
    n = accel.shape[0]
    given = {'accel': ctx.upload(np.ascontiguousarray(accel.T)), 'gyro': ctx.upload(np.ascontiguousarray(gyro.T))}    # [3][n][1]
    truth = {'ref_accel': np.zeros((n, 3)), 'ref_gyro': np.zeros((n, 3))}
    job = InclinometerJob(ctx, fs, truth, None, None, 1, algos=algos, gains=gains, dt=dt, start_bias=np.reshape(bias, (1, 3)),
                          given=given, stats=False, keep=True).run()
    return job, given


class MahonyFilter(object):
    '''
    Mahony filter (inclinometer_mahony.py:18-163), run on the GPU.
    '''
    mc_algo = 'mahony'

    def __init__(self):
        self.input = ['fs', 'gyro', 'accel']
        self.output = ['att_quat', 'wb', 'ab']
        self.batch = True
        self.results = None
        self.quat = None
        self.wb = None
        self.ab = None
        self.innovationLimit = 0.1
        self.kp_acc_high = 1
        self.kp_acc_low = 0.01
        self.ki_acc_high = 0.5
        self.ki_acc_low = 0.001
        self.ini = 0
        self.dt = 1.0
        self.q = np.array([1.0, 0.0, 0.0, 0.0])
        self.err_int = np.array([0.0, 0.0, 0.0])
        self.kp_acc = 1
        self.ki_acc = 0.001
        self.gyro_bias = np.array([0.0, 0.0, 0.0])
        self.tmp = np.array([0.0, 0.0, 0.0])

    def gains(self):
        """The launch parameters the public attributes stand for."""
        return dict(kp_high=float(self.kp_acc_high), kp_low=float(self.kp_acc_low), ki_high=float(self.ki_acc_high),
                    ki_low=float(self.ki_acc_low), innovation_limit=float(self.innovationLimit))

    def finish(self, quat, wb, ab, dt):
        """State the reference leaves after a run whose series are quat / wb / ab."""
        self.dt = dt
        self.quat, self.wb, self.ab = quat, wb, ab
        self.q = quat[-1].copy()
        self.gyro_bias = wb[-1].copy()
        self.tmp = ab[-1].copy()
        self.ini = 1

    def run(self, set_of_input):
        '''
        set_of_input: [fs, gyro (n, 3), accel (n, 3)], as the reference's run.
        '''
        dt = 1.0 / set_of_input[0]
        job, _ = _given_job(set_of_input[0], set_of_input[1], set_of_input[2], ('mahony',), self.gyro_bias, self.gains(), dt)
        try:
            self.finish(job.series('quat_mahony', [0])[0], job.series('wb', [0])[0], job.series('ab', [0])[0], dt)
        finally:
            job.release()

    def get_results(self):
        return [self.quat, self.wb, self.ab]

    def reset(self):
        self.ini = 0


class TiltAcc(object):
    '''
    Tilt sensor using only accelerometer (inclinometer_acc.py:17-63), run on the GPU.
    '''
    mc_algo = 'tilt'

    def __init__(self):
        self.name = 'StaticTilt'
        self.input = ['accel']
        self.output = ['att_quat']
        self.batch = True
        self.results = None
        self.ini = 0
        self.q = np.array([1.0, 0.0, 0.0, 0.0])
        self.err_int = np.array([0.0, 0.0, 0.0])
        self.kp_acc = 0.1
        self.ki_acc = 0.001

    def finish(self, quat):
        self.results = quat
        self.q = quat[-1].copy()

    def run(self, set_of_input):
        accel = np.asarray(set_of_input[0], dtype=np.float64)
        job, _ = _given_job(1.0, np.zeros_like(accel), accel, ('tilt',), np.zeros(3))
        try:
            self.finish(job.series('quat_tilt', [0])[0])
        finally:
            job.release()

    def get_results(self):
        return [self.results]

    def reset(self):
        self.ini = 0
