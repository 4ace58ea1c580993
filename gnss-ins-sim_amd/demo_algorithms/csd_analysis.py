"""Coherence plugin -- Welch's cross-spectral density between the six sensor axes (input ['fs','accel','gyro'], output
['csd_freq','coherence','csd_phase']), the two-series companion of psd_analysis.Psd with the same protocol: on host arrays the six
axes go to the device as one batch of six series, and inside this package's Sim the plugin is handed the device-resident sensor
series of ALL runs (run_device) and no host copy of them is made.  ``pairs`` is a sequence of ((name, axis), (name, axis)) with
name 'accel' or 'gyro' and axis 0..2, x-series and y-series; by default every distinct pair of the six axes, 15 columns in the
order (accel 0, accel 1), (accel 0, accel 2), .., (gyro 1, gyro 2).  coherence is |Pxy|^2 / (Pxx Pyy), csd_phase the angle of Pxy
(of y against x, radians); both are (nfreq, npairs)."""
import numpy as np

NAMES = ('accel', 'gyro')


def default_pairs():
    ends = [(nm, a) for nm in NAMES for a in range(3)]
    return [(ends[i], ends[j]) for i in range(len(ends)) for j in range(i + 1, len(ends))]


class Coherence(object):
    def __init__(self, pairs=None, nperseg=1024, step=None, window='hann', detrend=True):
        self.pairs = pairs
        self.nperseg, self.step, self.window, self.detrend = nperseg, step, window, detrend
        self.input = ['fs', 'accel', 'gyro']
        self.output = ['csd_freq', 'coherence', 'csd_phase']
        self.batch = True
        self.results = None

    def run(self, set_of_input):
        import ginsim
        fs, accel, gyro = set_of_input[0], np.asarray(set_of_input[1]), np.asarray(set_of_input[2])
        series = np.concatenate([accel.T, gyro.T], axis=0)                   # (6, n)
        pairs = default_pairs() if self.pairs is None else self.pairs
        table = [(NAMES.index(a[0]) * 3 + int(a[1]), NAMES.index(b[0]) * 3 + int(b[1])) for a, b in pairs]
        r = ginsim.welch_csd_host(ginsim.default_context(), series, fs, table, self.nperseg, self.step, self.window, self.detrend)
        self.results = [r.freq, r.coherence.T.copy(), r.phase.T.copy()]

    def run_device(self, sensor_job, fs):
        """Device protocol of this package's Sim: all runs of `sensor_job` (a ginsim.MonteCarloJob that kept its sensor
        series) at once.  Returns one [csd_freq, coherence, csd_phase] list per run, in run order."""
        freq, c = sensor_job.csd(fs, self.pairs, NAMES, nperseg=self.nperseg, step=self.step, window=self.window, detrend=self.detrend)
        per_run = [[freq, c['coherence'][r].T.copy(), c['phase'][r].T.copy()] for r in range(sensor_job.runs)]
        self.results = per_run[-1]
        return per_run

    def get_results(self):
        return self.results

    def reset(self):
        pass
