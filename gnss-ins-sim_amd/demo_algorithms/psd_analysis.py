"""Power-spectral-density plugin -- Welch's method on the six sensor axes (input ['fs','accel','gyro'], output
['psd_freq','psd_accel','psd_gyro']), the spectral companion of allan_analysis.Allan with the same protocol: the six axes go to
the device as one batch of six series, and inside this package's Sim the plugin is handed the device-resident sensor series of
ALL runs (run_device) and no host copy of them is made.  Densities are single-sided, unit^2 / Hz.  With ``multires=True`` the same
three outputs hold the stitched curve of the decimating octave cascade (ginsim.lpsd): the same estimate at fs, fs/2, fs/4, ..,
each level's best octave, down to the lowest frequency at which ``min_segments`` segments still fit."""
import numpy as np


class Psd(object):
    def __init__(self, nperseg=1024, step=None, window='hann', detrend=True, multires=False, min_segments=1):
        self.nperseg, self.step, self.window, self.detrend = nperseg, step, window, detrend
        self.multires, self.min_segments = bool(multires), min_segments
        self.input = ['fs', 'accel', 'gyro']
        self.output = ['psd_freq', 'psd_accel', 'psd_gyro']
        self.batch = True
        self.results = None

    def run(self, set_of_input):
        import ginsim
        fs, accel, gyro = set_of_input[0], np.asarray(set_of_input[1]), np.asarray(set_of_input[2])
        series = np.concatenate([accel.T, gyro.T], axis=0)                   # (6, n)
        if self.multires:
            p, freq, _ = ginsim.lpsd_host(ginsim.default_context(), series, fs, self.nperseg, self.step, self.window, self.detrend,
                                          self.min_segments)
        else:
            p, freq = ginsim.welch_psd_host(ginsim.default_context(), series, fs, self.nperseg, self.step, self.window, self.detrend)
        self.results = [freq, p[0:3].T.copy(), p[3:6].T.copy()]

    def run_device(self, sensor_job, fs):
        """Device protocol of this package's Sim: all runs of `sensor_job` (a ginsim.MonteCarloJob that kept its sensor
        series) at once.  Returns one [psd_freq, psd_accel, psd_gyro] list per run, in run order."""
        if self.multires:
            freq, p, _ = sensor_job.lpsd(fs, nperseg=self.nperseg, step=self.step, window=self.window, detrend=self.detrend,
                                         min_segments=self.min_segments)
        else:
            freq, p = sensor_job.psd(fs, nperseg=self.nperseg, step=self.step, window=self.window, detrend=self.detrend)
        per_run = [[freq, p['accel'][r], p['gyro'][r]] for r in range(sensor_job.runs)]
        self.results = per_run[-1]
        return per_run

    def get_results(self):
        return self.results

    def reset(self):
        pass
