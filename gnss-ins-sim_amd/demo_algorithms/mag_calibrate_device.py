"""The reference's soft / hard-iron magnetometer calibration on the GPU: ``MagCal`` (demo_algorithms/mag_calibrate.py) with the
same ``input`` / ``output`` / ``batch`` and ``run`` / ``get_results`` / ``reset``.

The reference's ``run`` stops at six ``input()`` prompts for the row ranges of the rotations about x, y and z, then calls its C
library once; ``MagCal(segments=((x0, xf), (y0, yf), (z0, zf)))`` takes the ranges as an argument instead.  ``Sim`` runs an
instance (``mc_algo`` 'magcal') over all Monte-Carlo runs in one launch of the calibration kernel (csrc/magcal.hip,
ginsim.MagCalJob), which makes every run's magnetometer samples itself; with ``segments=None`` the ranges come from the true
angular rate (segments_from_truth).  ``run([mag])`` on one (n, 3) array runs the same kernel on that series and needs the ranges.
The checkout's own class (demo_algorithms.mag_calibrate) stays hosted.

The algorithm fixes the x sensitivity at 1: ``soft_iron`` estimates inv(si) up to one common factor, and ``hard_iron[:3]`` is hi
times that factor.  fp64 only.
"""
import numpy as np

VERSION = '1.0'


def segments_from_truth(ref_gyro, hold=0.5, quiet=0.1):
    """The row ranges of the rotations about x, y and z from the true angular rate (n, 3): for axis a the longest stretch of
    consecutive samples with |w_a| >= hold * max|w_a| while both other |w| < quiet * max|w_a|.  ValueError when an axis never
    rotates alone."""
    w = np.abs(np.asarray(ref_gyro, dtype=np.float64))
    if w.ndim != 2 or w.shape[1] != 3:
        raise ValueError('ref_gyro must be an (n, 3) array')
    out = []
    for a in range(3):
        top = w[:, a].max()
        others = [k for k in range(3) if k != a]
        on = (w[:, a] >= hold * top) & (w[:, others[0]] < quiet * top) & (w[:, others[1]] < quiet * top) if top > 0.0 \
            else np.zeros(w.shape[0], dtype=bool)
        edges = np.diff(np.concatenate([[0], on.astype(np.int8), [0]]))
        starts, ends = np.nonzero(edges == 1)[0], np.nonzero(edges == -1)[0]
        if starts.size == 0:
            raise ValueError('segments_from_truth: no rotation about %s alone in this motion: give MagCal(segments=...)' % 'xyz'[a])
        k = int(np.argmax(ends - starts))
        out.append((int(starts[k]), int(ends[k])))
    return tuple(out)


class MagCal(object):
    '''
    Soft iron and hard iron calibration (mag_calibrate.py:21-112), run on the GPU:  mag_calibrated = si * mag_raw - hi.
    segments: ((x0, xf), (y0, yf), (z0, zf)), the rows of `mag` logged while rotating about x, y and z; None: from the truth
    when a Sim runs the plugin.
    '''
    mc_algo = 'magcal'

    def __init__(self, segments=None):
        self.input = ['mag']
        self.output = ['soft_iron', 'hard_iron', 'mag_cal']
        self.batch = True
        self.results = None
        self.segments = None if segments is None else self._shape_of(segments)

    @staticmethod
    def _shape_of(segments):
        from ginsim.magcal import check_segments
        seg = check_segments(segments, np.iinfo(np.int64).max)           # the upper bound is checked against the series at run time
        return tuple((seg[2 * a], seg[2 * a + 1]) for a in range(3))

    def finish(self, soft_iron, hard_iron, mag_cal):
        """State the reference leaves after a run: si (3, 3), hi (1, 4), the calibrated rows (nx + ny + nz, 3)."""
        self.results = [np.array(soft_iron, dtype=np.float64).reshape(3, 3), np.array(hard_iron, dtype=np.float64).reshape(1, 4), mag_cal]

    def run(self, set_of_input):
        '''
        set_of_input: [mag (n, 3)], as the reference's run.  Needs MagCal(segments=...): there is no truth to find them in.
        '''
        import ginsim
        if self.segments is None:
            raise ValueError('MagCal.run on a series needs the row ranges of the three rotations: MagCal(segments=((x0, xf), (y0, yf), (z0, zf)))')
        mag = np.ascontiguousarray(np.asarray(set_of_input[0], dtype=np.float64))
        if mag.ndim != 2 or mag.shape[1] != 3:
            raise ValueError('mag must be an (n, 3) array')
        from ginsim.magcal import check_segments
        check_segments(self.segments, mag.shape[0])
        ctx = ginsim.default_context()
        given = ctx.upload(np.ascontiguousarray(mag.T))                  # [3][n][1]
        job = None
        try:
            job = ginsim.MagCalJob(ctx, None, None, 1, self.segments, given=given, keep=True, n=mag.shape[0]).run()
            self.finish(job.soft_iron()[0], job.hard_iron()[0], job.mag_cal([0])[0])
        finally:
            if job is not None:
                job.release()
            given.free()

    def get_results(self):
        return self.results

    def reset(self):
        pass
