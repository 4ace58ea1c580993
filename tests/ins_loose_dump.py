"""The sensor dump and the comparison helpers of the InsLoose GPU tests (test infrastructure; no test in it, imported by tests only):
tests/test_gpu_ins_loose*.py.  What a kernel family adds is a subclass of Dump with its job / restate / bound in its own test file.

    ctx                                     -> the module-scoped fixture: every test file that imports it opens its own Context
    Dump(ctx, rf, n, runs, ...)             -> the device's own sensors and fixes of `runs` runs, on the device and on the host
    result(job)                             -> the outputs the restatements give, (runs, ...) as InsLooseJob.series returns them
    planes(job)                             -> every output as raw arrays, the run on the last axis of every one
    same_bits(a, b, runs_a, runs_b, keys)   -> assert two planes() equal bit for bit, whole or on the named runs
    held(what, got, bound)                  -> print 'what: k got (bound b), ...' and assert got[k] <= bound[k] for every key of got
"""
import numpy as np
import pytest

import ins_loose_aided_cases as ac
import ins_loose_cases as cs


@pytest.fixture(scope='module')
def ctx():
    import ginsim
    c = ginsim.Context(0)
    yield c
    c.close()


class Dump(object):
    """The device's own accel, gyro and odometer (ginsim_mc_run), fixes and magnetometer (ginsim_aux_sensors) of `runs` runs, on the
    device and on the host.

    n None: the whole profile.  truth_fn: the function that makes (ini, truth, stamps); profile and geo go to it when given.
    odo_err None: no odometer is dumped, and the launch keeps its free-integration trajectories instead.
    gps False: no fix at all (empty ref_gps / gps_time / gps_visibility and stamps; truth_gps keeps the profile's).
    vbx0: the initial forward speed the FILTER starts from (None: the profile's).
    vib: a vibration term of the accelerometer; it is in the dumped samples, and a job of the generated form is told it.
    mag_errs: ((name, mag_err), ...), one magnetometer series mag[name] per model; the fixes come with the first.
    flags: a function of the truth that gives the standstill signal.  **bias: ins_loose_cases.imu_errors'."""

    def __init__(self, ctx, rf, n, runs, seed=77, run_offset=0, fs=20.0, fs_gps=2.0, truth_fn=ac.outage_truth, profile=None, geo=None,
                 odo_err=ac.ODO_ERR, gps=True, vbx0=None, vib=None, mag_errs=(), flags=None, **bias):
        import ginsim
        self.rf, self.fs, self.runs, self.seed, self.run_offset, self.geo, self.vib = rf, fs, runs, seed, run_offset, geo, vib
        where = {}
        if profile is not None:
            where['profile'] = profile
        if geo is not None:
            where['geo'] = geo
        self.ini, truth, self.stamps = truth_fn(fs, rf, fs_gps, n, **where)
        if vbx0 is not None:
            self.ini = np.array(self.ini, dtype=np.float64)
            self.ini[3] = vbx0
        self.truth_gps = truth
        if not gps:
            truth = dict(truth, ref_gps=np.zeros((0, 6)), gps_time=np.zeros(0), gps_visibility=np.zeros(0))
            self.stamps = self.stamps[:0]
        self.truth = truth
        self.n = truth['ref_accel'].shape[0]
        if flags is not None:
            self.flags = flags(truth)
        self.acc_e, self.gyr_e = cs.imu_errors(**bias)
        kw = {'keep_traj': True} if odo_err is None else {'odo_err': odo_err}
        if vib is not None:
            kw['vib_accel'] = vib
        self.mc = ginsim.MonteCarloJob(ctx, fs, rf, truth, self.acc_e, self.gyr_e, self.ini, runs=runs, algos=('free',), seed=seed,
                                       run_offset=run_offset, keep_sensors=True, **kw).run()
        ids = np.arange(runs)
        self.accel, self.gyro = self.mc.sensors('accel', ids), self.mc.sensors('gyro', ids)
        self.given = {'accel': self.mc.buffer('accel'), 'gyro': self.mc.buffer('gyro')}
        if odo_err is not None:
            self.odo = self.mc.sensors('odo', ids)
            self.given['odo'] = self.mc.buffer('odo')
        self.mag_errs = dict(mag_errs)
        self.aux, self.gps, self.mag, self.given_mag = [], None, {}, {}
        aux = dict(seed=seed, run_offset=run_offset, gps_err=cs.GPS_ERR, ref_frame=rf)
        if mag_errs:
            for i, (name, err) in enumerate(mag_errs):
                self.aux.append(ginsim.AuxSensorJob(ctx, runs, ref_gps=truth['ref_gps'] if i == 0 else None, ref_mag=truth['ref_mag'],
                                                    mag_err=err, **aux).run())
                self.mag[name], self.given_mag[name] = self.aux[i].series('mag', ids), self.aux[i].buffer('mag')
        elif gps:
            self.aux.append(ginsim.AuxSensorJob(ctx, runs, ref_gps=truth['ref_gps'], **aux).run())
        if self.aux:                                                            # the fixes come with the first
            self.gps = self.aux[0].series('gps', ids)
            self.given['gps'] = self.aux[0].buffer('gps')
        self.model = ginsim.filter_model(fs, self.acc_e, self.gyr_e, cs.GPS_ERR)

    def job(self, ctx, given=False, truth=None, runs=None, **kw):
        """The InsLooseJob of this dump's case.  given: True for the dumped series, a dict for other buffers, False for the generated
        form.  kw: what the family passes, over the dump's seed and run offset and keep_traj=True."""
        import ginsim
        kw = dict(dict(seed=self.seed, run_offset=self.run_offset, keep_traj=True), **kw)
        if self.vib is not None and not given:
            kw['vib_accel'] = self.vib
        return ginsim.InsLooseJob(ctx, self.fs, self.rf, truth or self.truth, self.acc_e, self.gyr_e, cs.GPS_ERR, self.ini, runs or self.runs,
                                  given=(given if isinstance(given, dict) else self.given) if given else None, **kw)

    def given_with_mag(self, name):
        """The dumped series with the magnetometer series of the model `name`."""
        return dict(self.given, mag=self.given_mag[name])

    def _args(self):
        return (self.rf, self.fs, self.gyro, self.accel, self.ini, self.model, self.gps, self.stamps, self.truth['gps_visibility'])

    def release(self):
        for j in [self.mc] + self.aux:
            j.release()


def result(job):
    ids = np.arange(job.runs)
    out = {k: job.series(k, ids) for k in ('att', 'pos', 'vel', 'wb', 'ab')}
    out['pdiag_end'] = job.final_pdiag()
    if job.scalep is not None:
        k_end, sigma = job.final_scale()
        out['k_est'], out['pcross_end'] = job.series('odo_scale', ids), job.final_pcross()
        out['scale_end'] = job.ctx.download(job.scalep.out_scale_end, (2, job.runs)).T.copy()
        assert np.array_equal(out['scale_end'][:, 0], k_end) and np.array_equal(np.sqrt(out['scale_end'][:, 1]), sigma)
        assert np.array_equal(job.final_sigmas(), np.sqrt(np.concatenate([out['pdiag_end'], out['scale_end'][:, 1:2]], axis=1)))
    return out


def planes(job):
    """Every output of a job as raw arrays (bit comparisons); run is the last axis of every one."""
    R, n = job.runs, job.n
    out = {'traj': job.ctx.download(job.buffer('traj_loose'), (9, n, R)), 'wb': job.ctx.download(job.buffer('wb'), (3, n, R)),
           'ab': job.ctx.download(job.buffer('ab'), (3, n, R)), 'end': job.end_errors().T.copy(), 'pdiag': job.final_pdiag().T.copy(),
           'bias': np.concatenate(job.final_biases(), axis=1).T.copy()}
    if job.scalep is not None:
        out['scale'] = job.ctx.download(job.scalep.out_scale, (n, R))
        out['scale_end'] = job.ctx.download(job.scalep.out_scale_end, (2, R))
        out['pcross'] = job.ctx.download(job.scalep.out_pcross_end, (15, R))
    return out


def same_bits(a, b, runs_a=None, runs_b=None, keys=None):
    """Every key of a (or `keys`) holds the same bits in a and b; runs_a / runs_b: on those runs of a / of b only."""
    for k in a if keys is None else keys:
        x = a[k] if runs_a is None else a[k][..., runs_a]
        y = b[k] if runs_b is None else b[k][..., runs_b]
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64)), k


def held(what, got, bound):
    print(what + ': ' + ', '.join('%s %.2e (bound %.2e)' % (k, got[k], bound[k]) for k in got))
    for k in got:
        assert got[k] <= bound[k], (k, got[k], bound[k])
