"""CPU: the comparison helpers of the InsLoose GPU tests (tests/ins_loose_dump.py), which every bit comparison and every parity
bound of tests/test_gpu_ins_loose*.py goes through: same_bits and held on small arrays, result and planes on a stand-in job.  No
device and no library."""
import types

import numpy as np
import pytest

from ins_loose_dump import held, planes, result, same_bits

RUNS = 5


def arrays():
    """A planes()-shaped dict: the run on the last axis of every array."""
    rng = np.random.default_rng(7)
    return {'traj': rng.standard_normal((9, 4, RUNS)), 'pdiag': rng.standard_normal((15, RUNS)), 'scale': rng.standard_normal((4, RUNS))}


def copy_of(a):
    return {k: v.copy() for k, v in a.items()}


def bits(x):
    return np.array(x, dtype=np.uint64).view(np.float64)


def differs(a, b, **kw):
    with pytest.raises(AssertionError):
        same_bits(a, b, **kw)


# ------------------------------------------------------------------------------------------------- same_bits
def test_same_bits_sees_one_low_mantissa_bit():
    a = arrays()
    b = copy_of(a)
    same_bits(a, b)
    b['pdiag'][3, 2] = np.nextafter(b['pdiag'][3, 2], np.inf)
    assert np.allclose(a['pdiag'], b['pdiag'], rtol=1e-15, atol=0)
    with pytest.raises(AssertionError, match='pdiag'):
        same_bits(a, b)


def test_same_bits_tells_the_zeros_apart():
    a, b = {'x': np.array([0.0, 1.0])}, {'x': np.array([-0.0, 1.0])}
    assert np.array_equal(a['x'], b['x'])
    differs(a, b)


def test_same_bits_compares_nan_payloads():
    quiet, other = bits([0x7ff8000000000000]), bits([0x7ff8000000000001])
    assert np.isnan(quiet[0]) and np.isnan(other[0])
    same_bits({'x': quiet}, {'x': quiet.copy()})
    differs({'x': quiet}, {'x': other})


def test_same_bits_on_named_runs_only():
    a = arrays()
    b = copy_of(a)
    b['traj'][2, 1, 4] += 1.0                                                  # run 4 of b differs
    differs(a, b)
    same_bits(a, b, runs_a=[0, 2, 3], runs_b=[0, 2, 3])                        # a difference in an unnamed run passes
    differs(a, b, runs_a=[0, 4], runs_b=[0, 4])                                # and one in a named run fails
    small = {k: v[..., :3].copy() for k, v in a.items()}                       # run r of a launch of 3 is run r of the launch of 5
    same_bits(a, small, runs_a=np.arange(3))
    same_bits(small, a, runs_b=np.arange(3))
    differs(a, small, runs_a=np.arange(1, 4))
    shuffled = {k: v[..., ::-1].copy() for k, v in a.items()}
    same_bits(a, shuffled, runs_a=[0, 1], runs_b=[4, 3])


def test_same_bits_takes_a_slice_that_is_not_contiguous():
    a = arrays()
    every_other = {k: v[..., ::2] for k, v in a.items()}
    assert not every_other['traj'].flags['C_CONTIGUOUS']
    same_bits(every_other, {k: v[..., ::2].copy() for k, v in a.items()})
    same_bits(a, every_other, runs_a=slice(0, None, 2))
    differs(every_other, {k: v[..., 1::2] for k, v in a.items()}, runs_a=[0, 1], runs_b=[0, 1])


def test_same_bits_honours_keys_and_misses_no_key():
    a = arrays()
    b = copy_of(a)
    b['scale'][0, 0] = -b['scale'][0, 0]
    differs(a, b)
    same_bits(a, b, keys=('traj', 'pdiag'))
    differs(a, b, keys=('scale',))
    del b['scale']
    with pytest.raises(KeyError):
        same_bits(a, b)
    same_bits(b, a)                                                            # every key of the FIRST is compared


# ------------------------------------------------------------------------------------------------- held
def test_held_prints_the_line_and_holds_every_key(capsys):
    got, bound = {'att': 1.5e-14, 'pos': 2e-13}, {'att': 3e-13, 'pos': 2e-13, 'unused': 0.0}
    held('parity rf1 mask 7', got, bound)
    assert capsys.readouterr().out == 'parity rf1 mask 7: att 1.50e-14 (bound 3.00e-13), pos 2.00e-13 (bound 2.00e-13)\n'
    with pytest.raises(AssertionError, match='pos'):
        held('over', dict(got, pos=np.nextafter(2e-13, 1.0)), bound)
    assert capsys.readouterr().out.startswith('over: att 1.50e-14 (bound 3.00e-13), pos 2.00e-13 (bound')       # printed before it fails
    with pytest.raises(AssertionError, match='att'):
        held('nan', dict(got, att=np.nan), bound)                              # nan <= b is false
    with pytest.raises(KeyError):
        held('no bound', {'vel': 0.0}, bound)


# ------------------------------------------------------------------------------------------------- result, planes on a stand-in job
class Job(object):
    """What result() and planes() ask of an InsLooseJob, on host arrays: `buffers` holds the planes as the device lays them out."""

    def __init__(self, n=4, scale=False):
        rng = np.random.default_rng(11)
        self.runs, self.n, self.ctx = RUNS, n, self
        self.buffers = {'traj_loose': rng.standard_normal((9, n, RUNS)), 'wb': rng.standard_normal((3, n, RUNS)), 'ab': rng.standard_normal((3, n, RUNS))}
        self.end, self.pdiag = rng.standard_normal((RUNS, 9)), rng.random((RUNS, 15))
        self.scalep = None
        if scale:
            self.scalep = types.SimpleNamespace(out_scale='scale', out_scale_end='scale_end', out_pcross_end='pcross')
            self.buffers.update(scale=rng.standard_normal((n, RUNS)), scale_end=rng.random((2, RUNS)), pcross=rng.standard_normal((15, RUNS)))

    def buffer(self, name):
        return name

    def download(self, name, shape):
        assert self.buffers[name].shape == shape
        return self.buffers[name].copy()

    def series(self, key, ids):
        if key == 'odo_scale':
            return self.buffers['scale'].T[ids]
        rows = {'att': slice(0, 3), 'pos': slice(3, 6), 'vel': slice(6, 9)}
        plane = self.buffers[key] if key in ('wb', 'ab') else self.buffers['traj_loose'][rows[key]]
        return plane.transpose(2, 1, 0)[ids]

    def end_errors(self):
        return self.end

    def final_pdiag(self):
        return self.pdiag

    def final_biases(self):
        return self.buffers['wb'][:, -1].T, self.buffers['ab'][:, -1].T

    def final_scale(self):
        return self.buffers['scale_end'][0], np.sqrt(self.buffers['scale_end'][1])

    def final_pcross(self):
        return self.buffers['pcross'].T.copy()

    def final_sigmas(self):
        sig = np.sqrt(self.pdiag)
        return sig if self.scalep is None else np.concatenate([sig, self.final_scale()[1][:, None]], axis=1)


@pytest.mark.parametrize('scale', [False, True], ids=['15 states', '16 states'])
def test_planes_has_the_run_on_the_last_axis_of_every_array(scale):
    job = Job(scale=scale)
    p = planes(job)
    assert set(p) == {'traj', 'wb', 'ab', 'end', 'pdiag', 'bias'} | ({'scale', 'scale_end', 'pcross'} if scale else set())
    assert all(v.shape[-1] == RUNS and v.flags['C_CONTIGUOUS'] for v in p.values())
    r = 3
    assert np.array_equal(p['pdiag'][:, r], job.pdiag[r]) and np.array_equal(p['end'][:, r], job.end[r])
    assert np.array_equal(p['bias'][:, r], np.concatenate([job.buffers['wb'][:, -1, r], job.buffers['ab'][:, -1, r]]))
    assert np.array_equal(p['traj'][..., r], job.buffers['traj_loose'][..., r])
    same_bits(p, planes(job))
    job.pdiag[r, 7] = np.nextafter(job.pdiag[r, 7], 2.0)                       # one run of one job moves: the other runs still agree
    keep = np.setdiff1d(np.arange(RUNS), [r])
    same_bits(p, planes(job), runs_a=keep, runs_b=keep)
    differs(p, planes(job))


def test_result_adds_the_scale_state_and_checks_it_against_the_job():
    assert set(result(Job())) == {'att', 'pos', 'vel', 'wb', 'ab', 'pdiag_end'}
    job = Job(scale=True)
    out = result(job)
    assert set(out) == {'att', 'pos', 'vel', 'wb', 'ab', 'pdiag_end', 'k_est', 'pcross_end', 'scale_end'}
    assert out['att'].shape == (RUNS, 4, 3) and out['k_est'].shape == (RUNS, 4) and out['scale_end'].shape == (RUNS, 2)
    assert np.array_equal(out['scale_end'][:, 0], job.buffers['scale_end'][0])
    job.final_scale = lambda: (job.buffers['scale_end'][0] + 1.0, np.sqrt(job.buffers['scale_end'][1]))
    with pytest.raises(AssertionError):
        result(job)                                                            # the job's own accessor disagrees with its record
