"""Both sides of every size at which the library changes kernel, LDS split, grid shape or address width; BASELINE config 4 at
its full 1 048 576 runs; and the statistics of non-finite errors and of attitude errors on the -pi / +pi boundary.

Every threshold case asserts the kernel that ran (job.kernel_name()), so that a retuned threshold cannot quietly turn a case into
a test of the other kernel.  The only references are the oracles (C, NumPy, float C) and exact sums over the same doubles.
"""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    import ginsim
    c = ginsim.Context(0)
    yield c
    c.close()


def _blocks(R, width=88):
    """first / middle / last block of a launch; the last one ends at run R - 1 (the highest addresses)"""
    width = min(width, R)
    return sorted({(0, width), (max(R // 2 - width // 2 - 5, 0), width), (R - width, width)})


def _cut(truth, n):
    return {k: (v[:n] if hasattr(v, 'shape') and v.shape and v.shape[0] >= n else v) for k, v in truth.items()}


# ----------------------------------------------------------------------------------------------------------- A1 fp64 1024 wavefronts
@pytest.mark.parametrize('R', [65535, 65536, 65537])
@pytest.mark.parametrize('rf', [0, 1])
def test_fp64_split_and_plain_kernels_around_1024_wavefronts(ctx, R, rf):
    """mc_variant: one algorithm on ref_frame 0 runs the wave-specialised kernel up to 1024 wavefronts of runs and the plain one
    above; ref_frame 1 stays wave-specialised but changes its LDS split per CU.  Sampled runs vs the C oracle, sensors,
    trajectories and the end-point record."""
    import ginsim
    from ginsim import workloads
    from oracle import c_oracle
    fs, seed, off = 100.0, 4242, 3 * R + 11
    ini, truth, _ = workloads.truth_from_profile('turn_90deg', fs, rf)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    job = ginsim.MonteCarloJob(ctx, fs, rf, truth, acc, gyr, ini, runs=R, seed=seed, run_offset=off, keep_sensors=True,
                               keep_traj=True)
    split = 'split' in job.kernel_name()
    assert split == (rf == 1 or (R + 63) // 64 <= 1024), job.kernel_name()
    job.run()
    dev_end = job.end_errors('free')
    for first, count in _blocks(R):
        ids = np.arange(first, first + count)
        end, traj, sens = c_oracle.mc_run(seed, off + first, count, fs, rf, truth, acc, gyr, ini, keep=count)
        att, pos, vel = job.trajectories('free', ids)
        d_att = np.abs(np.mod(att - traj[:, :, 0:3] + np.pi, 2 * np.pi) - np.pi).max()
        d_vel = np.abs(vel - traj[:, :, 6:9]).max()
        if rf == 1:
            d_pos = np.abs(pos - traj[:, :, 3:6]).max()
            assert d_pos <= 2e-8, (first, d_pos)
        else:
            np.testing.assert_allclose(pos[:, :, 0:2], traj[:, :, 3:5], rtol=0, atol=1e-12)
            np.testing.assert_allclose(pos[:, :, 2], traj[:, :, 5], rtol=0, atol=1e-8)
        assert d_att <= 1e-9 and d_vel <= 1e-9, (first, d_att, d_vel)
        np.testing.assert_allclose(job.sensors('accel', ids), sens[:, :, 0:3], rtol=0, atol=1e-12)
        np.testing.assert_allclose(job.sensors('gyro', ids), sens[:, :, 3:6], rtol=0, atol=1e-14)
        d_end = np.abs(np.mod(dev_end[ids, :3] - end[:, :3] + np.pi, 2 * np.pi) - np.pi).max()
        assert d_end <= 1e-9
        np.testing.assert_allclose(dev_end[ids, 3:6], end[:, 3:6], rtol=1e-12 if rf == 0 else 0, atol=2e-8)
        np.testing.assert_allclose(dev_end[ids, 6:9], end[:, 6:9], rtol=0, atol=1e-9)
    job.release()


# ------------------------------------------------------------------------------------------------------ A2 fp32 32-bit descriptors
@pytest.mark.parametrize('R,n', [(65536, 5461), (65536, 5462), (65535, 5461), (65535, 5462), (262144, 1365), (262144, 1366)])
def test_fp32_wave_specialised_kernel_at_the_32_bit_offset_limit(ctx, R, n):
    """mc_variant_f32 keeps the wave-specialised kernel (three float planes per buffer descriptor, 32-bit byte offsets) only while
    12 n R < 2^32.  Everything kept; the sampled runs (the last one is run R - 1 at sample n - 1, the top of every descriptor)
    must equal the float oracle bit for bit in all nine trajectory components and both sensors."""
    import ginsim
    from ginsim import workloads
    from oracle import c_oracle
    fs, rf, seed, off = 200.0, 1, 777, 5 * R + 3
    ini, truth, _ = workloads.truth_from_profile('long_drive', fs, rf)
    t = _cut(truth, n)
    assert t['ref_accel'].shape[0] == n
    acc, gyr = workloads.imu_grade('mid-accuracy')
    job = ginsim.MonteCarloJob(ctx, fs, rf, t, acc, gyr, ini, runs=R, seed=seed, run_offset=off, keep_sensors=True,
                               keep_traj=True, precision='f32')
    split = 'split' in job.kernel_name()
    assert split == (12 * n * R < 2 ** 32), job.kernel_name()
    job.run()
    for first, count in _blocks(R, width=64):
        ids = np.arange(first, first + count)
        _, traj32, sens32, _ = c_oracle.mc_run_f32(seed, off + first, count, fs, rf, t, acc, gyr, ini, keep=count)
        att, dpos, vel = job.trajectories('free', ids, displacement=True)
        dev = np.concatenate([att, dpos, vel], axis=2).astype(np.float32)
        for c in range(9):
            assert np.array_equal(dev[:, :, c], traj32[:, :, c]), (first, c)
        assert np.array_equal(job.sensors('accel', ids).astype(np.float32), sens32[:, :, 0:3]), first
        assert np.array_equal(job.sensors('gyro', ids).astype(np.float32), sens32[:, :, 3:6]), first
    job.release()
    ctx.release_pool()


# ------------------------------------------------------------------------------------------------ A3 time-parallel sensor series
@pytest.mark.parametrize('runs,n,series,white_drift', [(1024, 2048, True, False), (1, 2048, True, False),
                                                       (1025, 2048, False, False), (1, 2047, False, False),
                                                       (1, 2048, True, True), (1, 8388609, True, False)])
def test_time_parallel_series_thresholds(ctx, runs, n, series, white_drift):
    """series_path_applies: runs <= 1024 and n >= 2048; chunk length 256..8192.  n = 8 388 609 gives L = 8192 and 1025 chunks
    in one run, past the 1024-chunks-per-run walk.  Sampled runs vs the C oracle at the per-sample tolerances of the
    existing time-parallel test."""
    import ginsim
    from ginsim import workloads
    from oracle import c_oracle
    if n > 200000:
        fs, prof = 5000.0, 'static_1800s'
    else:
        fs, prof = 200.0, 'long_drive'
    ini, truth, _ = workloads.truth_from_profile(prof, fs, 0)
    t = _cut(truth, n)
    assert t['ref_accel'].shape[0] == n
    acc, gyr = workloads.imu_grade('mid-accuracy')
    if white_drift:
        acc = dict(acc, b_corr=np.array([100.0, np.inf, 100.0]))
    job = ginsim.MonteCarloJob(ctx, fs, 0, t, acc, gyr, None, runs=runs, algos=(), seed=91, run_offset=17, keep_sensors=True)
    name = job.kernel_name()
    assert ('series_kernel' in name) == series, name
    if series:
        assert name == 'ginsim::series_kernel<%d>' % (1 if white_drift else 3), name
    job.run()
    pick = sorted({0, runs // 2, runs - 1})
    a_dev, g_dev = job.sensors('accel', pick), job.sensors('gyro', pick)
    for k, r in enumerate(pick):
        _, _, sens = c_oracle.mc_run(91, 17 + r, 1, fs, 0, t, acc, gyr, ini, keep=1)
        np.testing.assert_allclose(a_dev[k], sens[0, :, 0:3], rtol=0, atol=1e-12)
        np.testing.assert_allclose(g_dev[k], sens[0, :, 3:6], rtol=0, atol=1e-14)
    job.release()


# ------------------------------------------------------------------------------------------------- A4 end-point reduction, exact
def _exact_stats(x):
    """(mean, std ddof=0) of the doubles x, from correctly rounded sums (math.fsum): mean = fsum(x) / R; the deviations about
    that mean (exact for data far from zero: Sterbenz) give the variance, corrected by the mean's own residual."""
    R = x.size
    m = math.fsum(x) / R
    d = x - m
    r = math.fsum(d) / R
    var = math.fsum(d * d) / R - r * r
    return m + r, math.sqrt(max(var, 0.0))


def _planes(R, rng):
    """[9][R] synthetic end errors: each component a case of the reduction's conditioning."""
    e = np.empty((9, R))
    e[0] = 1e6 + 1e-6 * rng.standard_normal(R)                                   # common offset 1e6, spread 1e-6
    e[1] = 0.3                                                                   # all equal: std exactly 0
    e[2] = 0.0
    e[2, (R * 5) // 7] = -2.5                                                    # a single nonzero among zeros
    e[3] = rng.choice([-1.0, 1.0], R) * 10.0 ** rng.uniform(-8, 8, R)            # zero-centred, mixed sign, 1e-8 .. 1e8
    e[4] = -1e6 + 1e-6 * rng.standard_normal(R)
    e[5] = rng.standard_normal(R)
    e[6] = 1e-9 * rng.standard_normal(R) + 1e-7
    e[7] = rng.uniform(-np.pi, np.pi, R)
    e[8] = np.arange(R, dtype=np.float64)
    return e


def _reduce_three_ways(ctx, buf, R):
    """ginsim_end_stats, ginsim_end_stats_begin / _finish, and the one-rank ginsim_end_stats_all_*: one record, three paths"""
    import ginsim
    from ginsim import _lib
    lib = _lib.lib
    out = []
    s = _lib.Stats()
    _lib.check(lib.ginsim_end_stats(ctx.handle, buf.ptr, R, C.byref(s)))
    out.append(ginsim.StatsResult(s))
    _lib.check(lib.ginsim_end_stats_begin(ctx.handle, buf.ptr, R, 3))
    s = _lib.Stats()
    _lib.check(lib.ginsim_end_stats_finish(ctx.handle, 3, C.byref(s)))
    out.append(ginsim.StatsResult(s))
    _lib.check(lib.ginsim_end_stats_all_begin(ctx.handle, buf.ptr, R, 2))
    s = _lib.Stats()
    _lib.check(lib.ginsim_end_stats_all_finish(ctx.handle, 2, C.byref(s)))
    out.append(ginsim.StatsResult(s))
    return out


@pytest.fixture(scope='module')
def comm_ctx(ctx):
    ctx.comm_init(1, 0, ctx.comm_unique_id())
    return ctx


SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 65535, 65536, 65537, 3 * 65536 + 5, 2 ** 20]


def _check_against_exact(st, e, margins=None):
    R = e.shape[1]
    assert st.count == R
    np.testing.assert_array_equal(st.maxabs, np.abs(e).max(1))
    for c in range(9):
        m, sd = _exact_stats(e[c])
        big = np.abs(e[c]).max()
        assert abs(st.mean[c] - m) <= 1e-13 * big, (R, c, st.mean[c], m)
        if sd == 0.0:
            assert st.std[c] == 0.0, (R, c, st.std[c])
            continue
        err = abs(st.std[c] - sd) / sd
        if abs(m) <= 1e-3 * big:         # zero-centred: no cancellation anywhere
            assert err <= 1e-12, (R, c, err)
        else:                            # offset data: NumPy's own std of the same doubles is the bar
            err_np = abs(float(np.std(e[c])) - sd) / sd
            assert err <= 1e-7 and err <= max(16 * err_np, 1e-14), (R, c, err, err_np)
            if margins is not None:
                margins.append((R, c, err, err_np))


@pytest.mark.parametrize('R', SIZES)
def test_end_point_reduction_on_synthetic_planes_vs_exact_sums(comm_ctx, R):
    """stats_blocks caps the grid at 256 x 256 threads (grid-stride above 65 536 runs); sizes around every wave and block edge.
    mean within 1e-13 max|x|; std within 1e-12 (zero-centred) or 1e-7 and 16x NumPy's error (offset); max exact; the three
    device paths bit-identical."""
    ctx = comm_ctx
    e = _planes(R, np.random.default_rng(R))
    buf = ctx.upload(e)
    a, b, c = _reduce_three_ways(ctx, buf, R)
    np.testing.assert_array_equal(a.pack(), b.pack())
    np.testing.assert_array_equal(a.pack(), c.pack())
    margins = []
    _check_against_exact(a, e, margins)
    for R_, c_, err, err_np in margins:
        print('R=%d comp %d: std rel. error %.2e (numpy %.2e)' % (R_, c_, err, err_np))
    buf.free()


@pytest.mark.parametrize('R', [1, 65, 257, 65537, 2 ** 20])
def test_end_point_reduction_of_non_finite_errors_follows_numpy(comm_ctx, R):
    """__array_stats on non-finite errors: NaN anywhere -> NaN for max, avg and std; +inf -> max inf, avg inf, std NaN; -inf ->
    avg -inf; both infinities -> avg NaN.  Placed at the first, a middle and the last run."""
    ctx = comm_ctx
    rng = np.random.default_rng(7)
    e = rng.standard_normal((9, R)) + 2.0
    last, mid = R - 1, R // 2
    e[0, last] = np.nan
    e[1, 0] = np.nan
    e[2, mid] = np.inf
    e[3, last] = -np.inf
    e[4, 0], e[4, last] = np.inf, -np.inf
    e[5, mid], e[5, last] = np.nan, np.inf
    e[6, last] = np.inf
    buf = ctx.upload(e)
    with np.errstate(invalid='ignore'):
        from oracle import ins_np
        ref = ins_np.array_stats(e.T)
        for st in _reduce_three_ways(ctx, buf, R):
            np.testing.assert_array_equal(st.maxabs, ref['max'])
            np.testing.assert_array_equal(np.isnan(st.mean), np.isnan(ref['avg']))
            np.testing.assert_allclose(st.mean, ref['avg'], rtol=1e-13, equal_nan=True)
            np.testing.assert_array_equal(np.isnan(st.std), np.isnan(ref['std']))
            np.testing.assert_allclose(st.std, ref['std'], rtol=1e-12, equal_nan=True)
    buf.free()


# -------------------------------------------------------------------------------------------- A5 process-statistics segmentation
def _synthetic_traj(R, n, rng, ned):
    """(att, pos, vel) of R runs x n samples and a truth (ref_att, ref_pos, ref_vel): attitude errors that wrap; positions LLA
    (ned) or ECEF-sized"""
    ref_att = rng.uniform(-np.pi, np.pi, (n, 3))
    att = ref_att[None] + rng.uniform(-4.0, 4.0, (R, n, 3))
    if ned:
        ref_pos = np.column_stack([0.6 + 1e-5 * rng.standard_normal(n), 2.0 + 1e-5 * rng.standard_normal(n), 100 + rng.standard_normal(n)])
        pos = ref_pos[None] + np.concatenate([1e-6 * rng.standard_normal((R, n, 2)), rng.standard_normal((R, n, 1))], axis=2)
    else:
        ref_pos = 5e6 + 1e3 * rng.standard_normal((n, 3))
        pos = ref_pos[None] + rng.standard_normal((R, n, 3))
    ref_vel = rng.standard_normal((n, 3))
    vel = ref_vel[None] + 1e-2 * rng.standard_normal((R, n, 3))
    return att, pos, vel, ref_att, ref_pos, ref_vel


def _device_traj(att, pos, vel, dtype=np.float64):
    """[9][n][runs] as the kept-trajectory buffers hold them"""
    x = np.concatenate([att, pos, vel], axis=2)              # (R, n, 9)
    return np.ascontiguousarray(x.transpose(2, 1, 0)).astype(dtype)


def _process_stats(ctx, traj, ref, n, R, first, ned, origin=None):
    from ginsim import _lib
    out = np.empty((R, 3, 9))
    if origin is None:
        _lib.check(_lib.lib.ginsim_process_stats(ctx.handle, traj.ptr, ref.ptr, n, R, first, int(ned), _lib.dptr(out)))
    else:
        _lib.check(_lib.lib.ginsim_process_stats_f32(ctx.handle, traj.ptr, ref.ptr, n, R, first, int(ned), origin.ptr, 1, 0,
                                                     _lib.dptr(out)))
    return out


def _end_from_traj(ctx, traj, ref, n, R, ned, origin=None):
    import ginsim
    from ginsim import _lib
    s = _lib.Stats()
    if origin is None:
        _lib.check(_lib.lib.ginsim_end_stats_from_traj(ctx.handle, traj.ptr, ref.ptr, n, R, int(ned), C.byref(s)))
    else:
        _lib.check(_lib.lib.ginsim_end_stats_from_traj_f32(ctx.handle, traj.ptr, ref.ptr, n, R, int(ned), origin.ptr, 1, 0, C.byref(s)))
    return ginsim.StatsResult(s)


def _assert_proc_close(got, want, ned):
    tol = dict(rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got[:, :, 0:3], want[:, :, 0:3], **tol)
    np.testing.assert_allclose(got[:, :, 6:9], want[:, :, 6:9], **tol)
    if ned:     # the tolerance of test_device_process_stats_and_ned_match_reference
        np.testing.assert_allclose(got[:, :, 3:6], want[:, :, 3:6], rtol=1e-6, atol=2e-8)
    else:
        np.testing.assert_allclose(got[:, :, 3:6], want[:, :, 3:6], rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize('precision', ['f64', 'f32'])
@pytest.mark.parametrize('ned', [False, True])
@pytest.mark.parametrize('R', [1, 63, 65])
def test_process_stats_segments_with_few_samples(ctx, R, ned, precision):
    """process_stats_kernel cuts the window into kSeg = 4 segments: with fewer than four samples some are empty.  Windows of
    1, 2, 3, 4, 5, 8, 9 samples (the last: first_sample = n - 1) against ins_np.process_error_stats, the end point against
    array_stats; first_sample = n is refused."""
    from ginsim import _lib
    from oracle import ins_np
    rng = np.random.default_rng(100 * R + ned)
    n = 12
    att, pos, vel, ref_att, ref_pos, ref_vel = _synthetic_traj(R, n, rng, ned)
    origin = None
    if precision == 'f32':          # float series; positions as displacement from a zero origin
        att, pos, vel = (x.astype(np.float32).astype(np.float64) for x in (att, pos, vel))
        origin = ctx.upload(np.zeros((1, 3)))
    traj = ctx.upload(_device_traj(att, pos, vel, np.float32 if precision == 'f32' else np.float64))
    ref = ctx.upload(np.ascontiguousarray(np.concatenate([ref_att, ref_pos, ref_vel], axis=1)))
    for w in (1, 2, 3, 4, 5, 8, 9):
        first = n - w
        got = _process_stats(ctx, traj, ref, n, R, first, ned, origin)
        want = ins_np.process_error_stats(att, pos, vel, ref_att, ref_pos, ref_vel, first, pos_ned=ned)
        _assert_proc_close(got, want, ned)
        if w == 1:
            assert np.all(got[:, 2] == 0.0)
    end = _end_from_traj(ctx, traj, ref, n, R, ned, origin)
    e_end = ins_np.process_error_stats(att, pos, vel, ref_att, ref_pos, ref_vel, n - 1, pos_ned=ned)[:, 1, :]
    st = ins_np.array_stats(e_end)
    assert end.count == R
    np.testing.assert_allclose(end.mean, st['avg'], rtol=1e-12, atol=2e-8 if ned else 1e-9)
    np.testing.assert_allclose(end.std, st['std'], rtol=1e-9, atol=2e-8 if ned else 1e-9)
    np.testing.assert_allclose(end.maxabs, st['max'], rtol=1e-12, atol=2e-8 if ned else 1e-9)
    with pytest.raises(ValueError, match='bad sizes'):
        _process_stats(ctx, traj, ref, n, R, n, ned, origin)
    for b in (traj, ref) + ((origin,) if origin is not None else ()):
        b.free()


# ----------------------------------------------------------------------------------------- C non-finite and the -pi / +pi wrap
@pytest.mark.parametrize('precision', ['f64', 'f32'])
def test_kept_path_process_stats_of_non_finite_errors_follow_numpy(ctx, precision):
    """NaN / +-inf in kept trajectories, in different segments of the window: the per-run statistics and the end-point record
    follow the reference's NumPy reductions (NaN / inf where NumPy has them), and every other run is unaffected."""
    from oracle import ins_np
    rng = np.random.default_rng(5)
    R, n, first = 65, 40, 3
    att, pos, vel, ref_att, ref_pos, ref_vel = _synthetic_traj(R, n, rng, False)
    if precision == 'f32':
        att, pos, vel = (x.astype(np.float32).astype(np.float64) for x in (att, pos, vel))
    pos[3, 5, 1] = np.nan
    vel[10, first, 0] = np.inf
    vel[11, 7, 1], vel[11, 30, 1] = np.inf, -np.inf
    vel[12, n - 1, 2] = -np.inf
    att[64, n - 1, 1] = np.nan
    att[20, 20, 0] = np.inf                     # angle_range_pi(inf) is NaN
    pos[21, 1, 2] = np.nan                      # before the window: no effect on the process statistics
    origin = ctx.upload(np.zeros((1, 3))) if precision == 'f32' else None
    traj = ctx.upload(_device_traj(att, pos, vel, np.float32 if precision == 'f32' else np.float64))
    ref = ctx.upload(np.ascontiguousarray(np.concatenate([ref_att, ref_pos, ref_vel], axis=1)))
    with np.errstate(invalid='ignore'):
        got = _process_stats(ctx, traj, ref, n, R, first, False, origin)
        want = ins_np.process_error_stats(att, pos, vel, ref_att, ref_pos, ref_vel, first)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        np.testing.assert_array_equal(np.isinf(got), np.isinf(want))
        assert np.isnan(want).sum() >= 12 and np.isinf(want).sum() >= 4
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-9, equal_nan=True)
        end = _end_from_traj(ctx, traj, ref, n, R, False, origin)
        st = ins_np.array_stats(ins_np.process_error_stats(att, pos, vel, ref_att, ref_pos, ref_vel, n - 1)[:, 1, :])
        np.testing.assert_array_equal(end.maxabs, st['max'])
        np.testing.assert_allclose(end.mean, st['avg'], rtol=1e-12, atol=1e-9, equal_nan=True)
        np.testing.assert_array_equal(np.isnan(end.std), np.isnan(st['std']))
    for b in (traj, ref) + ((origin,) if origin is not None else ()):
        b.free()


def test_attitude_error_on_the_pi_boundary_wraps_as_angle_range_pi(ctx):
    """An attitude error of exactly -pi is +pi after angle_range_pi (a 2 pi difference in that sample's mean otherwise);
    nextafter(+-pi), +-3 pi and +-1e3 rad against ins_np.angle_range_pi, one run per value, both precisions' kernels."""
    from oracle import ins_np
    v = np.array([np.pi, -np.pi, np.nextafter(np.pi, 0), np.nextafter(-np.pi, 0), np.nextafter(np.pi, 4), np.nextafter(-np.pi, -4),
                  3 * np.pi, -3 * np.pi, 1e3, -1e3, 0.0, 2 * np.pi])
    R, n = v.size, 1
    att = np.zeros((R, n, 3))
    att[:, 0, 0], att[:, 0, 1], att[:, 0, 2] = v, -v, v[::-1]
    pos, vel = np.zeros((R, n, 3)), np.zeros((R, n, 3))
    z = np.zeros((n, 3))
    traj = ctx.upload(_device_traj(att, pos, vel))
    ref = ctx.upload(np.zeros((n, 9)))
    got = _process_stats(ctx, traj, ref, n, R, 0, False)
    want = ins_np.angle_range_pi(att[:, 0, :])
    np.testing.assert_allclose(got[:, 1, 0:3], want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(got[:, 0, 0:3], np.abs(want), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(got[:, 1, 0:3] == np.pi, want == np.pi)
    assert np.array_equal(ins_np.process_error_stats(att, pos, vel, z, z, z, 0)[:, 1, 0:3], want)
    traj.free()
    ref.free()


@pytest.mark.parametrize('rf', [0, 1])
def test_online_process_stats_of_a_run_that_went_nan(ctx, rf):
    """Online process statistics (proc_first) of a launch in which one run's initial forward speed is NaN (run r uses column r of
    the initial-state table; the online path takes generated sensors only): that run's statistics follow the reference's rule on
    its own kept trajectory -- NaN max / avg / std where its error has a NaN in the window, never the std = 0 of a clamp -- every
    other run is bit-identical to the same launch without the NaN, and the end-point statistics are NaN where NumPy's are."""
    import ginsim
    from ginsim import workloads
    from oracle import ins_np
    ini, truth = workloads.truth_from_profile('turn_90deg', 100.0, rf)[:2]
    acc, gyr = workloads.imu_grade('mid-accuracy')
    R, bad, first = 1500, 777, 200
    table = np.repeat(ini[:, None], R, axis=1)
    table[3, :] += 1e-3 * np.arange(R) / R      # no run starts on the truth: both launches take the same shifted sums
    nan_table = table.copy()
    nan_table[3, bad] = np.nan
    kw = dict(runs=R, algos=('free',), seed=3, keep_traj=True, proc_first=first)
    clean = ginsim.MonteCarloJob(ctx, 100.0, rf, truth, acc, gyr, table, **kw).run()
    job = ginsim.MonteCarloJob(ctx, 100.0, rf, truth, acc, gyr, nan_table, **kw).run()
    assert job.kernel_name() == clean.kernel_name()
    got, ok = job.process_stats_online('free'), clean.process_stats_online('free')
    others = np.arange(R) != bad
    np.testing.assert_array_equal(got[others], ok[others])
    att, pos, vel = job.trajectories('free', [bad])
    with np.errstate(invalid='ignore'):
        want = ins_np.process_error_stats(att, pos, vel, truth['ref_att'], truth['ref_pos'], truth['ref_vel'], first)[0]
        assert np.isnan(want).any()
        np.testing.assert_array_equal(np.isnan(got[bad]), np.isnan(want))
        np.testing.assert_allclose(got[bad], want, rtol=1e-7, atol=1e-9, equal_nan=True)
        np.testing.assert_array_equal(np.isnan(job.process_stats('free', first)[bad]), np.isnan(want))
        end = job.end_errors('free')
        np.testing.assert_array_equal(end[others], clean.end_errors('free')[others])
        st, ref = job.stats('free'), ins_np.array_stats(end)
        np.testing.assert_array_equal(np.isnan(st.maxabs), np.isnan(ref['max']))
        np.testing.assert_array_equal(np.isnan(st.mean), np.isnan(ref['avg']))
        np.testing.assert_array_equal(np.isnan(st.std), np.isnan(ref['std']))
        assert np.isnan(ref['max']).any()
    job.release()
    clean.release()


# ------------------------------------------------------------------------------------------------- B config 4 at 1 048 576 runs
def test_c4_full_size_one_launch_and_eight_contexts(ctx):
    """BASELINE config 4 (turn_90deg, 100 Hz, ref_frame 1, mid-accuracy) at 2^20 runs, statistics only: as one launch and as the
    drop-in's multi-context form (devices = [0] * 8, 131 072 runs per context).  Sampled end errors vs the C oracle (the last
    block ends at run 1 048 575), device statistics vs exact sums over the downloaded record, and the two forms identical."""
    import ginsim
    from ginsim import multi, workloads
    from oracle import c_oracle
    fs, rf, R, seed = 100.0, 1, 2 ** 20, 20260923
    ini, truth, _ = workloads.truth_from_profile('turn_90deg', fs, rf)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    one = ginsim.MonteCarloJob(ctx, fs, rf, truth, acc, gyr, ini, runs=R, seed=seed).run()
    e1 = one.end_errors('free')
    s1 = one.stats('free')
    one.release()
    assert np.all(np.isfinite(e1))
    for first, count in _blocks(R, width=64):
        end, _, _ = c_oracle.mc_run(seed, first, count, fs, rf, truth, acc, gyr, ini)
        ids = np.arange(first, first + count)
        assert np.abs(np.mod(e1[ids, :3] - end[:, :3] + np.pi, 2 * np.pi) - np.pi).max() <= 1e-9
        np.testing.assert_allclose(e1[ids, 3:6], end[:, 3:6], rtol=0, atol=2e-8)
        np.testing.assert_allclose(e1[ids, 6:9], end[:, 6:9], rtol=0, atol=1e-9)
    assert first + count == R
    _check_against_exact(s1, np.ascontiguousarray(e1.T))
    ds = multi.DeviceSet([0] * 8)
    js = multi.JobSet(ds, fs, rf, truth, acc, gyr, ini, R, seed=seed).run()
    assert [c for _, c in js.ranges] == [131072] * 8
    np.testing.assert_array_equal(js.end_errors('free'), e1)
    s8 = js.stats('free')
    assert s8.count == R
    np.testing.assert_array_equal(s8.maxabs, s1.maxabs)
    np.testing.assert_allclose(s8.mean, s1.mean, rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(s8.std, s1.std, rtol=1e-12)
    js.release()
    ds.close()
