"""The rare branches of nav_step / Att::step -- pitch fold, +-2 pi wrap, steps across 2^-6 and 0.25 rad, steps of 2 rad and more,
all of them on and next to a resync step, latitude steps of the same classes, non-finite input -- in EVERY kernel family that runs
the time step, on the constructed cases of tests/nav_branch_cases.py (what each case is there for is counted on the CPU by
tests/test_nav_branch_oracle.py).

fp64: every sample of every compared run against the C oracle (oracle_free_integration for given data, oracle_mc_run for generate
mode), nothing cut at the singularity; tolerance SURVEY 8(c) as tests/test_gpu_fuzz.py applies it, 1e-9 max(1, n / 1000) on
attitude (mod 2 pi) and on position / velocity relative to max(1, |x|).  Which runs are compared is decided by the oracle alone
(nav_branch_cases.compared).  Bit for bit: wave-specialised against plain, given data against generate mode (a zero-error IMU
reproduces the rates exactly, and the project holds the replay of materialised sensors to equal bits in tests/test_gpu_fuzz.py),
every run of (c) and (f) in shards of 1, 63 and 65 against the whole batch, fp32 against the float oracle.

Kernels reached (job.kernel_name(), asserted per family below; RF = 0 and 1):
    ginsim::mc_kernel<RF, 1 | 2 | 3, true, false, 0, false>         given data (also behind ginsim_free_integration)
    ginsim::mc_kernel_split<1, 1, false, 2, true, false>            one free integration as dispatched, ref_frame 1
    ginsim::mc_kernel_split<0, 1, false, 1, true, false>            ... ref_frame 0
    ginsim::mc_kernel<RF, 1, false, false, 0, false>                block_threads = 256: the plain kernel, EASY
    ginsim::mc_kernel<RF, 2, false, false, 0, false>                the odometer alone as dispatched (plain, EASY)
    ginsim::mc_kernel_split<1, 3, false, 1, true, false>            ('free', 'odo'): one producer group
    ginsim::mc_kernel_split<0, 3, true, 1, true, false>
    ginsim::mc_kernel<1, 3, false, false, 0, false>, <0, 3, false, true, 0, false>     the same, block_threads = 256
    ginsim::f32::mc_kernel_f32_split<...> (everything or nothing kept), ginsim::f32::mc_kernel_f32<...> (trajectories only; given data)

Measured error / tolerance, worst compared run per family over all cases (MI355X; the tolerance is NOT derived from these):
    given data 2.9e-3; free as dispatched 2.9e-3; free plain 2.9e-3; odo as dispatched 2.9e-3; both algorithms, one producer 2.9e-3;
    both plain 2.9e-3; end-point records with nothing kept 1.2e-4.  All of it c_ini_table (runs within 8e-6 of the pole); c_gyro_noise
    3e-5, the big-step and latitude cases below 1e-5.
"""
import numpy as np
import pytest

from conftest import load_golden, assert_traj_close
import nav_branch_cases as nb

pytestmark = pytest.mark.gpu
_WORST = {}


@pytest.fixture(scope='module')
def ctx():
    import ginsim
    c = ginsim.Context(0)
    yield c
    c.close()
    if _WORST:
        print('\nerror / tolerance, worst compared run per family: ' + ', '.join('%s %.3g' % kv for kv in sorted(_WORST.items())))


def _same_bits(a, b):
    """equal to the bit where either is a number, NaN at the same places (a NaN's payload is not part of any contract here)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb_ = np.isnan(a), np.isnan(b)
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    return bool(np.array_equal(na, nb_) and np.array_equal(a.view(u)[~na], b.view(u)[~nb_]))


def _job(ctx, c, algos, keep='traj', plain=False, precision='f64', first=0, count=None, ini=None):
    import ginsim
    count = c.runs if count is None else count
    job = ginsim.MonteCarloJob(ctx, c.fs, c.rf, c.truth, c.acc_err, c.gyr_err, c.ini if ini is None else ini, runs=count, algos=algos,
                               odo_err=nb.ODO_EXACT if 'odo' in algos else None, earth_rot=c.earth_rot, seed=c.seed, run_offset=c.off + first,
                               ini_first=first, keep_sensors=keep == 'all', keep_traj=keep in ('all', 'traj'), precision=precision)
    if plain:
        job.params.block_threads = 256
    return job


def _traj(job, algo, displacement=False):
    att, pos, vel = job.trajectories(algo, np.arange(job.runs), displacement=displacement) if displacement else job.trajectories(algo, np.arange(job.runs))
    return np.concatenate([att, pos, vel], axis=2)


def _given_job(ctx, c, algo, gyro, accel, precision='f64', first=0, count=None, ini=None):
    """the given-data kernel on device-resident [axis][sample][run] series"""
    import ginsim
    count = c.runs if count is None else count
    sl = slice(first, first + count)
    bufs = {'gyro': ctx.upload(np.ascontiguousarray(gyro[sl].transpose(2, 1, 0)))}
    if algo == 'free':
        bufs['accel'] = ctx.upload(np.ascontiguousarray(accel[sl].transpose(2, 1, 0)))
    else:
        bufs['odo'] = ctx.upload(np.ascontiguousarray(np.repeat(c.odo[:, None], count, axis=1)))
    job = ginsim.MonteCarloJob(ctx, c.fs, c.rf, c.truth, None, None, c.ini if ini is None else ini, runs=count, algos=(algo,), earth_rot=c.earth_rot,
                               ini_first=first, keep_traj=True, precision=precision, given=bufs)
    return job, bufs


def _host(ctx, c, algo, gyro, accel, first=0, count=None, ini=None):
    """ginsim_free_integration: host series in, host series out"""
    import ginsim
    count = c.runs if count is None else count
    sl = slice(first, first + count)
    att, pos, vel = ginsim.free_integration_host(ctx, algo, c.rf, c.fs, gyro[sl], accel=accel[sl] if algo == 'free' else None,
                                                 odo=np.repeat(c.odo[None, :], count, axis=0) if algo == 'odo' else None,
                                                 ini=c.ini if ini is None else ini, earth_rot=c.earth_rot, ini_first=first)
    return np.concatenate([att, pos, vel], axis=2)


def _hold(family, c, algo, got, ref, ok):
    """every sample of every compared run within the tolerance; prints and records error / tolerance"""
    r = nb.ratio(got[ok], ref[ok], c.n)
    worst = float(r.max())
    print('%-22s %-28s %-4s error / tolerance %.3g over %d runs' % (family, c.name, algo, worst, int(ok.sum())))
    _WORST[family] = max(_WORST.get(family, 0.0), worst)
    assert worst < 1.0, '%s %s %s: run %d is off by %.3g of the tolerance' % (family, c.name, algo, int(np.flatnonzero(ok)[np.argmax(r)]), worst)


def _hold_end(family, c, algo, end, ref_end, ok):
    """the end-point records (against a zero truth: the last state, the attitude wrapped) of the compared runs"""
    r = nb.ratio(end[ok][:, None, :], ref_end[ok][:, None, :], c.n)
    worst = float(r.max())
    print('%-22s %-28s %-4s end-point error / tolerance %.3g' % (family, c.name, algo, worst))
    _WORST[family] = max(_WORST.get(family, 0.0), worst)
    assert worst < 1.0, (family, c.name, algo, worst)


def _hold_bad(c, algo, got, ref, what):
    """(f): a bad run is non-finite exactly where the oracle's is, a number to the tolerance before, NaN in all nine planes from two
    samples after its first bad attitude on.  At the first bad sample and the next the pattern is held on the attitude only: with
    roll = Inf alone (trig NaN) the odometer's velocity is cp cy v, cp sy v, -sp v on the device, a number, where the oracle's full
    matrix product has 0 x NaN, and the position lags the velocity by a sample."""
    for run, first in c.bad.items():
        fin_got, fin_ref = np.isfinite(got[run]), np.isfinite(ref[run])
        fin_got[first:first + 2, 3:9] = fin_ref[first:first + 2, 3:9]
        assert np.array_equal(fin_got, fin_ref), '%s run %d: non-finite at other samples than the oracle' % (what, run)
        assert np.isnan(got[run, first + 2:]).all(), '%s run %d' % (what, run)
        assert not np.isfinite(got[run, first:, 0:3]).all(axis=1).any(), '%s run %d' % (what, run)
        if first > 0:
            assert nb.ratio(got[run:run + 1, :first], ref[run:run + 1, :first], c.n)[0] < 1.0, '%s run %d before the bad sample' % (what, run)


def _shards(runs):
    out, first, sizes = [], 0, (1, 63, 65)
    while first < runs:
        count = min(sizes[len(out) % 3], runs - first)
        out.append((first, count))
        first += count
    return out


def _given_families(ctx, c):
    """the given-data kernels, fp64: through ginsim_free_integration and as a job on device-resident series (which names its kernel);
    returns {algo: (runs, n, 9)}"""
    gyro, accel = nb.sensors(c.name)
    out = {}
    for algo in nb.ALGOS:
        ok, ref = nb.compared(c.name, algo), nb.oracle_given(c.name, algo)
        host = _host(ctx, c, algo, gyro, accel)
        _hold('given (C ABI)', c, algo, host, ref, ok)
        _hold_bad(c, algo, host, ref, 'given')
        job, bufs = _given_job(ctx, c, algo, gyro, accel)
        assert job.kernel_name() == 'ginsim::mc_kernel<%d, %d, true, false, 0, false>' % (c.rf, 1 if algo == 'free' else 2), job.kernel_name()
        dev = _traj(job.run(), algo)
        assert _same_bits(dev, host), '%s %s: the job on given series and ginsim_free_integration differ' % (c.name, algo)
        job.release()
        for b in bufs.values():
            b.free()
        out[algo] = host
    return out


@pytest.mark.parametrize('name', nb.NAMES)
def test_fp64_families_against_the_c_oracle_and_each_other(ctx, name):
    c = nb.cases()[name]
    given = _given_families(ctx, c)
    if not c.generate:
        return
    wd0 = 'true' if c.rf == 0 else 'false'          # the two-algorithm ref_frame 0 kernels take the general sensor model
    split_free = 'ginsim::mc_kernel_split<%d, 1, false, %d, true, false>' % (c.rf, 2 if c.rf == 1 else 1)
    families = [  # (family, algos, keep, plain, kernel name)
        ('free as dispatched', ('free',), 'traj', False, split_free),
        ('free plain (EASY)', ('free',), 'all', True, 'ginsim::mc_kernel<%d, 1, false, false, 0, false>' % c.rf),
        ('odo as dispatched', ('odo',), 'traj', False, 'ginsim::mc_kernel<%d, 2, false, false, 0, false>' % c.rf),
        ('both, one producer', ('free', 'odo'), 'traj', False, 'ginsim::mc_kernel_split<%d, 3, %s, 1, true, false>' % (c.rf, wd0)),
        ('both plain (EASY)', ('free', 'odo'), 'all', True, 'ginsim::mc_kernel<%d, 3, false, %s, 0, false>' % (c.rf, wd0)),
        ('both, nothing kept', ('free', 'odo'), 'none', False, 'ginsim::mc_kernel_split<%d, 3, %s, 1, true, false>' % (c.rf, wd0)),
        ('free, nothing kept', ('free',), 'none', False, None),     # ref_frame 0: whichever wave-specialised instantiation the dispatch reports
    ]
    got, ends = {}, {}
    for family, algos, keep, plain, want in families:
        job = _job(ctx, c, algos, keep, plain)
        kname = job.kernel_name()
        if want is not None:
            assert kname == want, (family, kname)
        else:
            assert 'mc_kernel_split<%d, 1, false' % c.rf in kname, (family, kname)
        job.run()
        for algo in algos:
            ok = nb.compared(name, algo)
            end_ref, ref = nb.oracle_mc(name, algo)
            ends[family, algo] = job.end_errors(algo)
            _hold_end(family, c, algo, ends[family, algo], end_ref, ok)
            for run in c.bad:
                assert np.isnan(ends[family, algo][run]).all(), 'the end-point record of a bad run is NaN'
            if keep != 'none':
                got[family, algo] = _traj(job, algo)
                _hold(family, c, algo, got[family, algo], ref, ok)
                _hold_bad(c, algo, got[family, algo], ref, family)
        if keep == 'all':       # the kept sensor series of a zero-error IMU are the rates themselves; with noise, the oracle's (test_gpu_fuzz.py)
            gyro, accel = nb.sensors(name)
            np.testing.assert_allclose(job.sensors('gyro', np.arange(c.runs)), gyro, rtol=0, atol=2e-14 if c.noisy else 0)
            np.testing.assert_allclose(job.sensors('accel', np.arange(c.runs)), accel, rtol=0, atol=2e-12 if c.noisy else 0)
        job.release()
    # bit for bit: wave-specialised against plain, every plane and the end-point records
    for a_family, b_family, algos in (('free as dispatched', 'free plain (EASY)', ('free',)), ('both, one producer', 'both plain (EASY)', nb.ALGOS)):
        for algo in algos:
            assert _same_bits(got[a_family, algo], got[b_family, algo]), '%s %s: %s and %s differ' % (name, algo, a_family, b_family)
            assert _same_bits(ends[a_family, algo], ends[b_family, algo]), '%s %s: end-point records' % (name, algo)
    for algo in nb.ALGOS:
        assert _same_bits(ends['both, nothing kept', algo], ends['both, one producer', algo]), 'nothing kept: other end-point records'
    assert _same_bits(ends['free, nothing kept', 'free'], ends['free as dispatched', 'free'])
    # given data against generate mode: the same rates through the same step, every sample of every run to the bit -- the four
    # threshold rows of (a) among them.  Not with noise: the given series are then the oracle's, 1e-14 from the device's own.
    for family, algo in () if c.noisy else (('free as dispatched', 'free'), ('free plain (EASY)', 'free'), ('odo as dispatched', 'odo'), ('both, one producer', 'odo'),
                         ('both plain (EASY)', 'free')):
        assert _same_bits(got[family, algo], given[algo]), '%s %s: %s differs from the given-data kernel' % (name, algo, family)


@pytest.mark.parametrize('name', [n for n in nb.NAMES if len(nb.cases()[n].run_counts) > 1])
def test_every_run_count_reproduces_the_batch(ctx, name):
    """(c): 1, 63, 64, 65 and 257 runs of the same batch (run r is global run offset + r whatever the launch holds): the
    wave-specialised and the plain kernel, both algorithms, against each other to the bit and against the oracle"""
    c = nb.cases()[name]
    whole = {}
    for count in sorted(c.run_counts, reverse=True):
        for plain in (False, True):
            job = _job(ctx, c, nb.ALGOS, 'traj', plain, count=count)
            assert ('split' in job.kernel_name()) != plain, job.kernel_name()
            job.run()
            for algo in nb.ALGOS:
                t, e = _traj(job, algo), job.end_errors(algo)
                if count == c.runs and not plain:
                    whole[algo] = (t, e)
                    _hold('run counts', c, algo, t, nb.oracle_mc(name, algo)[1], nb.compared(name, algo))
                assert _same_bits(t, whole[algo][0][:count]) and _same_bits(e, whole[algo][1][:count]), (name, count, plain, algo)
            job.release()


@pytest.mark.parametrize('name', [n for n in nb.NAMES if n[0] in 'cf'])
def test_shards_reproduce_every_run_of_the_batch(ctx, name):
    """(c), (f): each run alone or in shards of 1, 63 and 65 runs -- so that it changes its wavefront neighbours, among them one that
    folds, wraps, steps by more than 0.25 rad or is NaN at that very sample -- comes out with the bits it has in the whole batch"""
    c = nb.cases()[name]
    gyro, accel = nb.sensors(name)
    whole_given = {algo: _host(ctx, c, algo, gyro, accel) for algo in nb.ALGOS}
    for first, count in _shards(c.runs):
        for algo in nb.ALGOS:
            part = _host(ctx, c, algo, gyro, accel, first, count)
            assert _same_bits(part, whole_given[algo][first:first + count]), (name, 'given', algo, first, count)
    if not c.generate:
        return
    for plain in (False, True):
        job = _job(ctx, c, nb.ALGOS, 'traj', plain).run()
        whole = {algo: (_traj(job, algo), job.end_errors(algo)) for algo in nb.ALGOS}
        job.release()
        for first, count in _shards(c.runs):
            part = _job(ctx, c, nb.ALGOS, 'traj', plain, first=first, count=count)
            assert ('split' in part.kernel_name()) != plain
            part.run()
            for algo in nb.ALGOS:
                assert _same_bits(_traj(part, algo), whole[algo][0][first:first + count]), (name, plain, algo, first, count)
                assert _same_bits(part.end_errors(algo), whole[algo][1][first:first + count]), (name, plain, algo, first, count)
            part.release()


@pytest.mark.parametrize('name', [n for n in nb.NAMES if n[0] == 'f'])
def test_a_bad_run_leaves_its_neighbours_alone(ctx, name):
    """(f): every other run keeps the bits of a launch without the bad run; the bad run itself is held in the family tests"""
    c = nb.cases()[name]
    gyro, accel = nb.sensors(name)
    good = np.ones(c.runs, dtype=bool)
    good[list(c.bad)] = False
    clean_gyro = np.repeat(c.gyro[None], c.runs, axis=0)
    clean_ini = c.ini if c.clean_ini is None else c.clean_ini
    for algo in nb.ALGOS:
        bad = _host(ctx, c, algo, gyro, accel)
        clean = _host(ctx, c, algo, clean_gyro, accel, ini=clean_ini)
        assert np.isfinite(clean).all() and not np.isfinite(bad[list(c.bad)]).all()
        assert _same_bits(bad[good], clean[good]), (name, 'given', algo)
    if not c.generate:
        return
    for plain in (False, True):
        for keep in ('traj', 'none'):
            a = _job(ctx, c, nb.ALGOS, keep, plain).run()
            b = _job(ctx, c, nb.ALGOS, keep, plain, ini=clean_ini).run()
            for algo in nb.ALGOS:
                ea, eb = a.end_errors(algo), b.end_errors(algo)
                assert np.isfinite(eb).all() and np.isnan(ea[list(c.bad)]).all()
                assert _same_bits(ea[good], eb[good]), (name, plain, keep, algo)
                if keep == 'traj':
                    assert _same_bits(_traj(a, algo)[good], _traj(b, algo)[good]), (name, plain, algo)
            a.release()
            b.release()


def _f32_split(got):
    return got[..., 0:3], got[..., 3:6], got[..., 6:9]


@pytest.mark.parametrize('name', nb.NAMES)
def test_fp32_families_against_the_float_oracle(ctx, name):
    """precision='f32': the wave-specialised kernel (everything kept), the plain one (trajectories only; block_threads = 256) and
    the given-data kernel, bit for bit against oracle_mc_run_f32 / oracle_free_integration_f32 -- singularity, fold or NaN alike"""
    from oracle import c_oracle
    c = nb.cases()[name]
    gyro, accel = nb.sensors(name)
    for algo in nb.ALGOS:
        job, bufs = _given_job(ctx, c, algo, gyro, accel, precision='f32')
        assert 'mc_kernel_f32<%d, %d, true' % (c.rf, 1 if algo == 'free' else 2) in job.kernel_name(), job.kernel_name()
        dev = _traj(job.run(), algo, displacement=True).astype(np.float32)
        for r in range(c.runs):
            att, dpos, vel, _ = c_oracle.free_integration_f32(c.rf, c.fs, gyro[r], accel[r] if algo == 'free' else None, c.ini_of(r),
                                                              earth_rot=c.earth_rot, odo=c.odo if algo == 'odo' else None)
            assert _same_bits(dev[r], np.concatenate([att, dpos, vel], axis=1)), '%s %s run %d: fp32 given data' % (name, algo, r)
        job.release()
        for b in bufs.values():
            b.free()
    if not c.generate:
        return
    ref = {}
    for algo in nb.ALGOS:
        end, traj, _, _ = c_oracle.mc_run_f32(c.seed, c.off, c.runs, c.fs, c.rf, c.truth, c.acc_err, c.gyr_err, c.ini, algo=algo, odo_err=nb.ODO_EXACT,
                                              earth_rot=c.earth_rot, keep=c.runs)
        ref[algo] = (end, traj)
    for family, algos, keep, plain, split in (('split', nb.ALGOS, 'all', False, c.n >= 2), ('traj only', nb.ALGOS, 'traj', False, False),
                                              ('plain', ('free',), 'all', True, False), ('odo alone', ('odo',), 'traj', False, False),
                                              ('nothing kept', ('free',), 'none', False, c.n >= 2)):
        job = _job(ctx, c, algos, keep, plain, precision='f32')
        assert 'f32' in job.kernel_name() and ('split' in job.kernel_name()) == split, (family, job.kernel_name())
        job.run()
        for algo in algos:
            end = job.end_errors(algo)
            assert np.array_equal(end, ref[algo][0], equal_nan=True), '%s %s %s: fp32 end-point records' % (name, family, algo)
            if keep != 'none':
                dev = _traj(job, algo, displacement=True).astype(np.float32)
                assert _same_bits(dev, ref[algo][1]), '%s %s %s: fp32 trajectories' % (name, family, algo)
        job.release()


RESTARTS = [('e_latitude_small_mid', 32), ('e_latitude_resync', 32), ('d_big_steps_rf0_1Hz', 32), ('b_tumble_rf0', 32), ('b_tumble_rf0', 320),
            ('b_tumble_rf0', 416)]


@pytest.mark.parametrize('name, at', RESTARTS)
def test_a_resync_step_leaves_no_history_in_the_cache(ctx, name, at):
    """After a resync step (j + 1 = 0 mod 32) the cached sines and cosines of attitude and latitude are those a fresh start from that
    state evaluates, so in ref_frame 0 (where the stored position is the state itself) the odometer algorithm started from sample
    `at` with the rest of the series reproduces the rest of the run BIT FOR BIT -- in the given-data kernel and in the plain
    generate-mode kernel the odometer alone is dispatched to.  A time step that rotates its cache where it should re-evaluate it
    differs in the last bits of the trig and, with these step sizes, of what is stored a few samples on."""
    import ginsim
    c = nb.cases()[name]
    assert c.rf == 0 and c.runs == 1 and at % 32 == 0
    gyro, accel = nb.sensors(name)
    full = _host(ctx, c, 'odo', gyro, accel)[0]
    ini = np.concatenate([full[at, 3:6], [c.odo[at - 1], 0.0, 0.0], full[at, 0:3]])
    att, pos, vel = ginsim.free_integration_host(ctx, 'odo', 0, c.fs, gyro[0, at:], odo=c.odo[at:], ini=ini, earth_rot=c.earth_rot)
    rest = np.concatenate([att, pos, vel], axis=1)
    assert _same_bits(rest, full[at:]), '%s: the given-data kernel restarted at %d differs at sample %d' % (
        name, at, at + int(np.flatnonzero((rest != full[at:]).any(axis=1))[0]))
    truth = {k: v[at:] for k, v in c.truth.items()}
    whole = _job(ctx, c, ('odo',), 'traj').run()
    part = ginsim.MonteCarloJob(ctx, c.fs, 0, truth, nb.ZERO, nb.ZERO, ini, runs=1, algos=('odo',), odo_err=nb.ODO_EXACT, earth_rot=c.earth_rot,
                                seed=c.seed, keep_traj=True).run()
    assert part.kernel_name() == 'ginsim::mc_kernel<0, 2, false, false, 0, false>'
    assert _same_bits(_traj(part, 'odo')[0], _traj(whole, 'odo')[0, at:]), '%s: the generate-mode kernel restarted at %d' % (name, at)
    whole.release()
    part.release()


@pytest.mark.parametrize('tag, rf, use_g, erot', [('extg', 0, True, False), ('wgs', 0, False, True), ('rf1', 1, False, True)])
def test_odometer_plugin_on_the_tumble_fixture(ctx, tag, rf, use_g, erot):
    """What the unmodified reference's free_integration_odo returned on the tumble rates (folds, wraps, every sample): the
    given-data kernel and the zero-noise generate-mode kernels (odometer alone: plain; with the free integration: wave-specialised)"""
    import ginsim
    g = load_golden('t1_fixture_tumble_odo')
    ini = g['ini'] if use_g else g['ini'][:9]
    fs, n = float(g['fs']), g['gyro'].shape[0]
    att, pos, vel = ginsim.free_integration_host(ctx, 'odo', rf, fs, g['gyro'], odo=g['odo'], ini=ini, earth_rot=erot)
    assert_traj_close(att, pos, vel, g['att_' + tag], g['pos_' + tag], g['vel_' + tag], rtol=1e-10, what='given ' + tag)
    z = np.zeros((n, 3))
    accel = load_golden('t1_fixture_tumble')['accel']
    truth = {'ref_accel': accel, 'ref_gyro': g['gyro'], 'ref_odo': g['odo'], 'ref_att': z, 'ref_pos': z, 'ref_vel': z}
    for algos, split in ((('odo',), False), (('free', 'odo'), True)):
        job = ginsim.MonteCarloJob(ctx, fs, rf, truth, nb.ZERO, nb.ZERO, ini, runs=3, algos=algos, odo_err=nb.ODO_EXACT, earth_rot=erot, seed=1,
                                   keep_traj=True)
        assert ('split' in job.kernel_name()) == split, job.kernel_name()
        att, pos, vel = job.run().trajectories('odo', [0, 2])
        for r in range(2):
            assert_traj_close(att[r], pos[r], vel[r], g['att_' + tag], g['pos_' + tag], g['vel_' + tag], rtol=1e-10, what='%s %s run %d' % (algos, tag, r))
        job.release()
