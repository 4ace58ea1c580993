"""GPU: the magnetometer calibration kernel (csrc/magcal.hip) where the one configuration of tests/test_gpu_magcal.py never
goes -- the records of tests/magcal_records.py: hard iron of 500 uT in all eight octants (every sign pattern of the three normals,
rotated columns that keep one sign), si with its rows permuted / mirrored / rotated 45 degrees (every component selected by
vecMax), noise levels 0 .. 5 uT, ranges that touch both ends of the series, lie out of series order, overlap, or are 3 .. 10 rows
short; the same error models in the generated form, 64-bit seeds and run offsets, run counts around the wavefront and the
workgroup, non-finite runs and their wavefront neighbours, undetermined inputs, the drop-in Sim.

Every comparison is against the NumPy restatement (tests/magcal_ref.py) or the reference library's golden (signs.npz) evaluated on
the host, except where bit-identity under another launch shape is the property.  The tolerance of a record is measured on the
reference side, per record and quantity (magcal_records.bounds): 16 x max(E, S, eps |q|), E the float64 restatement's distance
from the same steps in 80-bit long doubles, S what it moves by when the rows inside a range are permuted.  No cap: at |hi| = 500
the raw sums are 100 x those of the goldens and the restatement itself is 5e-9 from the library.  Nothing here reads a reference
checkout."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, REPO  # noqa: F401  (the suite's paths)
import magcal_ref
import magcal_records as rec
from test_gpu_full_size import _record

pytestmark = pytest.mark.gpu
SEED = 4242
CSV = os.path.join(GOLDEN, 'magcal', 'motion_def_mag_cal.csv')
NAMES = ('soft_iron', 'hard_iron', 'mag_cal')


def _ctx():
    import ginsim
    return ginsim.default_context()


def _outputs(job):
    return job.soft_iron().copy(), job.hard_iron().copy(), job.mag_cal(np.arange(job.runs))


def _given(mag, seg):
    """One launch of the given form on a host series (R, n, 3), mag_cal kept -> (soft_iron, hard_iron, mag_cal)."""
    import ginsim
    ctx = _ctx()
    R, n, _ = mag.shape
    buf = ctx.upload(np.ascontiguousarray(mag.transpose(2, 1, 0)))                 # [3][n][R]
    job = ginsim.MagCalJob(ctx, None, None, R, seg, given=buf, keep=True, n=n)
    try:
        return _outputs(job.run())
    finally:
        job.release()
        buf.free()


def _generated(err, runs, seg, seed=SEED, run_offset=0, also_given=False, series=True):
    """The generated form with an error model, and the series AuxSensorJob materialises for the same seed and run ids.
    -> (outputs, mag (runs, n, 3)[, outputs of the given form on the materialised device buffer])."""
    import ginsim
    ref = rec.truth()['ref_mag']
    aux = ginsim.AuxSensorJob(_ctx(), runs, seed=seed, run_offset=run_offset, ref_mag=ref, mag_err=err).run()
    gen = ginsim.MagCalJob(_ctx(), ref, err, runs, seg, seed=seed, run_offset=run_offset, keep=True)
    giv = ginsim.MagCalJob(_ctx(), None, None, runs, seg, given=aux._bufs['mag'], keep=True, n=aux.n) if also_given else None
    try:
        out = (_outputs(gen.run()), aux.series('mag', np.arange(runs)) if series else None)
        return out + ((_outputs(giv.run()),) if also_given else ())
    finally:
        gen.release()
        aux.release()
        if giv is not None:
            giv.release()


def _per_run(got, want):
    """(R, 3): max |got - want| per run for soft_iron, hard_iron, mag_cal."""
    return np.stack([np.max(np.abs(a - b).reshape(a.shape[0], -1), axis=1) for a, b in zip(got, want)], axis=1)


def _held(got, bd, what, runs=None):
    """Every run finite and within its own bound in all three outputs; -> (worst difference (3,), its share of the bound (3,))."""
    ix = np.arange(got[0].shape[0]) if runs is None else np.asarray(runs)
    for a, b in zip(got, bd['want']):
        assert a.shape == b.shape and np.isfinite(a[ix]).all() and np.isfinite(b[ix]).all(), what
    d, tol = _per_run(got, bd['want'])[ix], bd['tol'][ix]
    share = (d / tol).max(axis=0)
    print('%-28s max |device - restatement|  %.3g %.3g %.3g   tolerance (largest) %.3g %.3g %.3g   worst share of a record\'s bound %.3g %.3g %.3g'
          % ((what,) + tuple(d.max(axis=0)) + tuple(tol.max(axis=0)) + tuple(share)))
    assert np.all(d <= tol), (what, [(int(ix[r]), NAMES[q], d[r, q], tol[r, q]) for r, q in zip(*np.nonzero(d > tol))][:8])
    return d.max(axis=0), share


def _bits(a, b, runs=None):
    return all(np.array_equal(x if runs is None else x[runs], y if runs is None else y[runs]) for x, y in zip(a, b))


def _err(hi, si=None, std=None):
    t = rec.truth()
    return {'si': t['si'] if si is None else si, 'hi': np.asarray(hi, dtype=np.float64), 'std': t['std'] if std is None else std}


def _margins(prefix, d, share):
    out = {}
    for k, name in enumerate(NAMES):
        out['%s_%s' % (prefix, name)] = d[k]
        out['%s_%s_share_of_tol' % (prefix, name)] = share[k]
    return out


# ------------------------------------------------------------------------------------------------- 1. values
def test_values_of_every_record_in_the_given_form():
    """`octants`, `axes`, `levels` on the goldens' two range sets, `octants` on ranges that touch both ends / lie out of series
    order / overlap, and the `short` ranges: one launch per range set, every run another configuration, mag_cal kept.  All three
    outputs finite and within the record's own bound; soft_iron and hard_iron also within bound + lib_vs_restatement of what the
    reference's library gave for the record (signs.npz).
    Measured on the MI355X (the margins file of _record, entry magcal_edges_values), max |device - restatement| for soft_iron /
    hard_iron / mag_cal and the largest share of a record's own bound that any record used:
      octants (full, unequal)  2.3e-13 / 8.8e-09 / 8.8e-09   bounds up to 6.7e-11 / 1.7e-07 / 1.7e-07   share 0.10
      axes                     2.5e-13 / 4.9e-09 / 4.9e-09   bounds up to 6.3e-11 / 1.5e-07 / 1.4e-07   share 0.075
      levels                   3.4e-13 / 3.9e-08 / 3.9e-08   bounds up to 2.5e-10 / 8.2e-07 / 8.1e-07   share 0.097 (the noise-free record at 500)
      ends, order              as `full` to the digit (the same rows at other places of the series)
      overlap                  2.2e-13 / 6.5e-08 / 6.5e-08   bounds up to 2.3e-10 / 7.6e-06 / 7.7e-06   share 0.11
      overlap_ill              1.0e-13 / 1.1e-02 / 6.7e-03   bounds 1.4e-10 / 0.84 / 0.52                share 0.014
      short (3, 4, 10 rows)    1.4e-06 / 7.1e-04 / 2.0e-04   bounds up to 3.2e-05 / 1.6e-02 / 3.8e-03   share 0.22 (x range of 4 rows)
      against libmagcal.so (40 records)  soft_iron 4.6e-13, hard_iron 6.8e-09
    The degree-3 raw moments at |u| ~ 500 cost nothing that the reference's own raw sums do not: the device is as far from the
    float64 restatement as that is from the 80-bit one (E up to 6.1e-9 with noise, 2.5e-8 without)."""
    signs = dict(np.load(os.path.join(GOLDEN, 'magcal', 'signs.npz'), allow_pickle=False))
    lib = {str(k): i for i, k in enumerate(signs['names'])}
    margins, seen, held_to_lib = {}, set(), 0
    for b in rec.value_batches():
        bd = rec.bounds(b['mag'], b['segments'])
        got = _given(b['mag'], b['segments'])
        for g, ix in b['groups'].items():
            d, share = _held(got, bd, '%s / %s' % (b['name'], g), ix)
            key = g if g != 'octants' or b['name'] in ('full', 'unequal') else 'octants_' + b['name']
            for k, v in _margins(key, d, share).items():
                margins[k] = max(margins.get(k, 0.0), v)
            for k, name in enumerate(NAMES):
                margins['%s_%s_tol_largest' % (key, name)] = max(margins.get('%s_%s_tol_largest' % (key, name), 0.0), float(bd['tol'][ix, k].max()))
            seen.add(g)
        for r, k in enumerate(b['names']):
            i = lib.get('%s/%s' % (b['name'], k))
            if i is None:
                continue
            held_to_lib += 1
            dl = np.array([np.max(np.abs(got[0][r] - signs['soft_iron'][i])), np.max(np.abs(got[1][r] - signs['hard_iron'][i]))])
            assert np.all(dl <= bd['tol'][r, :2] + signs['lib_vs_restatement'][i, :2]), (b['name'], k, dl)
            margins['library_soft_iron'] = max(margins.get('library_soft_iron', 0.0), dl[0])
            margins['library_hard_iron'] = max(margins.get('library_hard_iron', 0.0), dl[1])
    assert seen == set(rec.VALUE_GROUPS) | {'short', 'overlap_ill'} and held_to_lib == len(lib) == 40
    print(margins)
    _record('magcal_edges_values', **margins)


# ------------------------------------------------------------------------------------------------- 2. generated form
def test_generated_form_with_the_octant_error_models():
    """MagCalJob(ref_mag, {'si', 'hi', 'std'}) for hi = 500 x the eight sign vectors, 70 runs each (a wavefront and a tail):
    against the restatement on the series AuxSensorJob materialises with the same seed and run ids, the bound measured on that
    series; and the given form on that device buffer is the generated form bit for bit.
    Measured on the MI355X (entry magcal_edges_generated): 3.7e-13 / 8.0e-09 / 8.1e-09, at most 0.11 of a record's bound."""
    worst, share = np.zeros(3), np.zeros(3)
    for k, (name, cfg) in enumerate(rec.octants500_configs()):
        R, seg = 70, rec.UNEQUAL if k % 2 else rec.FULL
        gen, mag, giv = _generated(_err(cfg['hi']), R, seg, run_offset=3 * k, also_given=True)
        assert _bits(gen, giv), name
        d, s = _held(gen, rec.bounds(mag, seg), 'generated ' + name)
        worst, share = np.maximum(worst, d), np.maximum(share, s)
    _record('magcal_edges_generated', **_margins('octants500', worst, share))


# ------------------------------------------------------------------------------------------------- 3. the 64-bit key
@pytest.mark.parametrize('seed,run_offset,low', [(2 ** 63 + 12345, 0, (12345, 0)), (SEED, 2 ** 32 + 7, (SEED, 7))], ids=['seed', 'run_offset'])
def test_high_words_of_the_seed_and_of_the_run_offset_reach_the_rng(seed, run_offset, low):
    """seed = 2**63 + 12345 and run_offset = 2**32 + 7, hi = (-500, 500, -500), 66 runs: the generated form against the restatement
    on AuxSensorJob's series for the same key, the given form on that buffer bit for bit, and other numbers than with the low words
    alone (seed 12345, run_offset 7).
    Measured on the MI355X (entries magcal_edges_key64_seed, _run_offset): 1.8e-13 / 7.7e-09 / 7.7e-09 and 1.7e-13 / 9.1e-09 /
    9.0e-09, at most 0.12 of a record's bound."""
    R, err = 66, _err([-500.0, 500.0, -500.0])
    gen, mag, giv = _generated(err, R, rec.FULL, seed=seed, run_offset=run_offset, also_given=True)
    assert _bits(gen, giv)
    d, s = _held(gen, rec.bounds(mag, rec.FULL), 'key %d / %d' % (seed, run_offset))
    lo, lomag = _generated(err, R, rec.FULL, seed=low[0], run_offset=low[1])
    assert not np.array_equal(mag, lomag)
    for a, b in zip(gen[:2], lo[:2]):
        assert np.isfinite(b).all() and not (a == b).any()
    _record('magcal_edges_key64_' + ('seed' if run_offset == 0 else 'run_offset'), **_margins('hi500', d, s))


# ------------------------------------------------------------------------------------------------- 4. run counts
@pytest.fixture(scope='module')
def launch_1024():
    err = _err([-500.0, 500.0, -500.0])
    return err, _generated(err, 1024, rec.UNEQUAL, series=False)[0]


@pytest.mark.parametrize('R', [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_run_r_of_any_launch_is_run_r_of_a_1024_run_launch(launch_1024, R):
    """The generated form with mag_cal kept at run counts on both sides of a wavefront and of the 256-thread workgroup: run r
    equals, bit for bit in all three outputs, run r of one 1024-run launch (the run ids are global; the [3][rows][R] strides of
    mag_cal and the r >= runs tail of the last workgroup change with R).  For R = 257 also the given form on the materialised
    [3][n][257] buffer: the generated form bit for bit, and every run against the restatement.
    Measured on the MI355X (entry magcal_edges_runs_257): 2.6e-13 / 7.9e-09 / 7.9e-09, at most 0.087 of a record's bound; every
    other comparison of this test is bit for bit."""
    err, big = launch_1024
    if R != 257:
        got = _generated(err, R, rec.UNEQUAL, series=False)[0]
    else:
        got, mag, giv = _generated(err, R, rec.UNEQUAL, also_given=True)
        assert _bits(got, giv)
        d, s = _held(giv, rec.bounds(mag, rec.UNEQUAL), 'given, 257 runs')
        _record('magcal_edges_runs_257', **_margins('hi500', d, s))
    assert all(a.shape[0] == R and np.isfinite(a).all() for a in got)
    assert _bits(got, big, np.arange(R))


# ------------------------------------------------------------------------------------------------- 5. non-finite runs
def test_non_finite_runs_and_their_wavefront_neighbours():
    """A 130-run batch of `octants` records, one non-finite sample in the runs at lanes 0, 31, 32, 63, 64 (and 1, 30, 33, 62, 65,
    129): a NaN at the first / a middle / the last row of each of the three ranges, a +inf, a -inf.  The masks of soft_iron,
    hard_iron and mag_cal of those runs equal the restatement's (every element of every output: the sensitivities couple the
    ranges); every other run is bit-identical to the same batch launched with those runs left finite; and that launch, which
    comes after, is within the records' bounds in every run.
    Measured on the MI355X (entry magcal_edges_after_nonfinite): 2.6e-13 / 6.1e-09 / 6.0e-09, at most 0.098 of a record's bound."""
    b, clean = rec.nonfinite_batch()
    bad = np.array(sorted(b['poisoned']))
    ok = np.setdiff1d(np.arange(130), bad)
    got = _given(b['mag'], b['segments'])
    want = magcal_ref.calibrate_series(b['mag'][bad], b['segments'])
    for name, a, w in zip(NAMES, got, want):
        assert np.array_equal(np.isfinite(a[bad]), np.isfinite(w)), name
        assert np.array_equal(np.isnan(a[bad]), np.isnan(w)), name
        assert (~np.isfinite(a[bad])).reshape(len(bad), -1).any(axis=1).all() and np.isfinite(a[ok]).all(), name
    after = _given(clean, b['segments'])
    assert _bits(got, after, ok)
    d, s = _held(after, rec.bounds(clean, b['segments']), 'after the non-finite launch')
    _record('magcal_edges_after_nonfinite', **_margins('octants', d, s))


# ------------------------------------------------------------------------------------------------- 6. undetermined inputs
def test_undetermined_inputs_leave_their_neighbours_and_the_next_launch_alone():
    """An x range of 1 row, of 2 rows, the same range given for two axes (every run of such a launch); and, inside a 72-run batch
    on the whole rotations, a run whose x-range rows are multiplied by 0 (a plane through the origin: M^T 1 = 0, M^T M = 0) and a
    run whose y-range rows are its x-range rows.  The launches return, the other 70 runs are bit-identical to the batch without
    those two, and the launch that follows is within its records' bounds.

    The VALUES and the non-finite MASKS of the undetermined runs are not compared: on these inputs the reference's libmagcal.so
    and the restatement themselves disagree (1-row range and twice-the-same range: different non-finite masks; 2-row range: finite
    in both, soft_iron 1.5 apart).  The normal equations are singular in exact arithmetic and the result is whatever rounding
    leaves of them; the device sums in another order.  What the device gave is printed (MI355X: 1-row x range: the first two
    rows of soft_iron finite -- the fused multiply-adds leave a non-zero pivot -- where the restatement has NaN everywhere, the
    rest NaN; 2-row x range: finite everywhere and up to 1.5 from the restatement in soft_iron; the same range twice: soft_iron
    equal to the restatement's in the digits printed, hard_iron NaN in most runs and finite in one where the restatement has
    NaN; the zeroed x range NaN in every output, as the restatement)."""
    for b, clean in rec.undetermined_batches():
        got = _given(b['mag'], b['segments'])
        und = b['groups']['undetermined']
        want = magcal_ref.calibrate_series(b['mag'][und], b['segments'])
        for r, run in enumerate(und[:4]):
            print('%s run %d (%s): device soft_iron %s hard_iron %s finite mag_cal rows %d / %d;  restatement soft_iron %s hard_iron %s' % (
                b['name'], run, b['names'][run], got[0][run].ravel(), got[1][run], int(np.isfinite(got[2][run]).all(axis=1).sum()),
                got[2].shape[1], want[0][r].ravel(), want[1][r]))
        if clean is None:
            continue
        ok = np.setdiff1d(np.arange(b['mag'].shape[0]), und)
        after = _given(clean, b['segments'])
        assert _bits(got, after, ok) and all(np.isfinite(a[ok]).all() for a in got)
        _held(after, rec.bounds(clean, b['segments']), 'after the undetermined launches')


# ------------------------------------------------------------------------------------------------- 7. through the drop-in Sim
def test_sim_with_a_hard_iron_of_500_in_a_flipping_octant():
    """Sim with set_mag_error({'si': si, 'hi': [-500, 500, -500]}) and MagCal(segments=...), 8 runs: dmgr.soft_iron / hard_iron /
    mag_cal against the restatement on dmgr.mag, within the bound of that series.  The x and z normals are negated in every run.
    Measured on the MI355X (entry magcal_edges_sim): 1.5e-13 / 4.4e-09 / 4.4e-09, at most 0.050 of a record's bound."""
    from gnss_ins_sim.sim import imu_model, ins_sim
    from demo_algorithms.mag_calibrate_device import MagCal
    t = dict(np.load(os.path.join(GOLDEN, 'magcal', 'truth.npz'), allow_pickle=False))
    R, fs = 8, float(t['fs'])
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=9, gps=False)
    imu.set_mag_error({'si': t['si'].copy(), 'hi': np.array([-500.0, 500.0, -500.0])})
    sim = ins_sim.Sim([fs, 0.0, fs], CSV, ref_frame=1, imu=imu, algorithm=MagCal(segments=rec.FULL), seed=SEED, geo_mag_n=t['geo_mag_n'])
    sim.run(R)
    d = sim.dmgr
    mag = np.stack([d.mag.data[r] for r in range(R)])
    assert np.allclose(mag.mean(axis=(0, 1)) / 500.0, t['si'] @ np.array([-1.0, 1.0, -1.0]), atol=0.05)       # the error model arrived
    got = (np.stack([d.soft_iron.data['algo0_%d' % r] for r in range(R)]), np.stack([d.hard_iron.data['algo0_%d' % r] for r in range(R)])[:, 0],
           np.stack([d.mag_cal.data['algo0_%d' % r] for r in range(R)]))
    ch = rec.choices(mag, rec.FULL)
    assert np.array_equal(ch['flip'], np.tile([True, False, True], (R, 1)))
    worst, share = _held(got, rec.bounds(mag, rec.FULL), 'Sim, hi = (-500, 500, -500)')
    _record('magcal_edges_sim', **_margins('hi500', worst, share))
