"""Hand-built magnetometer records for the soft / hard-iron calibration, from seeds (test infrastructure: the golden's maker
tests/golden/make_golden_magcal.py and the tests build the same records with these functions; signs.npz stores outputs only).

    value_batches(), nonfinite_batch(), undetermined_batches() -> batches; a batch is a dict
        name, mag (R, n, 3) a GIVEN series per run, segments ((x0, xf), (y0, yf), (z0, zf)) rows of `mag`,
        names [R] the configuration of each run, groups {group name: run indices within the batch}
    configs()      -> the configurations behind them, {name: dict(group, si, hi, std, seed)}
    bounds(mag, segments) -> per run and quantity the tolerance a result on that record is held to, measured on the reference side only

Every run of a batch is another configuration (hard-iron octant, axis order of si, noise level), so that one launch mixes them
inside a wavefront and the sign branch of a range's normal diverges lane by lane.  mag = (ref_mag + hi) @ si.T + std * N as
pathgen.mag_gen makes it, ref_mag / si / std from tests/golden/magcal/truth.npz, N from np.random.RandomState(seed of the
configuration).

The ranges are the goldens' (`full`, `unequal`).  For the configurations of `octants` also: `ends` -- rows 2007 .. 13007 cut out
as a series of their own, the x range starting at its row 0 and the z range ending at its row n (rows 0 .. 1000 of the whole
profile do not rotate); `order` -- the profile's three thirds in reverse, so that the z rows come before the x rows; `overlap` --
ranges that share rows.
"""
import os

import numpy as np

import magcal_ref

assert np.finfo(np.longdouble).eps < 2e-19, 'the bound of a record is measured against 80-bit long doubles: this host has none'

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20261016
FACTOR = 16.0                   # the project's factor between a reference-side spread and a device tolerance (test_gpu_magcal._tol)
PERMUTATIONS = 20
FULL = ((2007, 3007), (7007, 8007), (12007, 13007))
UNEQUAL = ((2007, 3007), (7100, 7800), (12207, 12900))
OVERLAP = ((2007, 3007), (2500, 8007), (7500, 13007))
ENDS_ROWS = (2007, 13007)
ENDS = ((0, 1000), (5000, 6000), (10000, 11000))
ORDER_CUTS = (5000, 10000)      # the series is rows [10000, n) + [5000, 10000) + [0, 5000)
NONDIAG = np.array([[1.0, 0.3, -0.3], [0.3, 0.9, 0.3], [-0.3, 0.3, 1.1]])
SIGNS = [(a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)]
VALUE_GROUPS = ('octants', 'axes', 'levels')
# short ranges start half way through a rotation.  Chosen on the CPU among the starts 2007 / 2100 / 2250 / 2300 / 2500 / 2750 / 2900 by
# the bound of bounds() alone: a 3-row x range at 2007 or 2750 has tol = 2e-3 .. 3e-3 of the quantity, at 2500 at most 7.4e-5
SHORT = {'short_x3': ((2500, 2503), FULL[1], FULL[2]), 'short_x4': ((2500, 2504), FULL[1], FULL[2]),
         'short_x10': ((2500, 2510), FULL[1], FULL[2]), 'short_y10': (FULL[0], (7500, 7510), FULL[2]),
         'short_z10': (FULL[0], FULL[1], (12500, 12510))}
# With OVERLAP the y range holds half the x rotation and the z range half the y rotation: in the octants +++ and --- at |hi| = 500
# the y and z normals come out 8 degrees apart, the fitted radius is 179 / 2899 in place of 50, and the float64 restatement is
# 1.3e-4 / 1.5e-2 from the 80-bit one (every other octant record: at most 8.5e-8).  Those two stay in the launch and in the value
# comparison at their own bound, under a group of their own that the 1e-5 condition of the well-determined groups does not cover.
OVERLAP_ILL = ('oct500+++', 'oct500---')
UNDETERMINED = {'undet_1row': ((2500, 2501), FULL[1], FULL[2]), 'undet_2rows': ((2500, 2502), FULL[1], FULL[2]),
                'undet_same_range': (FULL[0], FULL[0], FULL[2])}
NONFINITE_LANES = (0, 31, 32, 63, 64, 1, 30, 33, 62, 65, 129)       # the wavefront edges of a 130-run batch, and their neighbours


def truth():
    t = np.load(os.path.join(HERE, 'golden', 'magcal', 'truth.npz'), allow_pickle=False)
    return {k: t[k] for k in ('ref_mag', 'si', 'std')}


def _sgn(s):
    return ''.join('+' if x > 0 else '-' for x in s)


def _rotz(deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _rotx(deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def configs():
    """{name: dict(group, si, hi, std, seed)} in a fixed order; the seed of a configuration is SEED + its position."""
    t = truth()
    si0, std0 = t['si'], float(t['std'][0])
    out = {}

    def add(group, name, si, hi, std=std0):
        out[name] = dict(group=group, si=np.array(si, dtype=np.float64), hi=np.array(hi, dtype=np.float64), std=float(std), seed=SEED + len(out))
    for mag in (500.0, 10.0, 100.0):
        for s in SIGNS:
            add('octants', 'oct%d%s' % (mag, _sgn(s)), si0, mag * np.array(s))
    variants = (('cyc1', si0[[1, 2, 0]]), ('cyc2', si0[[2, 0, 1]]), ('mirror', np.diag([1.0, -1.0, 1.0]) @ si0),
                ('rotz44', _rotz(44.0) @ si0), ('rotz46', _rotz(46.0) @ si0))
    for vn, si in variants:
        for s in ((1, -1, 1), (-1, 1, -1)):
            add('axes', '%s%s' % (vn, _sgn(s)), si, 500.0 * np.array(s))
    one = np.ones(3)
    add('levels', 'hi0', si0, 0.0 * one)
    add('levels', 'hi100', si0, 100.0 * one)
    add('levels', 'std5_hi0', si0, 0.0 * one, std=5.0)
    add('levels', 'std5_hi500', si0, 500.0 * np.array([1, -1, -1]), std=5.0)
    add('levels', 'std0_hi10', si0, 10.0 * np.array([-1, 1, 1]), std=0.0)
    add('levels', 'std0_hi500', si0, 500.0 * np.array([1, 1, -1]), std=0.0)
    add('levels', 'nondiag_hi10', NONDIAG, 10.0 * one)
    add('levels', 'nondiag_hi500', NONDIAG, 500.0 * np.array([-1, -1, 1]))
    # the y normal about (0, 0.87, -0.5): its largest, middle and smallest components are y, z, x, with y and z of opposite sign --
    # a vecMax that compared the third component with the first instead of with the running maximum picks z and flips wrongly
    for s in ((1, -1, 1), (-1, 1, -1)):
        add('axes', 'rotx-30%s' % _sgn(s), _rotx(-30.0) @ si0, 500.0 * np.array(s))
    return out


def series(cfg, ref_mag):
    """(n, 3): pathgen.mag_gen's expression with the configuration's own noise."""
    noise = np.random.RandomState(cfg['seed']).standard_normal(ref_mag.shape)
    return (ref_mag + cfg['hi']) @ cfg['si'].T + cfg['std'] * noise


def _batch(name, names, mag, segments, cfgs):
    groups = {}
    for i, nm in enumerate(names):
        groups.setdefault(cfgs[nm]['group'], []).append(i)
    return dict(name=name, mag=mag, segments=tuple((int(a), int(b)) for a, b in segments), names=list(names),
                groups={g: np.array(ix) for g, ix in groups.items()})


def _reordered(mag):
    a, b = ORDER_CUTS
    n = mag.shape[1]
    seg = tuple((lo + off, hi + off) for (lo, hi), off in zip(FULL, (n - a, n - a - b, -b)))
    return np.concatenate([mag[:, b:], mag[:, a:b], mag[:, :a]], axis=1), seg


def value_batches():
    """The batches compared by value: `octants`, `axes`, `levels` on the goldens' ranges, `octants` on the three other range
    sets, and the `short` ranges."""
    t, cfgs = truth(), configs()
    names = [k for k in cfgs if cfgs[k]['group'] in VALUE_GROUPS]
    mag = np.stack([series(cfgs[k], t['ref_mag']) for k in names])
    out = [_batch('full', names, mag, FULL, cfgs), _batch('unequal', names, mag, UNEQUAL, cfgs)]
    octs = [i for i, k in enumerate(names) if cfgs[k]['group'] == 'octants']
    onames, omag = [names[i] for i in octs], mag[octs]
    out.append(_batch('ends', onames, np.ascontiguousarray(omag[:, ENDS_ROWS[0]:ENDS_ROWS[1]]), ENDS, cfgs))
    out.append(_batch('order', onames, *_reordered(omag), cfgs=cfgs))
    b = _batch('overlap', onames, omag, OVERLAP, cfgs)
    ill = np.array([onames.index(k) for k in OVERLAP_ILL])
    b['groups'] = {'octants': np.setdiff1d(b['groups']['octants'], ill), 'overlap_ill': ill}
    out.append(b)
    few = [names.index(k) for k in ('oct500+++', 'oct500-+-', 'oct10+--', 'oct100--+', 'cyc1+-+', 'nondiag_hi500')]
    for sn, seg in SHORT.items():
        b = _batch(sn, [names[i] for i in few], mag[few], seg, cfgs)
        b['groups'] = {'short': np.arange(len(few))}
        out.append(b)
    return out


def octants500_configs():
    cfgs = configs()
    return [(k, cfgs[k]) for k in cfgs if k.startswith('oct500')]


def signs_records():
    """[(record name, (n, 3) series, segments)] of the records signs.npz holds the reference library's results for: the `octants`
    configurations at |hi| = 500 and the `axes` ones, on the goldens' two range sets."""
    out = []
    for b in value_batches()[:2]:
        for i, k in enumerate(b['names']):
            if k.startswith('oct500') or i in b['groups']['axes']:
                out.append(('%s/%s' % (b['name'], k), b['mag'][i], b['segments']))
    return out


def nonfinite_batch():
    """(batch, clean): 130 runs of `octants` records on the whole rotations; `batch` has one non-finite sample in the runs at
    NONFINITE_LANES -- a NaN at the first / a middle / the last row of each range, a +inf and a -inf -- and `clean` is the same
    batch with those runs left finite.  batch['poisoned'] = {lane: (row, axis, value)}."""
    t, cfgs = truth(), configs()
    octs = [k for k in cfgs if cfgs[k]['group'] == 'octants']
    names = [octs[i % len(octs)] for i in range(130)]
    rng = np.random.RandomState(SEED - 1)
    clean = np.stack([(t['ref_mag'] + cfgs[k]['hi']) @ cfgs[k]['si'].T + cfgs[k]['std'] * rng.standard_normal(t['ref_mag'].shape) for k in names])
    cases = [(row, np.nan) for a, b in FULL for row in (a, (a + b) // 2, b - 1)] + [(FULL[1][0] + 17, np.inf), (FULL[2][1] - 40, -np.inf)]
    mag, poisoned = clean.copy(), {}
    for k, (lane, (row, value)) in enumerate(zip(NONFINITE_LANES, cases)):
        mag[lane, row, k % 3] = value
        poisoned[lane] = (row, k % 3, value)
    b = _batch('nonfinite', names, mag, FULL, cfgs)
    b['groups'], b['poisoned'] = {'nonfinite': np.array(sorted(poisoned))}, poisoned
    return b, clean


def undetermined_batches():
    """Inputs whose result is whatever rounding leaves of an exactly singular system.  [(batch, clean or None)]: three batches
    whose RANGES make every run undetermined (1 row, 2 rows, the same range for two axes; clean is None), and one on the whole
    rotations in which run 5 has its x-range rows multiplied by 0 (a plane through the origin) and run 70 has its y-range rows
    replaced by its x-range rows (the same range twice, by data), with the batch without them."""
    t, cfgs = truth(), configs()
    octs = [k for k in cfgs if cfgs[k]['group'] == 'octants']
    names = [octs[(5 * i) % len(octs)] for i in range(72)]
    rng = np.random.RandomState(SEED - 2)
    clean = np.stack([(t['ref_mag'] + cfgs[k]['hi']) @ cfgs[k]['si'].T + cfgs[k]['std'] * rng.standard_normal(t['ref_mag'].shape) for k in names])
    out = []
    for un, seg in UNDETERMINED.items():
        b = _batch(un, names[:8], clean[:8], seg, cfgs)
        b['groups'] = {'undetermined': np.arange(8)}
        out.append((b, None))
    mag = clean.copy()
    mag[5, FULL[0][0]:FULL[0][1]] *= 0.0
    mag[70, FULL[1][0]:FULL[1][1]] = mag[70, FULL[0][0]:FULL[0][1]]
    b = _batch('undet_rows', names, mag, FULL, cfgs)
    b['groups'] = {'undetermined': np.array([5, 70])}
    out.append((b, clean))
    return out


# ------------------------------------------------------------------------------------------------- the bound of a record
def _delta(a, b):
    return np.max(np.abs(np.asarray(a, dtype=np.longdouble) - b).reshape(a.shape[0], -1), axis=1).astype(np.float64)


def bounds(mag, segments, seed=SEED):
    """The tolerance of each run of a series (R, n, 3) with its ranges, per quantity: dict(tol, E, S, want) with tol, E, S of shape
    (R, 3) -- columns soft_iron, hard_iron, mag_cal -- and want the float64 restatement.

        E   = max |restatement in float64 - restatement in np.longdouble|
        S   = max |delta| of the float64 restatement over PERMUTATIONS seeded permutations of the rows inside each range
        tol = FACTOR * max(E, S, eps * max |quantity|)

    Nothing of it comes from a device."""
    mag = np.asarray(mag, dtype=np.float64)
    rows = [mag[:, a:b] for a, b in segments]
    want = magcal_ref.calibrate(*rows)
    ext = magcal_ref.calibrate(*rows, dtype=np.longdouble)
    with np.errstate(invalid='ignore'):
        E = np.stack([_delta(w, x) for w, x in zip(want, ext)], axis=1)
        S = np.zeros_like(E)
        rng = np.random.RandomState(seed)
        lens = [b - a for a, b in segments]
        for _ in range(PERMUTATIONS):
            perms = [rng.permutation(k) for k in lens]
            rp = magcal_ref.calibrate(*[m[:, p] for m, p in zip(rows, perms)])
            back = np.concatenate([np.argsort(p) + off for p, off in zip(perms, np.cumsum([0] + lens[:-1]))])
            S = np.maximum(S, np.stack([_delta(rp[0], want[0]), _delta(rp[1], want[1]), _delta(rp[2][:, back], want[2])], axis=1))
        size = np.stack([np.max(np.abs(w).reshape(w.shape[0], -1), axis=1) for w in want], axis=1)
        tol = FACTOR * np.maximum(np.maximum(E, S), np.finfo(np.float64).eps * size)
    return dict(tol=tol, E=E, S=S, size=size, want=want)


def choices(mag, segments):
    """What the restatement's data-dependent branches take on each run: idx (R, 3) the component vecMax selects for the x, y, z
    range, flip (R, 3) whether that range's normal is negated, one_signed (R, 3) whether both rotated columns that range's ratio
    takes (max - min of) keep one sign over the range."""
    mag = np.asarray(mag, dtype=np.float64)
    rows = [mag[:, a:b] for a, b in segments]
    pick = [magcal_ref.normal_choice(m) for m in rows]
    orth = np.stack([magcal_ref.points_normal(m) for m in rows], axis=1)
    one = []
    for m, cols in zip(rows, ((2, 1), (2, 0), (1, 0))):
        u = np.einsum('rij,rkj->rki', orth, m)[:, :, cols]
        one.append(np.all((u.min(axis=1) > 0.0) | (u.max(axis=1) < 0.0), axis=1))
    return dict(idx=np.stack([p[0] for p in pick], axis=1), flip=np.stack([p[1] for p in pick], axis=1), one_signed=np.stack(one, axis=1))
