"""The checkpoint record of an InsLoose job against the restatement of a dump (test infrastructure; no test in it, imported by tests
only): tests/test_gpu_ins_loose_cons.py, tests/test_gpu_ins_loose_attitude.py and the vibration cases of
tests/test_gpu_ins_loose_all_cons_edges.py on an ins_loose_dump.Dump that has an odometer."""
import numpy as np

import ins_loose_aided_cases as ac
import ins_loose_cases as cs
import ins_loose_cons_ref as cref

COLUMNS = ['count'] + ['P_' + s for s in cref.STATES] + ['e2_' + s for s in cref.STATES[:9]] + ['nes_' + s for s in cref.STATES[:9]] \
    + ['nees_r', 'nees_v', 'nees_psi']


def nav_of(truth):
    return np.concatenate([truth['ref_att'], truth['ref_pos'], truth['ref_vel']], axis=1)


def restated(d, mask, every, samples, runs=None, accel=None, dtype=np.float64):
    """The restatement's record of Dump d over `runs` (None: all) at `samples`."""
    r = np.arange(d.runs) if runs is None else np.asarray(runs)
    acc = d.accel if accel is None else accel
    return cref.run(d.rf, d.fs, d.gyro[r], acc[r], d.ini, d.model, nav_of(d.truth), samples, None if d.gps is None else d.gps[r], d.stamps,
                    d.truth['gps_visibility'], dtype=dtype, odo=d.odo[r], aid=ac.aid(mask, every) if mask else None)


def cons_held(what, dev, d, mask, every, samples, **kw):
    """Assert the device record dev (m, 43) against the restatement within 16 x the restatement's own float64 error; print both."""
    lo, hi = restated(d, mask, every, samples, **kw), restated(d, mask, every, samples, dtype=np.longdouble, **kw)
    bound = cs.PARITY_MARGIN * cref.deviation(lo, hi)
    got = cref.deviation(dev, lo)
    worst = int(np.argmax(got / np.maximum(bound, 1e-300)))
    print('%s rf%d mask %d: largest deviation %.2e, smallest bound %.2e; tightest column %s %.2e (bound %.2e)'
          % (what, d.rf, mask, got.max(), bound[1:].min(), COLUMNS[worst], got[worst], bound[worst]))
    assert not dev[:, 37:].any()
    for k in range(37):
        assert got[k] <= bound[k], (what, COLUMNS[k], got[k], bound[k])
    return lo


def record(job):
    return job.consistency().pack()
