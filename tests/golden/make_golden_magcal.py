#!/usr/bin/env python3
"""Golden vectors of the magnetometer calibration by EXECUTING the unmodified reference: its Sim on motion_def_mag_cal.csv (9-axis,
set_mag_error with a non-trivial si and hi = [10, 10, 10]) with np.random.randn replaced by oracle.ref_shim (the engine's Philox
normals in the reference's call order, mag=True as the t3_mag9_* cases of make_golden.py), 3 runs; then the reference's own
demo_algorithms/mag_calibrate_lib/libmagcal.so called through ctypes exactly as mag_calibrate.py:77-86 calls it, with fixed row
ranges in place of the six prompts.  MagCal.run itself is not executed: it blocks on input() and opens a plot.

    cd /some/dir/outside/the/checkout && python /path/to/tests/golden/make_golden_magcal.py /path/to/reference   -> tests/golden/magcal/
    ... make_golden_magcal.py /path/to/reference signs      -> tests/golden/magcal/signs.npz alone (no Sim run; nothing else is rewritten)

Run it from a working directory outside the checkout (it sets sys.dont_write_bytecode: nothing is left behind in either tree).

  truth.npz            what the cases share: ref_mag, ref_gyro, geo_mag_n (the WMM value of the day the file was made), si, hi, std,
                       the seed; motion_def_mag_cal.csv next to it is the reference's profile as it is
  full.npz             the three whole rotations (samples 2007-3007, 7007-8007, 12007-13007)
  arc.npz              600 samples of each: one 360 degree turn at 60 deg/s
  unequal.npz          ranges of 1000, 700 and 693 samples
  norot.npz            the z range over a stretch without rotation: whatever the reference's divisions give (compared by mask)
  signs.npz            OUTPUTS only (soft_iron, hard_iron, lib_vs_restatement per record, the record names) of libmagcal.so on the
                       records of tests/magcal_records.signs_records(): hard iron of 500 uT in all eight octants, si with its rows
                       permuted, mirrored, rotated 45 +- 1 degrees about z -- every sign pattern of the three normals, every
                       component selected by vecMax.  The inputs are rebuilt by the builder.  Made on its own (argument `signs`):
                       the five files above are not rewritten by it, and a run without the argument does not write it.
Every other case holds, for 3 runs: the rows of each range, soft_iron / hard_iron / mag_cal from libmagcal.so, the ranges, and two measured
spreads, both reference-side only:
  lib_vs_restatement   max |delta| of (si, hi, mag_cal) between libmagcal.so and tests/magcal_ref.py
  reorder_spread       max |delta| of the restatement's (si, hi, mag_cal) over 20 random permutations of the rows inside each range
                       (sums change order, max / min do not): what another summation order is worth
"""
import ctypes
import os
import sys

sys.dont_write_bytecode = True

import numpy as np      # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'magcal')
SEED = 20261016
RUNS = 3
FS = 100.0
SI = np.array([[1.02, 0.01, -0.02], [0.03, 0.97, 0.01], [-0.01, 0.02, 1.05]])
HI = np.array([10.0, 10.0, 10.0])
CASES = {
    'full': ((2007, 3007), (7007, 8007), (12007, 13007)),
    'arc': ((2200, 2800), (7300, 7900), (12100, 12700)),
    'unequal': ((2007, 3007), (7100, 7800), (12207, 12900)),
    'norot': ((2007, 3007), (7007, 8007), (500, 1000)),
}


def lib_calibrate(lib, mag, seg):
    """mag_calibrate.py:57, 77-88 with the ranges given."""
    (x0, xf), (y0, yf), (z0, zf) = seg
    mag = mag.copy()
    si = np.zeros((3, 3))
    si_ptr = si.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    hi = np.zeros((1, 4))
    hi_ptr = hi.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    mx = mag[x0:xf, :].ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    my = mag[y0:yf, :].ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    mz = mag[z0:zf, :].ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    iRowNum = np.array((xf - x0, yf - y0, zf - z0), dtype='int32')
    iRowNum_ptr = iRowNum.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    lib.MagCalibrate(si_ptr, hi_ptr, mx, my, mz, iRowNum_ptr)
    return si, hi, np.vstack([mag[x0:xf], mag[y0:yf], mag[z0:zf]])


def spread(a, b):
    """max |a - b| over the elements finite in both (0 when there is none); the non-finite ones are compared by mask elsewhere."""
    ok = np.isfinite(a) & np.isfinite(b)
    return float(np.max(np.abs(a[ok] - b[ok]))) if ok.any() else 0.0


def signs(ref):
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    import magcal_ref
    import magcal_records
    lib = ctypes.cdll.LoadLibrary(os.path.join(ref, 'demo_algorithms', 'mag_calibrate_lib', 'libmagcal.so'))
    names, si, hi, lvr, same = [], [], [], [], True
    for name, mag, seg in magcal_records.signs_records():
        s, h, cal = lib_calibrate(lib, mag, seg)
        rs = magcal_ref.calibrate_series(mag, seg)
        names.append(name)
        si.append(s)
        hi.append(h[0])
        lvr.append([spread(s, rs[0]), spread(h[0], rs[1]), spread(cal, rs[2])])
        same = same and all(np.array_equal(np.isfinite(a), np.isfinite(b)) for a, b in ((s, rs[0]), (h[0], rs[1]), (cal, rs[2])))
    path = os.path.join(OUT, 'signs.npz')
    np.savez_compressed(path, names=np.array(names), soft_iron=np.stack(si), hard_iron=np.stack(hi), lib_vs_restatement=np.array(lvr),
                        mask_same=same)
    print('%-12s %7.1f KB  %d records  masks equal %-5s lib_vs_restatement (worst) %s' % (
        'signs.npz', os.path.getsize(path) / 1024, len(names), same, np.max(np.array(lvr), axis=0)))


def main(ref):
    sys.path.insert(0, ref)
    sys.path.insert(1, REPO)
    sys.path.insert(2, os.path.join(REPO, 'tests'))
    from gnss_ins_sim.sim import imu_model, ins_sim
    from gnss_ins_sim.geoparams import geomag
    from oracle.ref_shim import RandnShim, injected
    import magcal_ref
    csv = os.path.join(ref, 'demo_motion_def_files', 'motion_def_mag_cal.csv')
    os.makedirs(OUT, exist_ok=True)
    with open(csv) as f, open(os.path.join(OUT, 'motion_def_mag_cal.csv'), 'w') as g:
        g.write(f.read())
    imu = imu_model.IMU(accuracy='mid-accuracy', axis=9, gps=False)
    imu.mag_err = dict(imu.mag_err)             # set_mag_error writes into the module's built-in model otherwise
    imu.set_mag_error({'si': SI.copy(), 'hi': HI.copy()})
    sim = ins_sim.Sim([FS, 0.0, FS], csv, ref_frame=1, imu=imu, mode=None, env=None, algorithm=None)
    # the number of samples: one run of the reference without noise injection tells it
    sim0 = ins_sim.Sim([FS, 0.0, FS], csv, ref_frame=1, imu=imu, mode=None, env=None, algorithm=None)
    sim0.run(1)
    n = sim0.dmgr.ref_mag.data.shape[0]
    shim = RandnShim(SEED, n, imu.accel_err['b_corr'], imu.gyro_err['b_corr'], mag=True)
    with injected(shim):
        sim.run(RUNS)
    assert shim.run == RUNS and not shim.queue
    d = sim.dmgr
    mag = np.stack([d.mag.data[i] for i in range(RUNS)])
    gm = geomag.GeoMag("WMM.COF")
    f = gm.GeoMag(32.0, 120.0, 0.0)
    np.savez_compressed(os.path.join(OUT, 'truth.npz'), seed=SEED, runs=RUNS, fs=FS, n=n, si=SI, hi=HI, std=np.asarray(imu.mag_err['std'], dtype=np.float64) * np.ones(3),
                        ref_mag=d.ref_mag.data, ref_gyro=d.ref_gyro.data, geo_mag_n=np.array([f.bx, f.by, f.bz]) / 1000.0,
                        mag_rows=np.array([0, 1, n // 2, n - 1]), mag_at_rows=mag[:, [0, 1, n // 2, n - 1]])
    lib = ctypes.cdll.LoadLibrary(os.path.join(ref, 'demo_algorithms', 'mag_calibrate_lib', 'libmagcal.so'))
    rng = np.random.RandomState(SEED)
    for name, seg in CASES.items():
        res = [lib_calibrate(lib, mag[r], seg) for r in range(RUNS)]
        si, hi, cal = (np.stack([x[k] for x in res]) for k in range(3))
        rows = [mag[:, a:b] for a, b in seg]
        rs = magcal_ref.calibrate(*rows)
        lvr = [spread(si, rs[0]), spread(hi[:, 0], rs[1]), spread(cal, rs[2])]
        ro = [0.0, 0.0, 0.0]
        for _ in range(20):
            perms = [rng.permutation(b - a) for a, b in seg]
            rp = magcal_ref.calibrate(*[m[:, p] for m, p in zip(rows, perms)])
            back = np.concatenate([np.argsort(p) + off for p, off in zip(perms, np.cumsum([0] + [b - a for a, b in seg[:-1]]))])
            ro = [max(ro[0], spread(rp[0], rs[0])), max(ro[1], spread(rp[1], rs[1])), max(ro[2], spread(rp[2][:, back], rs[2]))]
        mask_same = all(np.array_equal(np.isfinite(a), np.isfinite(b)) for a, b in ((si, rs[0]), (hi[:, 0], rs[1]), (cal, rs[2])))
        finite = bool(np.isfinite(si).all() and np.isfinite(hi).all() and np.isfinite(cal).all())
        path = os.path.join(OUT, name + '.npz')
        np.savez_compressed(path, seed=SEED, segments=np.array(seg), rows_x=rows[0], rows_y=rows[1], rows_z=rows[2],
                            soft_iron=si, hard_iron=hi, mag_cal=cal, lib_vs_restatement=np.array(lvr), reorder_spread=np.array(ro),
                            finite=finite, mask_same=mask_same)
        print('%-12s %7.1f KB  finite %-5s masks equal %-5s lib_vs_restatement %s  reorder_spread %s' % (
            name + '.npz', os.path.getsize(path) / 1024, finite, mask_same, np.array(lvr), np.array(ro)))


if __name__ == '__main__':
    reference = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.environ['GNSS_INS_SIM_REFERENCE'])
    if sys.argv[2:] == ['signs']:
        signs(reference)
    elif sys.argv[2:]:
        sys.exit('usage: make_golden_magcal.py REFERENCE [signs]')
    else:
        main(reference)
