"""Shared inputs of the aided-InsLoose tests (tests/test_ins_loose_aided_oracle.py on the CPU, tests/test_gpu_ins_loose_aided.py on the
device): the outage profile's truth with the odometer's, the odometer model, and the constants the CPU test measures and
the device test is held to."""
import functools

import numpy as np

import ins_loose_cases as cs

ODO_ERR = {'scale': 0.99, 'stdv': 0.1}
NHC_STD = 0.05

# Measured by tests/test_ins_loose_aided_oracle.py::test_restatement_consistency / test_outage_benefit: 1024 runs drawn from the filter's
# own model with np.random.default_rng(ins_loose_cases.CONSISTENCY_SEED) (accel, gyro, GPS as the unaided case draws them, then the
# odometer), the outage profile at 20 Hz with 2 Hz GPS, 'mid-accuracy' IMU, ODO_ERR, NHC_STD, a block at every sample, ref_frame 1.
# RMS end error over sqrt(mean pdiag_end) for the 15 states.  Mask 1 lies in [0.7, 1.4]; mask 7 is bounded above only (see the test).
# ref_frame 1, the LEVEL outage profile only; for the tilted profile and ref_frame 0 see ins_loose_mag_cases.CONSISTENCY_BY_PROFILE.
CONSISTENCY_RATIOS = {
    1: (1.016, 1.016, 0.931, 1.009, 0.986, 0.941, 0.951, 0.980, 1.014, 1.017, 1.014, 0.999, 0.999, 0.972, 0.980),
    7: (0.981, 0.911, 0.475, 0.946, 0.832, 0.694, 0.855, 0.903, 0.992, 1.005, 1.011, 1.005, 0.998, 0.972, 0.978),
}
# Horizontal position 1 sigma [m] across those runs at the outage's first sample / its last sample / 5 s later / the profile's end,
# for masks 0 (GPS only), 1 (+ odometer) and 7 (+ odometer + NHC).
OUTAGE_TABLE = {
    0: (0.164, 1.237, 0.536, 0.505),
    1: (0.124, 0.799, 0.370, 0.368),
    7: (0.074, 0.186, 0.203, 0.225),
}


@functools.lru_cache(maxsize=None)
def outage_truth(fs, ref_frame, fs_gps, n=None, profile=cs.OUTAGE_CSV):
    """ins_loose_cases.outage_truth with 'ref_odo' (n,), the truth forward speed."""
    import ginsim
    from ginsim import workloads
    ini, truth, stamps = cs.outage_truth(fs, ref_frame, fs_gps, n, profile)
    ini_m, seg = workloads.parse_motion(profile)
    raw = ginsim.pathgen(ini_m, seg, fs, fs_gps, workloads.HIGH_MOBILITY, ref_frame, gps=True)
    truth = dict(truth, ref_odo=np.ascontiguousarray(raw['odo'][:truth['ref_accel'].shape[0], 2]))
    truth['ref_odo'].setflags(write=False)
    return ini, truth, stamps


def outage_samples(truth, stamps, fs, fs_gps):
    """The four instants of OUTAGE_TABLE as IMU sample indices: the first invisible fix, the sample before the first visible fix
    after it, 5 s after that, the last sample."""
    hidden = np.nonzero(np.asarray(truth['gps_visibility']) == 0)[0]
    first, last = int(stamps[hidden[0]]), int(stamps[hidden[-1]]) + int(round(fs / fs_gps)) - 1
    return [first, last, last + 1 + int(round(5 * fs)), truth['ref_accel'].shape[0] - 1]


def aid(mask, every=1, odo_err=ODO_ERR, nhc_std=NHC_STD, **kw):
    """The aiding numbers (ginsim.ins_loose.aiding_model) of a row mask: 1 odometer, 6 the two constraints, 7 both."""
    assert mask in (1, 6, 7)
    from ginsim.ins_loose import aiding_model
    return aiding_model(odo_err, dict({'odo': bool(mask & 1), 'nhc': bool(mask & 6), 'every': every, 'nhc_std': nhc_std}, **kw))


def aid_options(mask, every=1, nhc_std=NHC_STD, **kw):
    """The same as the `aid` dict InsLooseJob takes."""
    return dict({'odo': bool(mask & 1), 'nhc': bool(mask & 6), 'every': every, 'nhc_std': nhc_std}, **kw)


def aid_kw(mask, every=1, **kw):
    """The keywords of an InsLooseJob aided by the rows of `mask`, under kw; mask 0: kw alone, no aiding argument at all."""
    return dict(dict(odo_err=ODO_ERR, aid=aid_options(mask, every)), **kw) if mask else kw
