"""The bands the consistency checkpoints of InsLoose are held to (test infrastructure; no test in it, imported by tests only):
tests/test_ins_loose_cons_oracle.py measures them on the restatement, tests/test_gpu_ins_loose_cons.py holds the device to them."""
import numpy as np

BAND = (0.7, 1.4)                                       # the project's band for RMS error / predicted sigma
NEES_BAND = (3 * BAND[0] ** 2, 3 * BAND[1] ** 2)        # the same band on a 3-dimensional normalised squared error: [1.47, 5.88]
SETTLED = 15.0                                          # seconds: from here on both ends of the bands hold, before it the upper only


def in_bands(time, ratio, nees, lower=True):
    """Assert the bands on (m, 9) ratios and (m, 3) block NEES at the instants `time`; lower: hold the lower ends from SETTLED on."""
    late = np.asarray(time) >= SETTLED
    assert late.any() and not late.all()
    assert np.all(ratio <= BAND[1]), ratio
    assert np.all(nees <= NEES_BAND[1]), nees
    if lower:
        assert np.all(ratio[late] >= BAND[0]), ratio[late]
        assert np.all(nees[late] >= NEES_BAND[0]), nees[late]
