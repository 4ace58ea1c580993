"""The five series analyses on ONE context: their finishing launches write into one pinned result buffer of the context
(csrc/api_series.hip, result_buffer), which grows to the largest result asked for so far and is never shrunk.  What could go wrong
is a family reading results of another family's size or epoch after a regrow, so the sequence below makes the buffer be created,
grow twice and then serve three smaller results, and every result is compared bit for bit with the same call on a context of its own.

The sizes, from the growth rule `doubles + doubles / 4 + 64`:
  1. allan_var, 1 series, n = 90, fs = 1: 9 averaging factors in one decade level, 9 sums; the buffer is created with 75 doubles
     (the issue that asked for this test counted 10 factors and 18 doubles, 86; the plan, ginsim.allan_plan, reports 9 -- m = 10
     would open a second decade, and ceil(log10(90 // 9)) is 1 -- and calls 2 and 3 exceed either capacity, so n stays)
  2. welch_psd, 1 series, n = 512, nperseg = 256: 129 doubles > 75, grows to 225
  3. welch_csd, 2 series, pairs (0,0), (0,1), (1,0): 4 * 3 * 129 = 1548 doubles > 225, grows to 1999
  4. lpsd, 1 series, n = 2048, nperseg = 64: fewer bins than 1999, no growth
  5. oallan_var, 2 series, n = 90: 9 * (2 + 1) = 27 doubles
  6. allan_var as in 1: must still be the first result."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAIRS = [(0, 0), (0, 1), (1, 0)]


def _steps():
    import ginsim
    rng = np.random.default_rng(20261021)
    a90, a512, b512, a2048, b90 = (rng.standard_normal(s) for s in ((1, 90), (1, 512), (2, 512), (1, 2048), (2, 90)))
    allan = ('allan_var', lambda c: ginsim.allan_var_host(c, a90, 1.0))
    return [allan,
            ('welch_psd', lambda c: ginsim.welch_psd_host(c, a512, 1.0, 256)),
            ('welch_csd', lambda c: (lambda r: (r.pxx, r.pyy, r.pxy, r.freq))(ginsim.welch_csd_host(c, b512, 1.0, PAIRS, 256))),
            ('lpsd', lambda c: ginsim.lpsd_host(c, a2048, 1.0, 64)),
            ('oallan_var', lambda c: ginsim.oallan_var_host(c, b90, 1.0)),
            allan]


def test_families_share_the_result_buffer_through_its_growths():
    import ginsim
    steps = _steps()
    assert ginsim.allan_plan(0, 90, 1, 90, 1.0)[0] == 9                 # the count the docstring's capacities start from
    shared = ginsim.Context(0)
    try:
        got = [call(shared) for _, call in steps]
    finally:
        shared.close()
    assert got[1][0].shape == (1, 129) and got[2][0].shape == (3, 129) and got[4][0].shape == (2, 9) and got[3][0].shape[1] < 1999
    for k, ((name, call), mine) in enumerate(zip(steps, got)):
        own = ginsim.Context(0)
        try:
            want = call(own)
        finally:
            own.close()
        assert len(mine) == len(want)
        differ = [int(np.sum(np.ascontiguousarray(m).view(np.uint8) != np.ascontiguousarray(w).view(np.uint8))) if m.shape == w.shape
                  else -1 for m, w in zip(mine, want)]
        print('step %d %-10s shapes %s: differing bytes per output %s' % (k + 1, name, [m.shape for m in mine], differ))
        assert all(np.all(np.isfinite(m)) for m in mine)
        assert differ == [0] * len(mine), (k + 1, name)
