"""The exact Allan reference of tests/allan_exact.py and its tolerance, without a device: the fsum path against the long-double
path, the oracle's list of factors, and the float64 NumPy oracle (oracle/ins_np.py allan_var) against the tolerance on every
input family test_gpu_allan_edges.py uses -- the oracle forms means of unshifted samples, the case the tolerance is derived for,
so it must pass, and on the 1e6-offset rows it comes closest."""
import numpy as np
import pytest

import allan_cases as ac
import allan_exact as ax
from oracle import ins_np


def _oracle_ratio(x, fs):
    ea, tau = ax.exact(x, fs)
    oa, ot = ins_np.allan_var(x, fs)
    np.testing.assert_array_equal(tau, ot)
    tol = ax.bound(x, ea, ax.factors(x.size, fs)[1])
    return ax.ratio(oa, ea, tol), float(np.nanmax(np.abs(oa / ea - 1.0))), tol


def test_factors_are_the_oracles():
    keys = [(n, ac.fs_of(n)) for n in list(ac.LEVEL0) + list(ac.FUSE) + list(ac.FORCED) + list(ac.NONFINITE)] + list(ac.POWERS) + list(ac.NTAU)
    for n, fs in keys:
        mult, levels = ax.factors(n, fs)
        tau = ins_np.allan_var(np.zeros(n), fs)[1]
        np.testing.assert_array_equal(np.array([m * (1.0 / fs) for m in mult]), tau)
        assert levels == (0 if not mult else len(str(mult[-1])))
    keep = ax.sampled_factors(90009, 1.0)
    assert keep == {1, 5, 9, 10, 50, 90, 100, 500, 900, 1000, 5000, 9000, 10000}


@pytest.mark.skipif(not ax.WIDE, reason='long double is not wider than double here: exact() takes the fsum path alone')
@pytest.mark.parametrize('n', [2000, 2521, 10089, 25219])
def test_fsum_equals_long_double(n):
    """Both paths are exact to ~1e-15; their roundings differ (one correctly rounded d per pair against 64-bit bin sums)."""
    fs = ac.fs_of(n)
    for x in ac.rows(40, n, fs):
        a, b = ax.exact_fsum(x, fs), ax.exact_longdouble(x, fs)
        assert np.isfinite(a).all() and a.size == len(ax.factors(n, fs)[0])
        np.testing.assert_allclose(a, b, rtol=1e-13)
    for x in ac.nonfinite_rows(n, fs):
        a, b, o = ax.exact_fsum(x, fs), ax.exact_longdouble(x, fs), ins_np.allan_var(x, fs)[0]
        np.testing.assert_array_equal(np.isfinite(a), np.isfinite(b))
        np.testing.assert_array_equal(np.isfinite(a), np.isfinite(o))
        k = np.isfinite(a)
        np.testing.assert_allclose(a[k], b[k], rtol=1e-13)
    only = ax.sampled_factors(n, fs)
    part = ax.exact_fsum(ac.rows(40, n, fs)[1], fs, only)
    full = ax.exact_fsum(ac.rows(40, n, fs)[1], fs)
    mult = ax.factors(n, fs)[0]
    for i, m in enumerate(mult):
        assert (part[i] == full[i]) if m in only else np.isnan(part[i])


@pytest.mark.parametrize('n', [2520 * 4, 2520 * 4 + 9, 2520 * 40 - 1, 25200 * 3 + 2527, 252000 + 10])
def test_oracle_is_within_the_bound_on_the_offset_and_ramp_rows(n):
    """The inputs of test_allan_chunk_boundaries_strided_series_and_drift (test_gpu_allan.py holds the device to 2e-7 of the oracle
    there because the ORACLE's means round): row 0 has an offset of 1e6 and no ramp -- the oracle comes within 0.025 of the bound,
    3.8e-9 at worst; the ramp rows have an Allan variance so large that the bound is the 1e-10 floor and the oracle's error 1e-5 of
    it."""
    fs = 100.0
    t = np.arange(n) / fs
    for s in range(4):
        x = ac.series(10 + s, n) + 1.0e6 * (s + 1) + 3.0e3 * s * t
        r, rel, tol = _oracle_ratio(x, fs)
        print('n %d row %d: oracle / exact - 1 = %.2e, %.3g of the bound (%.2e .. %.2e)' % (n, s, rel, r, tol.min(), tol.max()))
        assert r <= 1.0, (s, r)
        assert tol.min() >= 1e-10 and tol.max() < 4e-7
        if s == 0:
            assert tol.max() > 1e-8                 # the offset row is where the derived term counts


@pytest.mark.parametrize('n', [2559, 25219, 100799])
def test_oracle_is_within_the_bound_on_the_edge_rows(n):
    """The four row families of test_gpu_allan_edges.py, and what the bound makes of them: the floor where there is no offset
    (plain, scaled by 1e-9: the bound is scale invariant) or a ramp, the derived term on the 1e6 offset."""
    fs = ac.fs_of(n)
    rws = ac.rows(40, n, fs)
    tols = []
    for x in rws:
        r, rel, tol = _oracle_ratio(x, fs)
        assert r <= 1.0, r
        tols.append(tol)
    assert tols[0].max() < 1.2e-10 and tols[3].max() < 1.2e-10 and tols[1].max() > 1e-8
    # a result that is off by 1e-6 in one factor is outside it on every row
    for x, tol in zip(rws, tols):
        ea, _ = ax.exact(x, fs)
        bad = ea.copy()
        bad[len(bad) // 2] *= 1.0 + 1e-6
        assert ax.ratio(bad, ea, tol) > 1.0
