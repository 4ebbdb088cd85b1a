"""The host's numpy truncate_phase against the longdouble arbiter (trunc_oracle.py) under the rule of trunc_cases.py: what the
device call is measured with.  For the host itself the rule reduces to its cap -- allowed <= 1e-7 for every field of every case --
plus the exact zeros, and the known answer l_tr = l_full, where the fit is exact: cl = β, γᵗ = γ, ϵᵗ = ϵ, fᵗ = 1 - β₀."""
import numpy as np
import pytest

import trunc_cases as tc
import trunc_oracle as to

L_TR = (1, 2, 3, 10, 17, 33, 60, 121, 128)
POINTS = [(case, l_tr) for case in tc.CASES for l_tr in L_TR if l_tr <= tc.L_FULL[case]]


def test_gauss_jordan_solves_in_longdouble():
    rng = np.random.default_rng(3)
    A = rng.standard_normal((9, 9)).astype(np.longdouble)
    A = A @ A.T + 9 * np.eye(9, dtype=np.longdouble)
    B = rng.standard_normal((9, 2)).astype(np.longdouble)
    X = to.gauss_jordan(A, B)
    assert X.dtype == np.longdouble and float(np.max(np.abs(A @ X - B))) < 1e-16
    with pytest.raises(np.linalg.LinAlgError):
        to.gauss_jordan(np.zeros((2, 2), np.longdouble), np.ones((2, 1), np.longdouble))


@pytest.mark.parametrize("case,l_tr", POINTS)
def test_host_against_arbiter(rtamd, case, l_tr):
    """nP = 4: the oracle's ∂/∂nᵣ, ∂/∂nᵢ, the direction to another case's set and a random one"""
    g, dirs = tc.greek_set(case)
    ref = tc.arbiter(case, l_tr, 4)
    hg, hc = tc.host_arrays(rtamd, l_tr, g, dirs)
    report = []
    tc.check(f"{case} l_tr={l_tr}", hg, hc, hg, hc, ref, l_tr, report)
    lim = max(r[4] for r in report)
    print(f"{case} l_tr={l_tr}: κ = {ref['kappa']}, largest d_host = {max(r[3] for r in report):.2e}, largest allowed = {lim:.2e}")
    assert lim <= tc.CAP
    assert float(ref["kappa"].max()) <= 2.4e7 * 1.01
    # the values of the Dual run are those of the plain run
    plain = rtamd.scattering.truncate_phase(rtamd.scattering.δBGE(l_tr, 2.0), tc.optics(rtamd, g))
    assert np.array_equal(tc.stack(plain), hg[0]) and 1.0 - plain.fᵗ == hc[0]


@pytest.mark.parametrize("case", sorted(tc.CASES))
def test_known_answer_at_full_length(rtamd, case):
    """l_tr = l_full: the basis spans the phase function, so the fit returns the coefficients it was built from"""
    g, dirs = tc.greek_set(case)
    L = g.shape[1]
    ref = tc.arbiter(case, L, 2)
    hg, hc = tc.host_arrays(rtamd, L, g, dirs[:2])
    tc.check(f"{case} l_tr=l_full", hg, hc, hg, hc, ref, L)
    lim = tc.allowed(tc.distances(hg, hc, ref), ref)
    c0 = g[1, 0]
    known = np.array([g[0] / c0, g[1] / c0, g[2], g[3] / c0, g[4], g[5] / c0])   # cl = β: (a - (β - cl)) / c₀ = a / β₀
    for side, (gr, c) in (("arbiter", (ref["greek"][0].astype(np.float64), float(ref["c0"][0]))), ("host", (hg[0], hc[0]))):
        for q, name in enumerate(to.ROWS):
            d = float(np.max(np.abs(gr[q] - known[q])) / np.max(np.abs(known[q])))
            print(f"{case} {side} {name}: {d:.1e} (allowed {lim[(0, name)]:.1e})")
            assert d <= lim[(0, name)], (side, name, d)
        assert abs(c - c0) / abs(c0) <= lim[(0, "c₀")], (side, c, c0)
