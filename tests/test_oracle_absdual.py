"""The forward-mode oracle of the absorption path (tests/absdual_oracle.py) against oracle/absref.py -- values, central
differences, its own np.longdouble form -- and the product's host mirror of the Dual run (absorption.line_prefactors_dual,
absorption.optics_partials, CubicSpline.derivative) against that oracle.  No GPU."""
import numpy as np
import pytest

import absdual_oracle as ado
from oracle import absref

GRID = np.linspace(12999.5, 13002.5, 777)
# (p, T, vmr, wing cut-off): the grid resolves the lines, both branches of w occur
CASES = [(930.0, 288.0, 0.21, 1.0), (5.0, 215.0, 0.21, 1.0), (480.0, 262.25, 0.3, 0.4)]


def lines24():
    import rtamd
    tab = rtamd.absorption.synthetic_o2a_lines(24, 12999.0, 13003.0, seed=11)
    tab.E_lower[::5] = -1.0     # "no temperature correction" rows (compute_absorption_cross_section.jl:96)
    return tab


def hit_columns(tab):
    """product HitranTable -> the read_hitran-style columns the oracles take"""
    return {"mol": tab.mol, "iso": tab.iso, "νᵢ": tab.νᵢ, "Sᵢ": tab.Sᵢ, "γ_air": tab.γ_air, "γ_self": tab.γ_self,
            "E_lower": tab.E_lower, "n_air": tab.n_air, "δ_air": tab.δ_air}


@pytest.fixture(scope="module")
def oracle64():
    """the Float64 oracle of the three cases, computed once: [(sigma, J, (nu, gd, y, S, i0, i1))]"""
    hit = hit_columns(lines24())
    out = []
    for p, T, vmr, wing in CASES:
        prm = ado.line_parameters_dual(hit, GRID, p, T, vmr, wing)
        nu, gd, y, S, i0, i1 = prm
        sig, J = ado.voigt_sum_dual(nu.v, gd.v, y.v, S.v, nu.d.T, gd.d.T, y.d.T, S.d.T, i0, i1, GRID)
        out.append((sig, J, prm))
    return out


def test_both_branches_of_w_occur(oracle64):
    for (_, _, (nu, gd, y, _, i0, i1)) in oracle64:
        far = near = False
        for j in range(nu.v.size):
            x = ado.C_SQRTLN2 / gd.v[j] * (GRID[i0[j] - 1:i1[j]] - nu.v[j])
            far |= bool(np.any(np.abs(x) + y.v[j] >= 8))
            near |= bool(np.any(np.abs(x) + y.v[j] < 8))
        assert far and near


@pytest.mark.parametrize("case", range(3))
def test_values_against_absref(oracle64, case):
    p, T, vmr, wing = CASES[case]
    ref = absref.absorption_cross_section(hit_columns(lines24()), GRID, p, T, vmr, wing)
    err = np.max(np.abs(oracle64[case][0] - ref))
    print(f"case {case}: oracle value vs absref {err / ref.max():.2e} of max")
    assert err <= 1e-14 * ref.max()


@pytest.mark.parametrize("case", range(3))
def test_partials_against_central_differences(oracle64, case):
    """Bar 1e-4 max|d_k sigma|: set by the truncation of the difference (relative step 1e-4); a missing term or a wrong sign
    shows at 1e-2 or more.  Measured: <= 4e-6."""
    p, T, vmr, wing = CASES[case]
    hit = hit_columns(lines24())
    J = oracle64[case][1]
    i0, i1 = oracle64[case][2][4:]
    for k, x in enumerate((p, T)):
        h = 1e-4 * x
        hi, lo = [p, T], [p, T]
        hi[k] += h
        lo[k] -= h
        for q in (hi, lo):   # the windows are integer decisions: the difference is meaningful only if they do not move
            w = absref.line_parameters(hit, GRID, q[0], q[1], vmr, wing)[4:]
            assert np.array_equal(w[0], i0) and np.array_equal(w[1], i1)
        fd = (absref.absorption_cross_section(hit, GRID, hi[0], hi[1], vmr, wing) -
              absref.absorption_cross_section(hit, GRID, lo[0], lo[1], vmr, wing)) / (2 * h)
        err = np.max(np.abs(J[:, k] - fd)) / np.max(np.abs(fd))
        print(f"case {case} partial {k}: oracle vs central difference {err:.2e} of max")
        assert err <= 1e-4


@pytest.mark.parametrize("case", range(3))
def test_float64_against_longdouble(oracle64, case):
    """The Float64 oracle is conditioned at 1e-15: what makes the 1e-13 bar of the GPU test meaningful."""
    p, T, vmr, wing = CASES[case]
    sl, Jl = ado.cross_section_dual(hit_columns(lines24()), GRID, p, T, vmr, wing, FT=np.longdouble)
    assert sl.dtype == np.longdouble and np.finfo(np.longdouble).eps < 1e-18
    sig, J = oracle64[case][:2]
    errs = [float(np.max(np.abs(sig - sl)) / sl.max())] + [float(np.max(np.abs(J[:, k] - Jl[:, k])) / np.max(np.abs(Jl[:, k]))) for k in (0, 1)]
    print(f"case {case}: Float64 vs longdouble oracle (sigma, d/dp, d/dT) {errs}")
    assert max(errs) <= 1e-14


@pytest.mark.parametrize("case", range(3))
def test_product_line_prefactors_dual(oracle64, case):
    import rtamd
    ab = rtamd.absorption
    p, T, vmr, wing = CASES[case]
    pf, dnu, dgd, dy, dS = ab.line_prefactors_dual(lines24(), GRID, p, T, vmr=vmr, wing_cutoff=wing)
    nu, gd, y, S, i0, i1 = oracle64[case][2]
    assert np.array_equal(pf.ind_start, i0) and np.array_equal(pf.ind_stop, i1) and np.array_equal(pf.ν, nu.v)
    for a in (dnu, dgd, dy, dS):
        assert a.shape == (nu.v.size, 2)
    assert np.array_equal(dnu, nu.d.T)
    assert np.all(dgd[:, 0] == 0) and np.all(dS[:, 0] == 0)
    np.testing.assert_allclose(dgd[:, 1], gd.d[1], rtol=1e-15)
    np.testing.assert_allclose(dy, y.d.T, rtol=4e-15)
    tab = lines24()
    fixed = tab.E_lower[(GRID.min() - wing < tab.νᵢ) & (tab.νᵢ < GRID.max() + wing)] == -1
    assert fixed.any() and np.all(dS[fixed, 1] == 0) and np.all(S.d[1][fixed] == 0)
    np.testing.assert_allclose(dS[:, 1], S.d[1], rtol=1e-6)   # Float32 spline set-ups differ by 3e-8 in d ln Q / dT
    with pytest.raises(ValueError):
        ab.line_prefactors_dual(lines24(), GRID, p, T, vmr=vmr, wing_cutoff=wing, qratio=ab.linear_rotor_qratio)


def test_spline_derivative_is_the_derivative_of_the_piece():
    import rtamd
    ab = rtamd.absorption
    sp = ab.CubicSpline(ab.get_TQ(7, 1), ab.get_TT(7, 1))
    for T in (215.3, 262.25, 288.4):     # inside a piece: the Float32 coefficients make the pieces meet only to 1e-7
        h = 1e-3
        fd = (sp(T + h) - sp(T - h)) / (2 * h)
        assert abs(sp.derivative(T) - fd) <= 1e-6 * abs(fd)


def test_optics_partials_against_complex_step():
    """`+(::CoreScatteringOpticalProperties, ::CoreAbsorptionOpticalProperties)` (types.jl:672-678): tau = tau_x + tau_abs,
    varpi = tau_x varpi_x / tau; complex step h = 1e-20 along tau_abs."""
    import rtamd
    rng = np.random.default_rng(4)
    tau_x, varpi_x = rng.uniform(0.01, 2.0, (50, 3)), rng.uniform(0.2, 1.0, (50, 3))
    tau_abs, d = rng.uniform(0.0, 3.0, (50, 3)), rng.normal(size=(50, 3))
    tau = tau_x + tau_abs
    varpi = (tau_x * varpi_x) / tau
    sp = rtamd.absorption.optics_partials(tau, varpi, d)
    assert isinstance(sp, rtamd.ScenePartial) and sp.dzw is None
    tc = tau_x + (tau_abs + 1e-20j * d)
    vc = (tau_x * varpi_x) / tc
    np.testing.assert_allclose(sp.dτ, tc.imag / 1e-20, rtol=1e-14)
    np.testing.assert_allclose(sp.dϖ, vc.imag / 1e-20, rtol=1e-14)
