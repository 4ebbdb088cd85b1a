"""The oracle of the selectable absorption model (tests/lineshape_oracle.py: the reference's Doppler, Lorentz and Voigt line shapes and
w(::HumlicekWeidemann32VoigtErrorFunction, z) on Dual numbers) against closed forms, scipy's Faddeeva function, central differences
and its own np.longdouble form, and the product's host-side handling of `broadening=` / `cef=`.  No GPU."""
import numpy as np
import pytest

import absdual_oracle as ado
import lineshape_oracle as lso
import voigt_cases as vc

GRID = np.linspace(12999.5, 13002.5, 777)
CASE = (930.0, 288.0, 0.21, 1.0)      # (p, T, vmr, wing cut-off): the grid resolves the lines


def lines24():
    import rtamd
    tab = rtamd.absorption.synthetic_o2a_lines(24, 12999.0, 13003.0, seed=11)
    tab.E_lower[::5] = -1.0
    return tab


def test_voigt_hw32sd_is_the_existing_oracle():
    a = lso.with_gamma_l(vc.window_case("all", "listed"))
    nu, gd, gl, y, S, dnu, dgd, dgl, dy, dS, i0, i1 = a
    sig, J = lso.lineshape_sum_dual("voigt_sd", *a, vc.EDGE_GRID)
    sig_o, J_o = ado.voigt_sum_dual(nu, gd, y, S, dnu, dgd, dy, dS, i0, i1, vc.EDGE_GRID)
    assert np.array_equal(sig, sig_o) and np.array_equal(J, J_o) and sig.max() > 0


def one_line(shape, g, nu, gd, gl, S):
    one = lambda v: np.array([float(v)])
    g = np.atleast_1d(np.asarray(g, dtype=np.float64))
    return lso.lineshape_sum_dual(shape, one(nu), one(gd), one(gl), one(0.3), one(S), None, None, None, None, None, [1], [g.size], g)[0]


def test_closed_forms():
    """Doppler: S c / gamma_d at the centre and exp(-cLn2) of it at a distance of gamma_d (one half up to the truncation of cLn2,
    1.4e-13); Lorentz: S / (pi gamma_l) at the centre, half of it at a distance of gamma_l.  A handful of correctly rounded
    operations each: rtol 1e-14.  The line sits at 0, so the distances are exact."""
    gd, gl, S = 0.0123456, 0.045, 3.7e-23
    sD = one_line("doppler", [0.0, gd], 0.0, gd, gl, S)
    np.testing.assert_allclose(sD[0], S * lso.C_SQRTLN2_DIV_SQRTPI / gd, rtol=1e-14)
    np.testing.assert_allclose(sD[1], sD[0] * np.exp(-lso.C_LN2), rtol=1e-14)
    assert 0 < abs(sD[1] / sD[0] - 0.5) < 2e-13
    sL = one_line("lorentz", [0.0, gl], 0.0, gd, gl, S)
    np.testing.assert_allclose(sL[0], S / (np.pi * gl), rtol=1e-14)
    np.testing.assert_allclose(sL[1], 0.5 * sL[0], rtol=1e-14)


W_Y = (1e-4, 1e-2, 0.5, 3.0)


def w_points():
    """x from 0 to 40 in steps of 1/8 and, for every y, the points |x| + y = 15 -+ 2^-20 and the tie itself"""
    x = np.arange(0, 321) / 8.0
    return [(y, np.unique(np.concatenate([x, [15 - y - 2.0 ** -20, 15 - y, 15 - y + 2.0 ** -20]]))) for y in W_Y]


def test_hw32voigt_against_wofz():
    """Re w of w(::HumlicekWeidemann32VoigtErrorFunction, z) against scipy.special.wofz, point by point relative to Re wofz, for
    y in W_Y and |x| up to 40, with points just below, on and just above |x| + y = 15.  The distance is the approximations' own
    (Humlicek's region I is a one-term asymptotic form, Weideman's N = 32 expansion is used up to |z| = 15, far beyond humlicek2's
    |x| + y = 8); the bars are twice what the reference's statements give in Float64 on a CPU:
        region I  (|x| + y > 15):   measured 8.411e-05 (at y = 3)      bar 1.682e-04
        weideman32a (elsewhere):    measured 2.489e-08 (at y = 1e-4)   bar 4.978e-08
    """
    from scipy.special import wofz
    worst = {"region I": 0.0, "weideman32a": 0.0}
    for y, x in w_points():
        z = x + 1j * y
        far = lso.region1(z)
        assert far.any() and (~far).any()
        tie = np.flatnonzero(np.abs(x) + y == 15.0)
        assert tie.size == 1 and not far[tie[0]] and not far[tie[0] - 1] and far[tie[0] + 1]      # strictly greater
        w = lso.w_hw32voigt_dual(ado.Dual(z, np.zeros((2,) + z.shape, dtype=complex)), np.float64).v
        ref = wofz(z)
        err = np.abs(w.real - ref.real) / np.abs(ref.real)
        for name, m in (("region I", far), ("weideman32a", ~far)):
            worst[name] = max(worst[name], float(err[m].max()))
        print(f"y = {y:g}: region I {err[far].max():.3e}, weideman32a {err[~far].max():.3e}")
    print(worst)
    assert worst["region I"] <= 1.682e-4 and worst["weideman32a"] <= 4.978e-8


@pytest.mark.parametrize("shape", lso.NEW_SHAPES)
def test_partials_against_central_differences(shape):
    """The rule and the bar of test_oracle_absdual.py::test_partials_against_central_differences: relative step 1e-4, 1e-4 of the
    column's maximum (the truncation of the difference; a missing term or a wrong sign shows at 1e-2 or more).  The differences
    are those of the value run in np.longdouble.  For HW32Voigt both steps keep the branch each (line, point) has at (p, T), as the
    Dual run differentiates the branch it takes: the two approximations differ by 8e-5 of w at |x| + y = 15, and a point that a
    step of 1e-4 carries across would add that jump, divided by the step, to the quotient (measured: 3.6e-3 of the maximum)."""
    p, T, vmr, wing = CASE
    hit = vc.hit_columns(lines24())
    prm = lso.line_parameters_dual(hit, GRID, p, T, vmr, wing)
    _, J = lso.cross_section_dual(shape, hit, GRID, p, T, vmr, wing)
    far = lso.region1_rows(prm[0].v, prm[1].v, prm[3].v, prm[5], prm[6], GRID)
    assert shape != "voigt15" or (far.any() and not far.all())
    for k, x in enumerate((p, T)):
        h = 1e-4 * x
        hi, lo = [p, T], [p, T]
        hi[k] += h
        lo[k] -= h
        val = []
        for q in (hi, lo):
            w = lso.line_parameters_dual(hit, GRID, q[0], q[1], vmr, wing)[5:]
            assert np.array_equal(w[0], prm[5]) and np.array_equal(w[1], prm[6])     # the windows do not move
            val.append(lso.cross_section_dual(shape, hit, GRID, q[0], q[1], vmr, wing, FT=np.longdouble, far=far)[0])
        fd = (val[0] - val[1]) / (2 * np.longdouble(h))
        err = float(np.max(np.abs(J[:, k] - fd)) / np.max(np.abs(fd)))
        print(f"{shape} partial {k}: oracle vs central difference {err:.2e} of max")
        assert np.max(np.abs(fd)) > 0 and err <= 1e-4


@pytest.mark.parametrize("shape", lso.NEW_SHAPES)
@pytest.mark.parametrize("name", ["all", "700_ragged"])
def test_float64_against_longdouble(shape, name):
    """The Float64 oracle within 1e-14 of the np.longdouble one, of each column's maximum, on block-edge cases the GPU test uses:
    what makes its bar of 1e-13 meaningful (test_oracle_absdual.py::test_float64_against_longdouble)."""
    a = lso.with_gamma_l(vc.window_case(name, "listed"))
    sig, J = lso.lineshape_sum_dual(shape, *a, vc.EDGE_GRID)
    sl, Jl = lso.lineshape_sum_dual(shape, *a, vc.EDGE_GRID, FT=np.longdouble)
    assert sl.dtype == np.longdouble and np.finfo(np.longdouble).eps < 1e-18 and sl.max() > 0
    errs = [float(np.max(np.abs(sig - sl)) / sl.max())] + [float(np.max(np.abs(J[:, k] - Jl[:, k])) / np.max(np.abs(Jl[:, k]))) for k in (0, 1)]
    print(f"{shape}, {name}: Float64 vs longdouble oracle (sigma, d/dp, d/dT) {errs}")
    assert max(errs) <= 1e-14


def test_python_argument_handling():
    import rtamd
    ab = rtamd.absorption
    for shape, (b, c) in lso.NAMES.items():
        assert ab.absorption_model(b, c) == lso.CODES[shape]
        assert ab.absorption_model(b[:-2], c[:-2]) == lso.CODES[shape]
    assert ab.absorption_model() == (0, 0)
    assert ab.absorption_model("Doppler()", "HumlicekWeidemann32VoigtErrorFunction") == (1, 1)
    for bad in (dict(broadening="Gauss()"), dict(cef="CPF12ErrorFunction()"), dict(cef="ErfcErrorFunction()"),
                dict(cef="ErfcHumliErrorFunctionVoigt"), dict(broadening="voigt"), dict(broadening=None), dict(cef=1)):
        with pytest.raises(ValueError, match="supported are"):
            ab.absorption_model(**bad)
    for f in (ab.compute_absorption_cross_section, ab.absorption_cross_section):     # raised before any GPU call
        with pytest.raises(ValueError, match="Voigt\\(\\), Doppler\\(\\), Lorentz\\(\\)"):
            f(lines24(), GRID, 930.0, 288.0, broadening="Galatry()")
    with pytest.raises(ValueError, match="HumlicekWeidemann32VoigtErrorFunction"):
        ab.compute_absorption_profile(None, lines24(), GRID, [930.0], [288.0], [1e24], 0.3, cef="CPF12ErrorFunction()")


def test_line_prefactors_carry_gamma_l():
    import rtamd
    ab = rtamd.absorption
    p, T, vmr, wing = CASE
    pf = ab.line_prefactors(lines24(), GRID, p, T, vmr, wing)
    assert ab.LinePrefactors(1, 2, 3, 4, 5, 6).γ_l is None        # positional construction as before
    np.testing.assert_allclose(pf.γ_l, pf.y * pf.γ_d / np.sqrt(ab.cLn2), rtol=4e-15)
    five = ab.line_prefactors_dual(lines24(), GRID, p, T, vmr, wing)
    six = ab.line_prefactors_dual(lines24(), GRID, p, T, vmr, wing, with_γ_l=True)
    assert len(five) == 5 and len(six) == 6 and all(np.array_equal(a, b) for a, b in zip(five[1:], six[1:5]))
    nu, gd, gl, y, S, i0, i1 = lso.line_parameters_dual(vc.hit_columns(lines24()), GRID, p, T, vmr, wing)
    np.testing.assert_allclose(six[0].γ_l, gl.v, rtol=4e-15)
    np.testing.assert_allclose(six[5], gl.d.T, rtol=4e-15)
