"""The oracle of the PCW Jacobian rows (tests/pcw_dual_oracle.py) against finite differences, and the host side of
aerosol_optics_jacobian.  No GPU.

The index rows of the oracle come from the polarisation identity on the Dual Mie coefficients; here they are compared with central
differences of the long-double pcw_sums at step h = 2^-24 (exact in Float64; at n_i = 0, where n_i - h is not a refractive index
the route takes, the one-sided three-point form).  Truncation h^2 f''' / 6 = 6e-16 f''' (one-sided: h^2 f''' / 3) and rounding
2^-63 / h = 2e-12 of the sums give a distance of 1e-12 .. 1e-10 (measured: <= 1.7e-11 with the central form, <= 1.2e-9 with the
one-sided one, whose f''' is that of the single radius of nquad1); the bound is 1e-8 of each row's largest magnitude.  A wrong sign or
factor in the oracle is a distance of order 1."""
import math

import numpy as np
import pytest

import pcw_dual_oracle as pdo
import pcw_oracle as po

H = 2.0 ** -24
FD_BOUND = 1e-8
LD = np.longdouble


def _finite_difference(r, wx, lam, n_r, n_i, r_max, which):
    run = lambda dr, di: po.pcw_sums(r, wx, lam, n_r + dr, n_i + di, r_max)
    step = (lambda t: run(t, 0.0)) if which == 0 else (lambda t: run(0.0, t))
    if which == 1 and n_i == 0.0:
        f0, f1, f2 = step(0.0), step(H), step(2 * H)
        return tuple((-3 * f0[q] + 4 * f1[q] - f2[q]) / LD(2 * H) for q in ("greek", "C"))
    fp, fm = step(H), step(-H)
    return tuple((fp[q] - fm[q]) / LD(2 * H) for q in ("greek", "C"))


@pytest.mark.parametrize("case", ["n31", "n32", "nquad1", "n33_r64"])
def test_index_rows_against_finite_differences(case):
    r_max, _, lam, n_r, n_i, _, _ = {**po.SMALL_CASES, **po.MID_CASES}[case]
    r, wx, N = po.case_inputs(case, LD)
    o = pdo.pcw_sums_dual(r, wx, lam, n_r, n_i, r_max)
    assert o["N"] == N and o["greek"].shape == (3, 6, 2 * N - 1) and o["C"].shape == (3, 2)
    for which, name in enumerate(("n_r", "n_i")):
        g_fd, C_fd = _finite_difference(r, wx, lam, n_r, n_i, r_max, which)
        g, C = o["greek"][1 + which], o["C"][1 + which]
        for q in range(6):
            d = float(np.abs(g[q] - g_fd[q]).max() / np.abs(g_fd[q]).max())
            print(f"{case}: d/d{name} of greek row {q}: oracle - finite difference = {d:.3e} of the largest (bound {FD_BOUND:.0e})")
            assert d <= FD_BOUND, (case, name, q, d)
        d = float(np.abs(C - C_fd).max() / np.abs(C_fd).max())
        print(f"{case}: d/d{name} of C: oracle - finite difference = {d:.3e}")
        assert d <= FD_BOUND, (case, name, d)


def test_pair_partials_are_the_polarisation_of_the_pair_averages():
    """the pair rows of the oracle against central differences of pair_averages on the long-double coefficients (n32: n_i = 0.1)"""
    import mie_oracle as mo
    r_max, _, lam, n_r, n_i, _, _ = po.SMALL_CASES["n32"]
    r, wx, N = po.case_inputs("n32", LD)
    rows = pdo.pair_averages_dual(r, wx, lam, n_r, n_i, N)
    assert rows.shape == (3, 4, N, N)
    x = (2 * mo.pi_of(LD) / LD(lam)) * r

    def pairs(dr, di):
        ar, ai, br, bi, n_max_i = mo.mie_ab(x, n_r + dr, n_i + di, LD, n_rows=N)
        return np.array(po.pair_averages(ar + 1j * ai, br + 1j * bi, wx, n_max_i))

    for which, (p, m) in enumerate(((pairs(H, 0.0), pairs(-H, 0.0)), (pairs(0.0, H), pairs(0.0, -H)))):
        fd = (p - m) / LD(2 * H)
        d = float(np.abs(rows[1 + which] - fd).max() / np.abs(fd).max())
        print(f"n32: pair partials, parameter {which}: oracle - finite difference = {d:.3e}")
        assert d <= FD_BOUND


# ---- the host side of aerosol_optics_jacobian ---------------------------------------------------------------------------------

def _models(sc):
    aer = sc.Aerosol(sc.LogNormal(math.log(0.3), math.log(2.0)), 1.3, 0.001)
    return (sc.make_mie_model(sc.PCW(), aer, 0.55, None, None, 1.0, 12), sc.make_mie_model(sc.NAI2(), aer, 0.55, None, None, 1.0, 12))


@pytest.mark.parametrize("wrt, nW, index", [(("r_m", "σ_g", "nᵣ", "nᵢ"), 3, True), (("nᵢ",), 1, True), (("σ_g",), 3, False),
                                            (("nᵣ", "r_m"), 3, True), ((), 1, False)])
def test_row_selection(rtamd, monkeypatch, wrt, nW, index):
    """the size rows only when wrt names r_m or σ_g, the index rows only when it names nᵣ or nᵢ; ONE device call; the partials come
    back in the order of wrt; the quotient rule as written"""
    sc = rtamd.scattering
    pcw, _ = _models(sc)
    r0, wx0, N = sc.pcw_inputs(pcw)
    calls = []

    def fake(r, w, lam, n_r, n_i, N_max, index_rows=False, device=0):
        calls.append((np.array(w), index_rows))
        nO = w.shape[0] + (2 if index_rows else 0)
        rng = np.random.default_rng(7)
        return rng.normal(size=(nO, 6, 2 * N_max - 1)), rng.uniform(1, 2, size=(nO, 2)), np.zeros(3)

    monkeypatch.setattr(rtamd._lib, "mie_pcw_dual", fake)
    aero, parts = sc.aerosol_optics_jacobian(pcw, wrt=wrt)
    assert len(calls) == 1 and len(parts) == len(wrt)
    w, index_rows = calls[0]
    assert w.shape == (nW, r0.size) and index_rows is index
    assert np.array_equal(w[0], wx0)                                  # row 0 is the value call's w_x, to the bit
    rows = (("r_m", "σ_g") if nW == 3 else ()) + (("nᵣ", "nᵢ") if index else ())
    greek, C, _ = fake(r0, w, 0.55, 1.3, 0.001, N, index)
    Cs, Ce = C[0]
    assert np.array_equal(aero.greek_coefs.β, ((1 / Cs) * greek[0])[1]) and aero.ω̃ == Cs / Ce and aero.k == Ce and aero.fᵗ == 1.0
    for p, got in zip(wrt, parts):
        k = 1 + rows.index(p)
        want = (1 / Cs) * greek[k] - greek[0] * C[k, 0] / Cs ** 2
        assert np.array_equal(got.greek_coefs.α, want[0]) and np.array_equal(got.greek_coefs.ζ, want[5])
        assert got.ω̃ == C[k, 0] / Ce - Cs * C[k, 1] / Ce ** 2 and got.k == C[k, 1] and got.fᵗ == 0.0


def test_size_rows_are_the_nai2_rows_before_the_area_factor(rtamd):
    sc = rtamd.scattering
    pcw, nai2 = _models(sc)
    r, w, N, index_rows, rows = sc.pcw_jacobian_inputs(pcw, sc.ALL_AEROSOL_PARAMETERS)
    r2, w2 = sc._radii_and_weight_rows(nai2, True)
    assert index_rows and rows == sc.ALL_AEROSOL_PARAMETERS and N == int(sc.get_n_max(2 * math.pi * 1.0 / 0.55))
    assert np.array_equal(r, r2) and np.array_equal(4 * math.pi * r ** 2 * w, w2)
    assert abs(w[0].sum() - 1) < 1e-14 and abs(w[1].sum()) < 1e-13 and abs(w[2].sum()) < 1e-13   # w_x is normalised for every parameter


@pytest.mark.parametrize("wrt", [("r_m", "r_m"), ("λ",), ("nᵣ", "n_i")])
def test_wrt_validation(rtamd, wrt):
    sc = rtamd.scattering
    for model in _models(sc):
        with pytest.raises(ValueError, match="wrt must be distinct names"):
            sc.aerosol_optics_jacobian(model, wrt=wrt)


def test_nai2_route_delegates_unchanged(rtamd, monkeypatch):
    sc = rtamd.scattering
    _, nai2 = _models(sc)
    seen, token = [], object()
    monkeypatch.setattr(sc, "compute_aerosol_optical_properties", lambda *a, **k: (seen.append((a, k)), token)[1])
    monkeypatch.setattr(rtamd._lib, "mie_pcw_dual", lambda *a, **k: pytest.fail("the PCW call on a NAI2() model"))
    assert sc.aerosol_optics_jacobian(nai2, wrt=["nᵢ", "r_m"]) is token
    assert sc.aerosol_optics_jacobian(nai2) is token
    assert seen == [((nai2,), dict(autodiff=True, wrt=("nᵢ", "r_m"))), ((nai2,), dict(autodiff=True, wrt=sc.ALL_AEROSOL_PARAMETERS))]
    assert rtamd.aerosol_optics_jacobian is sc.aerosol_optics_jacobian
