"""The Mie / NAI-2 oracle (tests/mie_oracle.py) against independent knowledge, and the host side of
radiativetransfer.jl_amd/scattering.py (quadratures, tables, weight rows, normalisation, δ-BGE truncation) against the oracle.
No GPU: the device sums are checked in test_gpu_mie.py."""
import math

import numpy as np
import pytest

import mie_oracle as mo

CASE2 = dict(r_max=1.0, nquad=37, lam=0.55, n_r=1.3, n_i=0.001, r_m=0.3, sigma_g=1.6)


@pytest.fixture(scope="module")
def case2():
    return mo.case_sums(**CASE2)


def test_twin_against_bessel_route():
    """a_n, b_n of the recurrences against Bohren & Huffman 4.53 with scipy's Bessel functions, relative to the largest
    coefficient.  Measured with this oracle: worst 1.62e-14 (x = 40, m = 1.3 + 0.001i; 1.55e-14 at x = 0.05); the bound is
    that value x 4."""
    worst = 0.0
    for m in (1.3 + 0.001j, 1.5 + 0.1j, 1.33 + 0j):
        for x in (0.05, 0.4, 4.1, 11.4, 40.0):
            ar, ai, br, bi, nm = mo.mie_ab(x, m.real, m.imag)
            a, b = mo.mie_ab_bessel(x, m, int(nm[0]))
            big = max(np.abs(a).max(), np.abs(b).max())
            d = max(np.abs(ar[:, 0] + 1j * ai[:, 0] - a).max(), np.abs(br[:, 0] + 1j * bi[:, 0] - b).max()) / big
            print(f"m = {m} x = {x}: n_max = {nm[0]}, twin - Bessel = {d:.3e}")
            worst = max(worst, d)
    assert worst <= 4 * 1.62e-14


def test_beta0_and_single_scattering_albedo(case2):
    """β₀ = 1 (the Gauss rule of 2 n_max - 1 nodes integrates f₁₁ exactly), ω̃ = 1 without absorption, 0 < ω̃ < 1 with it.
    Bound: every output is a sum of at most n_μ n_R n_max = 61 * 37 * 31 products rounded to 2^-53, 7.8e-12 if all errors add."""
    bound = 61 * 37 * 31 * 2.0 ** -53
    Cs, Ce = case2["C"][0]
    print("β₀ - 1 =", case2["greek"][0, 1, 0] / Cs - 1, " ω̃ =", Cs / Ce)
    assert abs(case2["greek"][0, 1, 0] / Cs - 1) <= bound
    assert 0 < Cs / Ce < 1
    g, ω, _ = mo.aerosol_optics(**{**CASE2, "n_i": 0.0, "n_r": 1.33})
    print("n_i = 0: β₀ - 1 =", g[1, 0] - 1, " ω̃ - 1 =", ω - 1)
    assert abs(ω - 1) <= bound and abs(g[1, 0] - 1) <= bound
    g, ω, _ = mo.aerosol_optics(0.5, 20, 0.76, 1.5, 0.1, 0.3, 1.6)
    assert 0 < ω < 1 and abs(g[1, 0] - 1) <= bound


def test_rayleigh_limit(rtamd):
    """r_max = 0.004 µm at λ = 0.76 µm (x <= 0.033): the Greek coefficients against get_greek_rayleigh(0.0) -- this pins the sign
    of γ and which amplitude is S₁ -- and f₁₁ against ¾ (1 + μ²).  Measured with this oracle: 5.31e-4 (ζ₂; the first
    correction in x²) and 3.71e-4; asserted at twice that."""
    args = (0.004, 8, 0.76, 1.3, 0.001, 0.001, 1.6)
    g, _, _ = mo.aerosol_optics(*args)
    R = rtamd.corert.get_greek_rayleigh(0.0)
    ref = np.stack([R.α, R.β, R.γ, R.δ, R.ϵ, R.ζ])
    d_greek, d_rest = np.abs(g[:, :3] - ref).max(), np.abs(g[:, 3:]).max()
    s = mo.case_sums(*args)
    d_phase = np.abs(s["bulk_f"][0, 0] / s["C"][0, 0] - 0.75 * (1 + s["mu"] ** 2)).max()
    print(f"greek - rayleigh = {d_greek:.3e}, l >= 3: {d_rest:.3e}, f11 - 3/4 (1 + mu^2) = {d_phase:.3e}")
    assert g[2, 2] > 0
    assert d_greek <= 2 * 5.31e-4 and d_rest <= 2 * 5.31e-4 and d_phase <= 2 * 3.71e-4


def test_host_quadrature_and_tables(rtamd, case2):
    """What the product's host layer uploads against the oracle's own: both sides perform the same recurrences in Float64, and the
    Newton iterations of the nodes end within a few ulp of each other (bound: 8 ulp of the node / weight, 1e-13 relative for
    the tables, whose three-term recurrences amplify a node's last bit by up to l²)."""
    sc = rtamd.scattering
    aer = sc.Aerosol(sc.LogNormal(math.log(CASE2["r_m"]), math.log(CASE2["sigma_g"])), CASE2["n_r"], CASE2["n_i"])
    inp = sc.mie_inputs(sc.make_mie_model(sc.NAI2(), aer, CASE2["lam"], None, None, CASE2["r_max"], CASE2["nquad"]))
    assert np.abs(inp.r - case2["r"]).max() <= 8 * 2.0 ** -53 and np.abs(inp.μ - case2["mu"]).max() <= 8 * 2.0 ** -53
    assert mo.rel_max(inp.w_μ, case2["w_mu"]) <= 1e-13
    assert mo.rel_max(inp.w[0], 4 * np.pi * case2["r"] ** 2 * case2["wx"]) <= 1e-13
    n_max = int(case2["n_max"].max())
    assert inp.π_.shape == (2 * n_max - 1, n_max) and np.array_equal(sc.get_n_max(case2["x"]), case2["n_max"])
    for mine, theirs in zip((inp.π_, inp.τ_), mo.mie_pi_tau(case2["mu"], n_max)):
        assert mo.rel_max(mine, theirs) <= 1e-13
    for mine, theirs in zip((inp.P, inp.P2, inp.R2, inp.T2), mo.legendre_tables(case2["mu"], case2["mu"].size)):
        assert mo.rel_max(mine, theirs) <= 1e-13


def _optics(rtamd, g, ω, k):
    return rtamd.corert.AerosolOptics(greek_coefs=rtamd.scattering._greek(np.asarray(g, dtype=np.float64)), ω̃=float(ω), fᵗ=1.0,
                                      k=float(k))


def test_truncate_phase(rtamd):
    """δ-BGE as the reference writes it: fᵗ = 1 - c₀, βᵗ₀ = 1, every array of length l_max, γᵗ and ϵᵗ zero below l = 2, ω̃ and k
    untouched, and Δ_angle without influence on the fit."""
    sc = rtamd.scattering
    g, ω, k = mo.aerosol_optics(**CASE2)
    aero = _optics(rtamd, g, ω, k)
    t = sc.truncate_phase(sc.δBGE(10, 2.0), aero)
    gc = t.greek_coefs
    for a in (gc.α, gc.β, gc.γ, gc.δ, gc.ϵ, gc.ζ):
        assert a.shape == (10,) and np.all(np.isfinite(a))
    assert gc.β[0] == 1.0 and 0 < t.fᵗ < 1
    assert np.all(gc.γ[:2] == 0) and np.all(gc.ϵ[:2] == 0) and gc.γ[2] != 0
    assert t.ω̃ == aero.ω̃ and t.k == aero.k
    # c₀ = 1 - fᵗ: the fit's first coefficient, from which the other rows are rebuilt (Eq. 38b)
    c0 = 1 - t.fᵗ
    cl = gc.β * c0
    assert np.allclose(gc.δ, (g[3, :10] - (g[1, :10] - cl)) / c0, rtol=0, atol=1e-12 * np.abs(gc.δ).max())
    t2 = sc.truncate_phase(sc.δBGE(10, 30.0), aero)
    assert np.array_equal(t2.greek_coefs.β, gc.β) and t2.fᵗ == t.fᵗ


def test_partials_against_central_differences(rtamd):
    """The autodiff=True host arithmetic -- the weight rows of ∂wₓ/∂(r_m, σ_g) and the quotient rules behind the sums -- fed the
    oracle's sums, against central differences of the oracle, each field relative to its largest partial.
    Step-halving on the CPU (relative steps 1e-2 ... 1e-5, both parameters): the difference falls by 4 per halving down to
    h = 1e-4 (6.7e-7 at 3e-4, 7.4e-8 at 1e-4, the Greek coefficients' σ_g partial being the worst) and meets the rounding floor
    of the Float64 differences (1e-8, ω̃) at 1e-5.  So h = 1e-4 and a bound of 2e-7: truncation 7.4e-8 plus rounding 1e-8, x 2."""
    sc = rtamd.scattering
    aer = sc.Aerosol(sc.LogNormal(math.log(CASE2["r_m"]), math.log(CASE2["sigma_g"])), CASE2["n_r"], CASE2["n_i"])
    inp = sc.mie_inputs(sc.make_mie_model(sc.NAI2(), aer, CASE2["lam"], None, None, CASE2["r_max"], CASE2["nquad"]), autodiff=True)
    assert inp.w.shape == (3, CASE2["nquad"])
    s = mo.nai2_sums(inp.r, inp.w / (4 * np.pi * inp.r ** 2), CASE2["lam"], CASE2["n_r"], CASE2["n_i"])
    _, partials = sc.optics_from_sums(s["C"], s["greek"])
    assert len(partials) == 2
    h = 1e-4
    for j, name in enumerate(("r_m", "sigma_g")):
        step = CASE2[name] * h
        hi = mo.aerosol_optics(**{**CASE2, name: CASE2[name] + step})
        lo = mo.aerosol_optics(**{**CASE2, name: CASE2[name] - step})
        d = [(a - b) / (2 * step) for a, b in zip(hi, lo)]
        gp = partials[j].greek_coefs
        mine = np.stack([gp.α, gp.β, gp.γ, gp.δ, gp.ϵ, gp.ζ])
        errs = (mo.rel_max(mine, d[0]), abs(partials[j].ω̃ - d[1]) / abs(d[1]), abs(partials[j].k - d[2]) / abs(d[2]))
        print(f"d/d{name}: greek {errs[0]:.2e}, ω̃ {errs[1]:.2e}, k {errs[2]:.2e}")
        assert max(errs) <= 2e-7
