"""The forward-mode twin of the Mie oracle (tests/mie_dual_oracle.py) against the oracle itself and against central differences
of it, and the host side of the refractive-index Jacobians in radiativetransfer.jl_amd/scattering.py (truncate_phase with partials,
aerosol_derivs, aerosol_optics_partial).  No GPU: the device's Dual run is checked in test_gpu_mie_dual.py."""
import functools
import math

import numpy as np
import pytest

import mie_oracle as mo
import mie_dual_oracle as md

MS = [(1.3, 0.001), (1.5, 0.1), (1.33, 0.0)]
XS = [0.05, 0.4, 4.1, 11.4, 40.0]
FLOOR = 2.0 ** -46
# (r_max, nquad_radius, λ, n_r, n_i, r_m, σ_g)
CASES = {
    "one_radius": (1.0, 1, 0.55, 1.3, 0.001, 0.3, 1.6),
    "case2": (1.0, 37, 0.55, 1.3, 0.001, 0.3, 1.6),
    "absorbing": (0.5, 20, 0.76, 1.5, 0.1, 0.3, 1.6),
    "no_absorption": (1.0, 33, 0.55, 1.33, 0.0, 0.3, 1.6),
}


@functools.lru_cache(maxsize=None)
def _twin_ab(n_r, n_i, dtype):
    n_max = int(mo.n_max_of(max(XS))) + 3
    return md.mie_ab_dual(XS, n_r, n_i, dtype, n_rows=n_max), n_max


def _complex(d, c):
    """(a, b) [2, n_rows, nX] complex of partial c (0: d/dn_r, 1: d/dn_i) of mie_ab_dual's output"""
    return np.stack([d[0].d[c] + 1j * d[1].d[c], d[2].d[c] + 1j * d[3].d[c]])


@pytest.mark.parametrize("n_r,n_i", MS)
@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_twin_value_is_the_oracle(n_r, n_i, dtype):
    """the value part of every Dual is computed by the oracle's operations in the oracle's order: bitwise equal"""
    d, n_max = _twin_ab(n_r, n_i, dtype)
    o = mo.mie_ab(XS, n_r, n_i, dtype, n_rows=n_max)
    for q in range(4):
        assert d[q].v.dtype == o[q].dtype and np.array_equal(d[q].v, o[q])
    assert np.array_equal(d[4], o[4])


def test_twin_sums_value_is_the_oracle():
    s, o = md.case_sums_dual(*CASES["case2"]), mo.case_sums(*CASES["case2"])
    for q in ("bulk_f", "C", "greek", "mu", "w_mu"):
        assert np.array_equal(s[q], o[q]), q


@pytest.mark.parametrize("n_r,n_i", MS)
def test_cauchy_riemann(n_r, n_i):
    """a_n, b_n are holomorphic in m = n_r + i n_i, so d/dn_i = i d/dn_r.  The twin carries the two partials independently; they
    agree to rounding.  Bound per x, relative to that x's largest partial: 8 x the distance between the twin's Float64 and
    long-double runs, at least 2^-46 (a coefficient is some sixty rounded operations; a smaller distance is chance)."""
    d64, _ = _twin_ab(n_r, n_i, np.float64)
    d80, _ = _twin_ab(n_r, n_i, np.longdouble)
    for j, x in enumerate(XS):
        big = np.abs(_complex(d64, 0)[:, :, j]).max()
        dist = max(float(np.abs(_complex(d64, c)[:, :, j] - _complex(d80, c)[:, :, j]).max() / big) for c in (0, 1))
        bound = max(8 * dist, FLOOR)
        cr = float(np.abs(_complex(d64, 1)[:, :, j] - 1j * _complex(d64, 0)[:, :, j]).max() / big)
        print(f"m = {n_r} + {n_i}i, x = {x}: |d/dn_i - i d/dn_r| = {cr:.3e}, bound {bound:.3e}")
        assert cr <= bound


@pytest.mark.parametrize("case", list(CASES))
def test_twin_against_central_differences(case):
    """The twin's bulk, C and Greek partials against central differences of mie_oracle.nai2_sums, all in long double, h = 1e-5.
    Bound: 4 x max |FD(h) - FD(2h)| relative to the largest magnitude of FD(h) -- the differences' own truncation error, three
    times which is FD(2h) - FD(h) -- and the test shows nothing unless that bound is itself <= 1e-6."""
    r_max, nquad, lam, n_r, n_i, r_m, σ_g = CASES[case]
    L = np.longdouble
    r, wr = mo.gauleg_norm(nquad, 0, r_max, L)
    wx = mo.weights_wx(r, wr, r_m, σ_g)
    twin = md.nai2_sums_dual(r, wx, lam, n_r, n_i)
    h = 1e-5

    def fd(c, step):
        hi = mo.nai2_sums(r, wx, lam, n_r + (step if c == 0 else 0.0), n_i + (step if c == 1 else 0.0))
        lo = mo.nai2_sums(r, wx, lam, n_r - (step if c == 0 else 0.0), n_i - (step if c == 1 else 0.0))
        return {q: (hi[q][0] - lo[q][0]) / (2 * L(step)) for q in ("bulk_f", "C", "greek")}

    for c, name in enumerate(("n_r", "n_i")):
        f1, f2 = fd(c, h), fd(c, 2 * h)
        for q in ("bulk_f", "C", "greek"):
            big = float(np.abs(f1[q]).max())
            bound = 4 * float(np.abs(f1[q] - f2[q]).max()) / big
            d = float(np.abs(twin["d_" + q][c] - f1[q]).max()) / big
            print(f"{case}: d {q} / d{name}: twin - FD = {d:.3e}, bound {bound:.3e}")
            assert bound <= 1e-6, (case, q, name, bound)
            assert d <= bound, (case, q, name, d, bound)


# ----------------------------------------------------------------------------------------------------------------------------
# host side of the product
# ----------------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _case2_optics():
    """(optics, [∂/∂n_r, ∂/∂n_i]) of case 2 from the twin's sums through the product's quotient rules"""
    import rtamd
    s = md.case_sums_dual(*CASES["case2"])
    return rtamd.scattering.optics_from_sums(np.concatenate([s["C"], s["d_C"]]), np.concatenate([s["greek"], s["d_greek"]]))


def _stack(g):
    return np.stack([g.α, g.β, g.γ, g.δ, g.ϵ, g.ζ])


@pytest.mark.parametrize("l_tr", [3, 10])
def test_truncate_phase_partials_against_complex_step(rtamd, l_tr):
    """truncate_phase(mod, aero, partials=) against the complex-step twin (step 1e-30 i in the Greek coefficients: no
    cancellation, no truncation error), on the oracle's case 2 optics and their n_r, n_i partials.  Both sides solve the same
    normal equations, so they differ by the conditioning of those: bound 64 κ 2^-52 relative to the largest magnitude of each
    field, κ the largest condition number of the three normal matrices (78 at l_max = 3, 8.4e4 at l_max = 10: bound <= 1.2e-9)."""
    sc = rtamd.scattering
    aero, partials = _case2_optics()
    g = aero.greek_coefs
    μ, w_μ = sc.gausslegendre(len(g.β))
    (f11, f12, _, _, f34, _), P, P2 = sc.reconstruct_phase(g, μ)
    fac = np.zeros(l_tr)
    for l in range(2, l_tr):
        fac[l] = math.sqrt(1.0 / ((l - 1.0) * l * (l + 1.0) * (l + 2.0)))
    κ = 0.0
    for B, f, first in ((P[:, :l_tr], f11, 0), (fac * P2[:, :l_tr], f12, 2), (fac * P2[:, :l_tr], f34, 2)):
        Bf = B[:, first:] / f[:, None]
        κ = max(κ, float(np.linalg.cond((w_μ[:, None] * Bf).T @ Bf)))
    bound = 64 * κ * 2.0 ** -52
    assert bound <= 1.2e-9
    value, d_value = sc.truncate_phase(sc.δBGE(l_tr, 2.0), aero, partials=partials)
    plain = sc.truncate_phase(sc.δBGE(l_tr, 2.0), aero)
    assert np.array_equal(_stack(value.greek_coefs), _stack(plain.greek_coefs)) and value.fᵗ == plain.fᵗ
    assert len(d_value) == 2
    worst = 0.0
    for p, dp, name in zip(partials, d_value, ("n_r", "n_i")):
        ref_v, ref_d = md.truncate_complex_step(l_tr, _stack(g), _stack(p.greek_coefs), μ, w_μ)
        assert mo.rel_max(_stack(value.greek_coefs), np.stack([ref_v[k] for k in md.GREEK_ORDER])) <= bound
        for k, mine in zip(md.GREEK_ORDER, _stack(dp.greek_coefs)):
            assert mine.shape == (l_tr,)
            if np.abs(ref_d[k]).max() == 0:         # γ, ϵ below l = 2 at l_max = 3 have no entries at all
                assert np.all(mine == 0)
                continue
            d = mo.rel_max(mine, ref_d[k])
            worst = max(worst, d)
            assert d <= bound, (name, k, d, bound)
        d = abs(dp.fᵗ - ref_d["fᵗ"]) / abs(ref_d["fᵗ"])
        worst = max(worst, d)
        assert d <= bound, (name, "fᵗ", d, bound)
        assert dp.ω̃ == p.ω̃ and dp.k == p.k
    print(f"l_max = {l_tr}: κ = {κ:.3g}, bound {bound:.3e}, largest distance to the complex step {worst:.3e}")


def test_aerosol_derivs_and_optics_partial(rtamd):
    """aerosol_derivs: [6 l_max + 2, nP] in the row order α, β, γ, δ, ϵ, ζ, ω̃, k.  aerosol_optics_partial: dω̃, dfᵗ at the aerosol,
    dZpp / dZmp at basis 1 + i_aer and exact zeros elsewhere; the moments are linear in the Greek coefficients, so
    Z(g + ∂g) - Z(g) is dZ to rounding (bound: 16 x 2^-52 of the largest |Z|, a sum of at most l_max = 10 products)."""
    sc, rt = rtamd.scattering, rtamd.corert
    aero, partials = _case2_optics()
    l_max = len(aero.greek_coefs.β)
    J = sc.aerosol_derivs(aero, partials)
    assert J.shape == (6 * l_max + 2, 2)
    for j, p in enumerate(partials):
        for q, a in enumerate(_stack(p.greek_coefs)):
            assert np.array_equal(J[q * l_max:(q + 1) * l_max, j], a)
        assert J[-2, j] == p.ω̃ and J[-1, j] == p.k
    assert J[-2, 1] < 0                      # more absorption, smaller single-scattering albedo
    with pytest.raises(ValueError):
        sc.aerosol_derivs(sc.truncate_phase(sc.δBGE(10, 2.0), aero), partials)

    trunc, d_trunc = sc.truncate_phase(sc.δBGE(10, 2.0), aero, partials=partials)
    m = rtamd.scenes.make_scene(3, 3, 6, 24, seed=4)
    m.aerosol_optics = [trunc, trunc]
    m.τ_aer = np.concatenate([m.τ_aer, m.τ_aer])
    M, N = m.params.max_m, 3 * len(m.quad_points.qp_μ)
    Zpp, Zmp = rt.z_bases(m)
    for i_aer in (0, 1):
        op = sc.aerosol_optics_partial(m, i_aer, d_trunc[0])
        assert isinstance(op, rt.OpticsPartial) and op.dτ_aer is None and op.w_p is None
        assert op.dZpp.shape == (M, 3, N, N) == Zpp.shape and op.dZmp.shape == (M, 3, N, N)
        other = [k for k in range(3) if k != 1 + i_aer]
        assert np.all(op.dZpp[:, other] == 0) and np.all(op.dZmp[:, other] == 0) and np.any(op.dZpp[:, 1 + i_aer] != 0)
        assert op.dω̃[i_aer] == d_trunc[0].ω̃ and op.dfᵗ[i_aer] == d_trunc[0].fᵗ and op.dω̃[1 - i_aer] == 0 and op.dfᵗ[1 - i_aer] == 0
        moved = rt.AerosolOptics(greek_coefs=sc._greek(_stack(trunc.greek_coefs) + _stack(d_trunc[0].greek_coefs)), ω̃=trunc.ω̃,
                                 fᵗ=trunc.fᵗ, k=trunc.k)
        m2 = rtamd.scenes.make_scene(3, 3, 6, 24, seed=4)
        m2.aerosol_optics = [moved if k == i_aer else trunc for k in range(2)]
        Zpp2, Zmp2 = rt.z_bases(m2)
        big = max(np.abs(Zpp2).max(), np.abs(Zmp2).max())
        assert np.abs((Zpp2 - Zpp) - op.dZpp).max() <= 16 * 2.0 ** -52 * big
        assert np.abs((Zmp2 - Zmp) - op.dZmp).max() <= 16 * 2.0 ** -52 * big
    dτ = np.ones_like(m.τ_aer)
    assert np.array_equal(sc.aerosol_optics_partial(m, 0, d_trunc[1], dτ_aer=dτ).dτ_aer, dτ)
    with pytest.raises(ValueError):
        sc.aerosol_optics_partial(m, 2, d_trunc[0])
