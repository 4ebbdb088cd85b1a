"""Phase-matrix Fourier moments on the device (mom_z_moments, csrc/mom_zmom.hip) against the extended-precision twin of the oracle's
compute_Z_moments (zmom_oracle.py) under the parity rule of DESIGN section 4,

    E_dev <= 4 E_host + 4 eps max(A_abs)        per (set, m) pair of matrices,

E = max |Z - Z_ld|, E_host that of corert.compute_Z_moments on the same input, A_abs the sums over l with every term replaced by its
absolute value: the allowance is taken over the host's own rounding error, not over the code under test, and a wrong branch, sign or
index costs errors of the order of max(A_abs) itself.  Then bitwise statements about layouts and batches, the stored Natraj Z-+, and the
device route through rt_run, a banded scene, rt_run_rrs and the Dual run.  Every test prints its largest E_dev / (E_host + eps max A_abs)."""
import dataclasses
import math
import unicodedata
from pathlib import Path

import numpy as np
import pytest

import bands_cases as bc
import helpers
import rtamd
import zmom_oracle as zo

pytestmark = pytest.mark.gpu
rt, L = rtamd.corert, rtamd._lib
GOLD = Path(__file__).parent / "golden"
POL = {1: rt.Stokes_I, 3: rt.Stokes_IQU, 4: rt.Stokes_IQUV}


def rows(g):
    return (g.α, g.β, g.γ, g.δ, g.ϵ, g.ζ)


def scaled(g, f):
    return rt.GreekCoefs(*(f * r for r in rows(g)))


def with_epsilon(g):
    """hg_like_greek with an ϵ row of the size of the others: the (3,4) / (4,3) entries of B carry weight"""
    hi = (np.arange(len(g.β)) >= 2).astype(np.float64)
    return dataclasses.replace(g, ϵ=0.3 * g.β * hi)


def on_device(model):
    return dataclasses.replace(model, params=dataclasses.replace(model.params, z_moments_on_device=True))


def check_parity(n, μ, greeks, m_first, M, Zd, what):
    """the parity rule for every (set, m) of a device result Zd = (Zpp, Zmp) [M, nG, N, N]; returns the largest ratio"""
    worst = 0.0
    for mi in range(M):
        for k, g in enumerate(greeks):
            m = m_first + mi
            Zh = rt.compute_Z_moments(POL[n](), μ, g, m)
            e_host, e_dev, eps_a, z_max = zo.parity(n, μ, rows(g), m, Zh, (Zd[0][mi, k], Zd[1][mi, k]))
            ratio = e_dev / (e_host + eps_a) if e_host + eps_a > 0 else 0.0
            worst = max(worst, ratio)
            assert np.all(np.isfinite(Zd[0][mi, k])) and np.all(np.isfinite(Zd[1][mi, k])), (what, k, m)
            assert zo.holds(e_host, e_dev, eps_a), (f"{what}: set {k}, m {m}: E_dev {e_dev:.3e}, E_host {e_host:.3e}, "
                                                    f"eps max A_abs {eps_a:.3e}, max |Z| {z_max:.3e}")
    print(f"{what}: largest E_dev / (E_host + eps max A_abs) = {worst:.3f}")
    return worst


# ---- 1. every branch of the recurrences ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 3, 1])
def test_branch_cover(n):
    """m = 0 .. 9 on a set of l_max = 9: the three m = 0 seeds, both m = 1 seeds, the m >= 2 seed on both sides of smu > 1e-8 (0.5 at
    m = 2, 0 above; the node mu = 1), the l = m + 1 step, the single-term moment m = 8 and m = 9 = l_max: zeros"""
    μ = np.array([1.0, 0.83, 0.41, 0.0071, 0.2])
    g = with_epsilon(rtamd.scenes.hg_like_greek(0.7, 9))
    Zd = rtamd.compute_Z_moments_batch(POL[n](), μ, [g], 10, device=0)
    assert Zd[0].shape == (10, 1, 5 * n, 5 * n)
    check_parity(n, μ, [g], 0, 10, Zd, f"branch cover n = {n}")
    assert not np.any(Zd[0][9]) and not np.any(Zd[1][9])
    assert np.abs(Zd[0][8]).max() > 0 and np.abs(Zd[1][0]).max() > 0
    if n == 4:   # ϵ reaches the result: the (3, 4) block of Z++ is not zero
        assert np.abs(Zd[0][1, 0][2::4, 3::4]).max() > 0


# ---- 2. ragged batch and tile edges ----------------------------------------------------------------------------------------------
def ragged_sets(depol=0.03):
    hg = rtamd.scenes.hg_like_greek(0.7, 33)
    return [rt.get_greek_rayleigh(depol), hg, scaled(hg, -1.0), scaled(hg, 0.0)]


def test_ragged_batch_on_the_c2_nodes():
    μ = rtamd.scenes.scene_C2(S=8, Nz=2).quad_points.qp_μ
    assert μ.size == 20 and np.any(μ == 1.0)
    sets = ragged_sets()
    Zd = rtamd.compute_Z_moments_batch(rt.Stokes_IQU(), μ, sets, 5, device=0)
    check_parity(3, μ, sets, 0, 5, Zd, "ragged batch, N = 60")
    for Z in Zd:
        assert not np.any(Z[3:, 0]) and not np.any(Z[:, 3])   # Rayleigh (l_max = 3) from m = 3 on; the all-zero set
        assert np.array_equal(Z[:, 2], -Z[:, 1]) and np.abs(Z[:, 1]).max() > 0   # the negated set (zeros of either sign are equal)


@pytest.mark.parametrize("n,nμ", [(4, 17), (3, 1), (4, 1), (1, 70)])
def test_tile_edges(n, nμ):
    """N = 68: one full tile and four columns; N = 3, 4: one node; N = 70 with n = 1"""
    μ = np.linspace(0.02, 1.0, nμ) if nμ > 1 else np.array([0.6])
    sets = [with_epsilon(rtamd.scenes.hg_like_greek(0.6, 14)), rt.get_greek_rayleigh(0.1)]
    Zd = rtamd.compute_Z_moments_batch(POL[n](), μ, sets, 3, device=0)
    check_parity(n, μ, sets, 0, 3, Zd, f"tile edges n = {n}, n_mu = {nμ}")


# ---- 3. long inner dimension, large m ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m_first", [0, 60, 119, 120])
def test_long_inner_dimension(m_first):
    μ = np.array([1.0, 0.93, 0.5, 0.11, 3.8e-4, 0.64])
    g = with_epsilon(rtamd.scenes.hg_like_greek(0.7, 121))
    Zd = rtamd.compute_Z_moments_batch(rt.Stokes_IQUV(), μ, [g], 1, m_first=m_first, device=0)
    check_parity(4, μ, [g], m_first, 1, Zd, f"l_max = 121, m = {m_first}")
    assert np.abs(Zd[0]).max() > 0


# ---- 4. layouts ------------------------------------------------------------------------------------------------------------------
def test_layouts_windows_and_batches_are_bitwise():
    μ = rtamd.scenes.scene_C2(S=8, Nz=2).quad_points.qp_μ[:7]
    hg = with_epsilon(rtamd.scenes.hg_like_greek(0.7, 12))
    sets = [rt.get_greek_rayleigh(0.03), hg, scaled(hg, -0.5), scaled(hg, 0.25), rt.get_greek_rayleigh(0.2), with_epsilon(rtamd.scenes.hg_like_greek(0.5, 7))]
    pol = rt.Stokes_IQUV()
    full = rtamd.compute_Z_moments_batch(pol, μ, sets, 6, device=0)
    again = rtamd.compute_Z_moments_batch(pol, μ, sets, 6, device=0)
    window = rtamd.compute_Z_moments_batch(pol, μ, sets, 3, m_first=2, device=0)
    for a, b, w in zip(full, again, window):
        assert np.array_equal(a, b) and np.array_equal(w, a[2:5])
    for k in (0, 1, 5):   # a set alone, and with the l_pad of the batch gone
        one = rtamd.compute_Z_moments_batch(pol, μ, [sets[k]], 6, device=0)
        assert np.array_equal(one[0][:, 0], full[0][:, k]) and np.array_equal(one[1][:, 0], full[1][:, k])
    # the Dual layout [N, N, K, M, P] for sets ordered k fastest, against the value layout [N, N, nG, M]
    raw = L.z_moments(4, μ, [rows(g) for g in sets], 6)
    for K in (2, 3, 6, 1):
        dual = L.z_moments(4, μ, [rows(g) for g in sets], 6, set_inner=K)
        assert dual[0].shape == (6 // K, 6, K, 28, 28)
        for p in range(6 // K):
            for k in range(K):
                assert np.array_equal(dual[0][p, :, k], raw[0][:, k + K * p]) and np.array_equal(dual[1][p, :, k], raw[1][:, k + K * p])
    assert np.array_equal(np.swapaxes(raw[0], -1, -2), full[0]) and raw[2] > 0.0


# ---- 5. known answer -------------------------------------------------------------------------------------------------------------
def test_natraj_z_from_the_device():
    g = np.load(GOLD / "natraj.npz")
    m = on_device(helpers.one_layer_rayleigh(rt, float(np.degrees(np.arccos(0.2))), g["vza"], g["vaz"], 0.5, 0.0))
    sc = rtamd.prepare_scene(m)
    assert sc.N == 136
    np.testing.assert_allclose(sc.Zmp, g["Zmp"], rtol=0, atol=1e-13)


# ---- 6. through the scene --------------------------------------------------------------------------------------------------------
def test_rt_run_with_device_z(cref):
    """the smallest configuration of test_gpu_rt_run.py::test_rt_run_parity, against the C oracle at that test's tolerance"""
    m = rtamd.scenes.make_scene(1, 3, 6, 24, seed=4)
    md = rtamd.scenes.make_scene(1, 3, 6, 24, seed=4, z_moments_on_device=True)
    assert md.params.z_moments_on_device and not m.params.z_moments_on_device
    p = cref.pack_scene(helpers.oracle_scene(m))
    Rr, Tr, info = cref.rt_run(p)
    assert info == 0
    Rd, Td = rtamd.rt_run(md)[:2]
    Rh, Th = rtamd.rt_run(m)[:2]
    for X, Xr, what in ((Rd, Rr, "R device Z vs oracle"), (Td, Tr, "T device Z vs oracle"), (Rd, Rh, "R device Z vs host Z"),
                        (Td, Th, "T device Z vs host Z")):
        helpers.assert_stokes_close(X, Xr, what=what)
    sd, sh = rtamd.prepare_scene(md), rtamd.prepare_scene(m)
    np.testing.assert_allclose(sd.Zpp, sh.Zpp, rtol=0, atol=1e-13)


def test_banded_scene_with_device_z():
    m = bc.banded(78, 2)
    md = on_device(m)
    Zh, Zd = rt.z_bases(m), rt.z_bases(md)
    assert Zd[0].shape == Zh[0].shape == (m.params.max_m, 7, 15, 15)
    greeks = [m.greek_rayleigh] + [a.greek_coefs for band in m.bands.aerosol_optics for a in band]
    check_parity(3, m.quad_points.qp_μ, greeks, 0, m.params.max_m, Zd, "banded scene, K = 7")
    with rt.make_handle(m) as h:
        R0, T0 = rt.run_scene_device_optics(h, m)
    with rt.make_handle(md) as h:
        R1, T1 = rt.run_scene_device_optics(h, md)
    helpers.assert_stokes_close(R1, R0, what="banded R, device Z vs host Z")
    helpers.assert_stokes_close(T1, T0, what="banded T, device Z vs host Z")


def test_rt_run_rrs_with_device_z():
    """the smallest case of test_gpu_rrs.py::test_rt_run_rrs_parity: the Raman Z of greek_raman through the device as well"""
    m = rtamd.scenes.make_scene(1, 3, 3, 24, seed=1 + 3 + 24, aerosol_total=0.1)
    md = on_device(m)
    vp = 0.02 * (1.0 + 0.1 * np.arange(5))
    RS = rt.RRS(greek_raman=rt.get_greek_rayleigh(0.2), ϖ_Cabannes=0.96, ϖ_λ1λ0=vp, i_λ1λ0=np.asarray([-4, -1, 2, 7, 3]), rrs_strict_reference=False)
    Zr_h, Zr_d = rt.raman_z(RS, m), rt.raman_z(RS, md)
    assert Zr_d[0].shape == Zr_h[0].shape
    np.testing.assert_allclose(Zr_d[0], Zr_h[0], rtol=0, atol=1e-13)
    np.testing.assert_allclose(Zr_d[1], Zr_h[1], rtol=0, atol=1e-13)
    got, ref = rt.rt_run_rrs(RS, md), rt.rt_run_rrs(RS, m)
    for k, what in enumerate(("R", "T")):
        helpers.assert_stokes_close(got[k], ref[k], what=f"RRS {what}, device Z vs host Z")
    assert np.abs(ref[2]).max() > 0
    for k, what in ((2, "ieR"), (3, "ieT")):
        helpers.assert_op_close(got[k], ref[k], 1e-9, f"RRS {what}, device Z vs host Z")


# ---- 7. through the Dual run -----------------------------------------------------------------------------------------------------
def test_aerosol_optics_partials_on_the_device():
    m = bc.banded(78, 2)
    hg = lambda g, f: rt.AerosolOptics(scaled(with_epsilon(rtamd.scenes.hg_like_greek(g, m.params.l_trunc)), f), 0.1 * f, 0.05)
    items = [(0, hg(0.6, 1.0), None, 0), (1, hg(0.7, -0.4), None, 2), (1, hg(0.5, 0.0), None, 1)]
    dev = rtamd.aerosol_optics_partials(m, items, device=0)
    one = rtamd.aerosol_optics_partial(m, *items[1], device=0)
    worst = 0.0
    for (i_aer, d, _, band), pd in zip(items, dev):
        ph = rtamd.aerosol_optics_partial(m, i_aer, d, None, band)
        k = 1 + i_aer + 2 * band
        assert pd.dZpp.shape == ph.dZpp.shape and np.array_equal(pd.dω̃, ph.dω̃) and np.array_equal(pd.dfᵗ, ph.dfᵗ)
        others = [j for j in range(7) if j != k]
        assert not np.any(pd.dZpp[:, others]) and not np.any(pd.dZmp[:, others])
        worst = max(worst, check_parity(3, m.quad_points.qp_μ, [d.greek_coefs], 0, m.params.max_m,
                                        (pd.dZpp[:, k:k + 1], pd.dZmp[:, k:k + 1]), f"dZ of item (aerosol {i_aer}, band {band})"))
    assert np.array_equal(one.dZpp, dev[1].dZpp) and np.array_equal(one.dZmp, dev[1].dZmp)


def test_chain_to_rt_run_dual_with_device_z():
    """test_gpu_mie_dual.py::test_chain_to_rt_run_dual with the derivative bases from the device: the Dual chain moves by rounding only
    (1e-10 of the largest |dR|, the suite's bar for two Float64 routes of one run)"""
    sc = rtamd.scattering
    kw_r, kw_i = (unicodedata.normalize("NFKC", s) for s in ("nᵣ", "nᵢ"))
    base = {"r_m": 0.3, "σ_g": 1.6, kw_r: 1.3, kw_i: 0.001, "λ": 0.55, "r_max": 1.0, "nquad_radius": 37, "truncation": sc.δBGE(10, 2.0)}
    m = rtamd.scenes.make_mie_scene(1, 3, 6, 24, seed=4, **base)
    md = on_device(m)
    aer = sc.Aerosol(sc.LogNormal(math.log(0.3), math.log(1.6)), 1.3, 0.001)
    mie = sc.make_mie_model(sc.NAI2(), aer, 0.55, rtamd.Stokes_I(), sc.δBGE(10, 2.0), 1.0, 37)
    aero, partials = sc.compute_aerosol_optical_properties(mie, autodiff=True, wrt=("nᵣ", "nᵢ"))
    _, d_trunc = sc.truncate_phase(mie.truncation_type, aero, partials=partials)
    ops_h = [sc.aerosol_optics_partial(m, 0, d) for d in d_trunc]
    ops_d = sc.aerosol_optics_partials(md, [(0, d, None, None) for d in d_trunc], device=md.params.architecture.device)
    with rt.make_handle(m) as h:
        R0, T0, dR0, dT0 = rt.rt_run_dual_device_optics(h, m, ops_h)
    with rt.make_handle(md) as h:
        R1, T1, dR1, dT1 = rt.rt_run_dual_device_optics(h, md, ops_d)
    helpers.assert_stokes_close(R1, R0, what="R, device Z vs host Z")
    for c in range(2):
        assert np.abs(dR0[c]).max() > 0
        helpers.assert_op_close(dR1[c], dR0[c], 1e-10, f"dR_SFI column {c}, device Z vs host Z")
        helpers.assert_op_close(dT1[c], dT0[c], 1e-10, f"dT_SFI column {c}, device Z vs host Z")
