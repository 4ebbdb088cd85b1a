"""Mie aerosol optics on the GPU (csrc/mom_mie.hip: mom_mie_nai2, mom_mie_coefficients) against the numpy oracle
(tests/mie_oracle.py), and the chain compute_aerosol_optical_properties -> truncate_phase -> scene -> rt_run.

Tolerance of the full call: relative to the largest magnitude of each output array, 8 x the distance between the Float64 and the
long-double run of the oracle ON THE SAME INPUTS of that case (never measured on the GPU result); the factor is the margin for the
GEMM's summation order."""
import functools
import math

import numpy as np
import pytest

import helpers
import mie_oracle as mo

pytestmark = pytest.mark.gpu

MS = [(1.3, 0.001), (1.5, 0.1), (1.33, 0.0)]
XS = [0.05, 0.4, 4.1, 11.4, 40.0]
# (r_max, nquad_radius, λ, n_r, n_i, r_m, σ_g); the kernel tiles the radii by 16 and gives a wavefront a second tile beyond
# 128 tiles (2048 radii)
CASES = {
    "one_radius": (1.0, 1, 0.55, 1.3, 0.001, 0.3, 1.6),
    "case2": (1.0, 37, 0.55, 1.3, 0.001, 0.3, 1.6),          # n_max 11 .. 31, n_mu = 61, three radius tiles
    "absorbing": (0.5, 20, 0.76, 1.5, 0.1, 0.3, 1.6),         # nmx from |y|
    "below_tile_edge": (1.0, 31, 0.55, 1.3, 0.001, 0.3, 1.6),
    "full_tile": (1.0, 32, 0.55, 1.3, 0.001, 0.3, 1.6),
    "above_tile_edge": (1.0, 33, 0.55, 1.3, 0.001, 0.3, 1.6),
    "second_tile_per_wave": (1.0, 2061, 0.55, 1.3, 0.001, 0.3, 1.6),   # 129 tiles over 128 chunks
}


def _model(rtamd, case):
    sc = rtamd.scattering
    r_max, nquad, lam, n_r, n_i, r_m, σ_g = CASES[case]
    aer = sc.Aerosol(sc.LogNormal(math.log(r_m), math.log(σ_g)), n_r, n_i)
    return sc.make_mie_model(sc.NAI2(), aer, lam, None, None, r_max, nquad)


@functools.lru_cache(maxsize=None)
def _inputs_and_oracle(case, autodiff):
    """host inputs of the product, the Float64 oracle on them, and the per-array bound from the long-double oracle"""
    import rtamd
    inp = rtamd.scattering.mie_inputs(_model(rtamd, case), autodiff)
    _, _, lam, n_r, n_i, _, _ = CASES[case]
    rows = inp.w / (4 * np.pi * inp.r ** 2)
    o64 = mo.nai2_sums(inp.r, rows, lam, n_r, n_i)
    o80 = mo.nai2_sums(inp.r.astype(np.longdouble), rows.astype(np.longdouble), lam, n_r, n_i)
    bound = {q: 8 * mo.rel_max(o64[q], o80[q]) for q in ("bulk_f", "C", "greek")}
    for k in range(1, rows.shape[0]):   # the partial rows on their own scale as well: they are smaller than the value row
        bound.update({(q, k): 8 * mo.rel_max(o64[q][k], o80[q][k]) for q in ("bulk_f", "C", "greek")})
    return inp, o64, bound


def _call(rtamd, inp, case, flags=0):
    _, _, lam, n_r, n_i, _, _ = CASES[case]
    return rtamd._lib.mie_nai2(inp.r, inp.w, lam, n_r, n_i, inp.w_μ, inp.π_, inp.τ_, inp.P, inp.P2, inp.R2, inp.T2, flags=flags)


@pytest.mark.parametrize("n_r,n_i", MS)
def test_coefficients_against_oracle(rtamd, n_r, n_i):
    """a_n, b_n per size parameter, relative to that size parameter's largest coefficient; bound: 8 x the distance between the
    Float64 and the long-double oracle at the same x (the recurrences amplify a last-bit difference in sin x, cos x alike)."""
    n_max = int(mo.n_max_of(max(XS))) + 3          # more rows than any x needs: the rest must be zeros
    a, b = rtamd._lib.mie_coefficients(XS, n_r, n_i, n_max)
    o64 = mo.mie_ab(XS, n_r, n_i, np.float64, n_rows=n_max)
    o80 = mo.mie_ab(XS, n_r, n_i, np.longdouble, n_rows=n_max)
    ref = np.stack([o64[0] + 1j * o64[1], o64[2] + 1j * o64[3]])
    ext = np.stack([o80[0] + 1j * o80[1], o80[2] + 1j * o80[3]])
    got = np.stack([a, b])
    for j, x in enumerate(XS):
        big = np.abs(ref[:, :, j]).max()
        bound = 8 * float(np.abs(ref[:, :, j] - ext[:, :, j]).max() / big)
        d = float(np.abs(got[:, :, j] - ref[:, :, j]).max() / big)
        print(f"m = {n_r} + {n_i}i, x = {x}: GPU - oracle = {d:.3e}, bound {bound:.3e}")
        assert d <= bound
        assert np.all(got[:, o64[4][j]:, j] == 0)


@pytest.mark.parametrize("case", list(CASES))
def test_full_call_against_oracle(rtamd, case):
    inp, o64, bound = _inputs_and_oracle(case, False)
    bulk, Cx, greek, ms = _call(rtamd, inp, case)
    assert bulk.shape == o64["bulk_f"].shape and greek.shape == o64["greek"].shape
    for name, got in (("bulk_f", bulk), ("C", Cx), ("greek", greek)):
        d = mo.rel_max(got, o64[name])
        print(f"{case}: {name}: GPU - oracle = {d:.3e}, bound {bound[name]:.3e} (factor used {8 * d / max(bound[name], 1e-300):.2f} of 8)")
        assert d <= bound[name], (case, name, d, bound[name])
    assert np.all(ms >= 0)


def test_partial_weight_rows(rtamd):
    """case 2 with nW = 3: the value row and the rows of ∂wₓ/∂r_m, ∂wₓ/∂σ_g; row 0 is bitwise the nW = 1 result (the rows have
    accumulators of their own)."""
    inp, o64, bound = _inputs_and_oracle("case2", True)
    assert inp.w.shape[0] == 3
    bulk, Cx, greek, _ = _call(rtamd, inp, "case2")
    for name, got in (("bulk_f", bulk), ("C", Cx), ("greek", greek)):
        d = mo.rel_max(got, o64[name])
        print(f"nW = 3: {name}: GPU - oracle = {d:.3e}, bound {bound[name]:.3e}")
        assert d <= bound[name]
        for k in (1, 2):
            d = mo.rel_max(got[k], o64[name][k])
            print(f"nW = 3: {name}[{k}]: GPU - oracle = {d:.3e}, bound {bound[name, k]:.3e}")
            assert d <= bound[name, k]
    inp1, _, _ = _inputs_and_oracle("case2", False)
    b1, C1, g1, _ = _call(rtamd, inp1, "case2")
    assert np.array_equal(b1[0], bulk[0]) and np.array_equal(C1[0], Cx[0]) and np.array_equal(g1[0], greek[0])


@pytest.mark.parametrize("case", ["case2", "second_tile_per_wave"])
def test_bitwise_repeatable_and_tile_k_bound(rtamd, case):
    """Two consecutive calls are bitwise equal (fixed-order reductions), and so is a call whose radius tiles all run to the global
    n_max (MOM_MIE_FULL_K): the tile rule leaves out exact zeros only."""
    inp, _, _ = _inputs_and_oracle(case, False)
    first, second, full = _call(rtamd, inp, case), _call(rtamd, inp, case), _call(rtamd, inp, case, flags=rtamd._lib.MOM_MIE_FULL_K)
    for a, b, c in zip(first[:3], second[:3], full[:3]):
        assert np.array_equal(a, b)
        assert np.array_equal(a, c)


def test_rejected_arguments(rtamd):
    lib, L = rtamd.load(), rtamd._lib
    inp, _, _ = _inputs_and_oracle("case2", False)
    tabs = [L.f64(t.T) for t in (inp.π_, inp.τ_, inp.P, inp.P2, inp.R2, inp.T2)]
    nR, n_mu, n_max, l_max = inp.r.size, inp.w_μ.size, tabs[0].shape[0], tabs[2].shape[0]
    out = [np.zeros((4, 4, n_mu)), np.zeros((4, 2)), np.zeros((4, 6, l_max)), np.zeros(3)]
    w4 = L.f64(np.repeat(inp.w, 4, axis=0))

    def call(r=inp.r, nR=nR, nW=1, lam=0.55, n_i=0.001, n_mu=n_mu, n_max=n_max, flags=0):
        r = L.f64(r)
        return lib.mom_mie_nai2(0, nR, L.dp(r), nW, L.dp(w4), lam, 1.3, n_i, n_mu, L.dp(L.f64(inp.w_μ)), n_max, L.dp(tabs[0]),
                                L.dp(tabs[1]), l_max, *[L.dp(t) for t in tabs[2:]], flags, *[L.dp(o) for o in out])

    assert call() == L.MOM_OK and call(nW=4) == L.MOM_OK
    swapped, negative = inp.r.copy(), inp.r.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    negative[0] = 0.0
    for kw in (dict(nR=0), dict(n_mu=0), dict(nW=0), dict(nW=5), dict(lam=0.0), dict(lam=-0.55), dict(n_i=-1e-3), dict(r=swapped),
               dict(r=negative), dict(n_max=n_max - 1), dict(flags=2)):
        assert call(**kw) == L.MOM_EINVAL, kw
        assert b"mom_mie_nai2" in lib.mom_last_global_error()
    x = L.f64([1.0, 40.0])
    o = [np.zeros((10, 2)) for _ in range(4)]
    assert lib.mom_mie_coefficients(0, 2, L.dp(x), 1.3, 0.0, 10, *[L.dp(a) for a in o]) == L.MOM_EINVAL   # n_max(40) = 64 > 10
    assert lib.mom_mie_coefficients(0, 2, L.dp(x), 1.3, -0.1, 64, *[L.dp(a) for a in o]) == L.MOM_EINVAL


def test_public_interface_and_rt_run(rtamd, cref):
    """compute_aerosol_optical_properties -> truncate_phase(δBGE(10, 2)) -> the Mie scene -> rt_run at the smallest configuration of
    test_gpu_rt_run.py, against the CPU oracle's rt_run fed the Mie oracle's aerosol optics (same truncation), at that test's
    tolerance.  Also autodiff=True's value is the plain call's, and compute_ref_aerosol_extinction is its k."""
    sc = rtamd.scattering
    kw = dict(r_m=0.3, σ_g=1.6, nᵣ=1.3, nᵢ=0.001, λ=0.55, r_max=1.0, nquad_radius=37, truncation=sc.δBGE(10, 2.0))
    m = rtamd.scenes.make_mie_scene(1, 3, 6, 24, seed=4, **kw)
    aer = sc.Aerosol(sc.LogNormal(math.log(0.3), math.log(1.6)), 1.3, 0.001)
    mie = sc.make_mie_model(sc.NAI2(), aer, 0.55, rtamd.Stokes_I(), sc.δBGE(10, 2.0), 1.0, 37)
    plain = sc.compute_aerosol_optical_properties(mie)
    g, ω, k = mo.aerosol_optics(*CASES["case2"])
    assert plain.fᵗ == 1.0 and 0 < plain.ω̃ < 1
    dual, partials = sc.compute_aerosol_optical_properties(mie, autodiff=True)
    assert dual.ω̃ == plain.ω̃ and np.array_equal(dual.greek_coefs.β, plain.greek_coefs.β) and len(partials) == 2
    assert sc.compute_ref_aerosol_extinction(mie) == plain.k
    assert len(m.aerosol_optics[0].greek_coefs.β) == 10 and 0 < m.aerosol_optics[0].fᵗ < 1
    R, T = rtamd.rt_run(m)[:2]
    ref_optics = sc.truncate_phase(sc.δBGE(10, 2.0), rtamd.corert.AerosolOptics(greek_coefs=sc._greek(g), ω̃=float(ω), fᵗ=1.0, k=float(k)))
    m_ref = rtamd.scenes.make_scene(1, 3, 6, 24, seed=4)
    m_ref.aerosol_optics = [ref_optics]
    Rr, Tr, info = cref.rt_run(cref.pack_scene(helpers.oracle_scene(m_ref)))
    assert info == 0
    print("rt_run: R", helpers.assert_stokes_close(R, Rr, what="R mie scene"), "T", helpers.assert_stokes_close(T, Tr, what="T mie scene"))
