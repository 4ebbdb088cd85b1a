"""The Dual run of the Mie aerosol optics on the GPU (csrc/mom_mie.hip: mom_mie_nai2_dual, mom_mie_coefficients_dual) -- partials
with respect to the refractive index (n_r, n_i) -- against the forward-mode numpy twin (tests/mie_dual_oracle.py), and the chain
Mie Dual -> truncate_phase(partials=) -> aerosol_optics_partial -> rt_run_dual_device_optics against central differences of the
value route.

Tolerances as in test_gpu_mie.py: per array and per row on the row's own scale, 8 x the distance between the Float64 and the
long-double run of the ORACLE on the same inputs (never measured on the GPU result), at least 2^-46."""
import functools
import math
import unicodedata

import numpy as np
import pytest

import mie_oracle as mo
import mie_dual_oracle as md

pytestmark = pytest.mark.gpu

MS = [(1.3, 0.001), (1.5, 0.1), (1.33, 0.0)]
XS = [0.05, 0.4, 4.1, 11.4, 40.0]
FLOOR = 2.0 ** -46
# (r_max, nquad_radius, λ, n_r, n_i, r_m, σ_g); the kernel tiles the radii by 16, the Dual form gives a block 16 of the n_mu rows
CASES = {
    "one_radius": (1.0, 1, 0.55, 1.3, 0.001, 0.3, 1.6),
    "case2": (1.0, 37, 0.55, 1.3, 0.001, 0.3, 1.6),
    "absorbing": (0.5, 20, 0.76, 1.5, 0.1, 0.3, 1.6),
    "no_absorption": (1.0, 33, 0.55, 1.33, 0.0, 0.3, 1.6),
    "below_tile_edge": (1.0, 31, 0.55, 1.3, 0.001, 0.3, 1.6),
    "full_tile": (1.0, 32, 0.55, 1.3, 0.001, 0.3, 1.6),
    "above_tile_edge": (1.0, 33, 0.55, 1.3, 0.001, 0.3, 1.6),
    "partial_mu_block": (0.05, 5, 0.55, 1.3, 0.001, 0.03, 1.6),       # n_mu = 27: a partial mu block, one radius tile
    "second_tile_per_wave": (1.0, 2061, 0.55, 1.3, 0.001, 0.3, 1.6),   # 129 tiles over 128 chunks
}
ARRAYS = ("bulk_f", "C", "greek")


def _model(rtamd, case):
    sc = rtamd.scattering
    r_max, nquad, lam, n_r, n_i, r_m, σ_g = CASES[case]
    aer = sc.Aerosol(sc.LogNormal(math.log(r_m), math.log(σ_g)), n_r, n_i)
    return sc.make_mie_model(sc.NAI2(), aer, lam, None, None, r_max, nquad)


@functools.lru_cache(maxsize=None)
def _inputs_and_oracle(case, autodiff=False):
    """host inputs of the product, the Float64 twin on them (weight row 0), and the bound of each index row of each array"""
    import rtamd
    inp = rtamd.scattering.mie_inputs(_model(rtamd, case), autodiff)
    _, _, lam, n_r, n_i, _, _ = CASES[case]
    row = inp.w[0] / (4 * np.pi * inp.r ** 2)
    o64 = md.nai2_sums_dual(inp.r, row, lam, n_r, n_i)
    o80 = md.nai2_sums_dual(inp.r.astype(np.longdouble), row.astype(np.longdouble), lam, n_r, n_i)
    bound = {(q, c): max(8 * mo.rel_max(o64["d_" + q][c], o80["d_" + q][c]), FLOOR) for q in ARRAYS for c in (0, 1)}
    bound.update({q: max(8 * mo.rel_max(o64[q], o80[q]), FLOOR) for q in ARRAYS})
    return inp, o64, bound


def _call(rtamd, inp, case, flags=0, dual=True):
    _, _, lam, n_r, n_i, _, _ = CASES[case]
    fn = rtamd._lib.mie_nai2_dual if dual else rtamd._lib.mie_nai2
    return fn(inp.r, inp.w, lam, n_r, n_i, inp.w_μ, inp.π_, inp.τ_, inp.P, inp.P2, inp.R2, inp.T2, flags=flags)


def _check_index_rows(case, got, o64, bound, nW):
    for q, arr in zip(ARRAYS, got):
        for c, name in enumerate(("n_r", "n_i")):
            d = mo.rel_max(arr[nW + c], o64["d_" + q][c])
            print(f"{case}: d {q} / d{name}: GPU - oracle = {d:.3e}, bound {bound[q, c]:.3e}")
            assert d <= bound[q, c], (case, q, name, d, bound[q, c])


@pytest.mark.parametrize("n_r,n_i", MS)
def test_coefficients_dual_against_oracle(rtamd, n_r, n_i):
    """da_n/dm, db_n/dm per size parameter against the twin's d/dn_r (the twin's own d/dn_i is i times that to rounding:
    test_oracle_mie_dual.py), relative to that size parameter's largest partial; a, b bitwise those of mie_coefficients; exact
    zeros above each x's own n_max in all eight arrays."""
    n_max = int(mo.n_max_of(max(XS))) + 3
    a, b, da, db = rtamd._lib.mie_coefficients_dual(XS, n_r, n_i, n_max)
    a0, b0 = rtamd._lib.mie_coefficients(XS, n_r, n_i, n_max)
    assert np.array_equal(a, a0) and np.array_equal(b, b0)
    o64 = md.mie_ab_dual(XS, n_r, n_i, np.float64, n_rows=n_max)
    o80 = md.mie_ab_dual(XS, n_r, n_i, np.longdouble, n_rows=n_max)
    got = np.stack([da, db])
    for c, rot in ((0, 1.0), (1, 1j)):          # d/dn_r = d/dm, d/dn_i = i d/dm
        ref = np.stack([o64[0].d[c] + 1j * o64[1].d[c], o64[2].d[c] + 1j * o64[3].d[c]])
        ext = np.stack([o80[0].d[c] + 1j * o80[1].d[c], o80[2].d[c] + 1j * o80[3].d[c]])
        for j, x in enumerate(XS):
            big = np.abs(ref[:, :, j]).max()
            bound = max(8 * float(np.abs(ref[:, :, j] - ext[:, :, j]).max() / big), FLOOR)
            d = float(np.abs(rot * got[:, :, j] - ref[:, :, j]).max() / big)
            print(f"m = {n_r} + {n_i}i, x = {x}, d/dn_{'ri'[c]}: GPU - oracle = {d:.3e}, bound {bound:.3e}")
            assert d <= bound
    for j in range(len(XS)):
        for arr in (a, b, da, db):
            assert np.all(arr[o64[4][j]:, j] == 0)


@pytest.mark.parametrize("case", list(CASES))
def test_index_rows_against_oracle(rtamd, case):
    """nW = 1: three output rows; row 0 is bitwise mie_nai2's, rows 1 and 2 are d/dn_r and d/dn_i of its sums"""
    inp, o64, bound = _inputs_and_oracle(case)
    bulk, Cx, greek, ms = _call(rtamd, inp, case)
    n_mu, l_max = inp.w_μ.size, inp.P.shape[1]
    assert bulk.shape == (3, 4, n_mu) and Cx.shape == (3, 2) and greek.shape == (3, 6, l_max)
    value = _call(rtamd, inp, case, dual=False)
    for got, want, q in zip((bulk, Cx, greek), value[:3], ARRAYS):
        assert np.array_equal(got[:1], want), q
        assert mo.rel_max(got[0], o64[q][0]) <= bound[q]
    _check_index_rows(case, (bulk, Cx, greek), o64, bound, 1)
    assert np.all(ms >= 0)


@pytest.mark.parametrize("case", ["case2", "second_tile_per_wave"])
def test_three_weight_rows_bitwise(rtamd, case):
    """nW = 3: rows 0..2 are bitwise the mie_nai2 result for the same three rows, rows 3 and 4 are within bound (and bitwise the
    index rows of the nW = 1 call: they have accumulators of their own); two calls are bitwise equal, and so is a call whose
    radius tiles all run to the global n_max (MOM_MIE_FULL_K)."""
    inp, _, _ = _inputs_and_oracle(case, True)
    inp1, o64, bound = _inputs_and_oracle(case)
    assert inp.w.shape[0] == 3
    first, second = _call(rtamd, inp, case), _call(rtamd, inp, case)
    full = _call(rtamd, inp, case, flags=rtamd._lib.MOM_MIE_FULL_K)
    value = _call(rtamd, inp, case, dual=False)
    one = _call(rtamd, inp1, case)
    for a, b, c, v, o in zip(first[:3], second[:3], full[:3], value[:3], one[:3]):
        assert a.shape[0] == 5
        assert np.array_equal(a, b)
        assert np.array_equal(a, c)
        assert np.array_equal(a[:3], v)
        assert np.array_equal(a[3:], o[1:])
    _check_index_rows(case, first[:3], o64, bound, 3)


def test_rejected_arguments(rtamd):
    lib, L = rtamd.load(), rtamd._lib
    inp, _, _ = _inputs_and_oracle("case2")
    tabs = [L.f64(t.T) for t in (inp.π_, inp.τ_, inp.P, inp.P2, inp.R2, inp.T2)]
    nR, n_mu, n_max, l_max = inp.r.size, inp.w_μ.size, tabs[0].shape[0], tabs[2].shape[0]
    out = [np.zeros((6, 4, n_mu)), np.zeros((6, 2)), np.zeros((6, 6, l_max)), np.zeros(3)]
    w4 = L.f64(np.repeat(inp.w, 4, axis=0))

    def call(r=inp.r, nR=nR, nW=1, lam=0.55, n_i=0.001, n_mu=n_mu, n_max=n_max, flags=0, null=None):
        r = L.f64(r)
        outs = [None if null == i else L.dp(o) for i, o in enumerate(out)]
        return lib.mom_mie_nai2_dual(0, nR, L.dp(r), nW, L.dp(w4), lam, 1.3, n_i, n_mu, L.dp(L.f64(inp.w_μ)), n_max, L.dp(tabs[0]),
                                     L.dp(tabs[1]), l_max, *[L.dp(t) for t in tabs[2:]], flags, *outs)

    assert call() == L.MOM_OK and call(nW=3) == L.MOM_OK and call(null=3) == L.MOM_OK      # gpu_ms may be null
    swapped, negative = inp.r.copy(), inp.r.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    negative[0] = 0.0
    for kw in (dict(nW=0), dict(nW=4), dict(nR=0), dict(n_mu=0), dict(lam=0.0), dict(lam=-0.55), dict(n_i=-1e-3), dict(r=swapped),
               dict(r=negative), dict(n_max=n_max - 1), dict(flags=2), dict(null=0), dict(null=1), dict(null=2)):
        assert call(**kw) == L.MOM_EINVAL, kw
        assert b"mom_mie_nai2_dual" in lib.mom_last_global_error()
    x = L.f64([1.0, 40.0])
    o = [np.zeros((64, 2)) for _ in range(8)]
    ptrs = [L.dp(a) for a in o]
    assert lib.mom_mie_coefficients_dual(0, 2, L.dp(x), 1.3, 0.0, 64, *ptrs) == L.MOM_OK
    for missing in range(4, 8):
        args = [None if i == missing else p for i, p in enumerate(ptrs)]
        assert lib.mom_mie_coefficients_dual(0, 2, L.dp(x), 1.3, 0.0, 64, *args) == L.MOM_EINVAL
        assert b"mom_mie_coefficients_dual" in lib.mom_last_global_error()
    assert lib.mom_mie_coefficients_dual(0, 2, L.dp(x), 1.3, 0.0, 10, *ptrs) == L.MOM_EINVAL      # n_max(40) = 64 > 10
    assert lib.mom_mie_coefficients_dual(0, 2, L.dp(x), 1.3, -0.1, 64, *ptrs) == L.MOM_EINVAL
    with pytest.raises(L.MomError, match="mom_mie_nai2_dual"):
        L.mie_nai2_dual(inp.r, w4[:4], 0.55, 1.3, 0.001, inp.w_μ, inp.π_, inp.τ_, inp.P, inp.P2, inp.R2, inp.T2)


def _stack(g):
    return np.stack([g.α, g.β, g.γ, g.δ, g.ϵ, g.ζ])


def test_public_interface(rtamd):
    """wrt = all four: the partials in the reference's order of x; the first two bitwise those of the default autodiff=True,
    the value bitwise the plain call's; a subset in the caller's order; ∂ω̃/∂n_i < 0; ∂k against the oracle's C row."""
    sc = rtamd.scattering
    mie = _model(rtamd, "case2")
    plain = sc.compute_aerosol_optical_properties(mie)
    _, two = sc.compute_aerosol_optical_properties(mie, autodiff=True)
    aero, four = sc.compute_aerosol_optical_properties(mie, autodiff=True, wrt=sc.ALL_AEROSOL_PARAMETERS)
    assert rtamd.ALL_AEROSOL_PARAMETERS == ("r_m", "σ_g", "nᵣ", "nᵢ") and len(four) == 4 and len(two) == 2
    assert np.array_equal(_stack(aero.greek_coefs), _stack(plain.greek_coefs)) and aero.ω̃ == plain.ω̃ and aero.k == plain.k
    for a, b in zip(four[:2], two):
        assert np.array_equal(_stack(a.greek_coefs), _stack(b.greek_coefs)) and a.ω̃ == b.ω̃ and a.k == b.k
    J = sc.aerosol_derivs(aero, four)
    assert J.shape == (6 * 61 + 2, 4) and np.all(np.isfinite(J))
    assert four[3].ω̃ < 0
    _, o64, bound = _inputs_and_oracle("case2")
    for c in (0, 1):
        d = abs(four[2 + c].k - o64["d_C"][c, 1]) / np.abs(o64["d_C"][c]).max()
        print(f"∂k/∂n_{'ri'[c]}: GPU - oracle = {d:.3e}, bound {bound['C', c]:.3e}")
        assert d <= bound["C", c]
    _, sub = sc.compute_aerosol_optical_properties(mie, autodiff=True, wrt=("nᵢ", "r_m"))
    assert np.array_equal(_stack(sub[0].greek_coefs), _stack(four[3].greek_coefs)) and sub[1].k == four[0].k
    _, only = sc.compute_aerosol_optical_properties(mie, autodiff=True, wrt=("nᵣ",))
    assert np.array_equal(_stack(only[0].greek_coefs), _stack(four[2].greek_coefs)) and only[0].ω̃ == four[2].ω̃
    with pytest.raises(ValueError):
        sc.compute_aerosol_optical_properties(mie, autodiff=True, wrt=("n_r",))


def test_chain_to_rt_run_dual(rtamd):
    """Refractive index -> Greek coefficients -> δ-BGE truncation -> phase-matrix bases -> rt_run_dual as one differentiable
    chain, against central differences of the VALUE route (plain Mie call, truncate_phase, rt_run) at n_r ± h and n_i ± h,
    h = 1e-4.  Bound: 4 x max |FD(h) - FD(2h)| relative to max |FD(h)|, from value runs only; unless that is <= 1e-3 the test
    shows nothing and fails."""
    sc, rt = rtamd.scattering, rtamd.corert
    # keyword names as Python spells them (identifiers are NFKC-normalised: the subscripts of nᵣ, nᵢ become plain letters)
    kw_r, kw_i = (unicodedata.normalize("NFKC", s) for s in ("nᵣ", "nᵢ"))
    base = {"r_m": 0.3, "σ_g": 1.6, kw_r: 1.3, kw_i: 0.001, "λ": 0.55, "r_max": 1.0, "nquad_radius": 37, "truncation": sc.δBGE(10, 2.0)}
    m = rtamd.scenes.make_mie_scene(1, 3, 6, 24, seed=4, **base)
    aer = sc.Aerosol(sc.LogNormal(math.log(0.3), math.log(1.6)), 1.3, 0.001)
    mie = sc.make_mie_model(sc.NAI2(), aer, 0.55, rtamd.Stokes_I(), sc.δBGE(10, 2.0), 1.0, 37)
    aero, partials = sc.compute_aerosol_optical_properties(mie, autodiff=True, wrt=("nᵣ", "nᵢ"))
    trunc, d_trunc = sc.truncate_phase(mie.truncation_type, aero, partials=partials)
    assert np.array_equal(trunc.greek_coefs.β, m.aerosol_optics[0].greek_coefs.β) and trunc.fᵗ == m.aerosol_optics[0].fᵗ
    ops = [sc.aerosol_optics_partial(m, 0, d) for d in d_trunc]
    with rt.make_handle(m) as h:
        R, T, dR, dT = rt.rt_run_dual_device_optics(h, m, ops)
    R0, T0 = rtamd.rt_run(m)[:2]
    assert np.allclose(R, R0, rtol=1e-12, atol=0) and np.allclose(T, T0, rtol=1e-12, atol=0)

    def value_run(**kw):
        return rtamd.rt_run(rtamd.scenes.make_mie_scene(1, 3, 6, 24, seed=4, **{**base, **kw}))[:2]

    h0 = 1e-4
    for c, name in enumerate(("nᵣ", "nᵢ")):
        fd = []
        key = (kw_r, kw_i)[c]
        for step in (h0, 2 * h0):
            hi, lo = value_run(**{key: base[key] + step}), value_run(**{key: base[key] - step})
            fd.append([(a - b) / (2 * step) for a, b in zip(hi, lo)])
        for mine, f1, f2, what in ((dR[c], fd[0][0], fd[1][0], "dR"), (dT[c], fd[0][1], fd[1][1], "dT")):
            big = float(np.abs(f1).max())
            bound = 4 * float(np.abs(f1 - f2).max()) / big
            d = float(np.abs(mine - f1).max()) / big
            print(f"{what}/d{name}: Dual chain - FD = {d:.3e}, bound {bound:.3e} (max |FD| = {big:.3e})")
            assert bound <= 1e-3, (what, name, bound)
            assert d <= bound, (what, name, d, bound)
