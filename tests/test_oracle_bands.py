"""Band-resolved aerosol optics on the host (corert.Bands, construct_layer_inputs, z_bases, absorption.optics_partials_host) against
the literal restatement of the reference's per-band algebra with materialised phase matrices (bands_oracle.py), and against the
paths for models without bands."""
import dataclasses

import numpy as np
import pytest

import bands_cases as bc
import bands_oracle as bo
import optics_dual_cases as oc
import rtamd

rt, ab = rtamd.corert, rtamd.absorption
CASES = [(S, nAer) for S in (78, 300) for nAer in (0, 1, 2)]


@pytest.fixture(scope="module")
def models():
    return {case: bc.banded(*case) for case in CASES}


@pytest.mark.parametrize("S,nAer", CASES)
def test_input_conditions(models, S, nAer):
    bc.assert_input_conditions(models[S, nAer], S, nAer)


@pytest.mark.parametrize("S,nAer", CASES)
def test_host_twin_is_the_restatement(models, S, nAer):
    """τ, ϖ, ndoubl, iface, τ_sum bitwise; Σ_k zw_k Z_k within 4 ulp of the materialised Z.  The weights re-associate two
    multiplications per `+` (oracle/momref.py: <= 1 ulp per TERM), so the ulp is that of the largest term zw_k Z_k of the entry:
    measured 4.0 at nAer = 2 (3.0 in ulp of Σ_k |zw_k Z_k|), 0 at nAer <= 1.  Where the terms of different bases cancel, the same
    distance is up to 128 ulp of the entry itself; no arithmetic on basis weights can do better there."""
    model = models[S, nAer]
    L = rt.construct_layer_inputs(model)
    bs = bo.band_scene(model)
    τ, ϖ, nd, iface, τ_sum = bo.layer_summary(bs)
    assert np.array_equal(L.τ, τ) and np.array_equal(L.ϖ, ϖ) and np.array_equal(L.τ_sum, τ_sum)
    assert np.array_equal(L.ndoubl, nd) and np.array_equal(L.iface, iface)
    assert L.zw.shape == (1 + 3 * nAer, S, bc.NZ)
    Zpp, Zmp = rt.z_bases(model)
    worst = 0.0
    for m in range(model.params.max_m):
        layers = bo.construct_core_optical_properties(bs, m)
        for z, lay in enumerate(layers):
            for Zb, Zref in ((Zpp[m], lay.Zpp), (Zmp[m], lay.Zmp)):
                got = np.zeros_like(Zref)
                for k in range(Zb.shape[0]):   # in basis order, one rounding per term and per addition
                    got = got + L.zw[k, :, z, None, None] * Zb[k][None]
                # a weighted sum of K terms: the bar is 4 ulp of the largest term of each entry
                scale = np.max(np.abs(L.zw[:, :, z, None, None] * Zb[:, None]), axis=0)
                err = np.abs(got - Zref)
                worst = max(worst, float(np.max(err / np.maximum(np.spacing(scale), 1e-300))))
                assert np.all(err <= 4 * np.spacing(scale)), (m, z)
    print(f"Σ zw Z vs materialised Z: worst {worst:.2f} ulp (bar 4)")


@pytest.mark.parametrize("S,nAer", CASES)
def test_weights_outside_the_band_are_zero(models, S, nAer):
    model = models[S, nAer]
    zw = rt.construct_layer_inputs(model).zw
    band_of = model.bands.band_of()
    for k in range(1, zw.shape[0]):
        outside = band_of != (k - 1) // max(nAer, 1)
        assert not np.any(zw[k, outside]) and not np.any(np.signbit(zw[k, outside]))


@pytest.mark.parametrize("S,nAer", [(78, 2), (300, 1), (78, 0)])
def test_partials_twin_against_the_complex_step(models, S, nAer):
    """optics_partials_host (banded) against Im / h of the restatement run on x + i h x': dτ, dϖ and the materialised dZ = Σ_k dzw_k Z_k
    to 1e-12 of each column's maximum"""
    model = models[S, nAer]
    ps = bc.parameters(model, 5)
    got = ab.optics_partials_host(model, ps)
    bs = bo.band_scene(model)
    Zpp, Zmp = rt.z_bases(model)
    K = Zpp.shape[1]
    ref = [bo.complex_step(bs, p, m=0) for p in ps]
    dτ, dϖ, dzw = oc.stack(got, K, S, bc.NZ)
    oc.assert_columns(dτ, np.array([r[0] for r in ref]), 1e-12, f"dτ twin vs complex step (S {S}, nAer {nAer})")
    oc.assert_columns(dϖ, np.array([r[1] for r in ref]), 1e-12, f"dϖ twin vs complex step (S {S}, nAer {nAer})")
    for Zb, k, name in ((Zpp[0], 2, "dZ⁺⁺"), (Zmp[0], 3, "dZ⁻⁺")):
        dZ = np.einsum("pksz,kij->psijz", dzw, Zb)
        oc.assert_columns(dZ, np.array([r[k] for r in ref]), 1e-12, f"{name} twin vs complex step (S {S}, nAer {nAer})")
    for q, g in zip(ps, got):
        assert (g.dzw is not None) == (nAer > 0 and any(x is not None for x in (q.w_rayl, q.dτ_aer, q.dω̃, q.dfᵗ)))


@pytest.mark.parametrize("nAer", [0, 2])
def test_one_band_is_the_unbanded_path(nAer):
    m = bc.unbanded(78, nAer)
    one = rt.with_bands(m, rt.Bands(np.array([0, 78]), m.τ_aer[None], [list(m.aerosol_optics)], np.array([m.ϖ_Cabannes])))
    a, b = rt.prepare_scene(m), rt.prepare_scene(one)
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        assert (x is None and y is None) or np.array_equal(x, y), f.name
    ps = oc.six_parameters(m)[2:]
    lead = lambda x: None if x is None else np.asarray(x)[None]
    ps1 = [dataclasses.replace(p, dτ_aer=lead(p.dτ_aer), dω̃=lead(p.dω̃), dfᵗ=lead(p.dfᵗ)) for p in ps]
    for x, y in zip(ab.optics_partials_host(m, ps), ab.optics_partials_host(one, ps1)):
        assert np.array_equal(x.dτ, y.dτ) and np.array_equal(x.dϖ, y.dϖ)
        assert (x.dzw is None and y.dzw is None) or np.array_equal(x.dzw, y.dzw)


def test_identical_bands_are_the_unbanded_layers():
    """three copies of the same aerosols: τ, ϖ, ndoubl, iface bitwise the unbanded model's, and the unbanded weights on the live bases"""
    m = bc.unbanded(300, 2)
    bs = bc.band_start(300)
    same = rt.with_bands(m, rt.Bands(bs, np.array([m.τ_aer] * 3), [list(m.aerosol_optics)] * 3, np.full(3, m.ϖ_Cabannes)))
    L0, L = rt.construct_layer_inputs(m), rt.construct_layer_inputs(same)
    assert np.array_equal(L.τ, L0.τ) and np.array_equal(L.ϖ, L0.ϖ) and np.array_equal(L.τ_sum, L0.τ_sum)
    assert np.array_equal(L.ndoubl, L0.ndoubl) and np.array_equal(L.iface, L0.iface)
    for b, sl in enumerate(same.bands.slices()):
        assert np.array_equal(L.zw[0, sl], L0.zw[0, sl])
        assert np.array_equal(L.zw[1 + 2 * b:3 + 2 * b, sl], L0.zw[1:, sl])
    Zpp0, _ = rt.z_bases(m)
    Zpp, _ = rt.z_bases(same)
    assert all(np.array_equal(Zpp[:, 1 + 2 * b:3 + 2 * b], Zpp0[:, 1:]) for b in range(3))


def test_bands_are_validated():
    m = bc.unbanded(78, 2)
    good = dict(band_start=np.array([0, 5, 78]), τ_aer=np.array([m.τ_aer] * 2), aerosol_optics=[list(m.aerosol_optics)] * 2, ϖ_Cabannes=np.ones(2))
    rt.with_bands(m, rt.Bands(**good))
    for bad in (dict(band_start=np.array([1, 5, 78])), dict(band_start=np.array([0, 5, 77])), dict(band_start=np.array([0, 5, 5, 78])),
                dict(τ_aer=m.τ_aer), dict(ϖ_Cabannes=np.ones(3)), dict(aerosol_optics=[list(m.aerosol_optics), []])):
        with pytest.raises(ValueError):
            rt.with_bands(m, rt.Bands(**{**good, **bad}))
    with pytest.raises(ValueError):
        rt.model_from_parameters(m.params, m.τ_rayl, m.τ_abs, m.τ_aer, m.aerosol_optics, bands=rt.Bands(**good))
    mb = rt.model_from_parameters(m.params, m.τ_rayl, m.τ_abs, bands=rt.Bands(**good))
    assert mb.bands.nBand == 2 and mb.bands.nAer == 2 and rt.prepare_scene(mb).K == 5


def test_band_aerosol_optics_partials_follow_the_values(monkeypatch):
    """band_aerosol_optics(autodiff=True) with the device call replaced by a family of raw optics that is linear in one parameter θ:
    the partials it returns (truncated optics per band, τ_aer through k_b and k_ref) against central differences of its value form"""
    sc = rtamd.scattering
    hg = rtamd.scenes.hg_like_greek
    raw0 = [rt.AerosolOptics(hg(g, 12), ω̃, 0.0, k) for g, ω̃, k in ((0.7, 0.95, 2.0), (0.6, 0.9, 1.4), (0.65, 0.93, 3.0))]
    draw = [rt.AerosolOptics(hg(g, 12), ω̃, 0.0, k) for g, ω̃, k in ((0.5, 0.02, 0.3), (0.4, -0.01, 0.2), (0.45, 0.01, -0.5))]
    six = lambda g: (g.α, g.β, g.γ, g.δ, g.ϵ, g.ζ)
    at = lambda θ: [rt.AerosolOptics(rt.GreekCoefs(*[x + θ * dx for x, dx in zip(six(a.greek_coefs), six(d.greek_coefs))]), a.ω̃ + θ * d.ω̃, 0.0,
                                     a.k + θ * d.k) for a, d in zip(raw0, draw)]
    θ = [0.0]

    def fake(model, λ, nᵣ=None, nᵢ=None, autodiff=False, wrt=()):
        assert len(λ) == 3 and len(nᵣ) == 3
        return (at(θ[0]), [[d] for d in draw]) if autodiff else at(θ[0])

    monkeypatch.setattr(sc, "compute_spectral_aerosol_optical_properties", fake)
    mie = sc.MieModel(None, sc.Aerosol(None, 1.3, 0.001), 0.55, None, sc.δBGE(5, 2.0), 1.0, 37)
    profile, τ_ref, h = np.array([0.2, 0.3, 0.5]), 0.4, 1e-6
    optics, τ_aer, d_optics, dτ_aer = sc.band_aerosol_optics(mie, [0.76, 1.6], 0.55, τ_ref, profile, autodiff=True, wrt=("θ",))
    assert np.array_equal(τ_aer, np.array([τ_ref * (o.k / 3.0) * profile for o in optics])) and dτ_aer.shape == (1, 2, 3)
    runs = []
    for s in (1, -1):
        θ[0] = s * h
        runs.append(sc.band_aerosol_optics(mie, [0.76, 1.6], 0.55, τ_ref, profile))
    fd = lambda f: (f(runs[0]) - f(runs[1])) / (2 * h)
    np.testing.assert_allclose(dτ_aer[0], fd(lambda r: r[1]), rtol=1e-8)
    for b in range(2):
        np.testing.assert_allclose(d_optics[b][0].greek_coefs.β, fd(lambda r: r[0][b].greek_coefs.β), rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(d_optics[b][0].fᵗ, fd(lambda r: r[0][b].fᵗ), rtol=1e-6, atol=1e-9)


def test_aerosol_optics_partial_places_a_band():
    """the glue from the Mie partials: a band's ∂(optics) lands in that band's entries and bases only"""
    model = bc.banded(78, 2)
    d = rt.AerosolOptics(rtamd.scenes.hg_like_greek(0.3, model.params.l_trunc), 0.01, -0.02)
    p = rtamd.scattering.aerosol_optics_partial(model, 1, d, band=2)
    assert p.dZpp.shape == rt.z_bases(model)[0].shape
    live = np.zeros(p.dZpp.shape[1], dtype=bool)
    live[1 + 1 + 2 * 2] = True
    assert np.abs(p.dZpp[:, live]).max() > 0 and not np.any(p.dZpp[:, ~live]) and not np.any(p.dZmp[:, ~live])
    assert p.dω̃[2, 1] == 0.01 and p.dfᵗ[2, 1] == -0.02 and np.count_nonzero(p.dω̃) == 1 and np.count_nonzero(p.dfᵗ) == 1
    with pytest.raises(ValueError):
        rtamd.scattering.aerosol_optics_partial(model, 1, d)
    with pytest.raises(ValueError):
        rtamd.scattering.aerosol_optics_partial(bc.unbanded(78, 2), 1, d, band=0)
