"""Test helper (not a test file): the band-resolved scenes, parameters and input conditions that test_oracle_bands.py and
test_gpu_bands.py share.  nStokes = 3, l_trunc 5 (N = 15), Nz = 3 unless stated otherwise."""
import dataclasses

import numpy as np

import optics_dual_cases as oc
import rtamd

rt = rtamd.corert
NZ = 3
# band edges inside a wavefront (5, 75; 130, 257) and one workgroup edge (256) inside a band
BAND_LENGTHS = {78: (5, 70, 3), 300: (130, 127, 43)}
# τ_aer of band b in layer z relative to the three-mode model's: the per-layer maximum of τ ϖ lies in band 0 for layer 0 and in band 2
# for the others, never in band 1 (whose aerosol the leakage tests change while ndoubl and the interface codes must stay)
τ_SCALE = np.array([[2.0, 0.6, 0.7], [0.3, 0.3, 0.3], [0.6, 3.0, 3.0]])


def band_start(S):
    return np.concatenate([[0], np.cumsum(BAND_LENGTHS[S])]).astype(np.int32)


def base_scene(S, nAer):
    m = rtamd.scenes.make_scene(3, 5, NZ, S, vza=(0.0, 60.0), vaz=(0.0, 45.0), absorption=True, aerosol_total=0.2 if nAer else 0.0, seed=11)
    assert len(m.quad_points.qp_μN) == 15
    return m


def unbanded(S, nAer):
    """the model the band-resolved ones start from: nAer = 2 is optics_dual_cases.three_mode_model"""
    base = base_scene(S, nAer)
    if nAer == 2:
        return oc.three_mode_model(base, seed=4)
    # as there: every ingredient of a layer within two orders of magnitude of the others, so that no column of partials is rounding noise
    rng = np.random.default_rng(5)
    τ_abs = rng.uniform(0.01, 1.0, base.τ_abs.shape)
    τ_rayl = base.τ_rayl * (rng.uniform(0.05, 0.3, NZ) / base.τ_rayl.mean(axis=0))[None, :]
    return dataclasses.replace(base, τ_rayl=τ_rayl, τ_abs=τ_abs, τ_aer=rng.uniform(0.02, 0.2, (nAer, NZ)))


def banded(S, nAer):
    """Three bands on S points.  nAer = 2: band 0 keeps the three-mode model's aerosols; bands 1 and 2 have their own Greek sets, ω̃,
    fᵗ ≠ 0 and τ_aer; in band 1 the second type has τ_aer = 0 in layer 0 (mode 2 there, mode 1 in the other bands); in band 2 τ_rayl ≡ 0
    in layer 2 (mode 0 there, in that band only).  ϖ_Cabannes differs per band."""
    m = unbanded(S, nAer)
    bs = band_start(S)
    l_trunc = m.params.l_trunc
    hg = lambda g: rtamd.scenes.hg_like_greek(g, l_trunc)
    ϖ_Cab = np.array([1.0, 0.97, 0.94])
    if nAer < 2:   # the Rayleigh depth takes the scaling too (as it falls from band to band in a real scene)
        τ_rayl = m.τ_rayl.copy()
        for b in range(3):
            τ_rayl[bs[b]:bs[b + 1]] *= τ_SCALE[b][None, :]
        m = dataclasses.replace(m, τ_rayl=τ_rayl)
    if nAer == 0:
        return rt.with_bands(m, rt.Bands(bs, np.zeros((3, 0, NZ)), [[], [], []], ϖ_Cab))
    if nAer == 1:
        optics = [[m.aerosol_optics[0]], [rt.AerosolOptics(hg(0.6), 0.85, 0.15)], [rt.AerosolOptics(hg(0.5), 0.9, 0.25)]]
        τ_aer = τ_SCALE[:, None, :] * m.τ_aer[None]
        return rt.with_bands(m, rt.Bands(bs, τ_aer, optics, ϖ_Cab))
    optics = [list(m.aerosol_optics),
              [rt.AerosolOptics(hg(0.6), 0.85, 0.15), rt.AerosolOptics(hg(0.75), 0.9, 0.0)],
              [rt.AerosolOptics(hg(0.5), 0.0, 0.1), rt.AerosolOptics(hg(0.65), 0.97, 0.25)]]
    τ_aer = τ_SCALE[:, None, :] * m.τ_aer[None]
    τ_aer[1, 1, 0] = 0.0
    τ_rayl = m.τ_rayl.copy()
    τ_rayl[bs[2]:bs[3], 2] = 0.0
    return rt.with_bands(dataclasses.replace(m, τ_rayl=τ_rayl), rt.Bands(bs, τ_aer, optics, ϖ_Cab))


def other_band_1(model):
    """`model` with another aerosol in band 1 only: other Greek sets, lower ω̃, 0.7 τ_aer.  Band 1 scatters less than before, so the
    per-layer maxima of τ ϖ (bands 0 and 2) and with them ndoubl and the interface codes stay."""
    bd = model.bands
    hg = lambda g: rtamd.scenes.hg_like_greek(g, model.params.l_trunc)
    optics = [list(band) for band in bd.aerosol_optics]
    optics[1] = [rt.AerosolOptics(hg(0.45 + 0.1 * x), 0.8 * a.ω̃, a.fᵗ) for x, a in enumerate(optics[1])]
    τ_aer = bd.τ_aer.copy()
    τ_aer[1] *= 0.7
    return rt.with_bands(model, rt.Bands(bd.band_start, τ_aer, optics, bd.ϖ_Cabannes))


def band_modes(model):
    """[nBand, nAer, Nz]: the case of the `+` each (band, type, layer) takes, by optics_dual_cases.modes on the band alone"""
    bd = model.bands
    return np.array([oc.modes(dataclasses.replace(model, τ_rayl=model.τ_rayl[sl], τ_abs=model.τ_abs[sl], τ_aer=bd.τ_aer[b],
                                                  aerosol_optics=bd.aerosol_optics[b], ϖ_Cabannes=bd.ϖ_Cabannes[b], bands=None))
                     for b, sl in enumerate(bd.slices())])


def assert_input_conditions(model, S, nAer):
    """what the issue asks of the inputs, asserted on the inputs"""
    bd = model.bands
    assert tuple(np.diff(bd.band_start)) == BAND_LENGTHS[S] and bd.band_start[-1] == S == model.τ_rayl.shape[0]
    inner = bd.band_start[1:-1]
    assert np.all(inner % 64 != 0), "band edges fall inside a wavefront"
    if S > 256:
        assert np.all(inner != 256) and inner[0] < 256 < inner[1], "one workgroup edge falls inside a band"
    assert bd.nAer == nAer and bd.nBand == 3
    L = rt.construct_layer_inputs(model)
    band_of_max = bd.band_of()[np.argmax(L.τ * L.ϖ, axis=0)]
    assert np.any(band_of_max == 0) and np.any(band_of_max > 0) and not np.any(band_of_max == 1), band_of_max
    if nAer == 0:
        return
    assert any(a.fᵗ != 0.0 for band in bd.aerosol_optics for a in band)
    if nAer == 2:
        md = band_modes(model)
        assert set(np.unique(md)) == {0, 1, 2}
        assert np.any(np.any(md != md[0:1], axis=0)), "a (type, layer) whose mode differs between bands"
        assert md[1, 1, 0] == 2 and md[0, 1, 0] == 1 and np.all(md[2, :, 2] == 0) and np.all(md[:2, 1, 2] == 1)


def parameters(model, P, seed=1):
    """P ∈ {1, 5} OpticsPartials with the band axis: w_gas, w_rayl, dτ_aer, dω̃ + dfᵗ and all of them at once (P = 1: that one).  Weights
    are O(1) and every absolute partial is O(its value); dω̃ of a type with ω̃ = 0 stays 0 (optics_dual_cases.six_parameters)."""
    rng = np.random.default_rng(seed)
    bd = model.bands
    u = lambda: rng.uniform(0.5, 1.5, NZ)
    ps = [rt.OpticsPartial(w_gas=u()), rt.OpticsPartial(w_rayl=u())]
    if bd.nAer:
        ps.append(rt.OpticsPartial(dτ_aer=bd.τ_aer * rng.uniform(0.5, 1.5, bd.τ_aer.shape)))
        ω̃ = np.array([[a.ω̃ for a in band] for band in bd.aerosol_optics])
        ps.append(rt.OpticsPartial(dω̃=-0.5 * ω̃, dfᵗ=rng.uniform(0.1, 0.3, ω̃.shape)))
    else:
        ps += [rt.OpticsPartial(w_gas=u(), w_rayl=u()), rt.OpticsPartial(w_gas=u())]
    ps.append(oc.combined(ps))
    assert len(ps) == 5
    return ps[-1:] if P == 1 else ps


def band_only(model, b, dτ_aer=False, dω̃=False, dZ=False):
    """one OpticsPartial that names only band b's aerosol: a scaling of its τ_aer, its ω̃, and / or its first type's basis itself"""
    bd = model.bands
    p = rt.OpticsPartial()
    if dτ_aer:
        p.dτ_aer = np.zeros_like(bd.τ_aer)
        p.dτ_aer[b] = bd.τ_aer[b]
    if dω̃:
        p.dω̃ = np.zeros((bd.nBand, bd.nAer))
        p.dω̃[b] = [-0.5 * a.ω̃ for a in bd.aerosol_optics[b]]
    if dZ:
        Zpp, Zmp = rt.z_bases(model)
        p.dZpp, p.dZmp = np.zeros_like(Zpp), np.zeros_like(Zmp)
        k = slice(1 + bd.nAer * b, 1 + bd.nAer * (b + 1))
        p.dZpp[:, k], p.dZmp[:, k] = 0.3 * Zpp[:, k], 0.3 * Zmp[:, k]
    return p
