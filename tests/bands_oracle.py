"""Test helper (not a test file): the oracle of band-resolved scenes.  constructCoreOpticalProperties restated literally for
models with per-band aerosols -- the loop over iBand of compEffectiveLayerProperties.jl:24-75 with createAero (:80-85), the `+` of
types.jl:632-678 on MATERIALISED phase matrices Z[S_b, N, N] (no basis weights anywhere) and the concatenation `*` of
types.jl:664-669 -- and its layers fed to the loop of oracle/momref.py (rt_kernel, create_surface_layer, interaction,
postprocessing_vza).  Complex inputs pass through the optics (complex step); the two all(. == 0) tests are then taken on the real
parts, as ForwardDiff takes them on the values."""
from dataclasses import dataclass
from typing import List

import numpy as np

import helpers
from oracle import momref as mr

H = 1e-20   # complex step: far below rounding, so Im / H is the exact forward-mode derivative of the statements


@dataclass
class Layer:
    """CoreScatteringOpticalProperties (types.jl:605-614) of one layer on the concatenated axis, Z materialised"""
    tau: np.ndarray     # [S]
    varpi: np.ndarray   # [S]
    Zpp: np.ndarray     # [S, N, N]
    Zmp: np.ndarray

    def Zfull(self):    # what momref.rt_kernel asks of a layer
        return self.Zpp, self.Zmp


@dataclass
class BandScene:
    base: mr.Scene                          # streams, Rayleigh, gas, surface, views: everything that has no band axis
    band_start: np.ndarray                  # [nBand + 1]
    tau_aer: np.ndarray                     # [nBand, nAer, Nz]
    aerosols: List[List[mr.AerosolOptics]]  # [nBand][nAer]
    varpi_cabannes: np.ndarray              # [nBand]


def band_scene(model) -> BandScene:
    bd = model.bands
    conv = lambda a: mr.AerosolOptics(mr.GreekCoefs(a.greek_coefs.α, a.greek_coefs.β, a.greek_coefs.γ, a.greek_coefs.δ, a.greek_coefs.ϵ,
                                                    a.greek_coefs.ζ), a.ω̃, a.fᵗ)
    return BandScene(helpers.oracle_scene(model), np.asarray(bd.band_start), np.asarray(bd.τ_aer),
                     [[conv(a) for a in band] for band in bd.aerosol_optics], np.asarray(bd.ϖ_Cabannes))


def _zero(x):
    return bool(np.all(np.real(x) == 0.0))


def _plus(x, y):
    """Base.:+(x::CoreScatteringOpticalProperties, y::CoreScatteringOpticalProperties), types.jl:632-661; x, y = (τ, ϖ, Z⁺⁺, Z⁻⁺)
    with τ, ϖ [S_b] or scalars and Z [N, N] (spectrally flat) or [S_b, N, N]"""
    xτ, xϖ, xZpp, xZmp = x
    yτ, yϖ, yZpp, yZmp = y
    τ = xτ + yτ
    wx = xτ * xϖ
    wy = yτ * yϖ
    w = wx + wy
    ϖ = w / τ
    if _zero(wx):
        return τ, ϖ, yZpp, yZmp
    if _zero(wy):
        return τ, ϖ, xZpp, xZmp
    wy = wy / w
    wx = wx / w
    wx = np.reshape(wx, (-1, 1, 1))
    wy = np.reshape(wy, (-1, 1, 1))
    return τ, ϖ, wx * xZpp + wy * yZpp, wx * xZmp + wy * yZmp


def _plus_abs(x, τ_abs):
    """Base.:+(x::CoreScatteringOpticalProperties, y::CoreAbsorptionOpticalProperties), types.jl:672-678"""
    xτ, xϖ, xZpp, xZmp = x
    τ = xτ + τ_abs
    wx = xτ * xϖ
    return τ, wx / τ, xZpp, xZmp


def _create_aero(τ_aer, a: mr.AerosolOptics, Zpp, Zmp):
    """createAero, compEffectiveLayerProperties.jl:80-85"""
    τ_mod = (1 - a.ft * a.omega) * τ_aer
    ϖ_mod = (1 - a.ft) * a.omega / (1 - a.ft * a.omega)
    return τ_mod, ϖ_mod, Zpp, Zmp


def construct_core_optical_properties(bs: BandScene, m: int, tau_rayl=None, tau_abs=None) -> List[Layer]:
    """constructCoreOpticalProperties(RS_type, iBand = 1:nBand, m, model): per band Rayleigh `+` each aerosol type `+` the gas, then
    per layer the product `*` over the bands.  tau_rayl / tau_abs override the base scene's (complex step)."""
    sc = bs.base
    τ_rayl = sc.tau_rayl if tau_rayl is None else tau_rayl
    τ_abs = sc.tau_abs if tau_abs is None else tau_abs
    nS, μ = sc.pol.n, sc.quad.qp_mu
    S, Nz = τ_rayl.shape
    N = nS * len(μ)
    RaylZpp, RaylZmp = mr.compute_Z_moments(nS, μ, sc.greek_rayleigh, m)
    band_layer_props = []
    for iB in range(len(bs.band_start) - 1):
        sl = slice(int(bs.band_start[iB]), int(bs.band_start[iB + 1]))
        combo = [(τ_rayl[sl, i], bs.varpi_cabannes[iB], RaylZpp, RaylZmp) for i in range(Nz)]
        for ia, a in enumerate(bs.aerosols[iB]):
            AerZpp, AerZmp = mr.compute_Z_moments(nS, μ, a.greek, m)
            aer = [_create_aero(bs.tau_aer[iB][ia, i], a, AerZpp, AerZmp) for i in range(Nz)]
            combo = [_plus(c, y) for c, y in zip(combo, aer)]
        band_layer_props.append([_plus_abs(c, τ_abs[sl, i]) for i, c in enumerate(combo)])
    layers = []
    for iz in range(Nz):
        parts = []
        for iB, props in enumerate(band_layer_props):   # expandOpticalProperties + cat(dims = 3), types.jl:664-669
            n = int(bs.band_start[iB + 1] - bs.band_start[iB])
            τ, ϖ, Zpp, Zmp = props[iz]
            full = lambda Z: np.broadcast_to(Z, (n, N, N))
            parts.append((np.broadcast_to(τ, (n,)), np.broadcast_to(ϖ, (n,)), full(Zpp), full(Zmp)))
        layers.append(Layer(*[np.concatenate([p[k] for p in parts]) for k in range(4)]))
    return layers


def layer_summary(bs: BandScene):
    """τ, ϖ [S, Nz], ndoubl, iface [Nz], τ_sum [S, Nz + 1] as rt_run derives them from the layers (extractEffectiveProps,
    get_dtau_ndoubl over the concatenated axis)"""
    layers = construct_core_optical_properties(bs, 0)
    ifaces, τ_sum = mr.extract_effective_props(layers)
    nd = [mr.get_dtau_ndoubl(l.tau, l.varpi, bs.base.quad.qp_mu)[1] for l in layers]
    return (np.array([l.tau for l in layers]).T, np.array([l.varpi for l in layers]).T, np.array(nd, dtype=np.int32),
            np.array(ifaces, dtype=np.int32), τ_sum)


def rt_run(bs: BandScene):
    """momref.rt_run (rt_run.jl:41-230) on the band-resolved layers: (R_SFI, T_SFI) [nVza, nStokes, S]"""
    sc = bs.base
    pol, quad = sc.pol, sc.quad
    S, Nz, N = sc.S, sc.Nz, sc.N
    nV = len(sc.vza)
    R_SFI, T_SFI = np.zeros((nV, pol.n, S)), np.zeros((nV, pol.n, S))
    added, surf, comp = mr.make_added_layer(N, S), mr.make_added_layer(N, S), mr.make_composite_layer(N, S)
    sinp = mr.surface_inputs(sc)
    for m in range(sc.max_m):
        weight = 0.5 if m == 0 else 1.0
        layers = construct_core_optical_properties(bs, m)
        ifaces, τ_sum_all = mr.extract_effective_props(layers)
        for iz in range(Nz):
            mr.rt_kernel(pol, quad, added, comp, layers[iz], ifaces[iz], τ_sum_all[:, iz], m, iz + 1, sc.strict_reference_indexing)
        mr.create_surface_layer(sc, sinp, surf, m, τ_sum_all[:, -1])
        mr.interaction(ifaces[-1], comp, surf)
        mr.postprocessing_vza(pol, comp, sc.vza, quad.qp_mu, m, sc.vaz, weight, R_SFI, T_SFI)
    return R_SFI, T_SFI


def complex_step(bs: BandScene, partial, m: int = 0):
    """The partials of τ, ϖ [S, Nz] and of the materialised Z⁺⁺, Z⁻⁺ [S, N, N, Nz] of Fourier moment m with respect to ONE parameter
    (a corert.OpticsPartial with the band axis, without w_p / w_T and without dZpp / dZmp: the ingredients' partials only)."""
    sc = bs.base
    Nz = sc.Nz
    nBand, nAer = bs.tau_aer.shape[:2]
    get = lambda x, shape: np.zeros(shape) if x is None else np.asarray(x, dtype=np.float64).reshape(shape)
    w_rayl, w_gas = get(partial.w_rayl, (Nz,)), get(partial.w_gas, (Nz,))
    dτ_aer, dω̃, dfᵗ = get(partial.dτ_aer, (nBand, nAer, Nz)), get(partial.dω̃, (nBand, nAer)), get(partial.dfᵗ, (nBand, nAer))
    moved = BandScene(sc, bs.band_start, bs.tau_aer + 1j * H * dτ_aer,
                      [[mr.AerosolOptics(a.greek, a.omega + 1j * H * dω̃[b, x], a.ft + 1j * H * dfᵗ[b, x]) for x, a in enumerate(band)]
                       for b, band in enumerate(bs.aerosols)], bs.varpi_cabannes)
    layers = construct_core_optical_properties(moved, m, sc.tau_rayl * (1 + 1j * H * w_rayl)[None, :], sc.tau_abs * (1 + 1j * H * w_gas)[None, :])
    im = lambda xs: np.stack([np.imag(x) / H for x in xs], axis=-1)
    return im([l.tau for l in layers]), im([l.varpi for l in layers]), im([l.Zpp for l in layers]), im([l.Zmp for l in layers])
