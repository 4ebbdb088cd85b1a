"""Mie aerosol optics (src/Scattering): make_mie_model(NAI2() or PCW(), ...), compute_aerosol_optical_properties,
compute_ref_aerosol_extinction, compute_wigner_values and truncate_phase(δBGE, ...).

The sums over radii, orders and angles run on the device (mom_mie_nai2, csrc/mom_mie.hip); the host builds what they read --
the radius quadrature, the Gauss nodes of the scattering angle, the π/τ and P/P²/R²/T² tables (O(n_μ²) recurrences, vectorised
over μ) -- and does the arithmetic that follows the sums: the division by the bulk C_sca and, for autodiff=True, the quotient
rule of the partial rows.  Partials with respect to the refractive index (nᵣ, nᵢ) come from the Dual run of the same kernels
(mom_mie_nai2_dual); truncate_phase and aerosol_optics_partial carry them on to rt_run_dual_device_optics.
compute_spectral_aerosol_optical_properties runs a whole array of wavelengths in one device call (mom_mie_nai2_spectral) on one
angle grid, whose tables the device builds itself (mom_mie_tables): there the host brings the nodes only.
A PCW() model takes the Domke-PCW route (mom_mie_pcw, csrc/mom_pcw.hip): the Greek coefficients expanded directly in the Mie
coefficients with Wigner 3j symbols, no angle quadrature -- the independent check of NAI-2.  The device produces the symbols in
registers, so the model's wigner_A / wigner_B are accepted and not needed; compute_wigner_values returns the reference's two tables
for whoever wants them (mom_wigner_tables).  The host brings the radii and w_x and divides by C_sca.  aerosol_optics_jacobian
returns the optics with their partials in (r_m, σ_g, nᵣ, nᵢ) on the model's own route: for PCW() one mom_mie_pcw_dual call.
Float64 only.  There is no CPU fallback.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from . import corert as rt


# ------------------------------------------------------------------------------------------
# types (src/Scattering/types.jl)
# ------------------------------------------------------------------------------------------


@dataclass
class LogNormal:
    """Distributions.LogNormal(μ, σ): ln r ~ Normal(μ, σ).  The reference builds it as LogNormal(log(r_m), log(σ_g))."""
    μ: float
    σ: float

    def pdf(self, r: np.ndarray) -> np.ndarray:
        r = np.asarray(r, dtype=np.float64)
        z = (np.log(r) - self.μ) / self.σ
        return np.exp(-0.5 * z * z) / (r * self.σ * math.sqrt(2.0 * math.pi))

    def dpdf(self, r: np.ndarray) -> np.ndarray:
        """∂pdf/∂(r_m, σ_g) [2, len(r)] for r_m = exp(μ), σ_g = exp(σ)."""
        r = np.asarray(r, dtype=np.float64)
        d = np.log(r) - self.μ
        p = self.pdf(r)
        dμ = p * d / self.σ ** 2
        dσ = p * (d * d / self.σ ** 3 - 1.0 / self.σ)
        return np.stack([dμ / math.exp(self.μ), dσ / math.exp(self.σ)])


@dataclass
class Aerosol:
    size_distribution: LogNormal
    nᵣ: float
    nᵢ: float


@dataclass
class NAI2:
    """Siewert's numerical angular integration (the default; the route that carries partials and wavelength batches)."""


@dataclass
class PCW:
    """Domke's expansion in Wigner 3j symbols (Sanghavi 2014, eq. 22-24); partials through aerosol_optics_jacobian."""


@dataclass
class δBGE:
    l_max: int
    Δ_angle: float = 0.0


@dataclass
class MieModel:
    computation_type: object      # NAI2 or PCW
    aerosol: Aerosol
    λ: float
    polarization_type: object
    truncation_type: Optional[δBGE]
    r_max: float
    nquad_radius: int
    wigner_A: Optional[np.ndarray] = None    # the reference's PCW models carry their tables; the device needs none
    wigner_B: Optional[np.ndarray] = None


def make_mie_model(computation_type, aerosol: Aerosol, λ: float, polarization_type, truncation_type, r_max: float,
                   nquad_radius: int, wigner_A=None, wigner_B=None) -> MieModel:
    """make_mie_model.jl: NAI2() takes the seven arguments; PCW() also takes the reference's wigner_A, wigner_B, which are kept on
    the model and not read (mom_mie_pcw produces the symbols itself)."""
    if not isinstance(computation_type, (NAI2, PCW)):
        raise NotImplementedError(f"computation type {computation_type!r}: NAI2() and PCW() are built")
    if isinstance(computation_type, NAI2) and (wigner_A is not None or wigner_B is not None):
        raise ValueError("wigner_A and wigner_B belong to a PCW() model")
    if aerosol.nᵢ < 0:
        raise ValueError("the imaginary part of the refractive index must be >= 0")
    return MieModel(computation_type, aerosol, float(λ), polarization_type, truncation_type, float(r_max), int(nquad_radius),
                    wigner_A, wigner_B)


# ------------------------------------------------------------------------------------------
# quadratures and tables
# ------------------------------------------------------------------------------------------


def gausslegendre(n: int):
    """Gauss-Legendre nodes (ascending) and weights on [-1, 1]: Newton's method on P_n, all nodes at once."""
    if n == 1:
        return np.zeros(1), np.full(1, 2.0)

    def p_and_dp(x):
        p0, p1 = np.ones_like(x), x.copy()
        for l in range(2, n + 1):
            p0, p1 = p1, ((2 * l - 1) * x * p1 - (l - 1) * p0) / l
        return p1, n * (x * p1 - p0) / (x * x - 1.0)

    x = np.cos(math.pi * (np.arange(n, 0, -1, dtype=np.float64) - 0.25) / (n + 0.5))
    for _ in range(20):
        p, dp = p_and_dp(x)
        x = x - p / dp
        if np.max(np.abs(p / dp)) < 4e-16:
            break
    x = 0.5 * (x - x[::-1])   # the nodes are symmetric: make them so to the last bit
    _, dp = p_and_dp(x)
    return x, 2.0 / ((1.0 - x * x) * dp * dp)


def gauleg(n: int, xmin: float, xmax: float, norm: bool = False):
    """mie_helper_functions.jl:177-182"""
    ξ, w = gausslegendre(n)
    ξ = (xmax - xmin) / 2 * ξ + (xmin + xmax) / 2
    w = w / w.sum() if norm else w * (xmax - xmin) / 2
    return ξ, w


def get_n_max(x):
    """mie_helper_functions.jl:17 (round: ties to even, as Julia's)"""
    x = np.asarray(x, dtype=np.float64)
    return np.rint(x + 4.05 * x ** (1 / 3) + 10).astype(np.int64)


def compute_mie_π_τ(μ: np.ndarray, nmax: int):
    """legendre_functions.jl:188-208 -> π, τ [n_μ, nmax] (column l - 1 = order l)"""
    μ = np.asarray(μ, dtype=np.float64)
    π_, τ_ = np.zeros((μ.size, nmax)), np.zeros((μ.size, nmax))
    π_[:, 0], τ_[:, 0] = 1.0, μ
    if nmax > 1:
        π_[:, 1], τ_[:, 1] = 3 * μ, 6 * μ ** 2 - 3
    for n in range(2, nmax):
        π_[:, n] = ((2 * n + 1) * μ * π_[:, n - 1] - (n + 1) * π_[:, n - 2]) / n
        τ_[:, n] = (n + 1) * μ * π_[:, n] - (n + 2) * π_[:, n - 1]
    return π_, τ_


def compute_legendre_poly(x: np.ndarray, nmax: int):
    """legendre_functions.jl:217-259 -> P, P², R², T² [len(x), nmax] (column l = degree l)"""
    x = np.asarray(x, dtype=np.float64)
    P, P2, R2, T2 = (np.zeros((x.size, nmax)) for _ in range(4))
    P[:, 0] = 1.0
    if nmax > 1:
        P[:, 1] = x
    if nmax > 2:
        P2[:, 2] = 3 * (1 - x ** 2)
        R2[:, 2] = math.sqrt(1.5) * (1 + x ** 2)
        T2[:, 2] = math.sqrt(6) * x
    for c in range(2, nmax):
        l = c - 1
        P[:, c] = ((2 * l + 1) * x * P[:, c - 1] - l * P[:, c - 2]) / (l + 1)
        if l >= 2:
            ia = (2 * l + 1) * x
            ib = math.sqrt((l + 2) * (l - 2)) * (l + 2) / l
            ic = 4.0 * (2 * l + 1) / ((l + 1) * l)
            id_ = math.sqrt((l + 3) * (l - 1)) * (l - 1) / (l + 1)
            P2[:, c] = (ia * P2[:, c - 1] - (l + 2) * P2[:, c - 2]) / (l - 1)
            R2[:, c] = (ia * R2[:, c - 1] - ib * R2[:, c - 2] - ic * T2[:, c - 1]) / id_
            T2[:, c] = (ia * T2[:, c - 1] - ib * T2[:, c - 2] - ic * R2[:, c - 1]) / id_
    return P, P2, R2, T2


# ------------------------------------------------------------------------------------------
# compute_aerosol_optical_properties (compute_NAI2.jl:16-182)
# ------------------------------------------------------------------------------------------


@dataclass
class MieInputs:
    """What mom_mie_nai2 reads for a model: everything the host prepares."""
    r: np.ndarray
    w: np.ndarray         # [nW, nR]: row 0 = 4π r² wₓ, rows 1, 2 = 4π r² ∂wₓ/∂(r_m, σ_g)
    μ: np.ndarray
    w_μ: np.ndarray
    π_: np.ndarray
    τ_: np.ndarray
    P: np.ndarray
    P2: np.ndarray
    R2: np.ndarray
    T2: np.ndarray


def _radii_and_wx_rows(model: MieModel, autodiff: bool):
    """(r, rows [nW, nR]) of the model: the radius quadrature, wₓ and (autodiff) ∂wₓ/∂(r_m, σ_g)"""
    aer = model.aerosol
    r, wᵣ = gauleg(model.nquad_radius, 0.0, model.r_max, norm=True)
    # compute_wₓ (mie_helper_functions.jl:266-276): wₓ = pdf wᵣ / Σ pdf wᵣ
    p = aer.size_distribution.pdf(r) * wᵣ
    rows = [p / p.sum()]
    if autodiff:
        for dp in aer.size_distribution.dpdf(r) * wᵣ:
            rows.append(dp / p.sum() - p * dp.sum() / p.sum() ** 2)
    return r, np.stack(rows)


def _radii_and_weight_rows(model: MieModel, autodiff: bool):
    """(r, w [nW, nR]) of the model: the radius quadrature and 4π r² times wₓ (and, autodiff, its partials)"""
    r, rows = _radii_and_wx_rows(model, autodiff)
    return r, 4 * math.pi * r ** 2 * rows


def mie_inputs(model: MieModel, autodiff: bool = False) -> MieInputs:
    r, w = _radii_and_weight_rows(model, autodiff)
    n_max = int(get_n_max(np.max(2 * math.pi / model.λ * r)))
    μ, w_μ = gausslegendre(2 * n_max - 1)
    π_, τ_ = compute_mie_π_τ(μ, n_max)
    P, P2, R2, T2 = compute_legendre_poly(μ, μ.size)
    return MieInputs(r, w, μ, w_μ, π_, τ_, P, P2, R2, T2)


ALL_AEROSOL_PARAMETERS = ("r_m", "σ_g", "nᵣ", "nᵢ")    # the reference's x (phase_function_autodiff.jl:48)
_SIZE_PARAMETERS, _INDEX_PARAMETERS = ALL_AEROSOL_PARAMETERS[:2], ALL_AEROSOL_PARAMETERS[2:]


def _device_call(model: MieModel, autodiff: bool, flags: int = 0, dual: bool = False):
    """mom_mie_nai2 on the model's inputs, or (dual) mom_mie_nai2_dual: two more output rows, ∂/∂nᵣ and ∂/∂nᵢ of row 0's sums"""
    inp = mie_inputs(model, autodiff)
    call = _lib.mie_nai2_dual if dual else _lib.mie_nai2
    return inp, call(inp.r, inp.w, model.λ, model.aerosol.nᵣ, model.aerosol.nᵢ, inp.w_μ, inp.π_, inp.τ_, inp.P, inp.P2, inp.R2, inp.T2,
                     flags=flags)


def _greek(g: np.ndarray) -> rt.GreekCoefs:
    return rt.GreekCoefs(α=g[0].copy(), β=g[1].copy(), γ=g[2].copy(), δ=g[3].copy(), ϵ=g[4].copy(), ζ=g[5].copy())


def optics_from_sums(C: np.ndarray, greek: np.ndarray):
    """The host arithmetic after the device sums: (AerosolOptics, [∂/∂θ of it for every further row]).  C [nW, 2] =
    bulk (C_sca, C_ext), greek [nW, 6, l_max] unnormalised.  A further row holds the partial of row 0's sums with respect to one
    parameter, whichever it is: a weight row of ∂wₓ/∂θ, or an index row of mom_mie_nai2_dual."""
    Cs, Ce = C[0]
    aero = rt.AerosolOptics(greek_coefs=_greek(greek[0] / Cs), ω̃=float(Cs / Ce), fᵗ=1.0, k=float(Ce))
    partials = []
    for k in range(1, C.shape[0]):
        dCs, dCe = C[k]
        dg = greek[k] / Cs - greek[0] * dCs / Cs ** 2
        partials.append(rt.AerosolOptics(greek_coefs=_greek(dg), ω̃=float(dCs / Ce - Cs * dCe / Ce ** 2), fᵗ=0.0, k=float(dCe)))
    return aero, partials


def compute_wigner_values(m_max: int, n_max: Optional[int] = None, l_max: Optional[int] = None):
    """compute_wigner_values(m_max, n_max, l_max) -> (wigner_A, wigner_B), indexed [m - 1, n - 1, l - 1]: the 3j symbols
    (m n l-1; -1 1 0) and (m n l-1; -1 -1 2), by the reference's recursions on the device (mom_wigner_tables).  The shorthand
    compute_wigner_values(N_max) is compute_wigner_values(2 N_max + 1, N_max + 1, 2 N_max + 1).  A table holds the symbols' values
    in every column, also where the column starts beyond m_max (the reference's memoised recursion leaves zeros there)."""
    if n_max is None and l_max is None:
        m_max, n_max, l_max = 2 * int(m_max) + 1, int(m_max) + 1, 2 * int(m_max) + 1
    elif n_max is None or l_max is None:
        raise TypeError("compute_wigner_values takes (N_max) or (m_max, n_max, l_max)")
    return _lib.wigner_tables(m_max, n_max, l_max)


def pcw_inputs(model: MieModel):
    """(r, wₓ, N_max) of a PCW model (compute_PCW.jl:30-36): N_max from r_max, not from the largest quadrature node"""
    r, wᵣ = gauleg(model.nquad_radius, 0.0, model.r_max, norm=True)
    p = model.aerosol.size_distribution.pdf(r) * wᵣ
    return r, p / p.sum(), int(get_n_max(2 * math.pi * model.r_max / model.λ))


def _pcw_optics(model: MieModel):
    """compute_PCW.jl:16-104: the device sums, then (1 / C_sca) times each of them"""
    r, wₓ, N_max = pcw_inputs(model)
    greek, C, _ = _lib.mie_pcw(r, wₓ, model.λ, model.aerosol.nᵣ, model.aerosol.nᵢ, N_max)
    Cs, Ce = C
    return rt.AerosolOptics(greek_coefs=_greek((1 / Cs) * greek), ω̃=float(Cs / Ce), fᵗ=1.0, k=float(Ce))


def _checked_wrt(wrt):
    wrt = tuple(wrt)
    unknown = [p for p in wrt if p not in ALL_AEROSOL_PARAMETERS]
    if unknown or len(set(wrt)) != len(wrt):
        raise ValueError(f"wrt must be distinct names out of {ALL_AEROSOL_PARAMETERS}, got {wrt}")
    return wrt


def pcw_jacobian_inputs(model: MieModel, wrt):
    """(r, w [nW, nR], N_max, index_rows, rows) of the mom_mie_pcw_dual call for `wrt`: the (r_m, σ_g) rows of wₓ only when `wrt` names
    one of them, the index rows only when it names nᵣ or nᵢ; rows: the parameter of each output row after row 0"""
    size_rows = any(p in _SIZE_PARAMETERS for p in wrt)
    index_rows = any(p in _INDEX_PARAMETERS for p in wrt)
    r, w = _radii_and_wx_rows(model, size_rows)
    rows = (_SIZE_PARAMETERS if size_rows else ()) + (_INDEX_PARAMETERS if index_rows else ())
    return r, w, int(get_n_max(2 * math.pi * model.r_max / model.λ)), index_rows, rows


def aerosol_optics_jacobian(model: MieModel, wrt=ALL_AEROSOL_PARAMETERS):
    """(optics, [∂optics/∂p for p in wrt]) on the model's own route, wrt a subset of ALL_AEROSOL_PARAMETERS = (r_m, σ_g, nᵣ, nᵢ): what
    the reference's compute_aerosol_optical_properties(model; autodiff=true) returns "using either computation type".  A NAI2()
    model: compute_aerosol_optical_properties(model, autodiff=True, wrt=wrt).  A PCW() model: ONE mom_mie_pcw_dual call -- the
    size-distribution partials are further weight rows, the index partials the Dual run -- and the host's quotient rule; the value
    is bitwise compute_aerosol_optical_properties(model).  The two routes share the radii and wₓ and nothing after them, so each
    checks the other's Jacobian."""
    wrt = _checked_wrt(wrt)
    if not isinstance(model.computation_type, PCW):
        return compute_aerosol_optical_properties(model, autodiff=True, wrt=wrt)
    r, w, N_max, index_rows, rows = pcw_jacobian_inputs(model, wrt)
    greek, C, _ = _lib.mie_pcw_dual(r, w, model.λ, model.aerosol.nᵣ, model.aerosol.nᵢ, N_max, index_rows=index_rows)
    Cs, Ce = C[0]
    aero = rt.AerosolOptics(greek_coefs=_greek((1 / Cs) * greek[0]), ω̃=float(Cs / Ce), fᵗ=1.0, k=float(Ce))
    partials = []
    for k in range(1, C.shape[0]):
        dCs, dCe = C[k]
        dg = (1 / Cs) * greek[k] - greek[0] * dCs / Cs ** 2
        partials.append(rt.AerosolOptics(greek_coefs=_greek(dg), ω̃=float(dCs / Ce - Cs * dCe / Ce ** 2), fᵗ=0.0, k=float(dCe)))
    return aero, [partials[rows.index(p)] for p in wrt]


def compute_aerosol_optical_properties(model: MieModel, autodiff: bool = False, wrt=_SIZE_PARAMETERS):
    """AerosolOptics(greek_coefs, ω̃, k, fᵗ = 1) of the model; with autodiff=True also the partials of every field with respect to
    the parameters named in `wrt`, a subset of ALL_AEROSOL_PARAMETERS = (r_m, σ_g, nᵣ, nᵢ): the median radius and geometric width
    of the log-normal size distribution and the real and imaginary part of the refractive index.  Returns
    (optics, [∂/∂p for p in wrt]), each partial an AerosolOptics holding the derivatives.  The size-distribution partials are
    further weight rows of the same sums (mom_mie_nai2); an index parameter takes the Dual run of the Mie coefficients
    (mom_mie_nai2_dual).  The default, (r_m, σ_g), is the call without `wrt`.
    The model's computation type chooses the route: NAI2() the sums over scattering angles, PCW() the expansion in Wigner 3j symbols
    (mom_mie_pcw), whose values this call returns; its partials are aerosol_optics_jacobian's (autodiff=True raises
    NotImplementedError here)."""
    if isinstance(model.computation_type, PCW):
        if autodiff:
            raise NotImplementedError("autodiff=True on a PCW() model: call aerosol_optics_jacobian(model, wrt), which takes either route")
        return _pcw_optics(model)
    if not autodiff:
        _, (_, C, greek, _) = _device_call(model, False)
        return optics_from_sums(C, greek)[0]
    wrt = _checked_wrt(wrt)
    if not any(p in _INDEX_PARAMETERS for p in wrt):
        _, (_, C, greek, _) = _device_call(model, True)
        rows = _SIZE_PARAMETERS
    else:
        size_rows = any(p in _SIZE_PARAMETERS for p in wrt)
        _, (_, C, greek, _) = _device_call(model, size_rows, dual=True)
        rows = (_SIZE_PARAMETERS if size_rows else ()) + _INDEX_PARAMETERS
    aero, partials = optics_from_sums(C, greek)
    return aero, [partials[rows.index(p)] for p in wrt]


@dataclass
class SpectralMieInputs:
    """What mom_mie_nai2_spectral reads for a model and a set of wavelengths: no tables, the device builds them from μ."""
    r: np.ndarray
    w: np.ndarray         # as MieInputs.w: it does not depend on λ
    μ: np.ndarray         # ONE grid for all wavelengths, sized for the shortest
    w_μ: np.ndarray
    n_max: np.ndarray     # [nL]: get_n_max at the largest radius, per wavelength
    n_top: int            # the largest of them: the row count of the π/τ tables
    l_max: int            # = n_μ


def spectral_mie_inputs(model: MieModel, λ, autodiff: bool = False) -> SpectralMieInputs:
    """r and w as mie_inputs(model) has them; the shared grid is gausslegendre(2 n_top - 1), n_top = get_n_max at the largest radius
    and the shortest wavelength (the grid the single call takes there); l_max = n_μ.  model.λ is not read."""
    λ = np.atleast_1d(np.asarray(λ, dtype=np.float64))
    if λ.size < 1 or not np.all(λ > 0):
        raise ValueError("λ must hold at least one positive wavelength")
    r, w = _radii_and_weight_rows(model, autodiff)
    n_max = np.array([int(get_n_max(np.max(2 * math.pi / l * r))) for l in λ])
    n_top = int(n_max.max())
    μ, w_μ = gausslegendre(2 * n_top - 1)
    return SpectralMieInputs(r, w, μ, w_μ, n_max, n_top, int(μ.size))


def compute_spectral_aerosol_optical_properties(model: MieModel, λ, nᵣ=None, nᵢ=None, autodiff: bool = False, wrt=_SIZE_PARAMETERS,
                                                max_batch: int = 0):
    """compute_aerosol_optical_properties at the wavelengths λ [nL] in ONE device call (mom_mie_nai2_spectral): a list of
    AerosolOptics, one per wavelength; with autodiff=True (list, [partials of wavelength j in the order of `wrt`]).  nᵣ, nᵢ [nL] are
    the refractive index per wavelength (default: the aerosol's constant index).  All wavelengths share the radii, the weight rows
    and ONE angle grid, that of the shortest wavelength (spectral_mie_inputs), whose tables the device builds; each wavelength's
    Greek coefficients are cut to the length 2 n_max(λ) - 1 the single call returns there -- what is cut off is rounding.  The Dual
    run is taken when `wrt` names an index parameter, as in compute_aerosol_optical_properties."""
    λ = np.atleast_1d(np.asarray(λ, dtype=np.float64))
    aer = model.aerosol
    nᵣ = np.full(λ.size, aer.nᵣ) if nᵣ is None else np.atleast_1d(np.asarray(nᵣ, dtype=np.float64))
    nᵢ = np.full(λ.size, aer.nᵢ) if nᵢ is None else np.atleast_1d(np.asarray(nᵢ, dtype=np.float64))
    if nᵣ.shape != λ.shape or nᵢ.shape != λ.shape:
        raise ValueError("λ, nᵣ and nᵢ must have the same length")
    if np.any(nᵢ < 0):
        raise ValueError("the imaginary part of the refractive index must be >= 0")
    rows, dual, size_rows = (), False, False
    if autodiff:
        wrt = _checked_wrt(wrt)
        dual = any(p in _INDEX_PARAMETERS for p in wrt)
        size_rows = not dual or any(p in _SIZE_PARAMETERS for p in wrt)
        rows = (_SIZE_PARAMETERS if size_rows else ()) + (_INDEX_PARAMETERS if dual else ())
    inp = spectral_mie_inputs(model, λ, size_rows)
    call = _lib.mie_nai2_spectral_dual if dual else _lib.mie_nai2_spectral
    _, C, greek, _ = call(inp.r, inp.w, λ, nᵣ, nᵢ, inp.μ, inp.w_μ, inp.n_top, inp.l_max, max_batch=max_batch)
    optics, partials = [], []
    for j in range(λ.size):
        aero, parts = optics_from_sums(C[j], greek[j][:, :, :2 * int(inp.n_max[j]) - 1])
        optics.append(aero)
        partials.append([parts[rows.index(p)] for p in wrt] if autodiff else [])
    return (optics, partials) if autodiff else optics


def aerosol_derivs(optics: rt.AerosolOptics, partials) -> np.ndarray:
    """The reference's `derivs` [6 l_max + 2, len(partials)]: one column per partial, the rows in the order of the Jacobian that
    convert_jacobian_result_to_aerosol_optics unpacks (phase_function_autodiff.jl:9-29): α, β, γ, δ, ϵ, ζ, then ω̃ and k."""
    l_max = len(optics.greek_coefs.β)
    out = np.zeros((6 * l_max + 2, len(partials)))
    for j, p in enumerate(partials):
        g = p.greek_coefs
        if any(len(a) != l_max for a in (g.α, g.β, g.γ, g.δ, g.ϵ, g.ζ)):
            raise ValueError("a partial's Greek coefficients do not have the length of the optics'")
        out[:, j] = np.concatenate([g.α, g.β, g.γ, g.δ, g.ϵ, g.ζ, [p.ω̃, p.k]])
    return out


def compute_ref_aerosol_extinction(model: MieModel) -> float:
    """compute_NAI2.jl:184-260: the bulk extinction cross section."""
    _, (_, C, _, _) = _device_call(model, False)
    return float(C[0, 1])


# ------------------------------------------------------------------------------------------
# δ-BGE truncation (truncate_phase.jl:95-220)
# ------------------------------------------------------------------------------------------


def reconstruct_phase(greek: rt.GreekCoefs, μ: np.ndarray):
    """mie_helper_functions.jl:198-229 -> (f₁₁, f₁₂, f₂₂, f₃₃, f₃₄, f₄₄), P, P²"""
    l_max = len(greek.α)
    P, P2, R2, T2 = compute_legendre_poly(μ, l_max)
    fac = np.zeros(l_max)
    for l in range(2, l_max):
        fac[l] = math.sqrt(1 / ((l - 1) * l * (l + 1) * (l + 2)))
    f11, f44 = P @ greek.β, P @ greek.δ
    f12, f34 = P2 @ (fac * greek.γ), P2 @ (fac * greek.ϵ)
    f22 = R2 @ (fac * greek.α) + T2 @ (fac * greek.ζ)
    f33 = R2 @ (fac * greek.ζ) + T2 @ (fac * greek.α)
    return (f11, f12, f22, f33, f34, f44), P, P2


def _weighted_fit(w_μ, B, f, first, dfs=()):
    """the normal equations of truncate_phase.jl:129-141 / 154-167: A_ij = Σ w B_i B_j / f², b_i = Σ w B_i / f, rows from `first`.
    With partials dfs of f also the forward-mode derivative of the solution: ∂c = A⁻¹ (∂b - ∂A c), with ∂(B / f) = -(B / f) ∂f / f."""
    Bf = B[:, first:] / f[:, None]
    A = (w_μ[:, None] * Bf).T @ Bf
    c = np.linalg.solve(A, Bf.T @ w_μ)
    if not len(dfs):
        return c
    dcs = []
    for df in dfs:
        dBf = -Bf * (df / f)[:, None]
        dA = (w_μ[:, None] * dBf).T @ Bf + (w_μ[:, None] * Bf).T @ dBf
        dcs.append(np.linalg.solve(A, dBf.T @ w_μ - dA @ c))
    return c, dcs


def truncate_phase(mod: δBGE, aero: rt.AerosolOptics, partials=None, device: Optional[int] = None):
    """truncate_phase(mod::δBGE, aero) as the reference writes it: three weighted least-squares fits over ALL Gauss nodes
    (Δ_angle is read, the index set it selects is never used), β, δ, α, ζ rescaled by c₀ = cl[1], γᵗ and ϵᵗ the fits themselves,
    ω̃ and k unchanged, fᵗ = 1 - c₀.
    With `partials` (AerosolOptics holding ∂aero/∂θ, as compute_aerosol_optical_properties(autodiff=True) returns them) the result
    is (truncated, [∂truncated/∂θ]): the forward-mode derivative of the fits and of the quotients, ∂fᵗ = -∂c₀, ∂ω̃ and ∂k passed on.
    device: None is the numpy text below; an int runs a batch of one on that device (truncate_phase_batch)."""
    if device is not None:
        return truncate_phase_batch(mod, [aero], None if partials is None else [partials], device=device)[0]
    g = aero.greek_coefs
    l_tr = int(mod.l_max)
    μ, w_μ = gausslegendre(len(g.β))
    (f11, f12, _, _, f34, _), P, P2 = reconstruct_phase(g, μ)
    _ = μ < rt.cosd(mod.Δ_angle)   # iμ of the reference: computed, not used
    fac = np.zeros(l_tr)
    for l in range(2, l_tr):
        fac[l] = math.sqrt(1.0 / ((l - 1.0) * l * (l + 1.0) * (l + 2.0)))
    nP = 0 if partials is None else len(partials)
    # the reconstruction is linear in the Greek coefficients: ∂f₁₁ = P ∂β, ∂f₁₂ and ∂f₃₄ from ∂γ and ∂ϵ
    dphase = [reconstruct_phase(p.greek_coefs, μ)[0] for p in partials] if nP else []
    fit = lambda B, f, first, q: _weighted_fit(w_μ, B, f, first, [d[q] for d in dphase]) if nP else (_weighted_fit(w_μ, B, f, first), [])
    cl, dcl = fit(P[:, :l_tr], f11, 0, 0)
    γᵗ, ϵᵗ = np.zeros(l_tr), np.zeros(l_tr)
    dγᵗ, dϵᵗ = [np.zeros(l_tr) for _ in range(nP)], [np.zeros(l_tr) for _ in range(nP)]
    if l_tr > 2:
        γᵗ[2:], dγ = fit(fac * P2[:, :l_tr], f12, 2, 1)
        ϵᵗ[2:], dϵ = fit(fac * P2[:, :l_tr], f34, 2, 4)
        for j in range(nP):
            dγᵗ[j][2:], dϵᵗ[j][2:] = dγ[j], dϵ[j]
    c0 = cl[0]
    βᵗ = cl / c0
    δᵗ = (g.δ[:l_tr] - (g.β[:l_tr] - cl)) / c0
    αᵗ = (g.α[:l_tr] - (g.β[:l_tr] - cl)) / c0
    ζᵗ = (g.ζ[:l_tr] - (g.β[:l_tr] - cl)) / c0
    out = rt.AerosolOptics(greek_coefs=rt.GreekCoefs(α=αᵗ, β=βᵗ, γ=γᵗ, δ=δᵗ, ϵ=ϵᵗ, ζ=ζᵗ), ω̃=aero.ω̃, fᵗ=float(1.0 - c0), k=aero.k)
    if partials is None:
        return out
    d_out = []
    for j, p in enumerate(partials):
        dg, dc, dc0 = p.greek_coefs, dcl[j], dcl[j][0]
        # (a - (β - cl)) / c₀ for a = δ, α, ζ; cl / c₀
        rescaled = lambda a, da: (da[:l_tr] - (dg.β[:l_tr] - dc)) / c0 - (a[:l_tr] - (g.β[:l_tr] - cl)) * dc0 / c0 ** 2
        d_out.append(rt.AerosolOptics(
            greek_coefs=rt.GreekCoefs(α=rescaled(g.α, dg.α), β=dc / c0 - cl * dc0 / c0 ** 2, γ=dγᵗ[j], δ=rescaled(g.δ, dg.δ), ϵ=dϵᵗ[j],
                                      ζ=rescaled(g.ζ, dg.ζ)), ω̃=p.ω̃, fᵗ=float(-dc0), k=p.k))
    return out, d_out


_warned_host_truncation = False


def _six(g: rt.GreekCoefs):
    return (g.α, g.β, g.γ, g.δ, g.ϵ, g.ζ)


def _device_truncation_built(mod: δBGE, optics, partials) -> bool:
    """What mom_truncate_phase covers: l_tr <= 128 and Float64 coefficients.  Anything else takes the host text, with ONE warning per
    process."""
    global _warned_host_truncation
    sets = list(optics) + [p for ps in (partials or []) for p in ps]
    f32 = any(np.asarray(r).dtype == np.float32 for o in sets for r in _six(o.greek_coefs))
    if int(mod.l_max) <= _lib.TRUNCATE_MAX and not f32:
        return True
    if not _warned_host_truncation:
        import warnings
        _warned_host_truncation = True
        warnings.warn(f"truncate_phase on the device covers l_max <= {_lib.TRUNCATE_MAX} in Float64; this and every later request "
                      "outside that takes the host path", RuntimeWarning, stacklevel=3)
    return False


def truncate_phase_batch(mod: δBGE, optics, partials=None, device: Optional[int] = 0):
    """[truncate_phase(mod, o) for o in optics], or with `partials` (one list of AerosolOptics per set)
    [truncate_phase(mod, o, p) for o, p in zip(optics, partials)], in ONE mom_truncate_phase call on `device`: the sets have one
    length l_full, the nodes are gausslegendre(l_full) as in truncate_phase, ω̃ and k pass through on the host.  Sets with fewer
    partials than the longest list are filled with zero derivative sets, whose rows are dropped again.
    A set whose fits met a zero or non-finite divisor or pivot raises np.linalg.LinAlgError naming it.  device = None, l_max > 128
    or Float32 coefficients: the host loop."""
    optics = list(optics)
    partials = None if partials is None else [list(p) for p in partials]
    if partials is not None and len(partials) != len(optics):
        raise ValueError("truncate_phase_batch: one list of partials per set")
    if not optics:
        return []
    if device is None or not _device_truncation_built(mod, optics, partials):
        return [truncate_phase(mod, o) if partials is None else truncate_phase(mod, o, partials[i]) for i, o in enumerate(optics)]
    l_full, l_tr = len(optics[0].greek_coefs.β), int(mod.l_max)
    nP = max((len(p) for p in partials), default=0) if partials is not None else 0
    greek = np.zeros((len(optics), 1 + nP, 6, l_full))
    for i, o in enumerate(optics):
        for j, a in enumerate([o] + (partials[i] if partials is not None else [])):
            rows = [np.asarray(r, dtype=np.float64) for r in _six(a.greek_coefs)]
            if any(r.shape != (l_full,) for r in rows):
                raise ValueError("truncate_phase_batch: every Greek set and derivative set of a batch has one length")
            greek[i, j] = rows
    μ, w_μ = gausslegendre(l_full)
    greek_t, c0, status, _ = _lib.truncate_phase(μ, w_μ, greek, l_tr, device=device)
    if status.any():
        i = int(np.flatnonzero(status)[0])
        fit = next(q for q in range(3) if (int(status[i]) >> q) & 1)
        raise np.linalg.LinAlgError(f"truncate_phase_batch: set {i}, fit {fit} ({'βγϵ'[fit]}): singular weighted fit "
                                    "(a zero or non-finite divisor or pivot)")
    out = []
    for i, o in enumerate(optics):
        sets = [rt.GreekCoefs(*(greek_t[i, j, q].copy() for q in range(6))) for j in range(1 + nP)]
        val = rt.AerosolOptics(greek_coefs=sets[0], ω̃=o.ω̃, fᵗ=float(1.0 - c0[i, 0]), k=o.k)
        if partials is None:
            out.append(val)
        else:
            out.append((val, [rt.AerosolOptics(greek_coefs=sets[1 + j], ω̃=p.ω̃, fᵗ=float(-c0[i, 1 + j]), k=p.k)
                              for j, p in enumerate(partials[i])]))
    return out


def _truncate_grouped(mod: δBGE, optics, partials, device: Optional[int]):
    """truncate_phase_batch for sets of several lengths: one call per distinct length, the results in the order of `optics`.  The
    spectral Mie call cuts each wavelength's set to its own 2 n_max(λ) - 1 terms and the Gauss nodes of the fits follow the length,
    so only sets of one length share a device call.  device = None: the host loop in the order of `optics`."""
    out = [None] * len(optics)
    lengths = [len(o.greek_coefs.β) for o in optics]
    for L in (sorted(set(lengths)) if device is not None else [None]):
        idx = [i for i in range(len(optics)) if L is None or lengths[i] == L]
        res = truncate_phase_batch(mod, [optics[i] for i in idx], None if partials is None else [partials[i] for i in idx], device=device)
        for i, r in zip(idx, res):
            out[i] = r
    return out


def aerosol_optics_partial(model: rt.vSmartMOM_Model, i_aer: int, d_optics: rt.AerosolOptics, dτ_aer=None, band: Optional[int] = None,
                           device: Optional[int] = None) -> rt.OpticsPartial:
    """The OpticsPartial of one parameter of aerosol i_aer (0-based) of the scene `model`, from ∂(aerosol optics)/∂θ as
    truncate_phase(..., partials=) returns it: dω̃ and dfᵗ at i_aer, dZpp / dZmp = compute_Z_moments of the derivative Greek
    coefficients (the moments are linear in them) at basis 1 + i_aer (basis 0 is Rayleigh), zeros elsewhere.  dτ_aer [nAer, Nz]
    is passed on (the scene's τ_aer is an input of its own; a caller that scales it with k supplies its partial).  The result goes
    into rt_run_dual_device_optics.
    A model with bands: `band` (0-based) names the band whose aerosol i_aer the partial belongs to; dω̃ / dfᵗ [nBand, nAer] and
    dZpp / dZmp [M, 1 + nAer nBand, N, N] are nonzero in that band's entries and basis 1 + i_aer + nAer band only, and dτ_aer
    [nBand, nAer, Nz] is passed on.  A parameter shared by several bands is the sum of its per-band partials (sum_partials).
    device: None forms the M derivative matrices on the host, an int in one mom_z_moments call on that device."""
    return aerosol_optics_partials(model, [(i_aer, d_optics, dτ_aer, band)], device=device)[0]


def aerosol_optics_partials(model: rt.vSmartMOM_Model, items, device: Optional[int] = None, resident: bool = False):
    """aerosol_optics_partial for every (i_aer, d_optics, dτ_aer, band) of `items`: the list of their OpticsPartials, with the
    derivative sets of ALL items and all moments formed in one compute_Z_moments_batch call -- with an int `device`, one
    mom_z_moments call; with None, the host function per (item, moment), bitwise what aerosol_optics_partial gives per item.
    resident = True: no matrix is formed; each partial carries its derivative Greek set as d_greeks = [(basis, set)] and the
    handle forms dZpp / dZmp in its own memory (mom_scene_stage_greek_partials)."""
    items = list(items)
    bands = model.bands
    nAer = len(model.aerosol_optics) if bands is None else bands.nAer
    pol, μ, M = model.params.polarization_type, model.quad_points.qp_μ, model.params.max_m
    for i_aer, d_optics, _, band in items:
        if (band is None) != (bands is None):
            raise ValueError("`band` goes with a model that has bands, and only with one")
        if not 0 <= i_aer < nAer:
            raise ValueError(f"i_aer = {i_aer} outside the model's {nAer} aerosols")
        if bands is not None and not 0 <= band < bands.nBand:
            raise ValueError(f"band = {band} outside the model's {bands.nBand} bands")
        aero = model.aerosol_optics[i_aer] if bands is None else bands.aerosol_optics[band][i_aer]
        if len(d_optics.greek_coefs.β) != len(aero.greek_coefs.β):
            raise ValueError("the derivative Greek coefficients do not have the length of the aerosol's")
    if not items:
        return []
    if not resident:
        Zp, Zm = rt.compute_Z_moments_batch(pol, μ, [it[1].greek_coefs for it in items], M, device=device)  # [M, len(items), N, N]
    N = pol.n * len(μ)
    out = []
    for j, (i_aer, d_optics, dτ_aer, band) in enumerate(items):
        K, k = (1 + nAer, 1 + i_aer) if bands is None else (1 + nAer * bands.nBand, 1 + i_aer + nAer * band)
        dZpp = dZmp = d_greeks = None
        if resident:
            d_greeks = [(k, d_optics.greek_coefs)]
        else:
            dZpp, dZmp = np.zeros((M, K, N, N)), np.zeros((M, K, N, N))
            dZpp[:, k], dZmp[:, k] = Zp[:, j], Zm[:, j]
        shape, at = ((nAer,), i_aer) if bands is None else ((bands.nBand, nAer), (band, i_aer))
        dω̃, dfᵗ = np.zeros(shape), np.zeros(shape)
        dω̃[at], dfᵗ[at] = d_optics.ω̃, d_optics.fᵗ
        out.append(rt.OpticsPartial(dτ_aer=None if dτ_aer is None else np.asarray(dτ_aer, dtype=np.float64), dω̃=dω̃, dfᵗ=dfᵗ, dZpp=dZpp,
                                    dZmp=dZmp, d_greeks=d_greeks))
    return out


def sum_partials(partials) -> rt.OpticsPartial:
    """The OpticsPartial of ONE parameter that acts through several ingredients (a size parameter of an aerosol that every band
    sees): the field-wise sum of the per-ingredient partials, None where none of them has the field."""
    import dataclasses
    out = rt.OpticsPartial()
    for p in partials:
        for f in dataclasses.fields(p):
            v, acc = getattr(p, f.name), getattr(out, f.name)
            if v is not None:
                setattr(out, f.name, v if acc is None else acc + v)
    return out


def band_aerosol_optics(mie_model: MieModel, λ_bands, λ_ref: float, τ_ref: float, profile, nᵣ=None, nᵢ=None, n_ref=None,
                        autodiff: bool = False, wrt=_SIZE_PARAMETERS, device: Optional[int] = None):
    """One aerosol type in every band of a band-resolved scene, as model_from_parameters.jl:117-165 sets it up: the Mie run at each
    band centre λ_bands [nBand] and at λ_ref in ONE compute_spectral_aerosol_optical_properties call over [λ_bands..., λ_ref],
    truncate_phase(mie_model.truncation_type) per band, and τ_aer[b] = τ_ref * (k_b / k_ref) * profile (profile [Nz]: the layers'
    shares of the column, getAerosolLayerOptProp).  nᵣ, nᵢ [nBand]: the refractive index per band (default: the aerosol's), n_ref =
    (nᵣ, nᵢ) at λ_ref (default: the aerosol's).  Returns (aerosol_optics [nBand], τ_aer [nBand, Nz]); with autodiff=True also
    (d_optics [nBand][len(wrt)], dτ_aer [len(wrt), nBand, Nz]): the partials of each band's truncated optics and of τ_aer, which
    depends on a parameter through k_b and k_ref.  An index parameter in `wrt` is the SAME change of every wavelength's index.
    device: None truncates band by band on the host; an int truncates all bands with all their partials in one truncate_phase_batch
    call on that device per distinct length of the bands' Greek sets (the spectral call cuts each to 2 n_max(λ) - 1 terms and the
    Gauss nodes of the fits follow that length, so only bands of one length share a call)."""
    λ_bands = np.atleast_1d(np.asarray(λ_bands, dtype=np.float64))
    nB = λ_bands.size
    profile = np.asarray(profile, dtype=np.float64).reshape(-1)
    aer = mie_model.aerosol
    nᵣ = np.full(nB, aer.nᵣ) if nᵣ is None else np.asarray(nᵣ, dtype=np.float64).reshape(nB)
    nᵢ = np.full(nB, aer.nᵢ) if nᵢ is None else np.asarray(nᵢ, dtype=np.float64).reshape(nB)
    n_ref = (aer.nᵣ, aer.nᵢ) if n_ref is None else n_ref
    res = compute_spectral_aerosol_optical_properties(mie_model, np.append(λ_bands, λ_ref), np.append(nᵣ, n_ref[0]), np.append(nᵢ, n_ref[1]),
                                                      autodiff=autodiff, wrt=wrt)
    raw, parts = res if autodiff else (res, None)
    k_ref = raw[nB].k
    res_t = _truncate_grouped(mie_model.truncation_type, raw[:nB], parts[:nB] if autodiff else None, device)
    optics = [r[0] for r in res_t] if autodiff else res_t
    d_optics = [r[1] for r in res_t] if autodiff else []
    τ_aer = np.array([τ_ref * (o.k / k_ref) * profile for o in optics])
    if not autodiff:
        return optics, τ_aer
    dτ_aer = np.array([[τ_ref * (d_optics[b][j].k / k_ref - optics[b].k * parts[nB][j].k / k_ref ** 2) * profile for b in range(nB)]
                       for j in range(len(tuple(wrt)))]).reshape(len(tuple(wrt)), nB, profile.size)
    return optics, τ_aer, d_optics, dτ_aer
