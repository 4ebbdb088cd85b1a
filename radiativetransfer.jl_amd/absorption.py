"""Host side of the line-by-line absorption path (src/Absorption of the reference).

The per-line prefactors are cheap O(nLines) host work and stay on the host exactly as in
compute_absorption_cross_section.jl:73-107; the O(nLines x window) line-shape sum -- the
reference's one-kernel-launch-per-line hot loop (:118-124) -- runs as ONE launch in
libmomcore.so (csrc/voigt.hip).  The absorption model -- HitranModel.broadening x HitranModel.CEF -- is selected by
`broadening=` and `cef=` (absorption_model below); the default is Voigt with HumlicekWeidemann32SDErrorFunction.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

from . import _lib

# src/Absorption/constants/constants.jl:7-17
c2 = 1.4387769
cMassMol = 1.66053873e-27
cLn2 = 0.6931471805599
cSqrt2Ln2 = 1.1774100225
cc_ = 2.99792458e8
cBolts_ = 1.3806503e-23
p_ref = 1013.25
t_ref = 296.0

# HitranModel.broadening / HitranModel.CEF as the YAML reader spells them (parameters_from_yaml.jl:114-115), with or without the
# parentheses -> the library's codes.  Doppler and Lorentz ignore the CEF, as the reference's line_shape! methods do.
BROADENINGS = {"Voigt": _lib.BROADENING_VOIGT, "Doppler": _lib.BROADENING_DOPPLER, "Lorentz": _lib.BROADENING_LORENTZ}
CEFS = {"HumlicekWeidemann32SDErrorFunction": _lib.CEF_HW32SD, "HumlicekWeidemann32VoigtErrorFunction": _lib.CEF_HW32VOIGT}


def _model_code(name, table, what):
    key = name[:-2] if isinstance(name, str) and name.endswith("()") else name
    if not isinstance(key, str) or key not in table:
        raise ValueError(f"unsupported {what} {name!r}: supported are " + ", ".join(f"{k}()" for k in table))
    return table[key]


def absorption_model(broadening="Voigt()", cef="HumlicekWeidemann32SDErrorFunction()"):
    """(broadening code, CEF code) of the reference's names; any other name (CPF12ErrorFunction and the Erfc* error functions
    included, which are not built) raises ValueError naming what is supported."""
    return _model_code(broadening, BROADENINGS, "broadening"), _model_code(cef, CEFS, "CEF")


_DEFAULT_MODEL = (_lib.BROADENING_VOIGT, _lib.CEF_HW32SD)


@dataclass
class HitranTable:
    """The columns of read_hitran's table (read_hitran.jl:14-68, types.jl:24-61) that the line shape needs."""
    mol: np.ndarray      # HITRAN molecule id per line
    iso: np.ndarray      # HITRAN isotopologue id per line
    νᵢ: np.ndarray
    Sᵢ: np.ndarray
    γ_air: np.ndarray
    γ_self: np.ndarray
    E_lower: np.ndarray  # E″ ; -1 means "no temperature correction"
    n_air: np.ndarray
    δ_air: np.ndarray


_HITRAN_FIELDS = [("mol", 2, int), ("iso", 1, int), ("νᵢ", 12, float), ("Sᵢ", 10, float), ("Aᵢ", 10, float),
                  ("γ_air", 5, float), ("γ_self", 5, float), ("E_lower", 10, float), ("n_air", 4, float),
                  ("δ_air", 8, float), ("global_upper_quanta", 15, str), ("global_lower_quanta", 15, str),
                  ("local_upper_quanta", 15, str), ("local_lower_quanta", 15, str), ("ierr", 6, str), ("iref", 12, str),
                  ("line_mixing_flag", 1, str), ("g_upper", 7, float), ("g_lower", 7, float)]


def read_hitran(filepath, mol: int = -1, iso: int = -1, ν_min: float = 0.0, ν_max: float = float("inf"),
                min_strength: float = 0.0) -> dict:
    """read_hitran (read_hitran.jl:14-68): parse a fixed-width HITRAN .par file into columns,
    keeping rows that match molecule / isotopologue / wavenumber range / minimum strength
    (-1 = any).  Unparseable numeric fields become 0 like the reference's `something(tryparse, 0)`."""
    cols = {name: [] for name, _, _ in _HITRAN_FIELDS}
    with open(filepath, "r") as fh:
        for ln in fh:
            ln = ln.rstrip("\n")
            vals, pos = [], 0
            for name, width, typ in _HITRAN_FIELDS:
                txt = ln[pos:pos + width]
                pos += width
                if typ is str:
                    vals.append(txt)
                else:
                    try:
                        vals.append(typ(txt))
                    except ValueError:
                        vals.append(typ(0))
            if (vals[0] == mol or mol == -1) and (vals[1] == iso or iso == -1) and (ν_min <= vals[2] <= ν_max) \
                    and vals[3] >= min_strength:
                for (name, _, _), v in zip(_HITRAN_FIELDS, vals):
                    cols[name].append(v)
    if not cols["mol"]:
        raise ValueError("No matching records found in the HITRAN file")
    return {k: (np.array(v) if not isinstance(v[0], str) else v) for k, v in cols.items()}


def hitran_table(cols: dict) -> HitranTable:
    """read_hitran's column dict -> HitranTable (make_hitran_model's input, make_model_helpers.jl)."""
    f = lambda k: np.asarray(cols[k], dtype=np.float64)
    return HitranTable(mol=np.asarray(cols["mol"], dtype=np.int64), iso=np.asarray(cols["iso"], dtype=np.int64),
                       νᵢ=f("νᵢ"), Sᵢ=f("Sᵢ"), γ_air=f("γ_air"), γ_self=f("γ_self"), E_lower=f("E_lower"),
                       n_air=f("n_air"), δ_air=f("δ_air"))


# ------------------------------------------------------------------------------------------
# TIPS-2017 partition sums and isotopologue weights (constants/TIPS_2017.jl, mol_weights.jl).
# The tables are the reference's NetCDF files, extracted for every HITRAN molecule they cover (ids 1-49, 157 (molecule,
# isotopologue) pairs; rounds 1-3 shipped ids 1-7) by tools/extract_tips.py into data/tips_2017_subset.npz (Float32 like the originals).
# ------------------------------------------------------------------------------------------

_TIPS = None


def _tips():
    global _TIPS
    if _TIPS is None:
        f = _lib.PKG_DIR / "data" / "tips_2017_subset.npz"
        if not f.exists():
            raise FileNotFoundError(f"{f} missing: run /opt/conda/bin/python3.9 tools/extract_tips.py")
        _TIPS = dict(np.load(f))
    return _TIPS


def mol_weight(mol: int, iso: int) -> np.float32:
    """mol_weight(mol, iso) (mol_weights.jl:23): Float32 g/mol; raises like check_exists for unfilled pairs."""
    t = _tips()
    mols = list(t["molecules"])
    if int(mol) not in mols or not (1 <= int(iso) <= t["mol_weight"].shape[1]):
        raise KeyError(f"No matching (mol, iso) pair ({mol}, {iso}) in the extracted tables (tools/extract_tips.py)")
    w = t["mol_weight"][mols.index(int(mol)), int(iso) - 1]
    if w == -1:
        raise KeyError("No matching (mol, iso) pair")
    return np.float32(w)


def get_TT(mol: int, iso: int) -> np.ndarray:
    return _tips()[f"T_{int(mol)}_{int(iso)}"]


def get_TQ(mol: int, iso: int) -> np.ndarray:
    return _tips()[f"Q_{int(mol)}_{int(iso)}"]


class CubicSpline:
    """DataInterpolations.CubicSpline(u, t) as `qoft!` uses it (compute_absorption_cross_section.jl:208-210; compat
    DataInterpolations 4, third-party, restated from its published source): second derivatives z from the
    tridiagonal system with rows [2(h_i + h_{i+1})] and right-hand side 0 at BOTH ends (first row 2 h_1 z_1 + h_1 z_2 = 0,
    not z_1 = 0), all in the element type of the data -- Float32 for the TIPS tables -- and a Float64 evaluation."""

    def __init__(self, u: np.ndarray, t: np.ndarray):
        FT = np.result_type(u.dtype, t.dtype).type
        u, t = u.astype(FT), t.astype(FT)
        n = len(t) - 1
        h = np.concatenate(([FT(0)], (t[1:] - t[:-1]).astype(FT), [FT(0)])).astype(FT)
        dl = h[1:n + 1].copy()
        dg = (FT(2) * (h[0:n + 1] + h[1:n + 2])).astype(FT)
        du = h[1:n + 1].copy()
        d = np.zeros(n + 1, dtype=FT)
        for i in range(1, n):
            d[i] = FT(6) * (u[i + 1] - u[i]) / h[i + 1] - FT(6) * (u[i] - u[i - 1]) / h[i]
        # LU of the (diagonally dominant: no interchange) tridiagonal matrix and the two substitutions, in FT
        for i in range(n):
            f = FT(dl[i] / dg[i])
            dg[i + 1] = FT(dg[i + 1] - f * du[i])
            d[i + 1] = FT(d[i + 1] - f * d[i])
        z = np.zeros(n + 1, dtype=FT)
        z[n] = FT(d[n] / dg[n])
        for i in range(n - 1, -1, -1):
            z[i] = FT((d[i] - du[i] * z[i + 1]) / dg[i])
        self.u, self.t, self.h, self.z = u, t, h[:n + 1], z

    def __call__(self, x: float) -> float:
        t, u, h, z = self.t, self.u, self.h, self.z
        i = int(np.searchsorted(t, x, side="right")) - 1        # searchsortedlast
        i = max(0, min(i, len(t) - 2))
        x = np.float64(x)
        I = z[i] * (t[i + 1] - x) ** 3 / (6 * h[i + 1]) + z[i + 1] * (x - t[i]) ** 3 / (6 * h[i + 1])
        C = (u[i + 1] / h[i + 1] - z[i + 1] * h[i + 1] / 6) * (x - t[i])
        D = (u[i] / h[i + 1] - z[i] * h[i + 1] / 6) * (t[i + 1] - x)
        return float(I + C + D)

    def derivative(self, x: float) -> float:
        """d/dx of the piece __call__ evaluates (the same interval): I + C + D differentiated term by term, as
        ForwardDiff carries a Dual abscissa through the evaluation."""
        t, u, h, z = self.t, self.u, self.h, self.z
        i = int(np.searchsorted(t, x, side="right")) - 1
        i = max(0, min(i, len(t) - 2))
        x = np.float64(x)
        dI = z[i + 1] * (3 * (x - t[i]) ** 2) / (6 * h[i + 1]) - z[i] * (3 * (t[i + 1] - x) ** 2) / (6 * h[i + 1])
        dC = u[i + 1] / h[i + 1] - z[i + 1] * h[i + 1] / 6
        dD = u[i] / h[i + 1] - z[i] * h[i + 1] / 6
        return float(dI + np.float64(dC) - np.float64(dD))


_SPLINES = {}


def qoft(mol: int, iso: int, T: float, T_ref: float = t_ref) -> float:
    """qoft!(M, I, T, T_ref, result) (compute_absorption_cross_section.jl:197-214): Q(T_ref)/Q(T) from the
    TIPS-2017 table of the isotopologue by cubic-spline interpolation."""
    key = (int(mol), int(iso))
    if key not in _SPLINES:
        TT, TQ = get_TT(*key), get_TQ(*key)
        _SPLINES[key] = (CubicSpline(TQ, TT), float(TT.min()), float(TT.max()))
    sp, Tmin, Tmax = _SPLINES[key]
    if not (Tmin < T < Tmax):
        raise AssertionError(f"TIPS2017: T ({T}) must be between {Tmin} K and {Tmax} K.")
    return sp(T_ref) / sp(T)


def qoft_dual(mol: int, iso: int, T: float, T_ref: float = t_ref):
    """qoft! on a Dual temperature: (Q(T_ref)/Q(T), its derivative with respect to T = -Q(T_ref) Q'(T) / Q(T)^2)."""
    rate = qoft(mol, iso, T, T_ref)     # range assertion and spline cache
    sp = _SPLINES[(int(mol), int(iso))][0]
    Qref, Q = sp(T_ref), sp(T)
    return rate, -(Qref / (Q * Q)) * sp.derivative(T)


def linear_rotor_qratio(T: float) -> float:
    """Q(T_ref)/Q(T) of a rigid linear rotor -- NOT what the reference uses (that is `qoft`); kept only as an
    explicit `qratio=` choice for synthetic line lists of molecules outside the extracted tables."""
    return t_ref / T


@dataclass
class LinePrefactors:
    ν: np.ndarray
    γ_d: np.ndarray
    y: np.ndarray
    S: np.ndarray
    ind_start: np.ndarray  # 1-based inclusive
    ind_stop: np.ndarray
    γ_l: Optional[np.ndarray] = None   # the Lorentz half width line_shape! takes next to y (:82-84)


def line_prefactors(h: HitranTable, grid: np.ndarray, pressure: float, temperature: float, vmr: float = 0.0,
                    wing_cutoff: float = 40.0, qratio: Optional[Callable[[float], float]] = None,
                    mol_weights: Optional[dict] = None) -> LinePrefactors:
    """compute_absorption_cross_section.jl:54-107: selection of lines inside the padded grid,
    pressure shift, Lorentz and Doppler half widths (Float32 square root of the Float32 isotopologue weight, as
    `sqrt(mol_weight(mol, iso))` evaluates), y, the TIPS-2017 temperature correction of the strength (`qoft!`) and the
    index window each line touches (linear interpolation of grid -> index with the reference's constant fill values outside
    the grid -- 1 for the start, n for the stop, on either side -- rounded half-to-even like Julia's `round`).  `qratio` overrides the partition-sum ratio (a callable of T); default = the reference's qoft.
    `mol_weights` {(mol, iso): g/mol} supplies isotopologue weights for (molecule, isotopologue) pairs the bundled tables do
    not hold (they cover HITRAN molecules 1-49 as the reference's NetCDF files do; tools/extract_tips.py)."""
    grid = np.asarray(grid, dtype=np.float64)
    temperature = float(temperature)
    keep = (grid.min() - wing_cutoff < h.νᵢ) & (h.νᵢ < grid.max() + wing_cutoff)
    ν0, S0 = h.νᵢ[keep], h.Sᵢ[keep]
    mol, iso = h.mol[keep], h.iso[keep]
    ν = ν0 + pressure / p_ref * h.δ_air[keep]
    γ_l = (h.γ_air[keep] * (1 - vmr) * pressure / p_ref + h.γ_self[keep] * vmr * pressure / p_ref) * \
          (t_ref / temperature) ** h.n_air[keep]
    pairs = sorted(set(zip(mol.tolist(), iso.tolist())))
    sqw = np.empty(ν0.size)
    rate = np.empty(ν0.size)
    E = h.E_lower[keep]
    for (M, I) in pairs:
        sel = (mol == M) & (iso == I)
        if mol_weights is not None and (M, I) in mol_weights:
            w = np.float32(mol_weights[(M, I)])
        else:
            try:
                w = mol_weight(M, I)
            except KeyError as e:
                raise KeyError(f"no isotopologue weight for HITRAN molecule {M}, isotopologue {I}: the bundled TIPS-2017 tables (HITRAN "
                               "molecules 1-49, as in the reference) do not hold this pair; pass mol_weights={(mol, iso): g_per_mol} "
                               "(and qratio=)") from e
        sqw[sel] = np.float64(np.sqrt(w))  # Float32 sqrt, then promoted
        if np.any(E[sel] != -1):
            rate[sel] = qratio(temperature) if qratio is not None else qoft(M, I, temperature, t_ref)
        else:
            rate[sel] = 1.0
    γ_d = ((cSqrt2Ln2 / cc_) * np.sqrt(cBolts_ / cMassMol) * np.sqrt(temperature) * ν0 / sqw)
    y = np.sqrt(cLn2) * γ_l / γ_d
    corr = rate * np.exp(c2 * E * (1 / t_ref - 1 / temperature)) * \
           (1 - np.exp(-c2 * ν0 / temperature)) / (1 - np.exp(-c2 * ν0 / t_ref))
    S = np.where(E != -1, S0 * corr, S0)
    idx = np.arange(1, grid.size + 1, dtype=np.float64)
    if grid.size > 1:
        # LinearInterpolation(grid, 1:n, extrapolation_bc = 1) / (… = n) (:60-61): the constant on BOTH sides of the grid
        n = float(grid.size)
        i0 = np.rint(np.interp(ν - wing_cutoff, grid, idx, left=1.0, right=1.0)).astype(np.int32)
        i1 = np.rint(np.interp(ν + wing_cutoff, grid, idx, left=n, right=n)).astype(np.int32)
    else:
        i0 = np.ones(ν.size, dtype=np.int32)
        i1 = np.ones(ν.size, dtype=np.int32)
    return LinePrefactors(ν, γ_d, y, S, i0, i1, γ_l)


def line_prefactors_dual(h: HitranTable, grid: np.ndarray, pressure: float, temperature: float, vmr: float = 0.0,
                         wing_cutoff: float = 40.0, qratio=None, mol_weights: Optional[dict] = None, with_γ_l: bool = False):
    """line_prefactors on ForwardDiff.Dual numbers with x = [p, T] (autodiff_helper.jl:17-51 through
    compute_absorption_cross_section.jl:79-101): returns the LinePrefactors (the values, as line_prefactors forms them) and
    dν, dγ_d, dy, dS, each [n, 2] with column 0 = d/dp and column 1 = d/dT -- the derivative of every statement as written,
    by the rule ForwardDiff applies to it.  Line selection, windows and the E″ != -1 test are taken on the values.  A
    `qratio` override has no known derivative and raises ValueError.  with_γ_l=True appends dγ_l [n, 2] as a sixth value (the
    partials of LinePrefactors.γ_l, which the Lorentz shape reads)."""
    if qratio is not None:
        raise ValueError("line_prefactors_dual: the derivative of a qratio override is unknown; the Dual run uses the reference's qoft!")
    pf = line_prefactors(h, grid, pressure, temperature, vmr, wing_cutoff, None, mol_weights)
    grid = np.asarray(grid, dtype=np.float64)
    T, p = float(temperature), float(pressure)
    keep = (grid.min() - wing_cutoff < h.νᵢ) & (h.νᵢ < grid.max() + wing_cutoff)
    ν0, S0, E, n_air = h.νᵢ[keep], h.Sᵢ[keep], h.E_lower[keep], h.n_air[keep]
    mol, iso = h.mol[keep], h.iso[keep]
    n = ν0.size
    z = np.zeros(n)
    dν = np.stack([(1 / p_ref) * h.δ_air[keep], z], axis=1)
    # γ_l = lin(p) (t_ref / T)^n
    lin = h.γ_air[keep] * (1 - vmr) * p / p_ref + h.γ_self[keep] * vmr * p / p_ref
    dlin = h.γ_air[keep] * (1 - vmr) / p_ref + h.γ_self[keep] * vmr / p_ref
    dγl_p = dlin * (t_ref / T) ** n_air
    dγl_T = lin * (n_air * (t_ref / T) ** (n_air - 1) * (-(t_ref / (T * T))))
    # γ_d = c sqrt(T) ν0 / sqrt(w): only the square root depends on T
    cg = (cSqrt2Ln2 / cc_) * np.sqrt(cBolts_ / cMassMol)
    sqw = _sqrt_weights(h, keep, mol_weights)
    dγd_T = cg * (1 / (2 * np.sqrt(T))) * ν0 / sqw
    dγd = np.stack([z, dγd_T], axis=1)
    # y = sqrt(ln 2) γ_l / γ_d, quotient rule
    ynum = np.sqrt(cLn2) * (lin * (t_ref / T) ** n_air)
    g = pf.γ_d
    dy = np.stack([np.sqrt(cLn2) * dγl_p * (1 / g), np.sqrt(cLn2) * dγl_T * (1 / g) + dγd_T * (-(ynum / (g * g)))], axis=1)
    # S = S0 rate e1 e2 / e3 where E″ != -1
    dS_T = np.zeros(n)
    for (M, I) in sorted(set(zip(mol.tolist(), iso.tolist()))):
        sel = (mol == M) & (iso == I) & (E != -1)
        if not np.any(sel):
            continue
        rate, drate = qoft_dual(M, I, T, t_ref)
        e1 = np.exp(c2 * E[sel] * (1 / t_ref - 1 / T))
        ex2 = np.exp(-c2 * ν0[sel] / T)
        e2, e3 = 1 - ex2, 1 - np.exp(-c2 * ν0[sel] / t_ref)
        de1 = e1 * (c2 * E[sel] * (1 / (T * T)))
        de2 = -(ex2 * (c2 * ν0[sel] / (T * T)))
        r1, dr1 = rate * e1, drate * e1 + rate * de1
        dS_T[sel] = S0[sel] * ((dr1 * e2 + r1 * de2) / e3)
    dS = np.stack([z, dS_T], axis=1)
    if with_γ_l:
        return pf, dν, dγd, dy, dS, np.stack([dγl_p, dγl_T], axis=1)
    return pf, dν, dγd, dy, dS


def _sqrt_weights(h: HitranTable, keep, mol_weights: Optional[dict] = None) -> np.ndarray:
    """Float64(sqrt(mol_weight(mol, iso)::Float32)) of the kept lines (compute_absorption_cross_section.jl:88)"""
    mol, iso = h.mol[keep], h.iso[keep]
    sqw = np.empty(mol.size)
    for (M, I) in sorted(set(zip(mol.tolist(), iso.tolist()))):
        w = np.float32(mol_weights[(M, I)]) if mol_weights is not None and (M, I) in mol_weights else mol_weight(M, I)
        sqw[(mol == M) & (iso == I)] = np.float64(np.sqrt(w))
    return sqw


# ------------------------------------------------------------------------------------------
# The InterpolationModel (Absorption/types.jl, make_model_helpers.jl:55-110): σ on a (ν, p, T) grid of ranges, kept on the device
# as the coefficients of a cubic B-spline interpolant (csrc/mom_lut.hip) and evaluated there.
# ------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Range:
    """first : step : first + step (length - 1), Julia's AbstractRange as the model's grids are given"""
    first: float
    step: float
    length: int

    @property
    def last(self) -> float:
        return self.first + self.step * (self.length - 1)

    def values(self) -> np.ndarray:
        return self.first + self.step * np.arange(self.length, dtype=np.float64)

    def astuple(self):
        return float(self.first), float(self.step), int(self.length)


def _as_range(r) -> Range:
    return r if isinstance(r, Range) else Range(*r)


@dataclass
class InterpolationModel:
    """InterpolationModel(itp, mol, iso, ν_grid, p_grid, t_grid) (Absorption/types.jl): `itp` is table `id` of handle `h`
    (mom_lut_*); iso = -1 for a table of mixed isotopologues."""
    h: object
    id: int
    mol: int
    iso: int
    ν_grid: Range
    p_grid: Range
    t_grid: Range
    build_ms: Optional[tuple] = None     # GPU time (fill, prefilter) of make_interpolation_model

    def close(self):
        """mom_lut_destroy; the handle frees whatever is left when it closes"""
        if self.id is not None:
            self.h.lut_destroy(self.id)
            self.id = None

    def _check_inside(self, ν, p, T):
        """the scaled interpolant has no extrapolation (compute_absorption_cross_section.jl:155-158 raises a BoundsError)"""
        for name, rng, v in (("nu", self.ν_grid, ν), ("p", self.p_grid, p), ("T", self.t_grid, T)):
            v = np.atleast_1d(np.asarray(v, dtype=np.float64))
            bad = ~((v >= rng.first) & (v <= rng.last))
            if np.any(bad):
                raise ValueError(f"{name} = {v[bad][0]!r} is outside the InterpolationModel's {name} axis [{rng.first}, {rng.last}]")


def interpolation_model_from_table(h, σ, ν_grid, p_grid, t_grid, mol: int = -1, iso: int = -1) -> InterpolationModel:
    """An InterpolationModel of a finished table σ [nν, np, nT] (the reference's cs_matrix): uploaded and prefiltered on the device
    (mom_lut_set_table).  The route of a model loaded from disk or derived from ABSCO on the host."""
    ν_grid, p_grid, t_grid = (_as_range(r) for r in (ν_grid, p_grid, t_grid))
    lut = h.lut_create(ν_grid.astuple(), p_grid.astuple(), t_grid.astuple())
    h.lut_set_table(lut, σ)
    return InterpolationModel(h, lut, int(mol), int(iso), ν_grid, p_grid, t_grid)


def make_interpolation_model(h, table: HitranTable, broadening, ν_grid, p_grid, t_grid, wing_cutoff: float = 40.0, vmr: float = 0.0,
                             cef="HumlicekWeidemann32SDErrorFunction()") -> InterpolationModel:
    """make_interpolation_model(hitran, broadening, ν_grid, p_grid, t_grid; wing_cutoff, vmr, CEF) (make_model_helpers.jl:55-99) on
    handle `h`: the lines inside the padded ν grid become the handle's resident line table, `broadening` / `cef` its absorption
    model, and mom_lut_build fills σ at every (p, T) node with the line-shape kernels and prefilters it -- nothing but the line
    table crosses the bus.  The grids are Range(first, step, length) (or such tuples)."""
    ν_grid, p_grid, t_grid = (_as_range(r) for r in (ν_grid, p_grid, t_grid))
    h.absorption_set_model(*absorption_model(broadening, cef))
    resident_line_table(h, table, ν_grid.values(), wing_cutoff)
    lut = h.lut_create(ν_grid.astuple(), p_grid.astuple(), t_grid.astuple())
    try:
        ms = h.lut_build(lut, vmr, wing_cutoff)
    except Exception:
        h.lut_destroy(lut)
        raise
    iso = int(table.iso[0]) if np.all(table.iso == table.iso[0]) else -1          # :94-95
    return InterpolationModel(h, lut, int(table.mol[0]), iso, ν_grid, p_grid, t_grid, build_ms=ms)


def save_interpolation_model(model: InterpolationModel, path) -> None:
    """save_interpolation_model (make_model_helpers.jl:101-104) as an .npz (in place of JLD2): the raw table and the three ranges."""
    with open(path, "wb") as fh:
        np.savez(fh, table=model.h.lut_get_table(model.id), nu_range=np.array(model.ν_grid.astuple()),
                 p_range=np.array(model.p_grid.astuple()), t_range=np.array(model.t_grid.astuple()), mol=model.mol, iso=model.iso)


def load_interpolation_model(h, path) -> InterpolationModel:
    """load_interpolation_model (make_model_helpers.jl:106-110) onto handle `h`: the saved table is prefiltered again on the device."""
    with np.load(path) as f:
        rng = lambda k: Range(float(f[k][0]), float(f[k][1]), int(f[k][2]))
        return interpolation_model_from_table(h, f["table"], rng("nu_range"), rng("p_range"), rng("t_range"), int(f["mol"]),
                                              int(f["iso"]))


def absorption_cross_section(h, grid, pressure: float, temperature: float, autodiff: bool = False, vmr: float = 0.0,
                             wing_cutoff: float = 40.0, device: int = 0, broadening="Voigt()",
                             cef="HumlicekWeidemann32SDErrorFunction()"):
    """absorption_cross_section(model, grid, p, T; autodiff) (autodiff_helper.jl:17-51): σ[nGrid], or with autodiff=True
    (σ, J[nGrid, 2]) -- the Jacobian with respect to x = [p, T] that ForwardDiff.jacobian! returns as result.derivs[1],
    from the Dual run of the line-shape kernel (mom_voigt_xsec_dual; mom_lineshape_xsec_dual for another absorption model).
    `h` is a HitranTable (line by line, the keywords apply) or an InterpolationModel (mom_lut_xsec on the model's handle: the grid
    is any set of wavenumbers inside the model's ν range; a ν, p or T outside the model's axes raises ValueError)."""
    if isinstance(h, InterpolationModel):
        grid = np.asarray(grid, dtype=np.float64)
        h._check_inside(grid, pressure, temperature)
        return h.h.lut_xsec(h.id, grid, pressure, temperature, jacobian=autodiff)
    model = absorption_model(broadening, cef)
    if not autodiff:
        return compute_absorption_cross_section(h, grid, pressure, temperature, vmr, wing_cutoff, device=device, broadening=broadening,
                                                cef=cef)
    if model != _DEFAULT_MODEL:
        pf, dν, dγd, dy, dS, dγl = line_prefactors_dual(h, grid, pressure, temperature, vmr, wing_cutoff, with_γ_l=True)
        return _lib.lineshape_xsec_dual(*model, pf.ν, pf.γ_d, pf.γ_l, pf.y, pf.S, dν, dγd, dγl, dy, dS, pf.ind_start, pf.ind_stop,
                                        np.asarray(grid, dtype=np.float64), device=device)
    pf, dν, dγd, dy, dS = line_prefactors_dual(h, grid, pressure, temperature, vmr, wing_cutoff)
    return _lib.voigt_xsec_dual(pf.ν, pf.γ_d, pf.y, pf.S, dν, dγd, dy, dS, pf.ind_start, pf.ind_stop,
                                np.asarray(grid, dtype=np.float64), device=device)


def optics_partials(tau, varpi, dtau_abs_k):
    """The partial of the layer optics with respect to one parameter that acts through the gas absorption only:
    `+(::CoreScatteringOpticalProperties, ::CoreAbsorptionOpticalProperties)` (types.jl:672-678) is τ = τ_x + τ_abs,
    ϖ = τ_x ϖ_x / τ, so dτ = dτ_abs and dϖ = -ϖ dτ_abs / τ (τ, ϖ: the sums, [nSpec, Nz], as the scene holds them); the
    weights of the phase-matrix bases do not depend on τ_abs.  Returns the corert.ScenePartial that rt_run_dual takes."""
    from .corert import ScenePartial
    tau, varpi, d = (np.asarray(x, dtype=np.float64) for x in (tau, varpi, dtau_abs_k))
    return ScenePartial(dτ=d.copy(), dϖ=-varpi * d / tau)


def optics_partials_host(model, partials, dtau_abs=None):
    """The numpy twin of k_optics_dual (mom_scene_set_optics_partials): corert.construct_layer_inputs restated in forward mode,
    statement by statement, with ForwardDiff's rules d(a b) = da b + db a and d(a / b) = da (1 / b) + db (-(a / b²)) --
    constructCoreOpticalProperties / createAero (compEffectiveLayerProperties.jl:1-85) and the `+` of types.jl:632-678 on Dual
    element types.  The all-zero tests of types.jl:641-661 are taken on the values, as ForwardDiff takes them.  `partials`: a
    sequence of corert.OpticsPartial; `dtau_abs` [2, nSpec, Nz]: the partials of model.τ_abs with respect to each layer's pressure
    and temperature (Handle.absorption_get_partials), needed when a w_p or w_T is nonzero.  Returns one corert.ScenePartial per
    parameter: dτ, dϖ [nSpec, Nz], dzw [K, nSpec, Nz] or None where the device leaves it absent, and the basis / surface fields.
    A model with bands (the twin of k_optics_bands_dual, mom_scene_set_optics_bands_partials): the same statements band by band
    with the band's aerosols, ϖ_Cabannes and the band's rows of dτ_aer [nBand, nAer, Nz], dω̃, dfᵗ [nBand, nAer]; K = 1 + nAer nBand,
    dzw exact zeros outside a point's own band."""
    from .corert import ScenePartial
    S, Nz = model.τ_rayl.shape
    bands = model.bands
    nAer = len(model.aerosol_optics) if bands is None else bands.nAer
    aer_shape = (nAer,) if bands is None else (bands.nBand, nAer)
    K = 1 + int(np.prod(aer_shape))
    zeros = np.zeros(Nz)
    row = lambda x: zeros if x is None else np.asarray(x, dtype=np.float64).reshape(Nz)
    div = lambda a, da, b, db: (a / b, da * (1.0 / b) + db * (-(a / (b * b))))
    out = []
    for q in partials:
        w_p, w_T, w_gas, w_rayl = row(q.w_p), row(q.w_T), row(q.w_gas), row(q.w_rayl)
        if dtau_abs is None and (np.any(w_p != 0.0) or np.any(w_T != 0.0)):
            raise ValueError("a nonzero w_p or w_T needs dtau_abs, the partials of τ_abs with respect to (p, T)")
        dτ_aer_q = np.zeros(aer_shape + (Nz,)) if q.dτ_aer is None else np.asarray(q.dτ_aer, dtype=np.float64).reshape(aer_shape + (Nz,))
        dω̃_q = np.zeros(aer_shape) if q.dω̃ is None else np.asarray(q.dω̃, dtype=np.float64).reshape(aer_shape)
        dfᵗ_q = np.zeros(aer_shape) if q.dfᵗ is None else np.asarray(q.dfᵗ, dtype=np.float64).reshape(aer_shape)
        dτ, dϖ, dzw = np.empty((S, Nz)), np.empty((S, Nz)), np.zeros((K, S, Nz))

        def one_band(sl, z, ϖ_Cabannes, aerosol_optics, τ_aer, dτ_aer, dω̃, dfᵗ):
            """one layer of one band (the whole axis without bands) -> dτ, dϖ [S_b], dw [1 + nAer, S_b]"""
            τz = model.τ_rayl[sl, z].copy()
            n = τz.size
            dτz = τz * w_rayl[z]
            ϖz, dϖz = np.full(n, float(ϖ_Cabannes)), np.zeros(n)
            w, dw = np.zeros((1 + nAer, n)), np.zeros((1 + nAer, n))
            w[0] = 1.0
            for a, aer in enumerate(aerosol_optics, start=1):
                # createAero on Duals
                fo, dfo = aer.fᵗ * aer.ω̃, dfᵗ[a - 1] * aer.ω̃ + dω̃[a - 1] * aer.fᵗ
                b, db = 1 - fo, -dfo
                τy, dτy = b * τ_aer[a - 1, z], db * τ_aer[a - 1, z] + dτ_aer[a - 1, z] * b
                c, dc = 1 - aer.fᵗ, -dfᵗ[a - 1]
                num, dnum = c * aer.ω̃, dc * aer.ω̃ + dω̃[a - 1] * c
                ϖy, dϖy = div(num, dnum, b, db)
                wy_s, dwy_s = τy * ϖy, dτy * ϖy + dϖy * τy
                # the `+` of types.jl:632-661
                wx, dwx = τz * ϖz, dτz * ϖz + dϖz * τz
                wy, dwy = np.full(n, wy_s), np.full(n, dwy_s)
                tot, dtot = wx + wy, dwx + dwy
                τn, dτn = τz + τy, dτz + dτy
                if np.all(wx == 0.0):
                    w[:], dw[:] = 0.0, 0.0
                    w[a] = 1.0
                elif not np.all(wy == 0.0):
                    fx, dfx = div(wx, dwx, tot, dtot)
                    fy, dfy = div(wy, dwy, tot, dtot)
                    dw = dw * fx[None, :] + dfx[None, :] * w
                    w = w * fx[None, :]
                    w[a], dw[a] = fy, dfy
                ϖz, dϖz = div(tot, dtot, τn, dτn)
                τz, dτz = τn, dτn
            # the gas term (types.jl:672-678)
            τa = model.τ_abs[sl, z]
            dτa = τa * w_gas[z]
            if dtau_abs is not None:
                dτa = dtau_abs[0][sl, z] * w_p[z] + dtau_abs[1][sl, z] * w_T[z] + dτa
            τn, dτn = τz + τa, dτz + dτa
            num, dnum = τz * ϖz, dτz * ϖz + dϖz * τz
            _, dϖz = div(num, dnum, τn, dτn)
            return dτn, dϖz, dw

        for z in range(Nz):
            if bands is None:
                dτ[:, z], dϖ[:, z], dzw[:, :, z] = one_band(slice(None), z, model.ϖ_Cabannes, model.aerosol_optics, model.τ_aer,
                                                            dτ_aer_q, dω̃_q, dfᵗ_q)
                continue
            for b, sl in enumerate(bands.slices()):
                dτ[sl, z], dϖ[sl, z], dw = one_band(sl, z, bands.ϖ_Cabannes[b], bands.aerosol_optics[b], bands.τ_aer[b],
                                                    dτ_aer_q[b], dω̃_q[b], dfᵗ_q[b])
                dzw[0, sl, z] = dw[0]
                dzw[1 + nAer * b:1 + nAer * (b + 1), sl, z] = dw[1:]
        has_zw = nAer > 0 and any(x is not None for x in (q.w_rayl, q.dτ_aer, q.dω̃, q.dfᵗ))
        out.append(ScenePartial(dτ=dτ, dϖ=dϖ, dzw=dzw if has_zw else None, dZpp=q.dZpp, dZmp=q.dZmp, dalbedo=q.dalbedo,
                                dRsurf=q.dRsurf, dalbedo_spec=q.dalbedo_spec))
    return out


def compute_absorption_cross_section(h: HitranTable, grid, pressure: float, temperature: float, vmr: float = 0.0,
                                     wing_cutoff: float = 40.0, qratio=None, device: int = 0, broadening="Voigt()",
                                     cef="HumlicekWeidemann32SDErrorFunction()") -> np.ndarray:
    """compute_absorption_cross_section(model::HitranModel, grid, p, T); by default with Voigt broadening and
    the HumlicekWeidemann32SD error function (the validated default, parameters_from_yaml.jl:115), with `broadening` / `cef`
    (absorption_model) any built method of line_shape! (:167-183).  Returns σ[nGrid] in cm²/molecule, computed on the GPU."""
    model = absorption_model(broadening, cef)
    pf = line_prefactors(h, grid, pressure, temperature, vmr, wing_cutoff, qratio)
    if model != _DEFAULT_MODEL:
        return _lib.lineshape_xsec(*model, pf.ν, pf.γ_d, pf.γ_l, pf.y, pf.S, pf.ind_start, pf.ind_stop,
                                   np.asarray(grid, dtype=np.float64), device=device)
    return _lib.voigt_xsec(pf.ν, pf.γ_d, pf.y, pf.S, pf.ind_start, pf.ind_stop, np.asarray(grid, dtype=np.float64),
                           device=device)


def resident_line_table(h, table: HitranTable, grid, wing_cutoff: float = 40.0):
    """Uploads ONE resident table of the absorber for mom_voigt_tau_abs_layer (device-side prefactors): the lines inside the
    padded grid (compute_absorption_cross_section.jl:54-72), sqrt(mol_weight) per line (Float32 square root, :88) and the
    TIPS-2017 spline tables of the isotopologues in use (qoft!, :197-214).  Returns the number of resident lines."""
    grid = np.asarray(grid, dtype=np.float64)
    keep = (grid.min() - wing_cutoff < table.νᵢ) & (table.νᵢ < grid.max() + wing_cutoff)
    mol, iso = table.mol[keep], table.iso[keep]
    E = table.E_lower[keep]
    pairs = sorted(set(zip(mol.tolist(), iso.tolist())))
    sqw = np.empty(mol.size)
    iso_index = np.full(mol.size, -1, dtype=np.int32)
    splines = []
    for (M, I) in pairs:
        sel = (mol == M) & (iso == I)
        sqw[sel] = np.float64(np.sqrt(mol_weight(M, I)))
        if np.any(E[sel] != -1):
            iso_index[sel] = len(splines)
            splines.append(CubicSpline(get_TQ(M, I), get_TT(M, I)))
    nTmax = max([len(sp.t) for sp in splines], default=0)
    tabs = np.zeros((3, len(splines), nTmax))
    for k, sp in enumerate(splines):
        n = len(sp.t)
        tabs[0, k, :n], tabs[1, k, :n], tabs[2, k, :n] = sp.t, sp.u, sp.z   # Float32 values, widened exactly
    cols = [table.νᵢ[keep], table.Sᵢ[keep], table.γ_air[keep], table.γ_self[keep], E, table.n_air[keep], table.δ_air[keep]]
    h.absorption_set_lines(cols, sqw, iso_index, [len(sp.t) for sp in splines] or [0], tabs[0], tabs[1], tabs[2])
    return int(mol.size)


def compute_absorption_profile(h, table, grid, p_full, T, vcd_dry, vmr, wing_cutoff: float = 40.0,
                               model_vmr: float = 0.0, qratio=None, begin: bool = True, device_prefactors: bool = False,
                               layer_by_layer: bool = False, dual: bool = False, broadening="Voigt()",
                               cef="HumlicekWeidemann32SDErrorFunction()"):
    """compute_absorption_profile!(τ_abs, absorption_model, grid, vmr, profile) (atmo_prof.jl:427-449) on the handle's
    resident τ_abs table: per layer the host builds the line prefactors (O(nLines)), the GPU adds
    σ(ν; p[iz], T[iz]) * vcd_dry[iz] * vmr[iz] into τ_abs[:, iz] (mom_voigt_tau_abs).  `vmr` scalar or per layer (the
    profile's mixing ratio); `model_vmr` is HitranModel.vmr, the self-broadening fraction of the line shape.
    begin=False adds another absorber to the same table (the reference's `+=` over molecules).  device_prefactors=True
    forms the per-line prefactors on the GPU from one resident line table (mom_absorption_set_lines) and runs ALL layers in
    two launches (mom_voigt_tau_abs_profile; returns their GPU time in ms); layer_by_layer=True keeps one
    mom_voigt_tau_abs_layer call per layer (same arithmetic, bitwise).  dual=True takes the Dual entry points on either route
    (mom_voigt_tau_abs_dual fed by line_prefactors_dual, or mom_voigt_tau_abs_profile_dual): the partials of τ_abs with
    respect to each layer's pressure and temperature accumulate in the handle's dtau_abs table (absorption_get_partials).
    `broadening` / `cef` (absorption_model) become the handle's absorption model (mom_absorption_set_model), which the
    device-prefactor entry points follow; on the host route another model than the default goes through
    mom_lineshape_tau_abs(_dual), which takes γ_l.
    `table` may be an InterpolationModel of this handle instead of a HitranTable: all layers in one launch of the table's evaluation
    kernel (mom_lut_tau_abs_profile; dual=True: its Dual run), accumulating into the same τ_abs / dτ_abs tables -- only `begin` and
    `dual` of the keywords apply; returns the GPU time in ms."""
    if isinstance(table, InterpolationModel):
        return _interpolated_profile(h, table, grid, p_full, T, vcd_dry, vmr, begin, dual)
    model = absorption_model(broadening, cef)
    h.absorption_set_model(*model)
    p_full, T, vcd_dry = (np.asarray(x, dtype=np.float64) for x in (p_full, T, vcd_dry))
    Nz = p_full.size
    assert T.size == Nz and vcd_dry.size == Nz
    vmr_arr = np.full(Nz, float(vmr)) if np.ndim(vmr) == 0 else np.asarray(vmr, dtype=np.float64)
    assert vmr_arr.size == Nz, "Length of VMR array has to match profile size or be uniform"
    if begin:
        h.absorption_begin(Nz, grid)
    if device_prefactors:   # one resident table, per layer only (p, T, vmr, vcd) cross the bus
        if qratio is not None:
            raise ValueError("device_prefactors uses the reference's qoft! (TIPS-2017); qratio overrides are host-route only")
        resident_line_table(h, table, grid, wing_cutoff)
        if dual:
            if layer_by_layer:
                raise ValueError("dual=True runs all layers in two launches; there is no layer-by-layer Dual entry point")
            return h.voigt_tau_abs_profile_dual(p_full, T, model_vmr, wing_cutoff, vcd_dry * vmr_arr)
        if layer_by_layer:
            for iz in range(Nz):
                h.voigt_tau_abs_layer(iz + 1, p_full[iz], T[iz], model_vmr, wing_cutoff, vcd_dry[iz] * vmr_arr[iz])
            return None
        return h.voigt_tau_abs_profile(p_full, T, model_vmr, wing_cutoff, vcd_dry * vmr_arr)   # all layers in two launches
    for iz in range(Nz):
        if model != _DEFAULT_MODEL:
            f = vcd_dry[iz] * vmr_arr[iz]
            if dual:
                pf, dν, dγd, dy, dS, dγl = line_prefactors_dual(table, grid, p_full[iz], T[iz], vmr=model_vmr, wing_cutoff=wing_cutoff,
                                                                qratio=qratio, with_γ_l=True)
                h.lineshape_tau_abs_dual(iz + 1, pf.ν, pf.γ_d, pf.γ_l, pf.y, pf.S, dν, dγd, dγl, dy, dS, pf.ind_start, pf.ind_stop, f)
            else:
                pf = line_prefactors(table, grid, p_full[iz], T[iz], vmr=model_vmr, wing_cutoff=wing_cutoff, qratio=qratio)
                h.lineshape_tau_abs(iz + 1, pf.ν, pf.γ_d, pf.γ_l, pf.y, pf.S, pf.ind_start, pf.ind_stop, f)
            continue
        if dual:
            pf, dν, dγd, dy, dS = line_prefactors_dual(table, grid, p_full[iz], T[iz], vmr=model_vmr, wing_cutoff=wing_cutoff,
                                                       qratio=qratio)
            h.voigt_tau_abs_dual(iz + 1, pf.ν, pf.γ_d, pf.y, pf.S, dν, dγd, dy, dS, pf.ind_start, pf.ind_stop, vcd_dry[iz] * vmr_arr[iz])
            continue
        pf = line_prefactors(table, grid, p_full[iz], T[iz], vmr=model_vmr, wing_cutoff=wing_cutoff, qratio=qratio)
        h.voigt_tau_abs(iz + 1, pf.ν, pf.γ_d, pf.y, pf.S, pf.ind_start, pf.ind_stop, vcd_dry[iz] * vmr_arr[iz])


def _interpolated_profile(h, model: InterpolationModel, grid, p_full, T, vcd_dry, vmr, begin: bool, dual: bool) -> float:
    """compute_absorption_profile for an InterpolationModel: one launch for all layers (mom_lut_tau_abs_profile, or its Dual run,
    which also adds into the handle's dtau_abs table); returns its GPU time in ms.  The line-by-line keywords do not apply."""
    if model.h is not h:
        raise ValueError("the InterpolationModel lives on another handle: its table is resident there")
    p_full, T, vcd_dry = (np.asarray(x, dtype=np.float64) for x in (p_full, T, vcd_dry))
    Nz = p_full.size
    assert T.size == Nz and vcd_dry.size == Nz
    vmr_arr = np.full(Nz, float(vmr)) if np.ndim(vmr) == 0 else np.asarray(vmr, dtype=np.float64)
    assert vmr_arr.size == Nz, "Length of VMR array has to match profile size or be uniform"
    model._check_inside(grid, p_full, T)
    if begin:
        h.absorption_begin(Nz, grid)
    return h.lut_tau_abs_profile(model.id, p_full, T, vcd_dry * vmr_arr, dual=dual)


def synthetic_o2a_lines(n_lines: int = 300, ν_lo: float = 12903.0, ν_hi: float = 13245.0, seed: int = 1234) -> HitranTable:
    """Seeded O2-A-like line list of SURVEY section 8d."""
    rng = np.random.default_rng(seed)
    ν = np.sort(rng.uniform(ν_lo, ν_hi, n_lines))
    return HitranTable(mol=np.full(n_lines, 7), iso=np.full(n_lines, 1), νᵢ=ν, Sᵢ=10.0 ** rng.uniform(-27, -23, n_lines),
                       γ_air=rng.uniform(0.03, 0.06, n_lines), γ_self=rng.uniform(0.03, 0.06, n_lines),
                       E_lower=rng.uniform(0.0, 2000.0, n_lines), n_air=np.full(n_lines, 0.7),
                       δ_air=np.full(n_lines, -0.005))
