"""Test helper (not a test file): the reference's three line_shape! methods (compute_absorption_cross_section.jl:167-183) and
w(::HumlicekWeidemann32VoigtErrorFunction, z) (complex_error_functions.jl:210-219) on the Dual numbers of tests/absdual_oracle.py,
restated in numpy independently of the product, in np.float64 and np.longdouble.

A shape is one of SHAPES: Voigt with either error function, Doppler, Lorentz.  Every statement is the reference's as written, with
its constants (cLn2 = 0.6931471805599, cSqrtLn2divSqrtPi, cSqrtLn2, Float64 pi); the partials follow by ForwardDiff's rules, the
branch |x| + y > 15 is taken on the values.  In np.longdouble the grid and the line centres are taken at their Float64 values, as
in absdual_oracle.py."""
import math

import numpy as np

import absdual_oracle as ado
from absdual_oracle import Dual, qoft_dual, seed
from oracle import absref

SHAPES = ("voigt_sd", "voigt15", "doppler", "lorentz")
NEW_SHAPES = SHAPES[1:]
# (broadening, CEF) as the YAML reader spells them, and the library's codes
NAMES = {"voigt_sd": ("Voigt()", "HumlicekWeidemann32SDErrorFunction()"), "voigt15": ("Voigt()", "HumlicekWeidemann32VoigtErrorFunction()"),
         "doppler": ("Doppler()", "HumlicekWeidemann32SDErrorFunction()"), "lorentz": ("Lorentz()", "HumlicekWeidemann32SDErrorFunction()")}
CODES = {"voigt_sd": (0, 0), "voigt15": (0, 1), "doppler": (1, 0), "lorentz": (2, 0)}
C_LN2 = 0.6931471805599            # constants/constants.jl
C_SQRTLN2 = 0.8325546111577
C_SQRTLN2_DIV_SQRTPI = 0.469718639319144059835


def weideman32a_dual(z: Dual, FT) -> Dual:
    """weideman32a (complex_error_functions.jl:170-190) on a complex Dual"""
    CT = np.clongdouble if FT is np.longdouble else np.complex128
    L = FT(math.sqrt(32 / math.sqrt(2)))
    iz = z * CT(1j)                      # 1im * real(z) - imag(z)
    rec = 1 / (L - iz)
    Z = (L + iz) * rec
    poly = Dual(np.full(z.v.shape, ado.A32[31], dtype=CT), np.zeros(z.d.shape, dtype=CT))
    for k in range(30, -1, -1):
        poly = FT(ado.A32[k]) + poly * Z
    return (FT(1 / math.sqrt(math.pi)) + 2 * poly * rec) * rec


def region1(z):
    """the branch of w(::HumlicekWeidemann32VoigtErrorFunction, z): abs(real(z)) + imag(z) > 15, on values"""
    return np.abs(z.real) + z.imag > 15


def w_hw32voigt_dual(z: Dual, FT, far=None) -> Dual:
    """w(::HumlicekWeidemann32VoigtErrorFunction, z) (:210-219): 1im * FT(1/sqrt(pi)) * z / (z*z - FT(0.5)) in region I.  `far`
    (optional) fixes the branch of every point instead of taking it on z -- for difference quotients, which must not step across
    the jump between the two approximations (8e-5 of w at |x| + y = 15)"""
    CT = np.clongdouble if FT is np.longdouble else np.complex128
    far = region1(z.v) if far is None else far
    with np.errstate(all="ignore"):      # both forms on every point; np.where keeps the one the branch takes
        w_far = (CT(1j) * FT(1 / math.sqrt(math.pi))) * z / (z * z - FT(0.5))
        w_near = weideman32a_dual(z, FT)
    return Dual(np.where(far, w_far.v, w_near.v), np.where(far, w_far.d, w_near.d))


def line_shape_dual(shape, g, nu: Dual, gd: Dual, gl: Dual, y: Dual, S: Dual, FT, far=None) -> Dual:
    """one line_shape! method on Duals: g the grid points (plain numbers), the five prefactors Duals that broadcast against it"""
    if shape == "doppler":
        return S * FT(C_SQRTLN2_DIV_SQRTPI) * (-FT(C_LN2) * ((g - nu) / gd) ** 2).exp() / gd
    if shape == "lorentz":
        return S * gl / (FT(np.pi) * (gl ** 2 + (g - nu) ** 2))
    x = FT(C_SQRTLN2) / gd * (g - nu)
    z = Dual(x.v + 1j * y.v, x.d + 1j * y.d)
    w = ado.w_hw32sd_dual(z, FT) if shape == "voigt_sd" else w_hw32voigt_dual(z, FT, far)
    return S * FT(C_SQRTLN2_DIV_SQRTPI) / gd * Dual(w.v.real, w.d.real)


def lineshape_sum_dual(shape, nu, gd, gl, y, S, dnu, dgd, dgl, dy, dS, i0, i1, grid, FT=np.float64, far=None):
    """line_shape! of `shape` on Duals summed over the lines in line order, each over its 1-based inclusive window.  nu .. S: [n];
    dnu .. dS: [n, 2] or None (zeros).  All lines at once as arrays [n, W] over each line's own window (W the longest one; every
    element the same operations as one line alone), then the sum in line order.  Returns sigma [nGrid], dsigma [nGrid, 2] in FT.
    far: see w_hw32voigt_dual and region1_rows."""
    grid = np.asarray(grid, dtype=np.float64).astype(FT)
    i0, i1 = np.asarray(i0, dtype=np.int64), np.asarray(i1, dtype=np.int64)
    n = len(nu)
    out, dout = np.zeros(grid.size, dtype=FT), np.zeros((2, grid.size), dtype=FT)
    if n == 0:
        return out, dout.T.copy()
    W = max(int(np.max(i1 - i0 + 1)), 1)
    idx = np.minimum(i0[:, None] - 1 + np.arange(W)[None, :], grid.size - 1)     # past a window's end: any point, never summed

    def col(v, d):
        dd = np.zeros((2, n, 1), dtype=FT) if d is None else np.asarray(d).astype(FT).T[:, :, None]
        return Dual(np.asarray(v).astype(FT)[:, None], dd)

    term = line_shape_dual(shape, grid[idx], col(nu, dnu), col(gd, dgd), col(gl, dgl), col(y, dy), col(S, dS), FT, far)
    for j in range(n):
        a, b = int(i0[j]) - 1, int(i1[j])
        if b > a:
            out[a:b] += term.v[j, :b - a]
            dout[:, a:b] += term.d[:, j, :b - a]
    return out, dout.T.copy()


def region1_rows(nu, gd, y, i0, i1, grid):
    """the branch of w(::HumlicekWeidemann32VoigtErrorFunction, z) at every (line, point of its window) in lineshape_sum_dual's
    layout [n, W], taken on the Float64 values"""
    grid = np.asarray(grid, dtype=np.float64)
    i0, i1 = np.asarray(i0, dtype=np.int64), np.asarray(i1, dtype=np.int64)
    W = max(int(np.max(i1 - i0 + 1)), 1)
    idx = np.minimum(i0[:, None] - 1 + np.arange(W)[None, :], grid.size - 1)
    x = C_SQRTLN2 / np.asarray(gd)[:, None] * (grid[idx] - np.asarray(nu)[:, None])
    return np.abs(x) + np.asarray(y)[:, None] > 15


def line_parameters_dual(hit: dict, grid, pressure, temperature, vmr, wing_cutoff, FT=np.float64):
    """The host loop (compute_absorption_cross_section.jl:73-107) on Duals, line by line, keeping gamma_l (:82-84), which line_shape!
    takes next to y.  Returns nu, gamma_d, gamma_l, y, S as Duals ([n], [2, n]) and the 1-based windows."""
    grid64 = np.asarray(grid, dtype=np.float64)
    grid_max, grid_min = grid64.max() + wing_cutoff, grid64.min() - wing_cutoff
    nG = grid64.size
    p, T = seed(pressure, 0, FT), seed(temperature, 1, FT)
    p64 = seed(pressure, 0, np.float64)
    cols = [[] for _ in range(5)]
    i0s, i1s = [], []
    for j in range(len(hit["Sᵢ"])):
        nu_j = float(hit["νᵢ"][j])
        if not (grid_min < nu_j < grid_max):
            continue
        nu = (nu_j + p64 / ado.P_REF * float(hit["δ_air"][j])).to(FT)
        gamma_l = (float(hit["γ_air"][j]) * (1 - vmr) * p / ado.P_REF + float(hit["γ_self"][j]) * vmr * p / ado.P_REF) * \
                  (ado.T_REF / T) ** float(hit["n_air"][j])
        sq = np.float64(np.sqrt(absref.mol_weight(int(hit["mol"][j]), int(hit["iso"][j]))))
        gamma_d = (FT(ado.C_SQRT2LN2) / FT(ado.CC)) * np.sqrt(FT(ado.C_BOLTZ) / FT(ado.C_MASS_MOL)) * T.sqrt() * nu_j / sq
        y = np.sqrt(FT(C_LN2)) * gamma_l / gamma_d
        S = seed(float(hit["Sᵢ"][j]), None, FT)
        E = float(hit["E_lower"][j])
        if E != -1:
            rate = qoft_dual(int(hit["mol"][j]), int(hit["iso"][j]), T, FT)
            S = S * rate * (FT(ado.C2) * E * (FT(1) / FT(ado.T_REF) - 1 / T)).exp() * \
                (1 - (-FT(ado.C2) * nu_j / T).exp()) / (1 - np.exp(-FT(ado.C2) * FT(nu_j) / FT(ado.T_REF)))
        if nG > 1:
            v = float(nu.v[0])
            a = int(np.rint(np.interp(v - wing_cutoff, grid64, np.arange(1, nG + 1), left=1, right=1)))
            b = int(np.rint(np.interp(v + wing_cutoff, grid64, np.arange(1, nG + 1), left=nG, right=nG)))
        else:
            a = b = 1
        for lst, q in zip(cols, (nu, gamma_d, gamma_l, y, S)):
            lst.append(q)
        i0s.append(a)
        i1s.append(b)
    cat = lambda L: Dual(np.concatenate([q.v for q in L]) if L else np.zeros(0, dtype=FT),
                         np.concatenate([q.d for q in L], axis=1) if L else np.zeros((2, 0), dtype=FT))
    return tuple(cat(c) for c in cols) + (np.array(i0s, dtype=np.int32), np.array(i1s, dtype=np.int32))


def cross_section_dual(shape, hit: dict, grid, pressure, temperature, vmr=0.0, wing_cutoff=40.0, FT=np.float64, far=None):
    """(sigma [nGrid], J [nGrid, 2]) = absorption_cross_section(...; autodiff = true) of a HitranModel with this shape"""
    nu, gd, gl, y, S, i0, i1 = line_parameters_dual(hit, grid, pressure, temperature, vmr, wing_cutoff, FT)
    return lineshape_sum_dual(shape, nu.v, gd.v, gl.v, y.v, S.v, nu.d.T, gd.d.T, gl.d.T, y.d.T, S.d.T, i0, i1, grid, FT, far)


# ---- the cases of tests/voigt_cases.py with gamma_l as a fifth prefactor ---------------------------------------------------------
def with_gamma_l(case, seed_=0):
    """a voigt_cases.window_case tuple -> (nu, gd, gl, y, S, dnu, dgd, dgl, dy, dS, i0, i1) with gamma_l = y gamma_d / sqrt(cLn2)
    and dgamma_l = 0.01 gamma_l N(0, 1), seeded"""
    nu, gd, y, S, dnu, dgd, dy, dS, i0, i1 = case
    gl = y * gd / np.sqrt(C_LN2)
    dgl = 0.01 * gl[:, None] * np.random.default_rng(1000 + seed_).normal(size=(len(gl), 2))
    return nu, gd, gl, y, S, dnu, dgd, dgl, dy, dS, i0, i1


def product_rule_terms(shape, g, nu, gd, gl, S, dnu, dgd, dgl, dS):
    """One line, np.longdouble: the sum of the magnitudes of the terms the product rule adds up for d_k sigma at every grid point,
    [nGrid, 2] -- the size d_k sigma is measured against where it crosses zero.
      Doppler: q = (g - nu) / gd, t = S c e / gd:  |dS c e / gd| + |t 2 ln2 q dnu / gd| + |t 2 ln2 q^2 dgd / gd| + |t dgd / gd|
      Lorentz: D = pi (gl^2 + (g - nu)^2), s = S gl / D:  |dS gl / D| + |S dgl / D| + |s pi 2 gl dgl / D| + |s pi 2 (g - nu) dnu / D|"""
    LD = np.longdouble
    g = np.asarray(g, dtype=np.float64).astype(LD)[:, None]
    nu, gd, gl, S = (LD(float(v)) for v in (nu, gd, gl, S))
    dnu, dgd, dgl, dS = (np.asarray(np.zeros(2) if v is None else v, dtype=np.float64).astype(LD).reshape(1, 2) for v in (dnu, dgd, dgl, dS))
    if shape == "doppler":
        q = (g - nu) / gd
        e = np.exp(-LD(C_LN2) * q * q)
        c = LD(C_SQRTLN2_DIV_SQRTPI)
        t = S * c * e / gd
        return np.abs(dS * c * e / gd) + np.abs(t * 2 * LD(C_LN2) * q * dnu / gd) + np.abs(t * 2 * LD(C_LN2) * q * q * dgd / gd) + np.abs(t * dgd / gd)
    assert shape == "lorentz"
    D = LD(np.pi) * (gl * gl + (g - nu) ** 2)
    s = S * gl / D
    return np.abs(dS * gl / D) + np.abs(S * dgl / D) + np.abs(s * LD(np.pi) * 2 * gl * dgl / D) + np.abs(s * LD(np.pi) * 2 * (g - nu) * dnu / D)
