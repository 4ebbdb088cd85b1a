"""Test helper (not a test file): forward-mode restatement of the reference's absorption cross section with x = [p, T].

absorption_cross_section(model, grid, p, T; autodiff = true) (src/Absorption/autodiff_helper.jl:17-51) runs
compute_absorption_cross_section (compute_absorption_cross_section.jl:73-122) on ForwardDiff.Dual numbers.  This file
carries a value and two partials (k = 0: pressure, k = 1: temperature) through every statement of that loop by the rule
ForwardDiff applies to it, in numpy, written independently of the product: the only things taken from elsewhere are the
DATA accessors of oracle/absref.py (tables, mol_weight, spline_second_derivatives, spline_eval).  w(z) runs on complex
numbers whose parts are Duals; both rational approximations are holomorphic, so that is a complex value with a complex
partial d_k w = w'(z) d_k z, which the same arithmetic rules produce.

Integer and boolean decisions (line selection, window indices, the branch |x| + y >= 8 of w, E'' != -1, the TIPS range) are
taken on the values, as ForwardDiff takes them.

Every function takes FT = np.float64 or np.longdouble.  In np.longdouble the pressure-shifted line centre, the grid and the
partition sums Q(T), Q'(T), Q(t_ref) are taken at their Float64 values: a line centre near 13 000 cm^-1 has an ulp of
1.8e-12, so rounding it differently is a change of the INPUT (1e-11 relative on sigma), not arithmetic error.
"""
import math

import numpy as np

from oracle import absref

C2 = 1.4387769            # constants/constants.jl:7-17
C_MASS_MOL = 1.66053873e-27
C_LN2 = 0.6931471805599
C_SQRT2LN2 = 1.1774100225
CC = 2.99792458e8
C_BOLTZ = 1.3806503e-23
P_REF = 1013.25
T_REF = 296.0
C_SQRTLN2_DIV_SQRTPI = 0.469718639319144059835
C_SQRTLN2 = 0.8325546111577

# weideman32a's a1..a32 (complex_error_functions.jl:173-180)
A32 = [2.5722534081245696e+00, 2.2635372999002676e+00, 1.8256696296324824e+00, 1.3455441692345453e+00,
       9.0192548936480144e-01, 5.4601397206393498e-01, 2.9544451071508926e-01, 1.4060716226893769e-01,
       5.7304403529837900e-02, 1.9006155784845689e-02, 4.5195411053501429e-03, 3.9259136070122748e-04,
       -2.4532980269928922e-04, -1.3075449254548613e-04, -2.1409619200870880e-05, 6.8210319440412389e-06,
       4.4015317319048931e-06, 4.2558331390536872e-07, -4.1840763666294341e-07, -1.4813078891201116e-07,
       2.2930439569075392e-08, 2.3797557105844622e-08, 8.1248960947953431e-10, -3.2080150458594088e-09,
       -5.2310170266050247e-10, 4.1537465934749353e-10, 1.1658312885903929e-10, -5.5441820344468828e-11,
       -2.1542618451370239e-11, 8.0314997274316680e-12, 3.7424975634801558e-12, -1.3031797863050087e-12]


class Dual:
    """value v [...] and partials d [2, ...] (real or complex), with ForwardDiff's rules for the operations the loop uses"""
    __array_ufunc__ = None   # numpy scalars and arrays defer to the reflected methods below

    def __init__(self, v, d):
        self.v, self.d = v, d

    @staticmethod
    def _c(x, like):
        """a plain number or array as the value type of `like` (Float32 table entries widen exactly)"""
        return np.asarray(x, dtype=like.v.dtype) if not np.iscomplexobj(x) else np.asarray(x)

    def __neg__(self):
        return Dual(-self.v, -self.d)

    def __add__(self, o):
        return Dual(self.v + o.v, self.d + o.d) if isinstance(o, Dual) else Dual(self.v + self._c(o, self), self.d)

    __radd__ = __add__

    def __sub__(self, o):
        return Dual(self.v - o.v, self.d - o.d) if isinstance(o, Dual) else Dual(self.v - self._c(o, self), self.d)

    def __rsub__(self, o):
        return Dual(self._c(o, self) - self.v, -self.d)

    def __mul__(self, o):
        if isinstance(o, Dual):
            return Dual(self.v * o.v, self.d * o.v + o.d * self.v)
        o = self._c(o, self)
        return Dual(self.v * o, self.d * o)

    __rmul__ = __mul__

    def __truediv__(self, o):
        if isinstance(o, Dual):   # ForwardDiff: da / b - db a / b^2
            q = self.v / o.v
            return Dual(q, self.d * (1 / o.v) + o.d * (-(self.v / (o.v * o.v))))
        o = self._c(o, self)
        return Dual(self.v / o, self.d / o)

    def __rtruediv__(self, o):    # number / Dual: -(q / b) db
        q = self._c(o, self) / self.v
        return Dual(q, -(q / self.v) * self.d)

    def __pow__(self, n):         # Dual ^ number: n x^(n-1) dx
        n = self._c(n, self)
        return Dual(self.v ** n, (n * self.v ** (n - 1)) * self.d)

    def sqrt(self):               # DiffRules: inv(2 sqrt(x))
        s = np.sqrt(self.v)
        return Dual(s, self.d * (1 / (2 * s)))

    def exp(self):
        e = np.exp(self.v)
        return Dual(e, self.d * e)

    def to(self, FT):
        CT = np.clongdouble if FT is np.longdouble else np.complex128
        T = CT if np.iscomplexobj(self.v) else FT
        return Dual(np.asarray(self.v, dtype=T), np.asarray(self.d, dtype=T))


def seed(x, k, FT, shape=(1,)):
    """the Dual of input x with partial 1 in slot k (k = None: a constant)"""
    d = np.zeros((2,) + shape, dtype=FT)
    if k is not None:
        d[k] = 1
    return Dual(np.full(shape, x, dtype=FT), d)


def spline_dual(u32, t32, z, h, x: Dual) -> Dual:
    """_interpolate(A::CubicSpline, t) of DataInterpolations 4 on a Dual abscissa: absref.spline_eval's statements (Float32
    table products, Float64 where the abscissa enters), the interval chosen on the value."""
    idx = int(np.searchsorted(t32, np.float64(x.v.reshape(-1)[0]), side="right"))
    idx = max(1, min(idx, t32.size - 1))
    i = idx - 1
    hi = h[idx]
    term_i = z[i] * (t32[i + 1] - x) ** 3 / (6 * hi) + z[i + 1] * (x - t32[i]) ** 3 / (6 * hi)
    term_c = (u32[i + 1] / hi - z[i + 1] * hi / 6) * (x - t32[i])
    term_d = (u32[i] / hi - z[i] * hi / 6) * (t32[i + 1] - x)
    return term_i + term_c + term_d


_SPL = {}


def qoft_dual(M: int, I: int, T: Dual, FT) -> Dual:
    """qoft! (:197-214): Q(t_ref) / Q(T) with the spline evaluated in Float64 (see the module text), then carried in FT"""
    tab = absref.tables()
    TT, TQ = tab[f"T_{M}_{I}"], tab[f"Q_{M}_{I}"]
    Tv = float(T.v.reshape(-1)[0])
    assert TT.min() < Tv < TT.max(), f"TIPS2017: T ({Tv}) must be between {TT.min()} K and {TT.max()} K."
    if (M, I) not in _SPL:
        _SPL[(M, I)] = absref.spline_second_derivatives(TQ, TT)
    z, h = _SPL[(M, I)]
    T64 = T.to(np.float64)
    Qt = spline_dual(TQ, TT, z, h, T64)
    assert float(Qt.v.reshape(-1)[0]) == absref.spline_eval(TQ, TT, z, h, Tv)   # the same piece, the same value
    Qref = absref.spline_eval(TQ, TT, z, h, T_REF)
    return np.asarray(Qref, dtype=FT) / Qt.to(FT)


def w_hw32sd_dual(z: Dual, FT) -> Dual:
    """w(::HumlicekWeidemann32SDErrorFunction, z) (complex_error_functions.jl:226-234) on a complex Dual [m]"""
    CT = np.clongdouble if FT is np.longdouble else np.complex128
    i1 = CT(1j)
    far = np.abs(z.v.real) + z.v.imag >= 8
    rsp = FT(1 / math.sqrt(math.pi))             # FT(1/sqrt(pi)): the Float64 number, as the reference writes it
    # humlicek2 (:24-30); t = imag(z) - im real(z) = -im z
    t = z * (-i1)
    u = t * t
    w_far = (t * (FT(1.410474) + u * rsp)) / (FT(3) / 4 + (u * (3 + u)))
    # weideman32a (:170-190); iz = im real(z) - imag(z) = im z
    L = FT(math.sqrt(32 / math.sqrt(2)))
    iz = z * i1
    rec = 1 / (L - iz)
    Z = (L + iz) * rec
    poly = Dual(np.full(z.v.shape, A32[31], dtype=CT), np.zeros(z.d.shape, dtype=CT))
    for k in range(30, -1, -1):
        poly = FT(A32[k]) + poly * Z
    w_near = (rsp + 2 * poly * rec) * rec
    return Dual(np.where(far, w_far.v, w_near.v), np.where(far, w_far.d, w_near.d))


def voigt_sum_dual(nu, gd, y, S, dnu, dgd, dy, dS, i0, i1, grid, FT=np.float64):
    """line_shape!(::Voigt) (:179-183) on Duals, summed over the lines in line order over each line's 1-based inclusive window.
    nu .. S: [n]; dnu .. dS: [n, 2] or None (zeros).  Returns sigma [nGrid], dsigma [nGrid, 2] in FT."""
    grid = np.asarray(grid, dtype=np.float64).astype(FT)
    n = len(nu)
    out, dout = np.zeros(grid.size, dtype=FT), np.zeros((2, grid.size), dtype=FT)

    def line(v, d, j):
        dd = np.zeros((2, 1), dtype=FT) if d is None else np.asarray(d)[j].astype(FT).reshape(2, 1)
        return Dual(np.asarray(v)[j:j + 1].astype(FT), dd)

    for j in range(n):
        a, b = int(i0[j]) - 1, int(i1[j])
        if b <= a:
            continue
        nj, gj, yj, Sj = line(nu, dnu, j), line(gd, dgd, j), line(y, dy, j), line(S, dS, j)
        x = FT(C_SQRTLN2) / gj * (grid[a:b] - nj)
        z = Dual(x.v + 1j * yj.v, x.d + 1j * yj.d)
        w = w_hw32sd_dual(z, FT)
        term = Sj * FT(C_SQRTLN2_DIV_SQRTPI) / gj * Dual(w.v.real, w.d.real)
        out[a:b] += term.v
        dout[:, a:b] += term.d
    return out, dout.T.copy()


def line_parameters_dual(hit: dict, grid, pressure, temperature, vmr, wing_cutoff, FT=np.float64):
    """The host loop (:73-107) on Duals, line by line.  Returns nu, gamma_d, y, S as Duals ([n], [2, n]) and the 1-based
    windows.  In np.longdouble nu is the Float64 number (module text)."""
    grid64 = np.asarray(grid, dtype=np.float64)
    grid_max, grid_min = grid64.max() + wing_cutoff, grid64.min() - wing_cutoff
    nG = grid64.size
    p, T = seed(pressure, 0, FT), seed(temperature, 1, FT)
    p64 = seed(pressure, 0, np.float64)
    cols = [[] for _ in range(4)]
    i0s, i1s = [], []
    for j in range(len(hit["Sᵢ"])):
        nu_j = float(hit["νᵢ"][j])
        if not (grid_min < nu_j < grid_max):
            continue
        nu = (nu_j + p64 / P_REF * float(hit["δ_air"][j])).to(FT)
        gamma_l = (float(hit["γ_air"][j]) * (1 - vmr) * p / P_REF + float(hit["γ_self"][j]) * vmr * p / P_REF) * \
                  (T_REF / T) ** float(hit["n_air"][j])
        sq = np.float64(np.sqrt(absref.mol_weight(int(hit["mol"][j]), int(hit["iso"][j]))))   # Float32 sqrt of a Float32
        gamma_d = (FT(C_SQRT2LN2) / FT(CC)) * np.sqrt(FT(C_BOLTZ) / FT(C_MASS_MOL)) * T.sqrt() * nu_j / sq
        y = np.sqrt(FT(C_LN2)) * gamma_l / gamma_d
        S = seed(float(hit["Sᵢ"][j]), None, FT)
        E = float(hit["E_lower"][j])
        if E != -1:
            rate = qoft_dual(int(hit["mol"][j]), int(hit["iso"][j]), T, FT)
            S = S * rate * (FT(C2) * E * (FT(1) / FT(T_REF) - 1 / T)).exp() * \
                (1 - (-FT(C2) * nu_j / T).exp()) / (1 - np.exp(-FT(C2) * FT(nu_j) / FT(T_REF)))
        if nG > 1:
            v = float(nu.v[0])
            lo = np.interp(v - wing_cutoff, grid64, np.arange(1, nG + 1), left=1, right=1)
            hi = np.interp(v + wing_cutoff, grid64, np.arange(1, nG + 1), left=nG, right=nG)
            a, b = int(np.rint(lo)), int(np.rint(hi))     # Base.round: ties to even
        else:
            a = b = 1
        for lst, q in zip(cols, (nu, gamma_d, y, S)):
            lst.append(q)
        i0s.append(a)
        i1s.append(b)
    cat = lambda L: Dual(np.concatenate([q.v for q in L]) if L else np.zeros(0, dtype=FT),
                         np.concatenate([q.d for q in L], axis=1) if L else np.zeros((2, 0), dtype=FT))
    return cat(cols[0]), cat(cols[1]), cat(cols[2]), cat(cols[3]), np.array(i0s, dtype=np.int32), np.array(i1s, dtype=np.int32)


def cross_section_dual(hit: dict, grid, pressure, temperature, vmr=0.0, wing_cutoff=40.0, FT=np.float64):
    """(sigma [nGrid], J [nGrid, 2]) = absorption_cross_section(...; autodiff = true)"""
    nu, gd, y, S, i0, i1 = line_parameters_dual(hit, grid, pressure, temperature, vmr, wing_cutoff, FT)
    return voigt_sum_dual(nu.v, gd.v, y.v, S.v, nu.d.T, gd.d.T, y.d.T, S.d.T, i0, i1, grid, FT)
