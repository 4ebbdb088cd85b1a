"""Test helper (not a test file): the numpy twin of the InterpolationModel (csrc/mom_lut.hip), written from the definition of
Interpolations.jl's `interpolate(A, BSpline(Cubic(Line(OnGrid()))))` scaled to three ranges, not from the kernels.

Per axis of n nodes the padded coefficients c_0 .. c_{n+1} solve, as ONE dense system,
    (c_{i-1} + 4 c_i + c_{i+1}) / 6 = f_i   (i = 1 .. n),      c_0 - 2 c_1 + c_2 = 0,      c_{n-1} - 2 c_n + c_{n+1} = 0,
axis after axis.  A point is evaluated at x = (value - first) / step + 1, i = clamp(floor(x), 1, n - 1), delta = x - i with the
cubic B-spline weights of c_{i-1} .. c_{i+2}, as a tensor product; the partials with respect to p and T are the differentiated
weights over the step (ForwardDiff through the weights; floor and clamp on the values).  Outside [first, last] of an axis: ValueError.

Shared by tests/test_oracle_lut.py (against scipy's natural CubicSpline, no GPU) and tests/test_gpu_lut.py.  The table of the
tests is computed once and cached; callers must not write into what they get."""
import functools

import numpy as np

# dyadic ranges (first, step, length): every node coordinate and every x of a node is exact
NU_RANGE = (12995.0, 0.0625, 97)
P_RANGE = (200.0, 150.0, 5)
T_RANGE = (200.0, 30.0, 4)
WING = 8.0


def nodes(rng):
    first, step, n = rng
    return first + step * np.arange(n)


def padded_system(n):
    """the (n + 2) x (n + 2) matrix of the prefilter equations; row 0 and row n + 1 are the boundary rows"""
    A = np.zeros((n + 2, n + 2))
    A[0, :3] = (1.0, -2.0, 1.0)
    A[n + 1, n - 1:] = (1.0, -2.0, 1.0)
    for i in range(1, n + 1):
        A[i, i - 1:i + 2] = (1.0 / 6.0, 4.0 / 6.0, 1.0 / 6.0)
    return A


def prefilter_axis(f, axis):
    f = np.moveaxis(np.asarray(f, dtype=np.float64), axis, 0)
    n = f.shape[0]
    rhs = np.zeros((n + 2,) + f.shape[1:])
    rhs[1:n + 1] = f
    c = np.linalg.solve(padded_system(n), rhs.reshape(n + 2, -1)).reshape(rhs.shape)
    return np.moveaxis(c, 0, axis)


def coefficients(table):
    """[nNu, nP, nT] -> [nNu + 2, nP + 2, nT + 2]"""
    c = np.asarray(table, dtype=np.float64)
    for axis in range(c.ndim):
        c = prefilter_axis(c, axis)
    return c


def cell(v, rng, name):
    """(i, delta) of the values v on a range; i is 1-based as in the text above"""
    first, step, n = rng
    v = np.asarray(v, dtype=np.float64)
    last = first + step * (n - 1)
    if np.any(~((v >= first) & (v <= last))):
        bad = v[~((v >= first) & (v <= last))].ravel()[0]
        raise ValueError(f"{name} = {bad!r} is outside the table's {name} axis [{first}, {last}]")
    x = (v - first) / step + 1.0
    i = np.clip(np.floor(x), 1, n - 1).astype(np.int64)
    return i, x - i


def weights(d):
    e = 1.0 - d
    return np.stack([e ** 3 / 6.0, 2.0 / 3.0 - d ** 2 + d ** 3 / 2.0, 2.0 / 3.0 - e ** 2 + e ** 3 / 2.0, d ** 3 / 6.0])


def dweights(d):
    e = 1.0 - d
    return np.stack([-(e ** 2) / 2.0, -2.0 * d + 3.0 * d ** 2 / 2.0, 2.0 * e - 3.0 * e ** 2 / 2.0, d ** 2 / 2.0])


class LutTwin:
    def __init__(self, table, nu_range=NU_RANGE, p_range=P_RANGE, t_range=T_RANGE):
        self.table = np.asarray(table, dtype=np.float64)
        self.ranges = (nu_range, p_range, t_range)
        assert self.table.shape == tuple(r[2] for r in self.ranges)
        self.c = coefficients(self.table)

    def evaluate(self, nu, p, T, jacobian=False):
        """sigma [n] at (nu [n], p, T), with jacobian=True also J [n, 2]: columns d/dp, d/dT"""
        i_nu, d_nu = cell(np.atleast_1d(nu), self.ranges[0], "nu")
        i_p, d_p = cell(p, self.ranges[1], "p")
        i_t, d_t = cell(T, self.ranges[2], "T")
        wp, wt, wn = weights(float(d_p)), weights(float(d_t)), weights(d_nu)          # [4], [4], [4, n]
        blk = self.c[:, int(i_p) - 1:int(i_p) + 3, int(i_t) - 1:int(i_t) + 3]          # [nNu + 2, 4, 4]
        taps = np.stack([blk[i_nu - 1 + a] for a in range(4)])                         # [4, n, 4, 4]
        sig = np.einsum("an,anbc,b,c->n", wn, taps, wp, wt)
        if not jacobian:
            return sig
        gp, gt = dweights(float(d_p)) / self.ranges[1][1], dweights(float(d_t)) / self.ranges[2][1]
        J = np.stack([np.einsum("an,anbc,b,c->n", wn, taps, gp, wt), np.einsum("an,anbc,b,c->n", wn, taps, wp, gt)], axis=1)
        return sig, J


def o2a_lines():
    """the 40 synthetic O2-A lines of the table, inside and around the nu range"""
    import rtamd
    nu = nodes(NU_RANGE)
    return rtamd.absorption.synthetic_o2a_lines(40, nu[0] - 2.0, nu[-1] + 2.0, seed=11)


def hit_columns(tab):
    return {"mol": tab.mol, "iso": tab.iso, "νᵢ": tab.νᵢ, "Sᵢ": tab.Sᵢ, "γ_air": tab.γ_air, "γ_self": tab.γ_self,
            "E_lower": tab.E_lower, "n_air": tab.n_air, "δ_air": tab.δ_air}


@functools.lru_cache(maxsize=None)
def reference_table():
    """sigma [97, 5, 4] of the line-by-line oracle (oracle/absref.py) at every (p, T) node; read-only"""
    from oracle import absref
    hit, nu = hit_columns(o2a_lines()), nodes(NU_RANGE)
    tab = np.empty((NU_RANGE[2], P_RANGE[2], T_RANGE[2]))
    for i, p in enumerate(nodes(P_RANGE)):
        for j, T in enumerate(nodes(T_RANGE)):
            tab[:, i, j] = absref.absorption_cross_section(hit, nu, p, T, 0.0, WING)
    tab.setflags(write=False)
    return tab


@functools.lru_cache(maxsize=None)
def reference_twin():
    return LutTwin(reference_table())


def synthetic_table(n_nu, n_p, n_t, seed=0):
    """a smooth positive table of any shape with the magnitude of a cross section (prefilter tests at the kernel's chunk edges)"""
    rng = np.random.default_rng(seed)
    k, i, j = np.meshgrid(np.arange(n_nu), np.arange(n_p), np.arange(n_t), indexing="ij")
    return 1e-24 * (1.5 + np.sin(0.37 * k + 0.9 * i) * np.cos(0.21 * k - 0.6 * j) + 0.3 * rng.uniform(size=k.shape))
