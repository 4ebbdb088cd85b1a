"""Test helper (not a test file, no fixtures): the cases tests/test_gpu_voigt_edges.py (the kernels of csrc/voigt.hip on the GPU) and
tests/test_oracle_voigt_edges.py (the same constructions against the oracles alone, no GPU) share.

A. one line whose x is the grid itself, for the per-point accuracy of w and w' on both branches;
B. windows on the boundaries of the 256-point blocks, holes in the ordered compaction, more than 256 candidates;
C. non-uniform wavenumber grids for the device-side prefactors (locate_interval's walk, clamps and bisection fallback);
D. temperatures on and next to the TIPS knots;
E. line lists whose windows are monotone in some layers and not in others.

References are computed once per case and cached; callers must not write into what they get."""
import contextlib
import dataclasses
import functools
import re
from pathlib import Path

import numpy as np

import absdual_oracle as ado
from oracle import absref

ROOT = Path(__file__).resolve().parents[1]
BLOCK = 256      # grid points per workgroup (kBlock of csrc/voigt.hip), also the size of a candidate batch


def kernel_constant(name):
    """the literal `name = <number>` of csrc/voigt.hip as a Float64"""
    text = (ROOT / "radiativetransfer.jl_amd" / "csrc" / "voigt.hip").read_text()
    return float(re.search(rf"\b{name} = ([0-9.eE+-]+)[,;]", text).group(1))


def hit_columns(tab):
    """product HitranTable -> the read_hitran-style columns the oracles take"""
    return {"mol": tab.mol, "iso": tab.iso, "νᵢ": tab.νᵢ, "Sᵢ": tab.Sᵢ, "γ_air": tab.γ_air, "γ_self": tab.γ_self,
            "E_lower": tab.E_lower, "n_air": tab.n_air, "δ_air": tab.δ_air}


def permuted(tab, perm):
    return type(tab)(**{f.name: getattr(tab, f.name)[perm] for f in dataclasses.fields(tab)})


# ---- A. per-point accuracy ---------------------------------------------------------------------------------------------
ACC_Y = (1e-8, 1e-4, 1e-2, 0.5, 2.0, 7.5, 8.0, 50.0, 1e4)
ACC_EXACT8 = (0.5, 2.0, 7.5)          # |x| + y == 8 holds exactly at |x| = 7.5, 6, 0.5: multiples of 2^-7
ACC_GAMMA_D = 0.8325546111577         # == cSqrtLn2, so b = cSqrtLn2 / gamma_d = 1.0 and x = grid - 0 = grid, exactly
# Partials of (nu, gamma_d, y, S), columns k = 0, 1; gamma_d, y, S relative to the value.  In the far wing
# Re w = y / (sqrt(pi) (x^2 + y^2)) to leading order, so with s = dS / S, g = dgamma_d / gamma_d, q = dy / y and
# theta = x^2 / (x^2 + y^2) in [0, 1]:  d_k sigma / sigma = s - g - q + 2 (g + q) theta + 2 x dnu / (x^2 + y^2).
# s > g + q + |dnu| / y_min keeps that away from zero on the whole far branch (the last term is at most 0.27 |dnu| there), so
# "relative to the arbiter's own value" is a norm of the arithmetic and not of a cancellation between the four terms.
ACC_DNU = np.array([[0.3, -0.2]])
ACC_REL = {"gd": np.array([[0.25, 0.5]]), "y": np.array([[0.5, 0.75]]), "S": np.array([[1.5, 2.5]])}


def accuracy_grid():
    """4095 points, symmetric about 0, ascending: |x| = 0 .. 9 in steps of 2^-7, then 895 geometrically spaced points to 1e6"""
    near = np.arange(0, 9 * 128 + 1) / 128.0
    pos = np.concatenate([near, np.geomspace(9.0, 1e6, 896)[1:]])
    return np.concatenate([-pos[:0:-1], pos])


def accuracy_line(y):
    """(nu, gd, y, S, dnu, dgd, dy, dS, i0, i1) of the one line, as the entry points take them"""
    n = accuracy_grid().size
    one = lambda v: np.array([float(v)])
    return (one(0.0), one(ACC_GAMMA_D), one(y), one(1.0), ACC_DNU.copy(), ACC_REL["gd"] * ACC_GAMMA_D, ACC_REL["y"] * y, ACC_REL["S"] * 1.0,
            np.array([1], dtype=np.int32), np.array([n], dtype=np.int32))


def accuracy_far(y):
    """the branch test of w on the values: x is the grid, exactly"""
    return np.abs(accuracy_grid()) + y >= 8.0


@functools.lru_cache(maxsize=None)
def accuracy_reference(y):
    """(sigma, J) of the arbiter (np.longdouble) and of the Float64 oracle for the row y"""
    line = accuracy_line(y)
    arb = ado.voigt_sum_dual(*line, accuracy_grid(), FT=np.longdouble)
    o64 = ado.voigt_sum_dual(*line, accuracy_grid())
    assert arb[0].dtype == np.longdouble and np.finfo(np.longdouble).nmant == 63
    return arb, o64


def accuracy_errors(y, sigma, J=None):
    """The distances of (sigma [, J]) from the arbiter of row y in the four norms, {norm: largest over the points}:
      far value, far partial: relative to the arbiter's own value at the point (each partial column);
      near value:   relative to a |1 / (L - i z)| / sqrt(pi), the size of the terms the rational form adds up (Re w itself is
                    what their cancellation leaves, down to 1e-10 of them at y = 1e-8);
      near partial: relative to the largest |partial| of the column over the near-branch points of the row.
    A branch without points in the row is left out."""
    (sa, Ja), _ = accuracy_reference(y)
    x = accuracy_grid().astype(np.longdouble)
    far = accuracy_far(y)
    near = ~far
    out = {}
    ds = np.abs(np.asarray(sigma).astype(np.longdouble) - sa)
    out["far value"] = float(np.max(ds[far] / np.abs(sa[far])))
    if near.any():
        L = np.longdouble(np.sqrt(32 / np.sqrt(2)))
        a = np.longdouble(ado.C_SQRTLN2_DIV_SQRTPI) / np.longdouble(ACC_GAMMA_D)
        size = a / np.sqrt((L + np.longdouble(y)) ** 2 + x * x) / np.sqrt(np.longdouble(np.pi))
        out["near value"] = float(np.max(ds[near] / size[near]))
    if J is not None:
        dJ = np.abs(np.asarray(J).astype(np.longdouble) - Ja)
        out["far partial"] = float(np.max(dJ[far] / np.abs(Ja[far])))
        if near.any():
            out["near partial"] = float(np.max(dJ[near] / np.abs(Ja[near]).max(axis=0)))
    return out


def pool(rows):
    """{norm: the largest over the rows that have it}"""
    out = {}
    for r in rows:
        for k, v in r.items():
            out[k] = max(out.get(k, 0.0), v)
    return out


# ---- B. windows on block boundaries, holes, candidate batches ----------------------------------------------------------
EDGE_GRID = np.linspace(100.0, 101.0, 777)      # blocks [1, 256], [257, 512], [513, 768], [769, 777] (1-based)
EMPTY = (300, 299)
WINDOWS = [(256, 256), (257, 257), (256, 257), (257, 512), (512, 513), (768, 769), (769, 777), (777, 777), EMPTY]


def monotone(i0, i1):
    """what sends a launch down the bisection path: starts and stops both non-decreasing in the line index"""
    return bool(np.all(np.diff(i0) >= 0) and np.all(np.diff(i1) >= 0))


def _window_lists():
    by_start = lambda w: sorted(w)
    out = {
        # [257, 512] and the empty [300, 299] cannot both stand in one monotone list (257 < 300 but 512 > 299): two monotone lists,
        # each window in at least one of them, the empty one between two others
        "monotone": by_start([w for w in WINDOWS if w != EMPTY]),
        "monotone_with_empty": by_start([w for w in WINDOWS if w != (257, 512)]),
        "all": by_start(WINDOWS),
        "wide": by_start(WINDOWS + [(1, 256), (1, 777)]),
    }
    # 600 lines on the whole grid: three batches of candidates in every block, the last one partial
    out["600_full"] = [(1, 777)] * 600
    # 700 lines: 64 .. 127 (the second wave of the first batch) start at 513 and miss the first two blocks -- a wave without a hit
    # there; every third of the others stops at 512 and misses the last two -- ragged masks in every wave
    out["700_ragged"] = [(513, 777) if 64 <= j < 128 else ((1, 512) if j % 3 == 0 else (1, 777)) for j in range(700)]
    # the same hole on the bisection path: a monotone list whose lines 64 .. 127 have the empty window [301, 300]
    out["700_monotone_hole"] = [(1, 300) if j < 64 else ((301, 300) if j < 128 else (301, 777)) for j in range(700)]
    return out


WINDOW_LISTS = _window_lists()
MONOTONE_LISTS = ("monotone", "monotone_with_empty", "600_full", "700_monotone_hole")
WINDOW_CASES = [(name, order) for name in WINDOW_LISTS for order in ("listed", "shuffled")]


@functools.lru_cache(maxsize=None)
def window_case(name, order):
    """(nu, gd, y, S, dnu, dgd, dy, dS, i0, i1) of a list of WINDOW_LISTS, as listed or shuffled (then not monotone)"""
    win = np.array(WINDOW_LISTS[name], dtype=np.int32)
    n = len(win)
    rng = np.random.default_rng(n)
    nu, gd, y = rng.uniform(100.0, 101.0, n), rng.uniform(5e-3, 2e-2, n), rng.uniform(0.05, 1.5, n)
    S = 10.0 ** rng.uniform(-22, -20, n)
    d = [1e-3 * rng.normal(size=(n, 2))] + [0.01 * q[:, None] * rng.normal(size=(n, 2)) for q in (gd, y, S)]
    a = [nu, gd, y, S] + d + [win[:, 0].copy(), win[:, 1].copy()]
    if order == "shuffled":
        perm = np.random.default_rng(1).permutation(n)
        a = [np.ascontiguousarray(q[perm]) for q in a]
        assert not monotone(a[8], a[9]) or len(set(WINDOW_LISTS[name])) == 1
    for q in a:
        q.setflags(write=False)
    return tuple(a)


def covered(i0, i1, n=EDGE_GRID.size):
    """which grid points lie in at least one window"""
    c = np.zeros(n, dtype=bool)
    for a, b in zip(i0, i1):
        c[a - 1:b] = True      # empty for b < a
    return c


def voigt_sum_dual_rows(nu, gd, y, S, dnu, dgd, dy, dS, i0, i1, grid):
    """ado.voigt_sum_dual for many lines: the statements of its loop body on all lines at once (arrays [n, W] over each line's own
    window, W the longest one; every element the same Float64 operations), then the sum over the windows in line order.  Bitwise
    ado.voigt_sum_dual (tests/test_oracle_voigt_edges.py asserts it) at a hundredth of the numpy calls."""
    FT = np.float64
    grid = np.asarray(grid, dtype=FT)
    i0, i1 = np.asarray(i0, dtype=np.int64), np.asarray(i1, dtype=np.int64)
    out, dout = np.zeros(grid.size), np.zeros((2, grid.size))
    if len(nu) == 0:
        return out, dout.T.copy()
    W = max(int(np.max(i1 - i0 + 1)), 1)
    idx = np.minimum(i0[:, None] - 1 + np.arange(W)[None, :], grid.size - 1)     # past a window's end: any point, never summed
    col = lambda v, d: ado.Dual(np.asarray(v, dtype=FT)[:, None], np.asarray(d, dtype=FT).T[:, :, None])
    nj, gj, yj, Sj = col(nu, dnu), col(gd, dgd), col(y, dy), col(S, dS)
    x = FT(ado.C_SQRTLN2) / gj * (grid[idx] - nj)
    z = ado.Dual(x.v + 1j * yj.v, x.d + 1j * yj.d)
    w = ado.w_hw32sd_dual(z, FT)
    term = Sj * FT(ado.C_SQRTLN2_DIV_SQRTPI) / gj * ado.Dual(w.v.real, w.d.real)
    for j in range(len(nu)):
        a, b = int(i0[j]) - 1, int(i1[j])
        if b > a:
            out[a:b] += term.v[j, :b - a]
            dout[:, a:b] += term.d[:, j, :b - a]
    return out, dout.T.copy()


@contextlib.contextmanager
def memoised_spline_setup():
    """oracle/absref.qoft solves the spline system of the isotopologue's table anew for every line; inside this context the same
    function is called once per table and its result reused (same code, same numbers)"""
    orig, memo = absref.spline_second_derivatives, {}

    def cached(u32, t32):
        key = (u32.tobytes(), t32.tobytes())
        if key not in memo:
            memo[key] = orig(u32, t32)
        return memo[key]

    absref.spline_second_derivatives = cached
    try:
        yield
    finally:
        absref.spline_second_derivatives = orig


@functools.lru_cache(maxsize=None)
def window_reference(name, order):
    """(sigma, J) of the Float64 oracle, summed in the case's own line order"""
    return voigt_sum_dual_rows(*window_case(name, order), EDGE_GRID)


# ---- C. non-uniform grids ----------------------------------------------------------------------------------------------
P_FULL = np.array([5.0, 120.0, 480.0, 930.0])
T_FULL = np.array([215.0, 231.5, 262.25, 288.0])
VCD = np.array([1.1e23, 2.4e24, 7.7e24, 1.3e25])
PROFILE_VMR, MODEL_VMR, WING = 0.3, 0.21, 8.0
GRID_NAMES = ("geometric", "two_bands", "jittered", "quadratic", "two_point", "three_point")
TIE_CHECKED = GRID_NAMES[:4]


def profile_grid(name):
    lo, hi, n = 12920.0, 13230.0, 4000
    if name == "geometric":
        return np.geomspace(lo, hi, n)
    if name == "two_bands":                       # a gap of 150 cm^-1 between two uniform bands
        return np.concatenate([np.linspace(lo, 13000.0, n // 2), np.linspace(13150.0, hi, n // 2)])
    if name == "jittered":                        # +-0.4 of the spacing keeps the order; sorted all the same
        u = np.linspace(lo, hi, n)
        return np.sort(u + np.random.default_rng(17).uniform(-0.4, 0.4, n) * (u[1] - u[0]))
    if name == "quadratic":
        return lo + (hi - lo) * np.linspace(0.0, 1.0, n) ** 2
    if name == "two_point":
        return np.array([lo, hi])
    if name == "three_point":
        return np.array([lo, 13100.0, hi])
    raise KeyError(name)


def o2a_lines():
    import rtamd
    return rtamd.absorption.synthetic_o2a_lines(400, seed=5)


def tie_distance(nu, grid, wing):
    """how close an interpolated window index (grid -> 1 .. n, as the oracle forms it) comes to a half-integer, where the
    rounding to the window would turn on the last bit"""
    idx = np.arange(1, grid.size + 1)
    v = np.concatenate([np.interp(nu - wing, grid, idx, left=1, right=1), np.interp(nu + wing, grid, idx, left=grid.size, right=grid.size)])
    return float(np.min(np.abs(v - np.floor(v) - 0.5)))


@functools.lru_cache(maxsize=None)
def _layer_reference(key, p, T, model_vmr, wing):
    tab, grid = _REGISTRY[key]
    hit = hit_columns(tab)
    with memoised_spline_setup():
        prm = absref.line_parameters(hit, grid, p, T, model_vmr, wing)
    dprm = ado.line_parameters_dual(hit, grid, p, T, model_vmr, wing)
    nu, gd, y, S, i0, i1 = dprm
    sig, J = voigt_sum_dual_rows(nu.v, gd.v, y.v, S.v, nu.d.T, gd.d.T, y.d.T, S.d.T, i0, i1, grid)
    return prm, dprm, sig, J


_REGISTRY = {}


def layer_reference(key, tab, grid, p, T, model_vmr, wing):
    """The oracles of one layer, cached under `key` (which must name (tab, grid) uniquely): absref.line_parameters, the Dual
    line parameters, and (sigma, J) of the forward-mode oracle.  The value reference of tau_abs is cref.voigt_xsec on the first
    entry, which the caller forms (the C oracle is a fixture)."""
    _REGISTRY.setdefault(key, (tab, np.asarray(grid, dtype=np.float64)))
    return _layer_reference(key, float(p), float(T), float(model_vmr), float(wing))


# window ends on grid nodes: a dyadic uniform grid, no pressure shift, a dyadic wing
NODE_GRID = 13000.0 + np.arange(1281) / 64.0     # 13000 .. 13020
NODE_WING = 1.5


def node_lines():
    """nu - wing on an interior node, on grid[0], nu + wing on grid[-1] (the x == grid[n - 1] branch of the interpolation) -- and
    each moved by one np.nextafter to either side, which for the two ends is outside the grid (the constant fill)"""
    import rtamd
    base = [13006.5, NODE_GRID[0] + NODE_WING, NODE_GRID[-1] - NODE_WING]
    nu = np.sort(np.array([f(v) for v in base for f in (lambda v: v, lambda v: np.nextafter(v, -np.inf), lambda v: np.nextafter(v, np.inf))]))
    tab = rtamd.absorption.synthetic_o2a_lines(nu.size, 13000.0, 13020.0, seed=2)
    tab.νᵢ[:] = nu
    tab.δ_air[:] = 0.0
    assert np.any(nu - NODE_WING == NODE_GRID[0]) and np.any(nu - NODE_WING < NODE_GRID[0]) and np.any(nu + NODE_WING == NODE_GRID[-1]) \
        and np.any(nu + NODE_WING > NODE_GRID[-1]) and np.any(np.isin(nu - NODE_WING, NODE_GRID[1:-1]))
    return tab


# ---- D. TIPS knots -----------------------------------------------------------------------------------------------------
TIPS_GRID = np.linspace(12990.0, 13010.0, 1000)
TIPS_WING = 2.0


def tips_lines():
    """small lower-state energies: S(T) stays finite and positive from 10 K to the top of the table; one row without correction"""
    import rtamd
    tab = rtamd.absorption.synthetic_o2a_lines(40, 12990.0, 13010.0, seed=8)
    tab.E_lower[:] = np.linspace(0.0, 60.0, 40)
    tab.E_lower[7] = -1.0
    return tab


def tips_temperatures(tab):
    """the first interval (the search starts at the second knot), three knots, the last interval"""
    import rtamd
    knots = np.asarray(rtamd.absorption.get_TT(int(tab.mol[0]), int(tab.iso[0])), dtype=np.float64)
    assert knots[0] == 1.0 and knots[1] == 20.0 and np.all(np.diff(knots[1:]) == 20.0) and {20.0, 240.0, 300.0} <= set(knots.tolist())
    return [10.0, 20.0, 240.0, 300.0, float(knots[-1]) - 10.0], knots


# ---- E. per-layer sortedness -------------------------------------------------------------------------------------------
SORT_GRID = np.linspace(12990.0, 13010.0, 3000)
SORT_WING, SORT_T = 1.5, 250.0


def flipping_lines():
    """pressure shifts of alternating sign: the window order of neighbouring lines flips once the shift exceeds their distance"""
    import rtamd
    tab = rtamd.absorption.synthetic_o2a_lines(200, 12990.0, 13010.0, seed=4)
    tab.δ_air[:] = np.where(np.arange(200) % 2 == 0, -0.03, 0.03)
    return tab


def crossing_lines():
    """Evenly spaced centres (0.1 cm^-1) with shifts of -+1 cm^-1 / atm: 0.01 cm^-1 between neighbours at 5 hPa, which keeps the order,
    1.8 cm^-1 at 930 hPa, which carries a line past eighteen others and its window past a whole block of 256 points.  The shifts of
    flipping_lines move a window by a few points; a block that bisects such a list loses only the last points of a far wing."""
    import rtamd
    tab = rtamd.absorption.synthetic_o2a_lines(200, 12990.0, 13010.0, seed=4)
    tab.νᵢ[:] = np.linspace(12990.05, 13009.95, 200)
    tab.δ_air[:] = np.where(np.arange(200) % 2 == 0, -1.0, 1.0)
    return tab


SORT_LINES = {"flipping": flipping_lines, "crossing": crossing_lines}


def steady_lines():
    """one common shift: monotone windows at every pressure"""
    import rtamd
    return rtamd.absorption.synthetic_o2a_lines(150, 12990.0, 13010.0, seed=6)
