"""The shape cases of the Mie kernels (csrc/mom_mie.hip) that the host layer never produces, shared by test_oracle_mie_shapes.py (CPU)
and test_gpu_mie_shapes.py: scattering.mie_inputs ties n_mu = 2 n_max - 1 = l_max to the largest radius, the C ABI does not.  The
inputs are built here directly: radii, four weight rows, Gauss nodes of any number, pi / tau tables with spare rows, Legendre
tables of any l_max.  Also the conditions under which a case reaches the edge it is named after, as functions of the oracle and
of the kernel's four tiling constants (read from the kernel's text, so that a retune fails a condition instead of hollowing out
a case), and the one comparison rule of these tests.

No test functions here, and nothing the product imports."""
import functools
import re
from dataclasses import dataclass
from pathlib import Path

import numpy as np

import mie_oracle as mo
import mie_dual_oracle as md

ROOT = Path(__file__).resolve().parents[1]
FLOOR = 2.0 ** -46          # of every bound, as in test_gpu_mie_dual.py
FACTOR = 8                  # x the Float64 / long-double distance of the oracle on the same inputs
ARRAYS = ("bulk_f", "C", "greek")
LAM = 0.55
M_WEAK, M_ABSORBING = (1.3, 0.001), (1.75, 0.44)
R_LO = 0.002


def kernel_constant(name):
    """the literal `name = <integer>` of csrc/mom_mie.hip"""
    text = (ROOT / "radiativetransfer.jl_amd" / "csrc" / "mom_mie.hip").read_text()
    return int(re.search(rf"\b{name} = ([0-9]+)[,;]", text).group(1))


def kernel_constants():
    """(kTileR, kMuBlock, kKStep, kMaxChunks): radii per tile, mu rows per block of the value form, k-step, most radius chunks"""
    return tuple(kernel_constant(k) for k in ("kTileR", "kMuBlock", "kKStep", "kMaxChunks"))


def round_up(a, b):
    return (a + b - 1) // b * b


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Shape:
    """what the oracle depends on: one oracle run (with all four weight rows) serves every case of the same Shape"""
    n_mu: int = 33
    l_max: int = 7
    nR: int = 37
    r_hi: float = 1.0
    spare_rows: int = 0           # n_rows - n_top
    m: tuple = M_WEAK
    r_lo: float = R_LO


@dataclass(frozen=True)
class Case:
    shape: Shape
    nW: int = 1


def weight_rows(r, dtype=None):
    """Four fixed rows of w_x over the radii r, [4, nR]: a log-normal density (median at 0.3 of the largest radius, geometric width
    1.6) normalised to sum 1, and that row times u - 0.4 (changes sign, as the row of dw_x / d sigma_g does), 1 + u^2 and exp(-u),
    u = 0 .. 1 across the radii.  1, u - 0.4, 1 + u^2 and exp(-u) are linearly independent functions, so the rows are linearly
    independent from four radii on, and no two are multiples of each other."""
    r = np.asarray(r, dtype=dtype)
    dt = r.dtype.type
    z = np.log(r / (dt(0.3) * r[-1])) / np.log(dt(1.6))
    p = np.exp(-z * z / 2) / r
    w0 = p / p.sum()
    u = (r - r[0]) / (r[-1] - r[0]) if r.size > 1 else np.zeros_like(r)
    return np.stack([w0, w0 * (u - dt(0.4)), w0 * (1 + u * u), w0 * np.exp(-u)])


def oracle_inputs(shape, dtype):
    """what the oracles read, in dtype: the Float64 radii, weight rows, nodes and weights, cast"""
    r = np.linspace(shape.r_lo, shape.r_hi, shape.nR).astype(dtype)       # the same Float64 radii in both precisions
    wx = weight_rows(np.linspace(shape.r_lo, shape.r_hi, shape.nR)).astype(dtype)   # and the same Float64 weights
    n_top = int(mo.n_max_of(2 * np.pi / LAM * shape.r_hi))
    mu64, w_mu64 = mo.gausslegendre(shape.n_mu)
    return dict(r=r, wx=wx, mu=mu64.astype(dtype), w_mu=w_mu64.astype(dtype), n_top=n_top, n_rows=n_top + shape.spare_rows)


@functools.lru_cache(maxsize=None)
def device_inputs(shape):
    """what the device call reads, in Float64: r, w [4, nR] = 4 pi r^2 w_x, w_mu, pi / tau [n_mu, n_rows], P, P2, R2, T2 [n_mu, l_max]"""
    inp = oracle_inputs(shape, np.float64)
    inp["w"] = 4 * np.pi * inp["r"] ** 2 * inp["wx"]
    inp["pi"], inp["tau"] = mo.mie_pi_tau(inp["mu"], inp["n_rows"])
    inp["legendre"] = mo.legendre_tables(inp["mu"], shape.l_max)
    return inp


@functools.lru_cache(maxsize=None)
def oracle(shape):
    """(o64, o80): mie_oracle.nai2_sums on the shape's inputs with all four weight rows, in Float64 and in long double"""
    out = []
    for dtype in (np.float64, np.longdouble):
        i = oracle_inputs(shape, dtype)
        out.append(mo.nai2_sums(i["r"], i["wx"], LAM, *shape.m, mu=i["mu"], w_mu=i["w_mu"], n_rows=i["n_rows"], l_max=shape.l_max))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def oracle_dual(shape):
    """(o64, o80): mie_dual_oracle.nai2_sums_dual on the shape's inputs with weight rows 0 .. 2 (all the Dual form takes)"""
    out = []
    for dtype in (np.float64, np.longdouble):
        i = oracle_inputs(shape, dtype)
        out.append(md.nai2_sums_dual(i["r"], i["wx"][:3], LAM, *shape.m, mu=i["mu"], w_mu=i["w_mu"], n_rows=i["n_rows"],
                                     l_max=shape.l_max))
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------------------
# the cases: each the smallest shape that reaches its edge
# ------------------------------------------------------------------------------------------------------------------------------

# 8 radius tiles; with r from 0.1 their last n_max are 18 20 22 24 25 27 29 31: every residue mod the k-step (from R_LO: 16 19 21 .. 31,
# none of residue 2), and six tiles end before the padded table does
TILE_K_R_LO = 0.1
TILE_K = Shape(nR=128, r_lo=TILE_K_R_LO)
CHUNK_WALK = Shape(n_mu=1025, l_max=8, nR=2057, r_hi=0.05)      # nMuBlk = 33, G = 62, 129 tiles = 2 * 62 + 5; n_max <= 14
MU_BLOCK = {f"mu_{n}": Case(Shape(n_mu=n)) for n in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65)}
GREEK = {f"lmax_{n}": Case(Shape(l_max=n)) for n in (1, 2, 3, 32, 38, 200)}
K_PADDING = {f"spare_{j}": Case(Shape(spare_rows=j)) for j in (0, 1, 2, 3, 9)}
ABSORBING = {"absorbing_mu_33": Case(Shape(m=M_ABSORBING)), "absorbing_tile_k": Case(Shape(nR=128, r_lo=TILE_K_R_LO, m=M_ABSORBING))}
WEIGHT_ROWS_VALUE = {f"nW_{n}": Case(Shape(), n) for n in (1, 2, 3, 4)}
WEIGHT_ROWS_DUAL = {f"nW_{n}": Case(Shape(), n) for n in (1, 2, 3)}
ONE_ROW = {**MU_BLOCK, **GREEK, **K_PADDING, "tile_k": Case(TILE_K), "chunk_walk": Case(CHUNK_WALK), **ABSORBING}
VALUE_CASES = {**ONE_ROW, **WEIGHT_ROWS_VALUE}
DUAL_CASES = {**ONE_ROW, **WEIGHT_ROWS_DUAL}
REPEAT_CASES = {"tile_k": Case(TILE_K), **K_PADDING, "chunk_walk": Case(CHUNK_WALK)}
SHAPES = {name: c.shape for name, c in ONE_ROW.items()}        # every distinct shape is among the one-row cases

# mom_mie_coefficients: x unsorted, spare rows, more than one wavefront and more than one block
X_LO, X_HI = 0.001, 343.7                  # 343.7: 30 um at 0.55 um
COEF_NX = (1, 63, 64, 65, 130)
COEF_MS = (M_WEAK, (1.33, 0.0), M_ABSORBING)
COEF_N_MAX = int(mo.n_max_of(X_HI)) + 3


def _stride(n):
    """the smallest stride >= 0.38 n that is coprime to n: i -> i * stride mod n is a permutation that puts grid points about
    0.38 n apart next to each other"""
    s = max(1, int(np.ceil(0.38 * n)))
    while np.gcd(s, n) != 1:
        s += 1
    return s


def coefficient_x(nX):
    """a fixed permutation of the log-spaced grid of nX size parameters from X_LO to X_HI (one point: X_HI): neighbouring lanes of
    k_mie_ab get trip counts (downward plus upward recurrence) from 70 to about 880"""
    grid = np.geomspace(X_LO, X_HI, nX) if nX > 1 else np.array([X_HI])
    return grid[(np.arange(nX) * _stride(nX)) % nX].copy()


# ------------------------------------------------------------------------------------------------------------------------------
# the conditions under which a case reaches its edge
# ------------------------------------------------------------------------------------------------------------------------------

def tile_last_n_max(n_max, tile_r):
    """the n_max of the last radius of each radius tile: where the tile's k-loop ends (rounded up to the k-step)"""
    n_max = np.asarray(n_max)
    return np.array([n_max[min(i + tile_r, n_max.size) - 1] for i in range(0, n_max.size, tile_r)])


def tile_k_conditions(n_max, n_rows, tile_r, k_step):
    """(residues mod k_step that the tiles' last n_max take, number of tiles whose k-loop ends before the padded table does)"""
    last = tile_last_n_max(n_max, tile_r)
    Kp = round_up(n_rows, k_step)
    return sorted(set(int(v) % k_step for v in last)), int(np.sum(np.array([round_up(int(v), k_step) for v in last]) < Kp))


def chunk_walk_conditions(n_mu, nR, tile_r, mu_block, max_chunks):
    """(nTiles, G, rows of the walk, live chunks of the last row) by the host's rule G = min(2048 / nMuBlk, kMaxChunks, nTiles)"""
    n_tiles = round_up(nR, tile_r) // tile_r
    G = max(1, min(2048 // (round_up(n_mu, mu_block) // mu_block), max_chunks, n_tiles))
    rows = (n_tiles + G - 1) // G
    return n_tiles, G, rows, n_tiles - (rows - 1) * G


# ------------------------------------------------------------------------------------------------------------------------------
# the comparison rule
# ------------------------------------------------------------------------------------------------------------------------------

def compare(got, o64, o80, names=ARRAYS):
    """Every array of `names`, and each of its rows (first axis) on the row's own scale: the distance of got to the Float64
    oracle, relative to the oracle's largest magnitude, against max(8 x the distance between the Float64 and the long-double
    oracle, 2^-46).  got: {name: array}; rows beyond those of got[name] are not looked at, so a call with fewer weight rows
    compares against the same oracle.  -> (violations: list of str, factors: {name: worst 8 d / bound over the array and its
    rows})."""
    bad, factors = [], {}
    for q in names:
        g = np.asarray(got[q])
        n = g.shape[0]
        a, b = np.asarray(o64[q])[:n], np.asarray(o80[q])[:n]
        assert g.shape == a.shape, (q, g.shape, a.shape)
        parts = [("", g, a, b)] + [(f"[{k}]", g[k], a[k], b[k]) for k in range(n)]
        worst = 0.0
        for tag, gg, aa, bb in parts:
            bound = max(FACTOR * mo.rel_max(aa, bb), FLOOR)
            d = mo.rel_max(gg, aa)
            worst = max(worst, FACTOR * d / bound)
            if not d <= bound:
                bad.append(f"{q}{tag}: distance {d:.3e} > bound {bound:.3e}")
        factors[q] = worst
    return bad, factors


def corruptions(o64):
    """Three wrong results a subtly wrong kernel could give, made from the Float64 oracle's own output (all four weight rows):
    one element of one mu row of bulk_f off by 1e-10 of the array's largest magnitude; weight rows 1 and 2 exchanged; the Greek
    coefficients one l too high (zero at l = 0)."""
    base = {q: np.array(o64[q], dtype=np.float64) for q in ARRAYS}
    one = {q: v.copy() for q, v in base.items()}
    one["bulk_f"][0, 2, one["bulk_f"].shape[2] // 2] += 1e-10 * np.abs(base["bulk_f"]).max()
    swapped = {q: v[[0, 2, 1, 3]] for q, v in base.items()}
    shifted = {q: v.copy() for q, v in base.items()}
    shifted["greek"][..., 1:] = base["greek"][..., :-1]
    shifted["greek"][..., 0] = 0
    return {"one element of bulk_f": one, "weight rows 1 and 2 exchanged": swapped, "greek shifted in l": shifted}
