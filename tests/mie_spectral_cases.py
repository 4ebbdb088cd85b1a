"""The cases of the spectral Mie call (mom_mie_nai2_spectral, csrc/mom_mie.hip), shared by test_oracle_mie_spectral.py (CPU) and
test_gpu_mie_spectral.py: a batch of wavelengths, each with its own refractive index, on ONE angle grid sized for the shortest
wavelength.  Here: the inputs, the conditions under which a case reaches its edges (through mie_shapes.kernel_constants, so that
a retune fails a condition instead of hollowing out a case), and the oracle of a batch -- mie_oracle.nai2_sums /
mie_dual_oracle.nai2_sums_dual per wavelength on the shared grid, in Float64 and in long double.

No test functions here, and nothing the product imports."""
import functools
from dataclasses import dataclass

import numpy as np

import mie_oracle as mo
import mie_dual_oracle as md
import mie_shapes as ms


@dataclass(frozen=True)
class SpectralCase:
    nR: int = 37
    r_lo: float = ms.R_LO
    r_hi: float = 1.0
    lam: tuple = (0.35, 0.55, 2.1)
    m: tuple = ((1.3, 0.001), (1.75, 0.44), (1.45, 0.0))
    n_mu: int = 0                 # 0: 2 n_top - 1, the grid of the shortest wavelength
    l_max: int = 0                # 0: n_mu


BASE = SpectralCase()                                       # n_max 39 / 31 / 19, n_mu = 77, Kp = 40
TILE_K = SpectralCase(nR=128, r_lo=ms.TILE_K_R_LO)
# mie_shapes.CHUNK_WALK at two wavelengths: G = 62 and 129 tiles, the whole boustrophedon walk with a partly live last row
CHUNK_WALK = SpectralCase(nR=ms.CHUNK_WALK.nR, r_hi=ms.CHUNK_WALK.r_hi, lam=(0.55, 0.8), m=(ms.M_WEAK, ms.M_ABSORBING),
                          n_mu=ms.CHUNK_WALK.n_mu, l_max=ms.CHUNK_WALK.l_max)
CASES = {"base": BASE, "tile_k": TILE_K, "chunk_walk": CHUNK_WALK}

# T3: the three wavelengths, then the first and the last again with other indices
BATCH5_LAM = (0.35, 0.55, 2.1, 0.35, 2.1)
BATCH5_M = ((1.3, 0.001), (1.75, 0.44), (1.45, 0.0), (1.45, 0.0), (1.3, 0.001))
BATCH5 = SpectralCase(lam=BATCH5_LAM, m=BATCH5_M)


def radii(case):
    return np.linspace(case.r_lo, case.r_hi, case.nR)


def n_max_per_wavelength(case):
    """[nL, nR]: the per-radius n_max of every wavelength"""
    r = radii(case)
    return np.stack([mo.n_max_of(2 * np.pi / lam * r) for lam in case.lam])


def n_top(case):
    """the row count of the shared pi / tau tables: the largest per-radius n_max over all wavelengths"""
    return int(n_max_per_wavelength(case).max())


def grid_size(case):
    return case.n_mu or 2 * n_top(case) - 1


def l_max_of(case):
    return case.l_max or grid_size(case)


@functools.lru_cache(maxsize=None)
def device_inputs(case):
    """what the spectral call reads, in Float64: r, w [4, nR] = 4 pi r^2 w_x, lam, n_r, n_i [nL], mu, w_mu, n_max, l_max"""
    r = radii(case)
    mu, w_mu = mo.gausslegendre(grid_size(case))
    inp = dict(r=r, w=4 * np.pi * r ** 2 * ms.weight_rows(r), lam=np.array(case.lam), n_r=np.array([m[0] for m in case.m]),
               n_i=np.array([m[1] for m in case.m]), mu=mu, w_mu=w_mu, n_max=n_top(case), l_max=l_max_of(case))
    for v in inp.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return inp


def _oracle_inputs(case, dtype):
    r64 = radii(case)
    mu64, w_mu64 = mo.gausslegendre(grid_size(case))
    return dict(r=r64.astype(dtype), wx=ms.weight_rows(r64).astype(dtype), mu=mu64.astype(dtype), w_mu=w_mu64.astype(dtype))


@functools.lru_cache(maxsize=None)
def oracle(case, dual=False):
    """[(o64, o80) per wavelength]: the single-wavelength oracle at that wavelength and index on the SHARED grid, with n_rows =
    the shared tables' row count and all the weight rows the form takes (four; the Dual twin three)"""
    out = []
    for lam, (n_r, n_i) in zip(case.lam, case.m):
        pair = []
        for dtype in (np.float64, np.longdouble):
            i = _oracle_inputs(case, dtype)
            if dual:
                pair.append(md.nai2_sums_dual(i["r"], i["wx"][:3], lam, n_r, n_i, mu=i["mu"], w_mu=i["w_mu"], n_rows=n_top(case),
                                              l_max=l_max_of(case)))
            else:
                pair.append(mo.nai2_sums(i["r"], i["wx"], lam, n_r, n_i, mu=i["mu"], w_mu=i["w_mu"], n_rows=n_top(case),
                                         l_max=l_max_of(case)))
        out.append(tuple(pair))
    return out


def compare_batch(got, pairs, dual_rows=0):
    """mie_shapes.compare per wavelength.  got: {name: [nL, rows, ...]}; pairs: oracle(case, dual).  With dual_rows = nW of a Dual
    call the value rows go against the twin's value part and the two index rows against its d_ arrays.
    -> [(wavelength, violation)]"""
    bad = []
    for j, (o64, o80) in enumerate(pairs):
        if dual_rows:
            b, _ = ms.compare({q: got[q][j][:dual_rows] for q in ms.ARRAYS}, o64, o80)
            b2, _ = ms.compare({"d_" + q: got[q][j][dual_rows:] for q in ms.ARRAYS}, o64, o80, tuple("d_" + q for q in ms.ARRAYS))
            b = b + b2
        else:
            b, _ = ms.compare({q: got[q][j] for q in ms.ARRAYS}, o64, o80)
        bad += [(j, v) for v in b]
    return bad
