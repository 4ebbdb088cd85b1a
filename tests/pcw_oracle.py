"""CPU oracle of the Domke-PCW aerosol optics (numpy, own text): a twin of the reference's statements in
src/Scattering/compute_PCW.jl:16-193, compute_wigner_values.jl:24-217 and compute_avg_anbns! / compute_avg_C_scatt_ext
(mie_helper_functions.jl:120-144, 258-263), fed with the Mie coefficients of tests/mie_oracle.mie_ab.  Like mie_oracle it takes a
dtype, so the same text runs in np.float64 and in np.longdouble, the arbiter between the Float64 oracle and the device.

The Wigner symbols are walked the way the reference's recursion unfolds: every (n, l) column starts at m = n + l (eq. 27, 28: a chain
over n) and runs downward in m with the three-term recursion of eq. 25, 26, the (0, 0, 0) symbol beside it in steps of two (eq. 29,
30), the (-1, -1, 2) symbol formed from both (eq. 31).  The reference memoises into tables and answers 0 for every request beyond
the table's extent, so a column with n + l > m_max comes out as zeros there; the walk here starts at n + l whatever the table holds
and keeps the symbol's true values.  wigner3j_exact is the Racah sum in integers, independent of all of it.

Nothing here is imported by the product."""
import math
from fractions import Fraction
from functools import lru_cache
from pathlib import Path

import numpy as np

import mie_oracle as mo

GOLDEN_DIR = Path(__file__).resolve().parent / "golden"


# ---- exact symbols ------------------------------------------------------------------------------------------------------------

@lru_cache(maxsize=None)
def _fact(n):
    return math.factorial(n)


def wigner3j_exact(j1, j2, j3, m1, m2, m3):
    """The 3j symbol by the Racah sum, exact up to the final square root (mpmath, 40 digits) -> float"""
    import mpmath as mp
    if m1 + m2 + m3 != 0 or j3 < abs(j1 - j2) or j3 > j1 + j2 or abs(m1) > j1 or abs(m2) > j2 or abs(m3) > j3:
        return 0.0
    delta = Fraction(_fact(j1 + j2 - j3) * _fact(j1 - j2 + j3) * _fact(-j1 + j2 + j3), _fact(j1 + j2 + j3 + 1))
    pre = delta * _fact(j1 + m1) * _fact(j1 - m1) * _fact(j2 + m2) * _fact(j2 - m2) * _fact(j3 + m3) * _fact(j3 - m3)
    s = Fraction(0)
    for t in range(max(0, j2 - j3 - m1, j1 - j3 + m2), min(j1 + j2 - j3, j1 - m1, j2 + m2) + 1):
        den = _fact(t) * _fact(j3 - j2 + t + m1) * _fact(j3 - j1 + t - m2) * _fact(j1 + j2 - j3 - t) * _fact(j1 - t - m1) * _fact(j2 - t + m2)
        s += Fraction((-1) ** t, den)
    if s == 0:
        return 0.0
    sq = s * s * pre
    with mp.workdps(40):
        root = mp.sqrt(mp.mpf(sq.numerator) / mp.mpf(sq.denominator))
        sign = (-1) ** ((j1 - j2 - m3) % 2) * (1 if s > 0 else -1)
        return float(sign * root)


def wigner_A_exact(m, n, l):
    """entry [m, n, l] (1-based, as the reference indexes) of wigner_A: (m n l-1; -1 1 0)"""
    return wigner3j_exact(m, n, l - 1, -1, 1, 0)


def wigner_B_exact(m, n, l):
    """entry [m, n, l] of wigner_B: (m n l-1; -1 -1 2)"""
    return wigner3j_exact(m, n, l - 1, -1, -1, 2)


# absolute bounds of a recursed symbol against the exact one; derived in tests/test_oracle_pcw.py
A_BOUND, B_BOUND = 2e-13, 1e-11


def in_range_samples(m_max, n_max, l_max, count=400, seed=20141224):
    """seeded (m, n, l), 1-based as the tables are indexed, inside the triangle |n - (l - 1)| <= m <= n + l - 1"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        m, n, l = int(rng.integers(1, m_max + 1)), int(rng.integers(1, n_max + 1)), int(rng.integers(1, l_max + 1))
        if abs(n - (l - 1)) <= m <= n + l - 1:
            out.append((m, n, l))
    return out


def out_of_range(m_max, n_max, l_max):
    """-> masks [m_max, n_max, l_max] of the entries outside the triangle, for wigner_A and for wigner_B (there also l - 1 < 2)"""
    m, n, l = np.ogrid[1:m_max + 1, 1:n_max + 1, 0:l_max]
    out = (m < np.abs(n - l)) | (m > n + l)
    return out, out | (l < 2)


@lru_cache(maxsize=None)
def exact_tables(m_max, n_max, l_max):
    A, B = np.zeros((m_max, n_max, l_max)), np.zeros((m_max, n_max, l_max))
    for l in range(1, l_max + 1):
        for n in range(1, n_max + 1):
            for m in range(max(abs(n - (l - 1)), 1), min(n + l - 1, m_max) + 1):
                A[m - 1, n - 1, l - 1] = wigner_A_exact(m, n, l)
                B[m - 1, n - 1, l - 1] = wigner_B_exact(m, n, l)
    return A, B


# ---- the reference's recursion --------------------------------------------------------------------------------------------------

def _real(v, dtype):
    return np.asarray(v).astype(dtype)


def compute_wigner_values(m_max, n_max=None, l_max=None, dtype=np.float64):
    """compute_wigner_values -> wigner_A, wigner_B [m_max, n_max, l_max], entry [m - 1, n - 1, l - 1] the symbol of (m, n, l - 1);
    zeros outside the triangle |n - (l - 1)| <= m <= n + l - 1 and, in wigner_B, for l - 1 < 2.  All columns advance together: the
    arrays below are [n_max, l_max], one step of the loop lowers every column's m by one."""
    if n_max is None:
        m_max, n_max, l_max = 2 * m_max + 1, m_max + 1, 2 * m_max + 1
    dt = np.dtype(dtype).type
    A, B = np.zeros((m_max, n_max, l_max), dtype), np.zeros((m_max, n_max, l_max), dtype)
    n = np.arange(1, n_max + 1, dtype=np.int64)[:, None] + np.zeros((1, l_max), np.int64)
    l = np.arange(0, l_max, dtype=np.int64)[None, :] + np.zeros((n_max, 1), np.int64)
    # eq. 28 and the chain of eq. 27 over n: the symbol at m = n + l
    start = np.zeros((n_max, l_max), dtype)
    l1 = l[0]
    start[0] = _real((-1) ** (l1 % 2), dtype) * np.sqrt(_real((l1 + 1) * (l1 + 2), dtype) / _real((2 * l1 + 1) * (2 * l1 + 2) * (2 * l1 + 3), dtype))
    for j in range(1, n_max):
        nn = j + 1
        num = nn * (2 * nn - 1) * ((nn + l1) ** 2 - 1)
        den = (nn + l1) * (2 * (nn + l1) + 1) * (nn * nn - 1)
        start[j] = -start[j - 1] * np.sqrt(_real(num, dtype) / _real(den, dtype))

    def D(k):   # eq. 26
        return (1 / _real(k, dtype)) * np.sqrt(_real((k * k - 1) * (k * k - (l - n) ** 2) * ((n + l + 1) ** 2 - k * k), dtype))

    m = n + l
    lo = np.maximum(np.abs(n - l), 1)
    a_cur, a_up = start.copy(), np.zeros((n_max, l_max), dtype)
    d_up = D(m + 1)
    w_same = (a_cur * 2) * np.sqrt(_real((n + l) * (n + l + 1) * n * (n + 1), dtype)) / _real(l * (l + 1) - (l + n) * (l + n + 1) - n * (n + 1), dtype)
    with np.errstate(all="ignore"):
        fac = np.where(l >= 2, np.power(_real(np.maximum((l - 1) * l * (l + 1) * (l + 2), 1), dtype), dt(-0.5)), 0)
    ni, li = np.nonzero(np.ones((n_max, l_max), bool))
    ni, li = ni.reshape(n_max, l_max), li.reshape(n_max, l_max)
    for t in range(int((n + l - lo).max()) + 1):
        live = m >= lo
        if t > 0:
            with np.errstate(all="ignore"):
                k = m + 1
                d_k = D(k)
                M_k = 1 - _real(n * (n + 1) - l * (l + 1), dtype) / _real(k * (k + 1), dtype)
                a_new = (1 / d_k) * (M_k * _real(2 * m + 3, dtype) * a_cur - d_up * a_up)
                a_up, a_cur, d_up = a_cur, np.where(live, a_new, 0), d_k
                if t % 2 == 0:   # eq. 29: the same parity as n + l; the other parity runs into m = n + l + 1 and is 0
                    w_same = -w_same * np.sqrt(_real((m + 2) ** 2 - (n - l) ** 2, dtype) / _real((m + 1) ** 2 - (n - l) ** 2, dtype)) * \
                        np.sqrt((1 - (1 / _real(n + l - m, dtype))) * (1 + (1 / _real(m + n + l + 2, dtype))))
        w = w_same if t % 2 == 0 else np.zeros((n_max, l_max), dtype)
        sg = 1 - 2 * ((m + n + l) % 2)
        with np.errstate(all="ignore"):
            b = (_real(sg, dtype) * fac) * (_real(m * (m + 1) + sg * n * (n + 1), dtype) * a_cur +
                                            (2 * np.sqrt(_real(np.maximum(m, 0) * (m + 1) * n * (n + 1), dtype))) * w)
        keep = live & (m <= m_max)
        A[m[keep] - 1, ni[keep], li[keep]] = a_cur[keep]
        kb = keep & (l >= 2)
        B[m[kb] - 1, ni[kb], li[kb]] = b[kb]
        m = m - 1
    return A, B


# ---- compute_aerosol_optical_properties(::MieModel{PCW}) -------------------------------------------------------------------------

def pair_averages(a, b, w, n_max_i):
    """compute_avg_anbns!: a, b complex [N, nR] (row n - 1 = order n), w [nR], n_max_i [nR] -> anam, anbm, bnam, bnbm complex
    [N, N], entry [m - 1, n - 1] for m >= n, zeros above the diagonal.  A radius enters where m < n_max_i and n < n_max_i (strict, as
    written).  The sum over the radii runs in their order (cumsum)."""
    N = a.shape[0]
    order = np.arange(1, N + 1)
    inc = (order[:, None] < n_max_i[None, :])                       # [N, nR]
    mask = inc[:, None, :] & inc[None, :, :]                        # [m, n, i]
    low = (order[:, None] >= order[None, :])[:, :, None]
    out = []
    for u, v in ((a, a), (a, b), (b, a), (b, b)):                   # conj(u_n) v_m
        t = (w[None, None, :] * np.conj(u)[None, :, :]) * v[:, None, :]
        t = np.where(mask & low, t, 0)
        out.append(np.cumsum(t, axis=2)[:, :, -1])
    return tuple(out)


def pcw_sums(r, wx, lam, n_r, n_i, r_max, ab_edit=None, pair_edit=None):
    """The sums of the PCW route in the dtype of r, none divided by C_sca: greek [6, 2 N - 1] (alpha .. zeta), C (C_sca, C_ext), the
    four pair averages, N = get_n_max(2 pi r_max / lam).  ab_edit and pair_edit, (a, b) -> (a, b), are for the sensitivity tests
    only: the first alters the Mie coefficients every sum reads, the second only those the pair averages read."""
    dt = r.dtype.type
    cdt = np.result_type(dt, np.complex64)
    pi = mo.pi_of(dt)
    k = 2 * pi / dt(lam)
    x = k * r
    N = int(mo.n_max_of(np.float64(2 * np.pi * float(r_max) / float(lam))))
    ar, ai, br, bi, n_max_i = mo.mie_ab(x, n_r, n_i, dt, n_rows=N)
    a, b = (ar + 1j * ai).astype(cdt), (br + 1j * bi).astype(cdt)
    if ab_edit is not None:
        a, b = ab_edit(a, b)
    order = np.arange(1, N + 1)
    w2 = (2 * order + 1).astype(dt)
    C_sca = np.sum((2 * pi / k ** 2 * w2) * ((np.abs(a) ** 2 + np.abs(b) ** 2) @ wx))
    C_ext = np.sum((2 * pi / k ** 2 * w2) * ((a + b).real @ wx))
    anam, anbm, bnam, bnbm = pair_averages(*((a, b) if pair_edit is None else pair_edit(a, b)), wx, n_max_i)
    an_m_bn, an_p_bn = (np.abs(a - b) ** 2) @ wx, (np.abs(a + b) ** 2) @ wx
    L = 2 * N - 1
    A, B = compute_wigner_values(N, N, L, dt)                       # [m, n, l]
    l = np.arange(L)[:, None, None]
    n = order[None, :, None]
    m = order[None, None, :]
    valid = (m >= np.maximum(l - n, n + 1)) & (m <= np.minimum(l + n, N))
    sg = (1 - 2 * ((l + n + m) % 2))
    At, Bt = A.transpose(2, 1, 0), B.transpose(2, 1, 0)            # [l, n, m]
    T = lambda M: M.T[None, :, :]                                   # [m, n] -> [1, n, m]
    p1 = (T(anam) + T(anbm) + T(bnam) + T(bnbm)).real
    p2 = (T(anam) - T(anbm) - T(bnam) + T(bnbm)).real
    coef2 = 2 * (2 * m + 1) * (2 * n + 1)
    last = lambda t: np.cumsum(np.where(valid, t, 0).reshape(L, -1), axis=1)[:, -1]
    dn = np.arange(N)
    Ad, Bd = A[dn, dn, :].T, B[dn, dn, :].T                         # [l, n]: the m = n entries
    c1 = (2 * order + 1)[None, :]
    sgl = (1 - 2 * (np.arange(L) % 2))[:, None]
    lastn = lambda t: np.cumsum(t, axis=1)[:, -1]
    S = {}
    for name, wig, wd in (("00", At, Ad), ("22", Bt, Bd)):
        S[name] = last((p1 * (wig * wig)) * coef2.astype(dt)) + lastn((an_p_bn[None, :] * (wd * wd)) * (c1 * c1).astype(dt))
        S[name + "m"] = last((p2 * (wig * wig)) * (coef2 * sg).astype(dt)) + lastn((an_m_bn[None, :] * (wd * wd)) * (c1 * c1 * sgl).astype(dt))
    avg = sg * (T(anam) + T(bnam) - T(anbm) - T(bnbm)) + (np.conj(T(anam)) - np.conj(T(bnam)) + np.conj(T(anbm)) - np.conj(T(bnbm)))
    first = last(avg * 2 * (2 * n + 1).astype(dt) * (2 * m + 1).astype(dt) * At * Bt)
    dg = lambda M: np.diagonal(M)[None, :]
    avg2 = dg(anam) - dg(anbm) + dg(bnam) - dg(bnbm)
    S["02"] = first + lastn(avg2 * 2 * c1.astype(dt) * c1.astype(dt) * Ad * Bd)
    coef = (2 * np.arange(L) + 1).astype(dt) * pi / k ** 2
    S = {q: coef * v for q, v in S.items()}
    greek = np.stack([S["22"] + S["22m"], S["00"] + S["00m"], S["02"].real, S["00"] - S["00m"], S["02"].imag, S["22"] - S["22m"]])
    return dict(greek=greek.astype(r.dtype), C=np.array([C_sca, C_ext], r.dtype), pairs=(anam, anbm, bnam, bnbm), N=N, a=a, b=b,
                n_max_i=n_max_i, an_p_bn=an_p_bn, an_m_bn=an_m_bn)


def case_sums(r_max, nquad, lam, n_r, n_i, r_m, sigma_g, dtype=np.float64):
    """pcw_sums of a whole model: the radius quadrature on [0, r_max] and LogNormal(log r_m, log sigma_g) of mie_oracle"""
    r, wr = mo.gauleg_norm(nquad, 0, r_max, dtype)
    wx = mo.weights_wx(r, wr, r_m, sigma_g)
    out = pcw_sums(r, wx, lam, n_r, n_i, r_max)
    out.update(r=r, wx=wx)
    return out


def aerosol_optics(r_max, nquad, lam, n_r, n_i, r_m, sigma_g, dtype=np.float64):
    """-> greek [6, 2 N - 1] (alpha .. zeta, times 1 / C_sca as compute_PCW.jl:86-91), omega = C_sca / C_ext, k = C_ext"""
    s = case_sums(r_max, nquad, lam, n_r, n_i, r_m, sigma_g, dtype)
    Cs, Ce = s["C"]
    return (1 / Cs) * s["greek"], Cs / Ce, Ce


# the three small cases: (r_max, nquad, lam, n_r, n_i, r_m, sigma_g) -> N = 31, 32, 16
SMALL_CASES = {
    "n31": (1.0, 60, 0.55, 1.3, 0.001, 0.3, 2.0),
    "n32": (1.07, 49, 0.55, 1.5, 0.1, 0.3, 2.0),
    "nquad1": (0.12, 1, 0.55, 1.33, 0.0, 0.3, 2.0),
}


# the five middle cases, the same fields: (r_max, nquad, lam, n_r, n_i, r_m, sigma_g), the last two the size distribution
# LogNormal(log r_m, log sigma_g), and the N_max each r_max is chosen for (MID_N_MAX; tests/test_oracle_pcw.py asserts it).  By what
# they reach in csrc/mom_pcw.hip, Np = N_max rounded up to 16:
#   n33_r64    Np = 48: macro tiles of 32 rows hold rows of two planes, a plane's last tile has one live row; 64 radii: no padding
#   n48_r100   Np = 48 = N_max: the same with full planes; 100 radii: the second trip of k_pcw_diag's loop over the radii
#   n49_r7     Np = 64; fewer radii than one chunk of 16; n_i = 0
#   n112_r650  Np = 112 = 7 x 16, 105 macro tiles, G = 39 < 41 chunks: two chunk groups take a second chunk, the largest radii
#   n300_r40   Np = 304 = 19 x 16; a lane of k_pcw_sums takes a second order n = tid + 257 (stored: tests/golden/pcw_n300.npz)
# The distributions sit at 0.6 .. 0.75 r_max and are narrow, so that the largest radii and the highest orders carry weight.
MID_CASES = {
    "n33_r64": (1.1716, 64, 0.55, 1.45, 0.01, 0.6 * 1.1716, 1.5),
    "n48_r100": (2.2761, 100, 0.55, 1.33, 0.005, 0.6 * 2.2761, 1.3),
    "n49_r7": (2.352, 7, 0.55, 1.5, 0.0, 0.6 * 2.352, 1.5),
    "n112_r650": (7.3745, 650, 0.55, 1.4, 0.002, 0.75 * 7.3745, 1.2),
    "n300_r40": (23.1109, 40, 0.55, 1.33, 0.005, 0.75 * 23.1109, 1.2),
}
MID_N_MAX = {"n33_r64": 33, "n48_r100": 48, "n49_r7": 49, "n112_r650": 112, "n300_r40": 300}
COMPUTED_MID_CASES = ("n33_r64", "n48_r100", "n49_r7")   # both oracle runs are made inside the tests; the other two are stored
PAIR_MID_CASES = COMPUTED_MID_CASES + ("n112_r650",)       # the cases whose pair averages are compared

# The rule of the device comparisons (PCW accuracy; section 4): relative to the array's largest magnitude, 8 x the
# distance of the Float64 oracle to its long-double run, and not below 2^-46: for a short sum that distance is a chance value (0.3 ulp
# on C at n48_r100).
BOUND_FLOOR = 2.0 ** -46


def rule_bound(x64, diff):
    """x64: the Float64 oracle's array, diff: it minus the long-double run's -> the bound, relative to max |x64|"""
    return max(8 * float(np.abs(diff).max()) / float(np.abs(x64).max()), BOUND_FLOOR)


def case_inputs(case, dtype=np.float64):
    """-> r, wx, N_max of a case: what the device calls take (mom_mie_pcw, mom_pcw_pair_averages)"""
    r_max, nquad, lam, _, _, r_m, sigma_g = {**SMALL_CASES, **MID_CASES}[case]
    r, wr = mo.gauleg_norm(nquad, 0, r_max, dtype)
    return r, mo.weights_wx(r, wr, r_m, sigma_g), int(mo.n_max_of(np.float64(2 * np.pi * float(r_max) / float(lam))))


def stored_case(case):
    """-> the arrays of tests/golden/pcw_n300.npz or pcw_n112.npz (make_golden.pcw_mid)"""
    return np.load(GOLDEN_DIR / ("pcw_" + case.split("_")[0] + ".npz"))


@lru_cache(maxsize=None)
def mid_reference(case):
    """What the device is compared with, once per process and to be left unchanged: r, wx, N; the Float64 oracle's greek, C and
    pairs on these inputs; d_greek [6, 2 N - 1] and d_C [2], its differences to the long-double oracle on the same (Float64) inputs;
    d_pairs [4], the largest such difference of each pair matrix.  Both runs are made here for the three cases where they take
    under a second.  n112_r650: the long-double run (7 s) is stored, the Float64 pair averages are formed here.  n300_r40 (23 s and
    97 s): both are stored, pairs is None."""
    r_max, _, lam, n_r, n_i, _, _ = MID_CASES[case]
    r, wx, N = case_inputs(case)
    if case in COMPUTED_MID_CASES:
        o64 = pcw_sums(r, wx, lam, n_r, n_i, r_max)
        o80 = pcw_sums(r.astype(np.longdouble), wx.astype(np.longdouble), lam, n_r, n_i, r_max)
        assert o64["N"] == o80["N"] == N
        return dict(r=r, wx=wx, N=N, greek=o64["greek"], C=o64["C"], pairs=o64["pairs"],
                    d_greek=(o64["greek"] - o80["greek"]).astype(np.float64), d_C=(o64["C"] - o80["C"]).astype(np.float64),
                    d_pairs=np.array([float(np.abs(a - b).max()) for a, b in zip(o64["pairs"], o80["pairs"])]))
    z = stored_case(case)
    assert np.array_equal(z["r"], r) and np.array_equal(z["wx"], wx) and int(z["params"][-1]) == N
    out = dict(r=r, wx=wx, N=N, greek=z["greek"], C=z["C"], pairs=None, d_greek=z["d_greek"], d_C=z["d_C"], d_pairs=None)
    if case == "n112_r650":
        ar, ai, br, bi, n_max_i = mo.mie_ab(2 * np.pi / np.float64(lam) * r, n_r, n_i, np.float64, n_rows=N)
        out.update(pairs=pair_averages(ar + 1j * ai, br + 1j * bi, wx, n_max_i), d_pairs=z["d_pairs"])
    return out


# ---- the symbols at the limit of mom_wigner_tables (n_max + l_max = 1900) --------------------------------------------------------

def wigner_column(n, l):
    """One (n, l) column of compute_wigner_values above, l the degree (the tables' third index minus one), as a scalar Float64
    walk: the same statements on numpy scalars, the integers Python's.  -> {m: (A, B)} for max(|n - l|, 1) <= m <= n + l.  The array
    form at (12, 950, 950) is 1900 steps on 950 x 950 arrays, minutes; tests/test_oracle_pcw.py holds the two forms bitwise equal."""
    f, sq = np.float64, np.sqrt
    s = f((-1) ** (l % 2)) * sq(f((l + 1) * (l + 2)) / f((2 * l + 1) * (2 * l + 2) * (2 * l + 3)))
    for nn in range(2, n + 1):
        s = -s * sq(f(nn * (2 * nn - 1) * ((nn + l) ** 2 - 1)) / f((nn + l) * (2 * (nn + l) + 1) * (nn * nn - 1)))

    def D(k):
        return (1 / f(k)) * sq(f((k * k - 1) * (k * k - (l - n) ** 2) * ((n + l + 1) ** 2 - k * k)))

    m, lo = n + l, max(abs(n - l), 1)
    a_cur, a_up, d_up = s, f(0), D(m + 1)
    w_same = (a_cur * 2) * sq(f((n + l) * (n + l + 1) * n * (n + 1))) / f(l * (l + 1) - (l + n) * (l + n + 1) - n * (n + 1))
    fac = np.power(np.array([f(max((l - 1) * l * (l + 1) * (l + 2), 1))]), f(-0.5))[0] if l >= 2 else f(0)
    out = {}
    for t in range(n + l - lo + 1):
        if t > 0:
            k = m + 1
            d_k = D(k)
            M_k = 1 - f(n * (n + 1) - l * (l + 1)) / f(k * (k + 1))
            a_new = (1 / d_k) * (M_k * f(2 * m + 3) * a_cur - d_up * a_up)
            a_up, a_cur, d_up = a_cur, a_new, d_k
            if t % 2 == 0:
                w_same = -w_same * sq(f((m + 2) ** 2 - (n - l) ** 2) / f((m + 1) ** 2 - (n - l) ** 2)) * \
                    sq((1 - (1 / f(n + l - m))) * (1 + (1 / f(m + n + l + 2))))
        w = w_same if t % 2 == 0 else f(0)
        sg = 1 - 2 * ((m + n + l) % 2)
        b = (f(sg) * fac) * (f(m * (m + 1) + sg * n * (n + 1)) * a_cur + (2 * sq(f(m * (m + 1) * n * (n + 1)))) * w)
        out[m] = (float(a_cur), float(b) if l >= 2 else 0.0)
        m -= 1
    return out


LIMIT_TABLE = (12, 950, 950)


def limit_samples(count=60, seed=19570104):
    """(m, n, l), 1-based as the tables are indexed, of the table LIMIT_TABLE: `count` seeded entries inside the triangle with
    n + (l - 1) >= 1700, then every entry of the eight columns next to n = l = 950 (the 3 x 3 corner without (948, 948))"""
    m_max, n_max, l_max = LIMIT_TABLE
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        n, d = int(rng.integers(n_max - 99, n_max + 1)), int(rng.integers(-m_max, m_max + 1))
        m, l = int(rng.integers(max(abs(d), 1), m_max + 1)), n - d + 1
        if 1 <= l <= l_max and n + l - 1 >= 1700 and (m, n, l) not in out:
            out.append((m, n, l))
    for n in range(n_max - 2, n_max + 1):
        for l in range(l_max - 2, l_max + 1):
            if (n, l) != (n_max - 2, l_max - 2):
                out += [(m, n, l) for m in range(max(abs(n - (l - 1)), 1), m_max + 1)]
    return out


@lru_cache(maxsize=None)
def limit_exact():
    """-> the samples and their exact symbols, arrays [len(samples)]"""
    s = limit_samples()
    return s, np.array([wigner_A_exact(*e) for e in s]), np.array([wigner_B_exact(*e) for e in s])
