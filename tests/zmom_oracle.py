"""The arbiter of the phase-matrix moments: oracle/momref.py::compute_Z_moments (compute_Z_matrices.jl:5-84 with
compute_associated_legendre_PRT, legendre_functions.jl:17-178) restated with every array and every scalar constant in ONE numpy
dtype, by default np.longdouble -- square roots through np.sqrt on that dtype, integer quotients formed in it.  The statements stand
in momref's order, so with dtype=np.float64 the result is bitwise momref's (test_zmoments_host.py); with the long type it is the
value the Float64 results of the host and of the device are measured against.

compute_Z_moments also returns A_abs = (A_abs++, A_abs-+): the same sums over l with every term Pi_l(mu_i)[a,b] B_l[b,c] Pi_l(mu_j)[c,d]
replaced by its absolute value, [n, n, nmu, nmu] like momref's A.  eps * max(A_abs) is the size of one rounding of the sum.

The parity rule for a (set, m) pair of matrices:  E_dev <= 4 E_host + 4 eps max(A_abs),  E = max |Z - Z_ld| over
both matrices, eps = 2^-52."""
import numpy as np

EPS = 2.0 ** -52

_prt_cache = {}


def compute_associated_legendre_PRT(mu, Lmax, dtype=np.longdouble):
    """P, R, T [len(mu), Lmax, Lmax] (index [imu, l, m]) in `dtype`, T sign-flipped as the reference returns it"""
    D = dtype
    sqrt = lambda x: np.sqrt(D(x))
    mu = np.asarray(mu, dtype=np.float64).astype(D)
    n = len(mu)
    P = np.zeros((n, Lmax, Lmax), dtype=D)
    R = np.zeros((n, Lmax, Lmax), dtype=D)
    T = np.zeros((n, Lmax, Lmax), dtype=D)
    smu = np.sqrt(D(1.0) - mu ** 2)
    cmu = mu
    for m in range(Lmax):
        for l in range(m, Lmax):
            if m == 0:
                if l == 0:
                    P[:, l, m] = 1
                elif l == 1:
                    P[:, l, m] = cmu
                elif l == 2:
                    P[:, l, m] = D(0.5) * (D(3.0) * cmu * cmu - D(1.0))
                    R[:, l, m] = D(0.5) * sqrt(1.5) * smu * smu
                else:
                    P[:, l, m] = (P[:, l - 1, m] * D(2 * l - 1) * cmu - P[:, l - 2, m] * D(l - 1)) / D(l)
                    Y = sqrt((l + 1) * (l - 3))
                    X = sqrt(l * l - 4)
                    R[:, l, m] = (R[:, l - 1, m] * D(2 * l - 1) * cmu - R[:, l - 2, m] * Y) / X
            elif m == 1:
                if l == 1:
                    P[:, l, m] = sqrt(0.5) * smu
                elif l == 2:
                    m1 = np.sqrt(D(1) / D(6))
                    cA = D(3) * cmu * smu
                    cB = sqrt(1.5) * smu
                    P[:, l, m] = m1 * cA
                    R[:, l, m] = -m1 * cmu * cB
                    T[:, l, m] = m1 * cB
                else:
                    m1 = np.sqrt(D(l - 1) / D(l + 1))
                    m2 = m1 * np.sqrt(D(l - 2) / D(l))
                    Y = D(l - 1 + m)
                    X = D(l - m)
                    P[:, l, m] = (m1 * P[:, l - 1, m] * D(2 * l - 1) * cmu - m2 * P[:, l - 2, m] * Y) / X
                    Z = D(2 * m * (2 * l - 1)) / D(l * (l - 1))
                    Y = (D(l + m - 1) / D(l - 1)) * sqrt((l - 3) * (l + 1))
                    X = (D(l - m) / D(l)) * sqrt(l * l - 4)
                    R[:, l, m] = (m1 * R[:, l - 1, m] * D(2 * l - 1) * cmu - m2 * R[:, l - 2, m] * Y
                                  + m1 * T[:, l - 1, m] * Z) / X
                    T[:, l, m] = (m1 * T[:, l - 1, m] * D(2 * l - 1) * cmu - m2 * T[:, l - 2, m] * Y
                                  + m1 * R[:, l - 1, m] * Z) / X
            else:
                if l == m:
                    fact1 = np.ones(n, dtype=D)
                    fact2 = np.ones(n, dtype=D)
                    sfull = smu
                    shalf = sfull / D(2)
                    for i in range(1, m + 1):
                        fact1 = fact1 * (D(2 * i - 1) * sfull) / sqrt(i * (i + m))
                        if i > 2:
                            fact2 = fact2 * shalf * np.sqrt(D(m + i) / D(i - 2))
                        else:
                            fact2 = fact2 * shalf
                    big = smu > D(1e-8)
                    safe = np.where(big, smu, D(1.0))
                    edge = D(0.5) if m == 2 else D(0.0)
                    Aii = np.where(big, fact2 * (D(1.0) + cmu * cmu) / (safe * safe), edge)
                    Aij = np.where(big, fact2 * (D(2) * cmu) / (safe * safe), edge)
                    P[:, l, m] = fact1
                    R[:, l, m] = Aii
                    T[:, l, m] = -Aij
                elif l == m + 1:
                    m1 = np.sqrt(D(1) / D(l + m))
                    X = D(l - m)
                    P[:, l, m] = (m1 * P[:, l - 1, m] * D(2 * l - 1) * cmu) / X
                    Z = D(2 * m * (2 * l - 1)) / D(l * (l - 1))
                    X = (D(l - m) / D(l)) * sqrt(l * l - 4)
                    R[:, l, m] = (m1 * R[:, l - 1, m] * D(2 * l - 1) * cmu + m1 * T[:, l - 1, m] * Z) / X
                    T[:, l, m] = (m1 * T[:, l - 1, m] * D(2 * l - 1) * cmu + m1 * R[:, l - 1, m] * Z) / X
                else:
                    m1 = np.sqrt(D(l - m) / D(l + m))
                    m2 = m1 * np.sqrt(D(l - m - 1) / D(l + m - 1))
                    Y = D(l - 1 + m)
                    X = D(l - m)
                    P[:, l, m] = (m1 * P[:, l - 1, m] * D(2 * l - 1) * cmu - m2 * P[:, l - 2, m] * Y) / X
                    Z = D(2 * m * (2 * l - 1)) / D(l * (l - 1))
                    Y = (D(l + m - 1) / D(l - 1)) * sqrt((l - 3) * (l + 1))
                    X = (D(l - m) / D(l)) * sqrt(l * l - 4)
                    R[:, l, m] = (m1 * R[:, l - 1, m] * D(2 * l - 1) * cmu - m2 * R[:, l - 2, m] * Y
                                  + m1 * T[:, l - 1, m] * Z) / X
                    T[:, l, m] = (m1 * T[:, l - 1, m] * D(2 * l - 1) * cmu - m2 * T[:, l - 2, m] * Y
                                  + m1 * R[:, l - 1, m] * Z) / X
    return P, R, -T


def _prt(mu, Lmax, dtype):
    """both signs of mu, computed once per (mu, Lmax, dtype): a test asks for many (set, m) pairs on one grid"""
    key = (np.asarray(mu, dtype=np.float64).tobytes(), int(Lmax), np.dtype(dtype).name)
    if key not in _prt_cache:
        _prt_cache[key] = (compute_associated_legendre_PRT(mu, Lmax, dtype),
                           compute_associated_legendre_PRT(-np.asarray(mu, dtype=np.float64), Lmax, dtype))
    return _prt_cache[key]


def _Pi_matrices(n, P, R, T, l, m, dtype):
    nmu = P.shape[0]
    Pi = np.zeros((nmu, n, n), dtype=dtype)
    Pi[:, 0, 0] = P[:, l, m]
    if n >= 3:
        Pi[:, 1, 1] = R[:, l, m]
        Pi[:, 1, 2] = -T[:, l, m]
        Pi[:, 2, 1] = -T[:, l, m]
        Pi[:, 2, 2] = R[:, l, m]
    if n == 4:
        Pi[:, 3, 3] = P[:, l, m]
    return Pi


def _B_matrix(n, g, l, dtype):
    """g: the six rows alpha, beta, gamma, delta, epsilon, zeta"""
    al, be, ga, de, ep, ze = (np.asarray(r, dtype=np.float64).astype(dtype) for r in g)
    z = dtype(0)
    if n == 1:
        return np.array([[be[l]]], dtype=dtype)
    if n == 3:
        return np.array([[be[l], ga[l], z], [ga[l], al[l], z], [z, z, ze[l]]], dtype=dtype)
    return np.array([[be[l], ga[l], z, z], [ga[l], al[l], z, z], [z, z, ze[l], ep[l]], [z, z, -ep[l], de[l]]], dtype=dtype)


def compute_Z_moments(nStokes, mu, greek_rows, m, dtype=np.longdouble):
    """greek_rows = (alpha, beta, gamma, delta, epsilon, zeta).  Returns Zpp, Zmp [N, N] (row i, column j) and (A_abs++, A_abs-+)."""
    D = dtype
    mu = np.asarray(mu, dtype=np.float64)
    assert np.all((0 < mu) & (mu <= 1)), "all mu within compute_Z_moments have to be in ]0,1]"
    n = len(mu)
    fact = D(0.5) if m == 0 else D(1.0)
    l_max = len(greek_rows[1])
    (P, R, T), (Pm, Rm, Tm) = _prt(mu, l_max, D)
    B = nStokes
    App = np.zeros((B, B, n, n), dtype=D)
    Amp = np.zeros((B, B, n, n), dtype=D)
    Bpp = np.zeros((B, B, n, n), dtype=D)
    Bmp = np.zeros((B, B, n, n), dtype=D)
    for l in range(m, l_max):
        Bl = _B_matrix(B, greek_rows, l, D)
        Pi = _Pi_matrices(B, P, R, T, l, m, D)
        Pim = _Pi_matrices(B, Pm, Rm, Tm, l, m, D)
        left = np.einsum("iab,bc->iac", Pi, Bl)
        App += np.einsum("iac,jcd->adij", left, Pi)
        Amp += np.einsum("iac,jcd->adij", left, Pim)
        aleft = np.einsum("iab,bc->iac", np.abs(Pi), np.abs(Bl))
        Bpp += np.einsum("iac,jcd->adij", aleft, np.abs(Pi))
        Bmp += np.einsum("iac,jcd->adij", aleft, np.abs(Pim))
    N = B * n
    Zpp = np.zeros((N, N), dtype=D)
    Zmp = np.zeros((N, N), dtype=D)
    for i in range(B):
        for j in range(B):
            sgn = D(1.0)
            if (i <= 1 and j >= 2) or (i >= 2 and j <= 1):
                sgn = D(-1.0)
            Zpp[i::B, j::B] = D(2) * fact * App[i, j]
            Zmp[i::B, j::B] = sgn * D(2) * fact * Amp[i, j]
    return Zpp, Zmp, (Bpp, Bmp)


def parity(nStokes, mu, greek_rows, m, Z_host, Z_dev):
    """(E_host, E_dev, eps max A_abs, max |Z_ld|) of one (set, m): Z_host, Z_dev = (Zpp, Zmp) in Float64"""
    Zp, Zm, (Ap, Am) = compute_Z_moments(nStokes, mu, greek_rows, m)
    err = lambda Z: float(max(np.max(np.abs(np.asarray(Z[0]).astype(np.longdouble) - Zp)),
                              np.max(np.abs(np.asarray(Z[1]).astype(np.longdouble) - Zm))))
    a_abs = float(max(Ap.max(), Am.max()))
    return err(Z_host), err(Z_dev), EPS * a_abs, float(max(np.max(np.abs(Zp)), np.max(np.abs(Zm))))


def holds(e_host, e_dev, eps_a):
    return e_dev <= 4.0 * e_host + 4.0 * eps_a
