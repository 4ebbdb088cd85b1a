"""CPU oracle of the Mie / NAI-2 aerosol optics (numpy, own text): a twin of the reference's statements
(src/Scattering/compute_NAI2.jl:16-182, mie_helper_functions.jl:17-71, 154-182, 266-276, legendre_functions.jl:188-259) that takes a
dtype, so that the same text runs in np.float64 and in np.longdouble (x87 extended precision: the arbiter between the Float64
oracle and the device, the role oracle/momref_ext.c has for the RT core), and an independent route to a_n, b_n through
Bohren & Huffman eq. 4.53 with Bessel functions of half-integer order from scipy, and from mpmath where Float64 Bessel functions no
longer arbitrate (x up to 343.7).  nai2_sums takes the shapes the reference ties together (n_mu, table rows, l_max) as free arguments.

Nothing here is imported by the product; the tests feed both sides the same physical parameters."""
import numpy as np


def pi_of(dtype):
    return 4 * np.arctan(dtype(1))


def gausslegendre(n, dtype=np.float64):
    """Gauss-Legendre nodes (ascending) and weights on [-1, 1] by Newton's method on P_n in `dtype`."""
    if n == 1:
        return np.zeros(1, dtype), np.full(1, 2, dtype)

    def legendre(x):
        a, b = np.ones_like(x), x.copy()
        for l in range(2, n + 1):
            a, b = b, ((2 * l - 1) * x * b - (l - 1) * a) / l
        return b, n * (x * b - a) / (x * x - 1)

    i = np.arange(n, 0, -1).astype(dtype)
    x = np.cos(pi_of(dtype) * (i - dtype(0.25)) / (n + dtype(0.5)))
    for _ in range(30):
        p, d = legendre(x)
        step = p / d
        x = x - step
        if np.max(np.abs(step)) < 4 * np.finfo(dtype).eps:
            break
    x = (x - x[::-1]) / 2
    _, d = legendre(x)
    return x, 2 / ((1 - x * x) * d * d)


def gauleg_norm(n, xmin, xmax, dtype=np.float64):
    """gauleg(n, xmin, xmax; norm = true): weights of a mean"""
    x, w = gausslegendre(n, dtype)
    return (dtype(xmax) - dtype(xmin)) / 2 * x + (dtype(xmin) + dtype(xmax)) / 2, w / w.sum()


def n_max_of(x):
    """get_n_max; an integer, so always from the Float64 value (round: ties to even as in Julia)"""
    x = np.asarray(x, dtype=np.float64)
    return np.rint(x + 4.05 * x ** (1 / 3) + 10).astype(np.int64)


def nmx_of(x, nmax, n_r, n_i):
    x = np.asarray(x, dtype=np.float64)
    return np.rint(np.maximum(nmax, np.abs(x * (n_r - n_i))) + 51).astype(np.int64)


def mie_ab(x, n_r, n_i, dtype=np.float64, n_rows=None):
    """compute_mie_ab! for all size parameters x at once -> a, b complex-as-pairs: (a_re, a_im, b_re, b_im), each
    [n_rows, len(x)] (row n - 1 = order n, zeros above each x's own n_max), and n_max [len(x)].
    Complex numbers are carried as real and imaginary parts and u / v is u conj(v) / |v|^2, the operations in the order
    of the reference's statements: the upward psi recurrence is only conditionally stable, so the order is part of the result."""
    x = np.atleast_1d(np.asarray(x, dtype=dtype))
    mr, mi = dtype(n_r), dtype(n_i)
    nmax = n_max_of(x)
    nmx = nmx_of(x, nmax, float(n_r), float(n_i))
    rows = int(nmax.max()) if n_rows is None else int(n_rows)
    assert rows >= nmax.max()
    yr, yi = x * mr, x * mi
    y2 = yr * yr + yi * yi
    iyr, iyi = yr / y2, -yi / y2
    Dr, Di = np.zeros((rows, x.size), dtype), np.zeros((rows, x.size), dtype)
    dr, di = np.zeros(x.size, dtype), np.zeros(x.size, dtype)
    for n in range(int(nmx.max()) - 1, 0, -1):
        live = n <= nmx - 1
        c = dtype(n + 1)
        qr, qi = c * iyr, c * iyi
        sr, si = dr + qr, di + qi
        s2 = sr * sr + si * si
        dr = np.where(live, qr - sr / s2, dr)
        di = np.where(live, qi + si / s2, di)
        if n <= rows:
            Dr[n - 1], Di[n - 1] = dr, di
    m2 = mr * mr + mi * mi
    psi0, psi1 = np.cos(x), np.sin(x)
    chi0, chi1 = -psi1, psi0
    out = [np.zeros((rows, x.size), dtype) for _ in range(4)]
    for n in range(1, int(nmax.max()) + 1):
        live = n <= nmax
        tn = dtype(2 * n - 1)
        with np.errstate(all="ignore"):   # lanes above their own n_max keep running (chi overflows there) and are masked below
            psi, chi = tn * psi1 / x - psi0, tn * chi1 / x - chi0
        er, ei = Dr[n - 1], Di[n - 1]
        nx = dtype(n) / x
        tar, tai = (er * mr + ei * mi) / m2 + nx, (ei * mr - er * mi) / m2
        tbr, tbi = (er * mr - ei * mi) + nx, er * mi + ei * mr
        res = []
        with np.errstate(all="ignore"):
            for tr, ti in ((tar, tai), (tbr, tbi)):
                nr_, ni_ = tr * psi - psi1, ti * psi
                qr, qi = (tr * psi + ti * chi) - psi1, (ti * psi - tr * chi) + chi1
                q2 = qr * qr + qi * qi
                res += [(nr_ * qr + ni_ * qi) / q2, (ni_ * qr - nr_ * qi) / q2]
        for o, v in zip(out, res):
            o[n - 1] = np.where(live, v, 0)
        psi0, psi1, chi0, chi1 = psi1, psi, chi1, chi
    return out[0], out[1], out[2], out[3], nmax


def mie_ab_bessel(x, m, n_max):
    """a_n, b_n, n = 1..n_max, by Bohren & Huffman eq. 4.53 with the Riccati-Bessel functions from scipy.special.jv / yv of order
    n + 1/2 (psi_n(z) = sqrt(pi z / 2) J_{n+1/2}(z), chi_n(z) = -sqrt(pi z / 2) Y_{n+1/2}(z), xi_n = psi_n - i chi_n)."""
    from scipy.special import jv, yv
    n = np.arange(0, n_max + 1)

    def psi(z):
        return np.sqrt(np.pi * z / 2) * jv(n + 0.5, z)

    def dpsi(p, z):   # psi_n' = psi_{n-1} - n psi_n / z, n >= 1
        return p[:-1] - n[1:] * p[1:] / z

    mx = m * x
    px, pmx = psi(x), psi(mx)
    xi = px - 1j * (-np.sqrt(np.pi * x / 2) * yv(n + 0.5, x))
    dpx, dpmx, dxi = dpsi(px, x), dpsi(pmx, mx), dpsi(xi, x)
    px, pmx, xi = px[1:], pmx[1:], xi[1:]
    a = (m * pmx * dpx - px * dpmx) / (m * pmx * dxi - xi * dpmx)
    b = (pmx * dpx - m * px * dpmx) / (pmx * dxi - m * xi * dpmx)
    return a, b


def mie_ab_mp(x, m, n_max, dps=60):
    """a_n, b_n, n = 1..n_max, by Bohren & Huffman eq. 4.53 in mpmath at `dps` digits: psi_n, chi_n and xi_n = psi_n - i chi_n from
    mpmath's besselj / bessely of order n + 1/2, no recurrence over n anywhere but in the derivative f_n' = f_{n-1} - n f_n / z.
    x (a Float64) and m (a complex128) are taken exactly.  The arbiter of mie_ab where scipy's Float64 Bessel functions are not
    (large x): it shares nothing with mie_ab and nothing with Float64 arithmetic.  -> complex128 arrays a, b [n_max]"""
    import mpmath as mp
    with mp.workdps(dps):
        xx, mm = mp.mpf(float(x)), mp.mpc(complex(m))
        zz = mm * xx
        half = mp.mpf(1) / 2
        root_x, root_z = mp.sqrt(mp.pi * xx / 2), mp.sqrt(mp.pi * zz / 2)
        psi_x = [root_x * mp.besselj(n + half, xx) for n in range(n_max + 1)]
        xi_x = [psi_x[n] + mp.j * (root_x * mp.bessely(n + half, xx)) for n in range(n_max + 1)]      # chi_n = -sqrt(.) Y
        psi_z = [root_z * mp.besselj(n + half, zz) for n in range(n_max + 1)]
        a, b = [], []
        for n in range(1, n_max + 1):
            d_psi_x = psi_x[n - 1] - n * psi_x[n] / xx
            d_xi_x = xi_x[n - 1] - n * xi_x[n] / xx
            d_psi_z = psi_z[n - 1] - n * psi_z[n] / zz
            a.append(complex((mm * psi_z[n] * d_psi_x - psi_x[n] * d_psi_z) / (mm * psi_z[n] * d_xi_x - xi_x[n] * d_psi_z)))
            b.append(complex((psi_z[n] * d_psi_x - mm * psi_x[n] * d_psi_z) / (psi_z[n] * d_xi_x - mm * xi_x[n] * d_psi_z)))
    return np.array(a), np.array(b)


def mie_pi_tau(mu, nmax):
    """compute_mie_pi_tau -> pi, tau [n_mu, nmax]"""
    p, t = np.zeros((mu.size, nmax), mu.dtype), np.zeros((mu.size, nmax), mu.dtype)
    p[:, 0], t[:, 0] = 1, mu
    p[:, 1], t[:, 1] = 3 * mu, 6 * mu * mu - 3
    for n in range(2, nmax):
        p[:, n] = ((2 * n + 1) * mu * p[:, n - 1] - (n + 1) * p[:, n - 2]) / n
        t[:, n] = (n + 1) * mu * p[:, n] - (n + 2) * p[:, n - 1]
    return p, t


def legendre_tables(x, nmax):
    """compute_legendre_poly -> P, P2, R2, T2 [len(x), nmax]"""
    dt = x.dtype.type
    P, P2, R2, T2 = (np.zeros((x.size, nmax), x.dtype) for _ in range(4))
    P[:, 0] = 1
    if nmax > 1:
        P[:, 1] = x
    if nmax > 2:
        P2[:, 2] = 3 * (1 - x * x)
        R2[:, 2] = np.sqrt(dt(3) / 2) * (1 + x * x)
        T2[:, 2] = np.sqrt(dt(6)) * x
    for c in range(2, nmax):
        l = c - 1
        P[:, c] = ((2 * l + 1) * x * P[:, c - 1] - l * P[:, c - 2]) / (l + 1)
        if l >= 2:
            ia = (2 * l + 1) * x
            ib = np.sqrt(dt((l + 2) * (l - 2))) * (l + 2) / l
            ic = dt(4) * (2 * l + 1) / ((l + 1) * l)
            id_ = np.sqrt(dt((l + 3) * (l - 1))) * (l - 1) / (l + 1)
            P2[:, c] = (ia * P2[:, c - 1] - (l + 2) * P2[:, c - 2]) / (l - 1)
            R2[:, c] = (ia * R2[:, c - 1] - ib * R2[:, c - 2] - ic * T2[:, c - 1]) / id_
            T2[:, c] = (ia * T2[:, c - 1] - ib * T2[:, c - 2] - ic * R2[:, c - 1]) / id_
    return P, P2, R2, T2


def lognormal_pdf(r, mu, sigma):
    """pdf of Distributions.LogNormal(mu, sigma)"""
    dt = r.dtype.type
    z = (np.log(r) - dt(mu)) / dt(sigma)
    return np.exp(-z * z / 2) / (r * dt(sigma) * np.sqrt(2 * pi_of(dt)))


def weights_wx(r, wr, r_m, sigma_g):
    """compute_w_x for LogNormal(log(r_m), log(sigma_g))"""
    dt = r.dtype.type
    w = lognormal_pdf(r, np.log(dt(r_m)), np.log(dt(sigma_g))) * wr
    return w / w.sum()


def nai2_sums(r, wx_rows, lam, n_r, n_i, *, mu=None, w_mu=None, n_rows=None, l_max=None):
    """The sums of compute_aerosol_optical_properties for the radii r and the rows of w_x (row 0 the weights themselves, further
    rows their partials), in the dtype of r, none divided by the bulk C_sca:
       bulk_f [nW, 4, n_mu] (f11, f33, f12, f34), C [nW, 2] (C_sca, C_ext), greek [nW, 6, l_max] (alpha .. zeta), mu, w_mu
    The reference ties every shape to n_top, the n_max of the largest radius; the device call does not, so neither does this:
    mu, w_mu: nodes and weights of any length (default: the Gauss rule of 2 n_top - 1 nodes); n_rows >= n_top: rows of the pi / tau
    tables and of the coefficient planes (default n_top; the further rows multiply exact zeros); l_max: default n_mu."""
    dt = r.dtype.type
    wx_rows = np.atleast_2d(wx_rows)
    k = 2 * pi_of(dt) / dt(lam)
    x = k * r
    n_top = int(n_max_of(np.max(x).astype(np.float64)))
    rows = n_top if n_rows is None else int(n_rows)
    ar, ai, br, bi, nmax = mie_ab(x, n_r, n_i, dt, n_rows=rows)
    assert rows >= n_top and rows == ar.shape[0]
    if mu is None:
        assert w_mu is None
        mu, w_mu = gausslegendre(2 * n_top - 1, dt)
    assert mu.dtype == r.dtype and w_mu.dtype == r.dtype and mu.shape == w_mu.shape
    p, t = mie_pi_tau(mu, rows)
    l = np.arange(1, rows + 1).astype(dt)
    c = ((2 * l + 1) / (l * (l + 1)))[:, None]
    a, b = c * (ar + 1j * ai), c * (br + 1j * bi)
    S1, S2 = t @ a + p @ b, p @ a + t @ b          # [n_mu, nR]
    h = dt(0.5) / (x * x)
    f = np.stack([h * (np.abs(S1) ** 2 + np.abs(S2) ** 2), h * (S1 * np.conj(S2) + S2 * np.conj(S1)).real,
                  -h * (np.abs(S1) ** 2 - np.abs(S2) ** 2), -h * (S1 * np.conj(S2) - S2 * np.conj(S1)).imag])
    w2 = (2 * l + 1)[:, None]
    C_sca = 2 * pi_of(dt) / k ** 2 * np.sum(w2 * (ar * ar + ai * ai + br * br + bi * bi), axis=0)
    C_ext = 2 * pi_of(dt) / k ** 2 * np.sum(w2 * (ar + br), axis=0)
    C = np.stack([wx_rows @ C_sca, wx_rows @ C_ext], axis=1)
    wr = 4 * pi_of(dt) * r * r * wx_rows
    bulk = np.einsum("fmi,ki->kfm", f, wr)
    l_max = mu.size if l_max is None else int(l_max)
    P, P2, R2, T2 = legendre_tables(mu, l_max)
    ll = np.arange(l_max).astype(dt)
    pre = (2 * ll + 1) / 2
    fac = np.zeros(l_max, dt)
    fac[2:] = pre[2:] * np.sqrt(1 / ((ll[2:] - 1) * ll[2:] * (ll[2:] + 1) * (ll[2:] + 2)))
    greek = np.zeros((wx_rows.shape[0], 6, l_max), dt)
    for kk in range(wx_rows.shape[0]):
        f11, f33, f12, f34 = (w_mu * bulk[kk, q] for q in range(4))
        greek[kk] = [fac * (f11 @ R2 + f33 @ T2), pre * (f11 @ P), fac * (f12 @ P2), pre * (f33 @ P), fac * (f34 @ P2),
                     fac * (f33 @ R2 + f11 @ T2)]
    return dict(bulk_f=bulk, C=C, greek=greek, mu=mu, w_mu=w_mu, x=x, n_max=nmax)


def case_sums(r_max, nquad, lam, n_r, n_i, r_m, sigma_g, dtype=np.float64):
    """nai2_sums of a whole model: radius quadrature on [0, r_max], LogNormal(log r_m, log sigma_g); also r and w_x"""
    r, wr = gauleg_norm(nquad, 0, r_max, dtype)
    wx = weights_wx(r, wr, r_m, sigma_g)
    out = nai2_sums(r, wx, lam, n_r, n_i)
    out.update(r=r, wx=wx)
    return out


def aerosol_optics(r_max, nquad, lam, n_r, n_i, r_m, sigma_g, dtype=np.float64):
    """-> greek [6, l_max] (alpha .. zeta, normalised by the bulk C_sca), omega = C_sca / C_ext, k = C_ext"""
    s = case_sums(r_max, nquad, lam, n_r, n_i, r_m, sigma_g, dtype)
    Cs, Ce = s["C"][0]
    return s["greek"][0] / Cs, Cs / Ce, Ce


def rel_max(a, b):
    """max |a - b| relative to the largest magnitude of b"""
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
