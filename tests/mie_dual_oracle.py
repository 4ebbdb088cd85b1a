"""Forward-mode twin of tests/mie_oracle.py for the partials with respect to the refractive index (n_r, n_i), and a complex-step
twin of truncate_phase (numpy, own text).

Every real quantity that depends on m = n_r + i n_i is a `Dual`: a value and TWO independent real partials (d/dn_r, d/dn_i), carried
through the statements of mie_oracle.mie_ab and mie_oracle.nai2_sums with the sum, product and quotient rules, as ForwardDiff
carries them through the reference (src/Scattering/phase_function_autodiff.jl:41-95).  The twin knows nothing of the Cauchy-Riemann
relations, so that it can test the device kernel, which carries one complex derivative d/dm and relies on them.  n_max and the
start of the downward recurrence are integers taken on the values (round(Int, ::Dual) takes the value).  The value parts are
computed by the same operations in the same order as mie_oracle's and are bitwise equal to them.

Nothing here is imported by the product."""
import numpy as np

import mie_oracle as mo


class Dual:
    """value v [...] and partials d [2, ...] (d/dn_r, d/dn_i)"""
    __slots__ = ("v", "d")
    __array_ufunc__ = None      # ndarray op Dual defers to the reflected methods below

    def __init__(self, v, d=None):
        self.v = np.asarray(v)
        self.d = np.zeros((2,) + self.v.shape, self.v.dtype) if d is None else d

    def __neg__(self):
        return Dual(-self.v, -self.d)

    def __add__(self, o):
        return Dual(self.v + o.v, self.d + o.d) if isinstance(o, Dual) else Dual(self.v + o, self.d + 0 * np.asarray(o))

    __radd__ = __add__

    def __sub__(self, o):
        return Dual(self.v - o.v, self.d - o.d) if isinstance(o, Dual) else Dual(self.v - o, self.d - 0 * np.asarray(o))

    def __rsub__(self, o):
        return Dual(o - self.v, 0 * np.asarray(o) - self.d)

    def __mul__(self, o):
        if isinstance(o, Dual):
            return Dual(self.v * o.v, self.d * o.v + self.v * o.d)
        return Dual(self.v * o, self.d * o)

    __rmul__ = __mul__

    def __truediv__(self, o):
        if isinstance(o, Dual):
            q = self.v / o.v
            return Dual(q, (self.d - q * o.d) / o.v)
        return Dual(self.v / o, self.d / o)

    def __rtruediv__(self, o):
        q = o / self.v
        return Dual(q, -(q * self.d) / self.v)


def where(mask, a, b):
    return Dual(np.where(mask, a.v, b.v), np.where(mask, a.d, b.d))


def mie_ab_dual(x, n_r, n_i, dtype=np.float64, n_rows=None):
    """mie_oracle.mie_ab with Duals -> (a_re, a_im, b_re, b_im) as Duals, v [n_rows, len(x)] and d [2, n_rows, len(x)], and n_max"""
    x = np.atleast_1d(np.asarray(x, dtype=dtype))
    one, zero = np.ones(x.size, dtype), np.zeros(x.size, dtype)
    mr, mi = Dual(np.full(x.size, dtype(n_r)), np.stack([one, zero])), Dual(np.full(x.size, dtype(n_i)), np.stack([zero, one]))
    nmax = mo.n_max_of(x)
    nmx = mo.nmx_of(x, nmax, float(n_r), float(n_i))
    rows = int(nmax.max()) if n_rows is None else int(n_rows)
    assert rows >= nmax.max()
    yr, yi = x * mr, x * mi
    y2 = yr * yr + yi * yi
    iyr, iyi = yr / y2, -yi / y2
    shape = (rows, x.size)
    Dr, Di = Dual(np.zeros(shape, dtype)), Dual(np.zeros(shape, dtype))
    dr, di = Dual(np.zeros(x.size, dtype)), Dual(np.zeros(x.size, dtype))
    for n in range(int(nmx.max()) - 1, 0, -1):
        live = n <= nmx - 1
        c = dtype(n + 1)
        qr, qi = c * iyr, c * iyi
        sr, si = dr + qr, di + qi
        s2 = sr * sr + si * si
        dr = where(live, qr - sr / s2, dr)
        di = where(live, qi + si / s2, di)
        if n <= rows:
            Dr.v[n - 1], Di.v[n - 1] = dr.v, di.v
            Dr.d[:, n - 1], Di.d[:, n - 1] = dr.d, di.d
    m2 = mr * mr + mi * mi
    psi0, psi1 = np.cos(x), np.sin(x)
    chi0, chi1 = -psi1, psi0
    out = [Dual(np.zeros(shape, dtype)) for _ in range(4)]
    for n in range(1, int(nmax.max()) + 1):
        live = n <= nmax
        tn = dtype(2 * n - 1)
        with np.errstate(all="ignore"):
            psi, chi = tn * psi1 / x - psi0, tn * chi1 / x - chi0
        er, ei = Dual(Dr.v[n - 1], Dr.d[:, n - 1]), Dual(Di.v[n - 1], Di.d[:, n - 1])
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
            o.v[n - 1] = np.where(live, v.v, 0)
            o.d[:, n - 1] = np.where(live, v.d, 0)
        psi0, psi1, chi0, chi1 = psi1, psi, chi1, chi
    return out[0], out[1], out[2], out[3], nmax


def nai2_sums_dual(r, wx, lam, n_r, n_i, *, mu=None, w_mu=None, n_rows=None, l_max=None):
    """mie_oracle.nai2_sums with Duals, with its keyword arguments: the value entries of nai2_sums for the weight rows wx (one row,
    or up to 3 as the device call takes), and d_bulk_f [2, 4, n_mu], d_C [2, 2], d_greek [2, 6, l_max]: the partials
    (d/dn_r, d/dn_i) of row 0's sums."""
    dt = r.dtype.type
    wx = np.atleast_2d(np.asarray(wx, dtype=r.dtype))
    assert 1 <= wx.shape[0] <= 3
    k = 2 * mo.pi_of(dt) / dt(lam)
    x = k * r
    n_top = int(mo.n_max_of(np.max(x).astype(np.float64)))
    rows = n_top if n_rows is None else int(n_rows)
    ar, ai, br, bi, nmax = mie_ab_dual(x, n_r, n_i, dt, n_rows=rows)
    assert rows >= n_top and rows == ar.v.shape[0]
    if mu is None:
        assert w_mu is None
        mu, w_mu = mo.gausslegendre(2 * n_top - 1, dt)
    assert mu.dtype == r.dtype and w_mu.dtype == r.dtype and mu.shape == w_mu.shape
    p, t = mo.mie_pi_tau(mu, rows)
    l = np.arange(1, rows + 1).astype(dt)
    c = ((2 * l + 1) / (l * (l + 1)))[:, None]
    a, b = c * (ar.v + 1j * ai.v), c * (br.v + 1j * bi.v)
    S1, S2 = t @ a + p @ b, p @ a + t @ b          # [n_mu, nR]
    # the amplitudes are linear in a, b: the partials of their real and imaginary parts, each [2, n_mu, nR]
    dS1r, dS1i = t @ (c * ar.d) + p @ (c * br.d), t @ (c * ai.d) + p @ (c * bi.d)
    dS2r, dS2i = p @ (c * ar.d) + t @ (c * br.d), p @ (c * ai.d) + t @ (c * bi.d)
    h = dt(0.5) / (x * x)
    f = np.stack([h * (np.abs(S1) ** 2 + np.abs(S2) ** 2), h * (S1 * np.conj(S2) + S2 * np.conj(S1)).real,
                  -h * (np.abs(S1) ** 2 - np.abs(S2) ** 2), -h * (S1 * np.conj(S2) - S2 * np.conj(S1)).imag])
    dn1 = 2 * (S1.real * dS1r + S1.imag * dS1i)      # d |S1|^2
    dn2 = 2 * (S2.real * dS2r + S2.imag * dS2i)
    # S1 conj(S2) + S2 conj(S1) = 2 (S1r S2r + S1i S2i);  Im(S1 conj(S2) - S2 conj(S1)) = 2 (S1i S2r - S1r S2i)
    dre = 2 * (dS1r * S2.real + S1.real * dS2r + dS1i * S2.imag + S1.imag * dS2i)
    dim = 2 * (dS1i * S2.real + S1.imag * dS2r - dS1r * S2.imag - S1.real * dS2i)
    df = np.stack([h * (dn1 + dn2), h * dre, -h * (dn1 - dn2), -h * dim], axis=1)      # [2, 4, n_mu, nR]
    w2 = (2 * l + 1)[:, None]
    pre_c = 2 * mo.pi_of(dt) / k ** 2
    C_sca = pre_c * np.sum(w2 * (ar.v * ar.v + ai.v * ai.v + br.v * br.v + bi.v * bi.v), axis=0)
    C_ext = pre_c * np.sum(w2 * (ar.v + br.v), axis=0)
    dC_sca = pre_c * np.sum(w2 * (2 * (ar.v * ar.d + ai.v * ai.d + br.v * br.d + bi.v * bi.d)), axis=1)     # [2, nR]
    dC_ext = pre_c * np.sum(w2 * (ar.d + br.d), axis=1)
    C = np.stack([wx @ C_sca, wx @ C_ext], axis=1)
    d_C = np.stack([dC_sca @ wx[0], dC_ext @ wx[0]], axis=1)
    wr = 4 * mo.pi_of(dt) * r * r * wx
    bulk = np.einsum("fmi,ki->kfm", f, wr)
    d_bulk = np.einsum("cfmi,i->cfm", df, wr[0])
    l_max = mu.size if l_max is None else int(l_max)
    P, P2, R2, T2 = mo.legendre_tables(mu, l_max)
    ll = np.arange(l_max).astype(dt)
    pre = (2 * ll + 1) / 2
    fac = np.zeros(l_max, dt)
    fac[2:] = pre[2:] * np.sqrt(1 / ((ll[2:] - 1) * ll[2:] * (ll[2:] + 1) * (ll[2:] + 2)))

    def project(bk):
        f11, f33, f12, f34 = (w_mu * bk[q] for q in range(4))
        return [fac * (f11 @ R2 + f33 @ T2), pre * (f11 @ P), fac * (f12 @ P2), pre * (f33 @ P), fac * (f34 @ P2),
                fac * (f33 @ R2 + f11 @ T2)]

    greek = np.zeros((wx.shape[0], 6, l_max), dt)
    for kk in range(wx.shape[0]):
        greek[kk] = project(bulk[kk])
    d_greek = np.zeros((2, 6, l_max), dt)
    for cc in range(2):
        d_greek[cc] = project(d_bulk[cc])
    return dict(bulk_f=bulk, C=C, greek=greek, mu=mu, w_mu=w_mu, x=x, n_max=nmax, d_bulk_f=d_bulk, d_C=d_C, d_greek=d_greek)


def case_sums_dual(r_max, nquad, lam, n_r, n_i, r_m, sigma_g, dtype=np.float64):
    r, wr = mo.gauleg_norm(nquad, 0, r_max, dtype)
    wx = mo.weights_wx(r, wr, r_m, sigma_g)
    out = nai2_sums_dual(r, wx, lam, n_r, n_i)
    out.update(r=r, wx=wx)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# complex-step twin of truncate_phase(δBGE(l_tr, .), aero)
# ------------------------------------------------------------------------------------------------------------------------------

GREEK_ORDER = ("α", "β", "γ", "δ", "ϵ", "ζ")


def truncate_complex_step(l_tr, greek, d_greek, mu, w_mu, h=1e-30):
    """The three weighted fits of the δ-BGE truncation (truncate_phase.jl:95-220) restated in complex arithmetic on
    greek + i h d_greek (both [6, l_max], rows α .. ζ), at the Gauss nodes mu with weights w_mu.  Returns (value, derivative):
    two dicts with α .. ζ [l_tr] and fᵗ; the derivative is Im(.) / h, free of subtractive cancellation."""
    g = np.asarray(greek, dtype=np.float64) + 1j * h * np.asarray(d_greek, dtype=np.float64)
    L = g.shape[1]
    P, P2, _, _ = mo.legendre_tables(np.asarray(mu, dtype=np.float64), L)
    fac_full = np.zeros(L)
    for l in range(2, L):
        fac_full[l] = np.sqrt(1 / ((l - 1) * l * (l + 1) * (l + 2)))
    f11 = P @ g[1]
    f12 = P2 @ (fac_full * g[2])
    f34 = P2 @ (fac_full * g[4])

    def fit(B, f, first):
        Bf = B[:, first:] / f[:, None]
        return np.linalg.solve((w_mu[:, None] * Bf).T @ Bf, Bf.T @ (w_mu + 0j))

    fac = fac_full[:l_tr]
    cl = fit(P[:, :l_tr] + 0j, f11, 0)
    γ, ϵ = np.zeros(l_tr, complex), np.zeros(l_tr, complex)
    if l_tr > 2:
        γ[2:] = fit(fac * P2[:, :l_tr] + 0j, f12, 2)
        ϵ[2:] = fit(fac * P2[:, :l_tr] + 0j, f34, 2)
    c0 = cl[0]
    # string keys: as keyword names Python would normalise ϵ and fᵗ to other characters
    full = {"α": (g[0, :l_tr] - (g[1, :l_tr] - cl)) / c0, "β": cl / c0, "γ": γ, "δ": (g[3, :l_tr] - (g[1, :l_tr] - cl)) / c0, "ϵ": ϵ,
            "ζ": (g[5, :l_tr] - (g[1, :l_tr] - cl)) / c0, "fᵗ": 1 - c0}
    return {k: np.real(v) for k, v in full.items()}, {k: np.imag(v) / h for k, v in full.items()}
