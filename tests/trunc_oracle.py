"""Extended-precision arbiter of the δ-BGE truncation (numpy longdouble, own text): truncate_phase(mod::δBGE, aero)
(src/Scattering/truncate_phase.jl:95-220) with its forward-mode partials, from Float64 Greek coefficients.  Everything after the
coefficients runs in `dtype`: the Gauss nodes (mie_oracle.gausslegendre), the tables (mie_oracle.legendre_tables), the
reconstruction of f₁₁, f₁₂, f₃₄ over all terms, the normal equations of the three fits over all nodes, a Gauss-Jordan elimination
with partial pivoting, A ∂c = ∂b - ∂A c, and the quotient rules.  It stands between the host's numpy truncate_phase and the device
call (the role mie_oracle has for the Mie sums in longdouble).

Nothing here is imported by the product."""
import numpy as np

import mie_oracle as mo

ROWS = ("α", "β", "γ", "δ", "ϵ", "ζ")
FIT_OF_ROW = (0, 0, 1, 0, 2, 0)   # the fit whose normal matrix feeds each Greek row (c₀: fit 0)


def gauss_jordan(A, B):
    """A⁻¹ B by Gauss-Jordan elimination with partial pivoting, in the dtype of A.  B [n, k]."""
    n = A.shape[0]
    M = np.concatenate([A, B], axis=1).copy()
    for j in range(n):
        p = j + int(np.argmax(np.abs(M[j:, j])))
        if M[p, j] == 0:
            raise np.linalg.LinAlgError("singular matrix")
        if p != j:
            M[[j, p]] = M[[p, j]]
        M[j] = M[j] / M[j, j]
        rows = np.arange(n) != j
        M[rows] = M[rows] - M[rows, j][:, None] * M[j][None, :]
    return M[:, n:]


def _fit(w, B, f, dfs):
    """c and [∂c] of one weighted fit: A = Bᵀ diag(w / f²) B, b = Bᵀ (w / f); ∂A = Bᵀ diag(-2 w ∂f / f³) B, ∂b = Bᵀ (-w ∂f / f²).
    Also the 2-norm condition number of A (formed in Float64 from the rounded matrix)."""
    A = B.T @ ((w / (f * f))[:, None] * B)
    b = B.T @ (w / f)
    c = gauss_jordan(A, b[:, None])[:, 0]
    dcs = []
    for df in dfs:
        dA = B.T @ ((-2 * w * df / (f * f * f))[:, None] * B)
        db = B.T @ (-w * df / (f * f))
        dcs.append(gauss_jordan(A, (db - dA @ c)[:, None])[:, 0])
    return c, dcs, float(np.linalg.cond(A.astype(np.float64)))


def truncate(l_tr, greek, d_greeks=(), n_mu=None, dtype=np.longdouble):
    """greek [6, l_full] (rows α .. ζ, Float64) and derivative sets d_greeks [nP, 6, l_full] truncated to l_tr terms on the n_mu
    Gauss-Legendre nodes of `dtype` (default l_full, as the reference takes them).  Returns dict(greek [1 + nP, 6, l_tr], c0 [1 + nP],
    kappa [3]): row 0 the truncated set, rows 1 .. nP its partials along each derivative set; fᵗ = 1 - c0[0], ∂fᵗ = -c0[1:];
    kappa: the condition numbers of the normal matrices of the β, γ, ϵ fits (1 for a fit that does not exist, l_tr <= 2)."""
    g = np.asarray(greek, dtype=np.float64).astype(dtype)
    dg = np.asarray(d_greeks, dtype=np.float64).astype(dtype).reshape(-1, 6, g.shape[1])
    l_full, nP = g.shape[1], dg.shape[0]
    μ, w = mo.gausslegendre(l_full if n_mu is None else int(n_mu), dtype)
    P, P2, _, _ = mo.legendre_tables(μ, l_full)
    l = np.arange(l_full).astype(dtype)
    fac = np.zeros(l_full, dtype)
    fac[2:] = np.sqrt(1 / ((l[2:] - 1) * l[2:] * (l[2:] + 1) * (l[2:] + 2)))
    phase = lambda s: (P @ s[1], P2 @ (fac * s[2]), P2 @ (fac * s[4]))   # f₁₁, f₁₂, f₃₄
    f, dfs = phase(g), [phase(d) for d in dg]
    out = np.zeros((1 + nP, 6, l_tr), dtype)
    κ = [1.0, 1.0, 1.0]
    cl, dcl, κ[0] = _fit(w, P[:, :l_tr], f[0], [d[0] for d in dfs])
    if l_tr > 2:
        B2 = fac[2:l_tr] * P2[:, 2:l_tr]
        for q, row in ((1, 2), (2, 4)):
            c, dc, κ[q] = _fit(w, B2, f[q], [d[q] for d in dfs])
            out[0, row, 2:] = c
            for j in range(nP):
                out[1 + j, row, 2:] = dc[j]
    c0 = cl[0]
    out[0, 1] = cl / c0
    for row in (0, 3, 5):
        out[0, row] = (g[row, :l_tr] - (g[1, :l_tr] - cl)) / c0
    c0s = np.zeros(1 + nP, dtype)
    c0s[0] = c0
    for j in range(nP):
        dc, dc0 = dcl[j], dcl[j][0]
        c0s[1 + j] = dc0
        out[1 + j, 1] = dc / c0 - cl * dc0 / c0 ** 2
        for row in (0, 3, 5):
            out[1 + j, row] = (dg[j, row, :l_tr] - (dg[j, 1, :l_tr] - dc)) / c0 - (g[row, :l_tr] - (g[1, :l_tr] - cl)) * dc0 / c0 ** 2
    return dict(greek=out, c0=c0s, kappa=np.array(κ))
