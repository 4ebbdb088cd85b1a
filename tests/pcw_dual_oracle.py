"""CPU oracle of the Jacobian rows of the Domke-PCW route (numpy, own text, a dtype like pcw_oracle): what mom_mie_pcw_dual and
mom_pcw_pair_averages_dual are compared with.

No new algorithm.  A size row is pcw_oracle.pcw_sums on the derivative weight row: every sum is linear in w.  An index row uses
the polarisation identity: every PCW sum is a real-quadratic form F in x = (a, b) (C_ext is linear), so its exact directional
derivative along d = (da, db) is (F(x + d) - F(x - d)) / 2 -- no step, no truncation error.  d = (da / dn_r, db / dn_r) or
(da / dn_i, db / dn_i) comes from mie_dual_oracle.mie_ab_dual, which carries two independent real partials and knows nothing of the
Cauchy-Riemann relations the device kernels rely on; it goes in through the ab_edit hook of pcw_sums.  The same identity on
pair_averages gives the pair partials, without any symbol.

Nothing here is imported by the product."""
import numpy as np

import mie_dual_oracle as mdo
import mie_oracle as mo
import pcw_oracle as po


def _ab_dual(r, lam, n_r, n_i, N):
    """a, b complex [N, nR], their partials da, db complex [2, N, nR] (d/dn_r, d/dn_i) and n_max,i, in the dtype of r"""
    dt = r.dtype.type
    cdt = np.result_type(dt, np.complex64)
    x = (2 * mo.pi_of(dt) / dt(lam)) * r
    ar, ai, br, bi, n_max_i = mdo.mie_ab_dual(x, n_r, n_i, dt, n_rows=N)
    a, b = (ar.v + 1j * ai.v).astype(cdt), (br.v + 1j * bi.v).astype(cdt)
    return a, b, (ar.d + 1j * ai.d).astype(cdt), (br.d + 1j * bi.d).astype(cdt), n_max_i


def pair_averages_dual(r, w_rows, lam, n_r, n_i, N, index_rows=True):
    """-> complex [nO, 4, N, N]: per row (anam, anbm, bnam, bnbm) as pcw_oracle.pair_averages returns them; rows 0 .. nW - 1 for the
    weight rows, then (index_rows) d/dn_r and d/dn_i of row 0"""
    w_rows = np.atleast_2d(w_rows)
    a, b, da, db, n_max_i = _ab_dual(r, lam, n_r, n_i, N)
    rows = [po.pair_averages(a, b, w, n_max_i) for w in w_rows]
    if index_rows:
        for c in range(2):
            plus = po.pair_averages(a + da[c], b + db[c], w_rows[0], n_max_i)
            minus = po.pair_averages(a - da[c], b - db[c], w_rows[0], n_max_i)
            rows.append(tuple((p - m) / 2 for p, m in zip(plus, minus)))
    return np.array(rows)


def pcw_sums_dual(r, w_rows, lam, n_r, n_i, r_max, index_rows=True):
    """-> dict(greek [nO, 6, 2 N - 1], C [nO, 2], N), none divided by C_sca, rows as pair_averages_dual"""
    w_rows = np.atleast_2d(w_rows)
    runs = [po.pcw_sums(r, w, lam, n_r, n_i, r_max) for w in w_rows]
    N = runs[0]["N"]
    greek, C = [o["greek"] for o in runs], [o["C"] for o in runs]
    if index_rows:
        _, _, da, db, _ = _ab_dual(r, lam, n_r, n_i, N)
        for c in range(2):
            plus = po.pcw_sums(r, w_rows[0], lam, n_r, n_i, r_max, ab_edit=lambda a, b: (a + da[c], b + db[c]))
            minus = po.pcw_sums(r, w_rows[0], lam, n_r, n_i, r_max, ab_edit=lambda a, b: (a - da[c], b - db[c]))
            greek.append((plus["greek"] - minus["greek"]) / 2)
            C.append((plus["C"] - minus["C"]) / 2)
    return dict(greek=np.array(greek), C=np.array(C), N=N)


def normalised(greek, C):
    """The host arithmetic after the sums: greek [nO, 6, L], C [nO, 2] -> (g [nO, 6, L], omega [nO], k [nO]): row 0 the optics
    ((1 / C_sca) greek, C_sca / C_ext, C_ext), a further row the partial of them by the quotient rule"""
    Cs, Ce = C[0]
    g, om, k = [(1 / Cs) * greek[0]], [Cs / Ce], [Ce]
    for j in range(1, len(C)):
        dCs, dCe = C[j]
        g.append((1 / Cs) * greek[j] - greek[0] * dCs / Cs ** 2)
        om.append(dCs / Ce - Cs * dCe / Ce ** 2)
        k.append(dCe)
    return np.array(g), np.array(om), np.array(k)


def omega_scale(C):
    """the size of the two terms each d omega = dC_sca / C_ext - C_sca dC_ext / C_ext^2 is the difference of, per partial row: what
    a distance between two d omega is relative to (at n_i = 0 the terms cancel to zero)"""
    Cs, Ce = C[0]
    return np.array([max(abs(dCs / Ce), abs(Cs * dCe / Ce ** 2)) for dCs, dCe in C[1:]], dtype=np.float64)
