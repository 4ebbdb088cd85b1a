"""Greek sets, derivative sets and the acceptance rule of the δ-BGE truncation tests (test_oracle_truncate.py on the host,
test_gpu_truncate.py on the device).  Everything is computed once per process and shared read-only.

The rule, for every output field (a Greek row or c₀; the value or one partial), relative to the field's largest magnitude:
    allowed = max(8 d_host, 4 κ_q 2⁻⁵², 2⁻⁴⁶)
d_host: the distance of the host's numpy truncate_phase to the longdouble arbiter (trunc_oracle) for that field; κ_q: the 2-norm
condition number of the normal matrix that feeds the field (β fit for α, β, δ, ζ, c₀; f₁₂ fit for γ; f₃₄ fit for ϵ).  An entry
that is an exact zero on the host (γᵗ, ϵᵗ at l < 2) has to be an exact zero.  allowed <= 1e-7 for every field, or the rule would
hide a failure: CAP.
One field has no magnitude of its own: at l_tr = 1, βᵗ = cl / c₀ is the constant 1 and its partial ∂c₀ / c₀ - c₀ ∂c₀ / c₀² is zero in
exact arithmetic (and rounding noise in the arbiter) but the difference of two rounded terms of magnitude |∂c₀ / c₀| in Float64.  Its distance is taken relative to that
magnitude (from the arbiter), under the same rule.  Every other field that is all zero in the arbiter has to be all zero."""
import functools

import numpy as np

import mie_dual_oracle as md
import trunc_oracle as to

CASES = {"case2": (1.0, 37, 0.55, 1.3, 0.001, 0.3, 1.6), "absorbing": (0.5, 20, 0.76, 1.5, 0.1, 0.3, 1.6),
         "bigger": (5.0, 300, 0.76, 1.3, 1e-8, 0.3, 1.6)}
L_FULL = {"case2": 61, "absorbing": 41, "bigger": 129}
OTHER = {"case2": "absorbing", "absorbing": "bigger", "bigger": "case2"}   # whose set the third direction points to
EPS, FLOOR, CAP = 2.0 ** -52, 2.0 ** -46, 1e-7
FIELDS = to.ROWS + ("c₀",)


def _pad(a, L):
    out = np.zeros(a.shape[:-1] + (L,))
    n = min(L, a.shape[-1])
    out[..., :n] = a[..., :n]
    return out


@functools.lru_cache(maxsize=None)
def _sums(case):
    s = md.case_sums_dual(*CASES[case])
    g, d = np.ascontiguousarray(s["greek"][0], dtype=np.float64), np.ascontiguousarray(s["d_greek"], dtype=np.float64)
    assert g.shape == (6, L_FULL[case]), g.shape
    return g, d


@functools.lru_cache(maxsize=None)
def greek_set(case, l_full=None):
    """(greek [6, l_full], d_greek [4, 6, l_full]) of a case, zero-padded (or cut) to l_full: the oracle's sums as they are (not
    divided by the bulk C_sca: the truncation is homogeneous in the set, and β₀ then has a derivative, so ∂c₀ is no rounding noise),
    their ∂/∂nᵣ and ∂/∂nᵢ, another case's set minus this one, and a seeded random direction of 1e-3 of each coefficient."""
    g, d = _sums(case)
    L = g.shape[1] if l_full is None else l_full
    g, d = _pad(g, L), _pad(d, L)
    rng = np.random.default_rng(sorted(CASES).index(case) + 7)
    rnd = 1e-3 * g * rng.standard_normal(g.shape)
    dirs = np.concatenate([d, [_pad(_sums(OTHER[case])[0], L) - g, rnd]])
    for a in (g, dirs):
        a.setflags(write=False)
    return g, dirs


def optics(rtamd, g):
    return rtamd.corert.AerosolOptics(greek_coefs=rtamd.corert.GreekCoefs(*(np.array(r) for r in g)), ω̃=0.9, fᵗ=0.0, k=2.0)


def stack(o):
    g = o.greek_coefs
    return np.array([g.α, g.β, g.γ, g.δ, g.ϵ, g.ζ])


def host_arrays(rtamd, l_tr, g, dirs, n_mu=None):
    """The host's numpy truncate_phase as (greek [1 + nP, 6, l_tr], c0 [1 + nP]); n_mu != l_full: on gausslegendre(n_mu), which
    truncate_phase takes through the module's name."""
    sc = rtamd.scattering
    real = sc.gausslegendre
    if n_mu is not None:
        sc.gausslegendre = lambda n: real(n_mu)
    try:
        res = sc.truncate_phase(sc.δBGE(l_tr, 2.0), optics(rtamd, g), [optics(rtamd, d) for d in dirs])
    finally:
        sc.gausslegendre = real
    return from_optics(res)


def from_optics(res):
    """(truncated, [partials]) of truncate_phase as the arrays above"""
    val, parts = res
    return (np.array([stack(val)] + [stack(p) for p in parts]), np.array([1.0 - val.fᵗ] + [-p.fᵗ for p in parts]))


@functools.lru_cache(maxsize=None)
def arbiter(case, l_tr, nP, l_full=None, n_mu=None):
    g, dirs = greek_set(case, l_full)
    return to.truncate(l_tr, g, dirs[:nP], n_mu=n_mu)


def distances(got_greek, got_c0, ref):
    """{(row of the Dual, field): distance to the arbiter relative to the field's largest magnitude}; a field that is all zero in
    the arbiter has distance 0.0 when it is all zero here and inf otherwise (∂βᵗ at l_tr = 1: relative to |∂c₀ / c₀|, see above)"""
    out = {}
    for r in range(ref["greek"].shape[0]):
        for q, name in enumerate(FIELDS):
            a = np.asarray(got_greek[r, q] if q < 6 else got_c0[r:r + 1], dtype=np.longdouble)
            b = ref["greek"][r, q] if q < 6 else ref["c0"][r:r + 1]
            top = float(np.max(np.abs(b)))
            if name == "β" and r > 0 and ref["greek"].shape[2] == 1:
                top = float(abs(ref["c0"][r] / ref["c0"][0]))
            out[(r, name)] = (float(np.max(np.abs(a - b))) / top) if top > 0 else (0.0 if not np.any(a) else np.inf)
    return out


def allowed(d_host, ref):
    κ = ref["kappa"]
    return {k: max(8.0 * d, 4.0 * float(κ[to.FIT_OF_ROW[FIELDS.index(k[1])] if k[1] != "c₀" else 0]) * EPS, FLOOR) for k, d in d_host.items()}


def assert_exact_zeros(got_greek, l_tr):
    """γᵗ and ϵᵗ below degree 2 (every entry when l_tr <= 2), value and partials: exact zeros"""
    assert not np.any(got_greek[:, [2, 4], :min(2, l_tr)])


def check(what, got_greek, got_c0, host_greek, host_c0, ref, l_tr, report=None):
    """the rule; returns the worst distance / allowed over the fields.  host_greek = None: without the host term, allowed =
    max(4 κ_q 2⁻⁵², 2⁻⁴⁶) -- for sets at which the host itself stands further from the arbiter than the cap lets the rule reach"""
    assert got_greek.shape == ref["greek"].shape and np.all(np.isfinite(got_greek)) and np.all(np.isfinite(got_c0)), what
    assert_exact_zeros(got_greek, l_tr)
    d_got = distances(got_greek, got_c0, ref)
    d_host = distances(host_greek, host_c0, ref) if host_greek is not None else dict.fromkeys(d_got, 0.0)
    lim = allowed(d_host, ref)
    worst = 0.0
    for k in d_got:
        if report is not None:
            report.append((what, k, d_got[k], d_host[k], lim[k]))
        assert lim[k] <= CAP, (what, k, lim[k])
        assert d_got[k] <= lim[k], (what, k, d_got[k], d_host[k], lim[k], ref["kappa"])
        worst = max(worst, d_got[k] / lim[k])
    return worst
