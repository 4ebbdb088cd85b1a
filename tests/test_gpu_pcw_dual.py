"""The Jacobian rows of the Domke-PCW route on the GPU (csrc/mom_pcw.hip: mom_mie_pcw_dual, mom_pcw_pair_averages_dual;
scattering.aerosol_optics_jacobian) against the value calls (bitwise), the numpy oracle (tests/pcw_dual_oracle.py) and the device's
NAI-2 Jacobian.

Tolerances.  Weight rows: bitwise what mom_mie_pcw / mom_pcw_pair_averages write for the row.  Index rows against the oracle: the
project's rule, po.rule_bound -- relative to the array's largest magnitude, 8 x the distance between the Float64 and the long-double
run of the oracle ON THE SAME INPUTS, floor 2^-46, never measured on the GPU result.  PCW against NAI-2 on the device: 8 x the
distance of the two CPU oracles (pcw_dual_oracle, mie_dual_oracle) on the case, computed here, floor 2^-46; at the reference's test
point the reference's own criterion, ||a - b||_2 <= sqrt(eps) max(||a||_2, ||b||_2) per field and parameter."""
import functools
import math

import numpy as np
import pytest

import mie_dual_oracle as mdo
import pcw_dual_oracle as pdo
import pcw_oracle as po

pytestmark = pytest.mark.gpu

SQRT_EPS = math.sqrt(np.finfo(np.float64).eps)
FIELDS = ("α", "β", "γ", "δ", "ϵ", "ζ")
PARAMETERS = ("r_m", "σ_g", "nᵣ", "nᵢ")
LD = np.longdouble
# more radius chunks (125) than chunk groups of the index rows' product (4096 / 6^2 = 113 at Np = 48): twelve groups take a second chunk
CASES = {**po.SMALL_CASES, **po.MID_CASES, "n33_r2000": (1.1716, 2000, 0.55, 1.45, 0.01, 0.6 * 1.1716, 1.5)}
REFERENCE_POINT = (30.0, 2500, 0.55, 1.3, 0.001, 0.3, 6.82)


def _model(rtamd, args, ctype):
    sc = rtamd.scattering
    r_max, nquad, lam, n_r, n_i, r_m, σ_g = args
    aer = sc.Aerosol(sc.LogNormal(math.log(r_m), math.log(σ_g)), n_r, n_i)
    return sc.make_mie_model(ctype, aer, lam, None, None, r_max, nquad)


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """the product's host inputs of the case: r, w [3, nR] (w_x and its r_m, σ_g rows), N_max"""
    import rtamd
    sc = rtamd.scattering
    r, w, N, _, _ = sc.pcw_jacobian_inputs(_model(rtamd, CASES[case], sc.PCW()), sc.ALL_AEROSOL_PARAMETERS)
    assert w.shape == (3, r.size)
    return r, w, N


def _groups(N, nR):
    """the chunk counts of csrc/mom_pcw.hip: radius chunks, chunk groups of the symmetric product and of the square one"""
    Np, chunks = -(-N // 16) * 16, -(-nR // 16)
    rows = 4 * Np // 32
    return chunks, min(max(4096 // (rows * (rows + 1) // 2), 1), chunks), min(max(4096 // (rows * rows), 1), chunks)


def _rel(got, x64, x80, what):
    """got against the Float64 oracle by the rule; prints the figures before it asserts"""
    big = float(np.abs(x64).max())
    if big == 0.0:
        assert not np.any(got), what
        return
    bound = po.rule_bound(x64, x64 - x80)
    d = float(np.abs(got - x64).max()) / big
    print(f"{what}: GPU - oracle = {d:.3e}, bound {bound:.3e} (largest {big:.3e})")
    assert d <= bound, (what, d, bound)


# ---- 1. the weight rows are the value calls', bitwise ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["n31", "n33_r64", "n49_r7", "n300_r40"])
def test_weight_rows_bitwise(rtamd, case):
    """n31: Np = 32, one row short; n33_r64: macro tiles spanning two planes; n49_r7: fewer radii than one chunk; n300_r40: a lane of
    k_pcw_sums takes a second order.  Every nW, with and without the index rows; a repeated call."""
    lib = rtamd._lib
    _, _, lam, n_r, n_i, _, _ = CASES[case]
    r, w, N = _inputs(case)
    sums = [lib.mie_pcw(r, w[k], lam, n_r, n_i, N)[:2] for k in range(3)]
    pairs = [np.array(lib.pcw_pair_averages(r, w[k], lam, n_r, n_i, N)) for k in range(3)]
    for nW in (1, 2, 3):
        for index_rows in (False, True):
            greek, C, ms = lib.mie_pcw_dual(r, w[:nW], lam, n_r, n_i, N, index_rows=index_rows)
            pr = lib.pcw_pair_averages_dual(r, w[:nW], lam, n_r, n_i, N, index_rows=index_rows)
            nO = nW + 2 * index_rows
            assert greek.shape == (nO, 6, 2 * N - 1) and C.shape == (nO, 2) and pr.shape == (nO, 4, N, N) and np.all(ms >= 0)
            assert np.all(np.isfinite(greek)) and np.all(np.isfinite(C)) and np.all(np.isfinite(pr))
            for k in range(nW):
                assert np.array_equal(greek[k], sums[k][0]) and np.array_equal(C[k], sums[k][1]), (case, nW, index_rows, k)
                assert np.array_equal(pr[k], pairs[k]), (case, nW, index_rows, k)
            assert np.all(pr[:, :, np.triu_indices(N, 1)[0], np.triu_indices(N, 1)[1]] == 0)
    again = lib.mie_pcw_dual(r, w, lam, n_r, n_i, N, index_rows=True)
    assert np.array_equal(again[0], greek) and np.array_equal(again[1], C)
    assert np.array_equal(lib.pcw_pair_averages_dual(r, w, lam, n_r, n_i, N, index_rows=True), pr)


# ---- 2. the pair-average partials -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["n31", "n32", "n33_r64", "n49_r7", "n300_r40", "n33_r2000"])
def test_pair_average_partials(rtamd, case):
    _, _, lam, n_r, n_i, _, _ = CASES[case]
    r, w, N = _inputs(case)
    w = w[:1] if case == "n33_r2000" else w
    chunks, G, GH = _groups(N, r.size)
    print(f"{case}: {chunks} radius chunks, G = {G} (symmetric product), G = {GH} (index rows' product)")
    if case == "n33_r2000":
        assert chunks > GH
    got = rtamd._lib.pcw_pair_averages_dual(r, w, lam, n_r, n_i, N, index_rows=True)
    o64 = pdo.pair_averages_dual(r, w, lam, n_r, n_i, N)
    o80 = pdo.pair_averages_dual(r.astype(LD), w.astype(LD), lam, n_r, n_i, N)
    assert got.shape == o64.shape == (w.shape[0] + 2, 4, N, N)
    for k in range(got.shape[0]):
        for q, name in enumerate(("anam", "anbm", "bnam", "bnbm")):
            _rel(got[k, q], o64[k, q], o80[k, q], f"{case}: row {k}: {name}")


# ---- 3. the index rows of the sums --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sums_oracles(case):
    """both runs of the oracle on the product's inputs, w_x alone: rows (value, d/dn_r, d/dn_i)"""
    r_max, _, lam, n_r, n_i, _, _ = CASES[case]
    r, w, N = _inputs(case)
    o64 = pdo.pcw_sums_dual(r, w[:1], lam, n_r, n_i, r_max)
    o80 = pdo.pcw_sums_dual(r.astype(LD), w[:1].astype(LD), lam, n_r, n_i, r_max)
    assert o64["N"] == o80["N"] == N
    return o64, o80


@pytest.mark.parametrize("case", list(po.SMALL_CASES) + ["n33_r64", "n49_r7"])
def test_index_rows_against_oracle(rtamd, case):
    """n49_r7 has n_i = 0: the derivative exists there (only a finite difference would be one-sided)"""
    _, _, lam, n_r, n_i, _, _ = CASES[case]
    r, w, N = _inputs(case)
    o64, o80 = _sums_oracles(case)
    greek, C, _ = rtamd._lib.mie_pcw_dual(r, w[:1], lam, n_r, n_i, N, index_rows=True)
    for k, row in ((1, "d/dn_r"), (2, "d/dn_i")):
        for q, name in enumerate(FIELDS):
            _rel(greek[k, q], o64["greek"][k, q], o80["greek"][k, q], f"{case}: {row} {name}")
        _rel(C[k], o64["C"][k], o80["C"][k], f"{case}: {row} C")   # (C_sca, C_ext) is one array, as in test_gpu_pcw(_shapes).py


# ---- 4. PCW against NAI-2: the purpose -------------------------------------------------------------------------------------------

def _rows(optics):
    g = optics.greek_coefs
    return np.stack([g.α, g.β, g.γ, g.δ, g.ϵ, g.ζ])


def _within(d_device, d_oracles, scale, what):
    """the two device routes' distance against 8 x the two CPU oracles' (floor 2^-46), both relative to `scale`; a scale of zero (a
    weight row that is zero: one radius) asks for no distance at all"""
    d_device, d_oracles, scale = float(d_device), float(d_oracles), float(scale)
    if scale == 0.0:
        assert d_device == 0.0, what
        return
    bound = max(8 * d_oracles / scale, po.BOUND_FLOOR)
    print(f"{what}: |PCW - NAI-2| = {d_device / scale:.3e} of {scale:.3e}, bound {bound:.3e}")
    assert d_device / scale <= bound, (what, d_device / scale, bound)


@pytest.mark.parametrize("case", list(po.SMALL_CASES))
def test_jacobian_against_nai2(rtamd, case):
    """all four parameters, the common leading coefficients, ω̃ and k.  The bound of each array is 8 x the distance of the two CPU
    oracles on the case (floor 2^-46), relative to the array's largest magnitude; ∂ω̃ is a difference of two terms that cancel at
    n_i = 0, so its distances are relative to the larger term (pdo.omega_scale)."""
    sc = rtamd.scattering
    args = CASES[case]
    r_max, _, lam, n_r, n_i, _, _ = args
    pcw, parts_p = sc.aerosol_optics_jacobian(_model(rtamd, args, sc.PCW()))
    nai, parts_n = sc.compute_aerosol_optical_properties(_model(rtamd, args, sc.NAI2()), autodiff=True, wrt=sc.ALL_AEROSOL_PARAMETERS)
    assert len(parts_p) == len(parts_n) == 4
    r, w, N = _inputs(case)
    op = pdo.pcw_sums_dual(r, w, lam, n_r, n_i, r_max)
    on = mdo.nai2_sums_dual(r, w, lam, n_r, n_i)
    gp, omp, kp = pdo.normalised(op["greek"], op["C"])
    Cn = np.concatenate([on["C"], on["d_C"]])
    gn, omn, kn = pdo.normalised(np.concatenate([on["greek"], on["d_greek"]]), Cn)
    L = min(gp.shape[2], gn.shape[2], len(pcw.greek_coefs.β), len(nai.greek_coefs.β))
    scale = pdo.omega_scale(Cn)
    for j, name in enumerate(PARAMETERS):
        a, b = _rows(parts_p[j])[:, :L], _rows(parts_n[j])[:, :L]
        _within(np.abs(a - b).max(), np.abs(gp[1 + j, :, :L] - gn[1 + j, :, :L]).max(), np.abs(gn[1 + j, :, :L]).max(), f"{case}: ∂/∂{name}: Greek")
        _within(abs(parts_p[j].ω̃ - parts_n[j].ω̃), abs(omp[1 + j] - omn[1 + j]), scale[j], f"{case}: ∂ω̃/∂{name}")
        _within(abs(parts_p[j].k - parts_n[j].k), abs(kp[1 + j] - kn[1 + j]), abs(kn[1 + j]), f"{case}: ∂k/∂{name}")
        assert parts_p[j].fᵗ == 0.0


def _norm_distance(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(a), np.linalg.norm(b)))


def test_jacobian_at_the_reference_test_point(rtamd):
    """LogNormal(log 0.3, log 6.82), r_max = 30, 2500 radii, N_max = 381: the two routes' Jacobians by the criterion the reference
    holds the two routes' values to (test_gpu_pcw.test_reference_test_point)"""
    sc = rtamd.scattering
    pcw, parts_p = sc.aerosol_optics_jacobian(_model(rtamd, REFERENCE_POINT, sc.PCW()))
    nai, parts_n = sc.compute_aerosol_optical_properties(_model(rtamd, REFERENCE_POINT, sc.NAI2()), autodiff=True,
                                                         wrt=sc.ALL_AEROSOL_PARAMETERS)
    assert len(pcw.greek_coefs.β) == 761
    L = min(761, len(nai.greek_coefs.β))
    for j, name in enumerate(PARAMETERS):
        for q, field in enumerate(FIELDS):
            d = _norm_distance(_rows(parts_p[j])[q, :L], _rows(parts_n[j])[q, :L])
            print(f"∂{field}/∂{name}: PCW - NAI-2 = {d:.3e} (criterion {SQRT_EPS:.3e})")
            assert d <= SQRT_EPS, (name, field, d)
        for what, a, b in (("ω̃", parts_p[j].ω̃, parts_n[j].ω̃), ("k", parts_p[j].k, parts_n[j].k)):
            print(f"∂{what}/∂{name}: PCW = {a!r}, NAI-2 = {b!r}")
            assert abs(a - b) <= SQRT_EPS * max(abs(a), abs(b)), (name, what)


# ---- 5. downstream ------------------------------------------------------------------------------------------------------------

def test_downstream_takes_the_jacobian(rtamd):
    sc = rtamd.scattering
    model = _model(rtamd, CASES["n31"], sc.PCW())
    aero, parts = sc.aerosol_optics_jacobian(model)
    value = sc.compute_aerosol_optical_properties(model)
    assert np.array_equal(_rows(aero), _rows(value)) and aero.ω̃ == value.ω̃ and aero.k == value.k and aero.fᵗ == value.fᵗ == 1.0
    l_max = len(aero.greek_coefs.β)
    derivs = sc.aerosol_derivs(aero, parts)
    assert derivs.shape == (6 * l_max + 2, 4) and np.all(np.isfinite(derivs)) and np.all(np.abs(derivs).max(axis=0) > 0)
    tr, d_tr = sc.truncate_phase(sc.δBGE(10, 2.0), aero, partials=parts)
    assert len(d_tr) == 4 and all(len(p.greek_coefs.β) == 10 and np.all(np.isfinite(_rows(p))) for p in d_tr)
    assert np.array_equal(_rows(tr), _rows(sc.truncate_phase(sc.δBGE(10, 2.0), value)))
    # one parameter alone: the same partial, from a call without the other rows
    _, only = sc.aerosol_optics_jacobian(model, wrt=("nᵢ",))
    assert np.array_equal(_rows(only[0]), _rows(parts[3])) and only[0].ω̃ == parts[3].ω̃ and only[0].k == parts[3].k
    with pytest.raises(NotImplementedError, match="aerosol_optics_jacobian"):
        sc.compute_aerosol_optical_properties(model, autodiff=True)


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------

def test_argument_errors(rtamd):
    lib, EINVAL = rtamd._lib, rtamd._lib.MOM_EINVAL
    assert (lib.MOM_PCW_MAX_WEIGHT_ROWS, lib.MOM_PCW_INDEX_ROWS) == (3, 1)
    r, w, N = _inputs("n31")
    good = dict(r=r, w=w, lam=0.55, n_r=1.3, n_i=0.001, N_max=N, index_rows=True)
    bad = [dict(w=w[:0]), dict(w=np.concatenate([w, w[:1]])), dict(flags=2), dict(flags=3), dict(lam=0.0), dict(lam=-1.0), dict(n_i=-0.1),
           dict(n_r=float("nan")), dict(r=r[::-1].copy()), dict(r=np.concatenate([[0.0], r[1:]])), dict(N_max=N - 1), dict(N_max=0),
           dict(N_max=lib.MOM_PCW_MAX_ORDER + 1)]
    for change in bad:
        with pytest.raises(rtamd.MomError) as e:
            lib.mie_pcw_dual(**{**good, **change})
        assert e.value.code == EINVAL and "mom_mie_pcw_dual" in str(e.value), change
    for change in (dict(w=w[:0]), dict(N_max=N - 1), dict(N_max=0), dict(lam=0.0)):
        args = {**good, **change}
        with pytest.raises(rtamd.MomError) as e:
            lib.pcw_pair_averages_dual(args["r"], args["w"], args["lam"], args["n_r"], args["n_i"], args["N_max"], index_rows=True)
        assert e.value.code == EINVAL and "mom_pcw_pair_averages_dual" in str(e.value), change
    raw = lib.load()
    greek, C = np.empty((5, 6, 2 * N - 1)), np.empty((5, 2))
    call = lambda r_, w_, g_, C_, nR=len(r): raw.mom_mie_pcw_dual(0, nR, r_, 3, w_, 0.55, 1.3, 0.001, N, 1, g_, C_, None)
    assert call(None, lib.dp(w), lib.dp(greek), lib.dp(C)) == EINVAL
    assert call(lib.dp(r), None, lib.dp(greek), lib.dp(C)) == EINVAL
    assert call(lib.dp(r), lib.dp(w), None, lib.dp(C)) == EINVAL
    assert call(lib.dp(r), lib.dp(w), lib.dp(greek), None) == EINVAL
    assert call(lib.dp(r), lib.dp(w), lib.dp(greek), lib.dp(C), nR=0) == EINVAL
    assert raw.mom_pcw_pair_averages_dual(0, len(r), lib.dp(r), 3, lib.dp(w), 0.55, 1.3, 0.001, N, 1, None) == EINVAL
    assert "mom_pcw_pair_averages_dual" in raw.mom_last_global_error().decode()
    # the value calls keep their list: the index flag is none of theirs
    with pytest.raises(rtamd.MomError) as e:
        lib.mie_pcw(r, w[0], 0.55, 1.3, 0.001, N, flags=lib.MOM_PCW_INDEX_ROWS)
    assert e.value.code == EINVAL and "mom_mie_pcw:" in str(e.value)
