"""The Domke-PCW aerosol optics on the GPU (csrc/mom_pcw.hip: mom_mie_pcw, mom_wigner_tables, mom_pcw_pair_averages) against the
numpy oracle (tests/pcw_oracle.py), the exact Wigner symbols, the device's own NAI-2 run and the reference's stored PCW result.

Tolerances.  Device against the PCW oracle: the project's rule -- relative to each array's largest magnitude, 8 x
the distance between the Float64 and the long-double run of the oracle ON THE SAME INPUTS (never measured on the GPU result); the
device differs from the Float64 oracle by the association order of its sums only.  Symbols against the exact ones: the absolute
bounds derived in tests/test_oracle_pcw.py.  PCW against NAI-2 on the device at small sizes: 8 x 1.9e-13 absolute, the difference of
the two CPU oracles on these cases (coefficients of up to 4.6).  The reference's test point: the reference's own criterion, isapprox
with rtol = sqrt(eps) -- per field ||a - b||_2 <= sqrt(eps) max(||a||_2, ||b||_2), and the scalar form for omega and k."""
import functools
import math
from pathlib import Path

import numpy as np
import pytest

import mie_oracle as mo
import pcw_oracle as po

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "pcw_aerosol_optics.npz"
SQRT_EPS = math.sqrt(np.finfo(np.float64).eps)
FIELDS = ("α", "β", "γ", "δ", "ϵ", "ζ")


def _model(rtamd, args, ctype):
    sc = rtamd.scattering
    r_max, nquad, lam, n_r, n_i, r_m, σ_g = args
    aer = sc.Aerosol(sc.LogNormal(math.log(r_m), math.log(σ_g)), n_r, n_i)
    return sc.make_mie_model(ctype, aer, lam, None, None, r_max, nquad)


@functools.lru_cache(maxsize=None)
def _inputs_and_oracle(case):
    """the product's host inputs of the case, the Float64 oracle on them and the long-double one"""
    import rtamd
    args = po.SMALL_CASES[case]
    r, wx, N = rtamd.scattering.pcw_inputs(_model(rtamd, args, rtamd.scattering.PCW()))
    r_max, _, lam, n_r, n_i, _, _ = args
    o64 = po.pcw_sums(r, wx, lam, n_r, n_i, r_max)
    o80 = po.pcw_sums(r.astype(np.longdouble), wx.astype(np.longdouble), lam, n_r, n_i, r_max)
    assert o64["N"] == N
    return r, wx, N, o64, o80


def _greek_rows(optics):
    g = optics.greek_coefs
    return np.stack([g.α, g.β, g.γ, g.δ, g.ϵ, g.ζ])


# ---- 1. the symbols -------------------------------------------------------------------------------------------------------------

def test_wigner_tables_every_entry(rtamd):
    A, B = rtamd.compute_wigner_values(25, 13, 25)
    Ae, Be = po.exact_tables(25, 13, 25)
    assert A.shape == B.shape == (25, 13, 25)
    dA, dB = float(np.abs(A - Ae).max()), float(np.abs(B - Be).max())
    print(f"(25, 13, 25): max |A - exact| = {dA:.3e} (bound {po.A_BOUND:.0e}), max |B - exact| = {dB:.3e} (bound {po.B_BOUND:.0e})")
    assert dA <= po.A_BOUND and dB <= po.B_BOUND
    outA, outB = po.out_of_range(25, 13, 25)
    assert np.all(A[outA] == 0) and np.all(B[outB] == 0)
    A2, B2 = rtamd.compute_wigner_values(25, 13, 25)
    assert np.array_equal(A, A2) and np.array_equal(B, B2)


def test_wigner_tables_sampled_shorthand(rtamd):
    """compute_wigner_values(120) = (241, 121, 241), 56 MB per table: most columns start above the table (n + l - 1 up to 361)"""
    A, B = rtamd.compute_wigner_values(120)
    assert A.shape == B.shape == (241, 121, 241)
    dA = dB = 0.0
    for m, n, l in po.in_range_samples(241, 121, 241):
        dA = max(dA, abs(A[m - 1, n - 1, l - 1] - po.wigner_A_exact(m, n, l)))
        dB = max(dB, abs(B[m - 1, n - 1, l - 1] - po.wigner_B_exact(m, n, l)))
    print(f"(241, 121, 241), 400 samples: max |A - exact| = {dA:.3e}, max |B - exact| = {dB:.3e}")
    assert dA <= po.A_BOUND and dB <= po.B_BOUND
    outA, outB = po.out_of_range(241, 121, 241)
    assert np.all(A[outA] == 0) and np.all(B[outB] == 0)
    A2, B2 = rtamd.compute_wigner_values(120)
    assert np.array_equal(A, A2) and np.array_equal(B, B2)


# ---- 2. the pair averages -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["n31", "n32"])
def test_pair_averages(rtamd, case):
    """N_max = 31 (one row short of two tiles) and 32 (the multiple-of-16 edge); 60 and 49 radii, no multiples of 16; four radius
    chunks, so the chunk sum runs.  Relative to each matrix's largest magnitude."""
    r, wx, N, o64, o80 = _inputs_and_oracle(case)
    _, _, lam, n_r, n_i, _, _ = po.SMALL_CASES[case]
    got = rtamd._lib.pcw_pair_averages(r, wx, lam, n_r, n_i, N)
    for name, g, a, b in zip(("anam", "anbm", "bnam", "bnbm"), got, o64["pairs"], o80["pairs"]):
        big = float(np.abs(a).max())
        bound = 8 * float(np.abs(a - b).max()) / big
        d = float(np.abs(g - a).max()) / big
        print(f"{case}: {name}: GPU - oracle = {d:.3e}, bound {bound:.3e} (largest {big:.3e})")
        assert g.shape == (N, N) and d <= bound
        assert np.all(np.triu(g, 1) == 0)
    again = rtamd._lib.pcw_pair_averages(r, wx, lam, n_r, n_i, N)
    assert all(np.array_equal(x, y) for x, y in zip(got, again))


# ---- 3. the public call at small sizes --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(po.SMALL_CASES))
def test_sums_against_oracle(rtamd, case):
    r, wx, N, o64, o80 = _inputs_and_oracle(case)
    _, _, lam, n_r, n_i, _, _ = po.SMALL_CASES[case]
    greek, C, ms = rtamd._lib.mie_pcw(r, wx, lam, n_r, n_i, N)
    assert greek.shape == (6, 2 * N - 1) and np.all(ms >= 0)
    for q, name in enumerate(FIELDS):
        big = float(np.abs(o64["greek"][q]).max())
        bound = 8 * float(np.abs(o64["greek"][q] - o80["greek"][q]).max()) / big
        d = float(np.abs(greek[q] - o64["greek"][q]).max()) / big
        print(f"{case}: {name}: GPU - oracle = {d:.3e}, bound {bound:.3e}")
        assert d <= bound, (case, name, d, bound)
    bound = 8 * mo.rel_max(o64["C"], o80["C"])
    d = mo.rel_max(C, o64["C"])
    print(f"{case}: C: GPU - oracle = {d:.3e}, bound {bound:.3e}")
    assert d <= bound


@pytest.mark.parametrize("case", list(po.SMALL_CASES))
def test_public_call_against_oracle_and_nai2(rtamd, case):
    sc = rtamd.scattering
    args = po.SMALL_CASES[case]
    model = _model(rtamd, args, sc.PCW())
    aero = sc.compute_aerosol_optical_properties(model)
    r, wx, N, o64, o80 = _inputs_and_oracle(case)
    assert aero.fᵗ == 1.0 and len(aero.greek_coefs.β) == 2 * N - 1
    g = _greek_rows(aero)
    n64, n80 = (1 / o64["C"][0]) * o64["greek"], (1 / o80["C"][0]) * o80["greek"]
    for q, name in enumerate(FIELDS):
        big = float(np.abs(n64[q]).max())
        bound = 8 * float(np.abs(n64[q] - n80[q]).max()) / big
        d = float(np.abs(g[q] - n64[q]).max()) / big
        print(f"{case}: {name}: public call - oracle = {d:.3e}, bound {bound:.3e}")
        assert d <= bound, (case, name, d, bound)
    # ω̃ and k are host arithmetic on the device's C, which test_sums_against_oracle holds to the rule
    _, lam, n_r, n_i = args[1], args[2], args[3], args[4]
    _, C, _ = rtamd._lib.mie_pcw(r, wx, lam, n_r, n_i, N)
    assert aero.ω̃ == C[0] / C[1] and aero.k == C[1]
    # the device's own NAI-2 run: the common leading coefficients (NAI-2 sizes its arrays from the largest quadrature node)
    nai = sc.compute_aerosol_optical_properties(_model(rtamd, args, sc.NAI2()))
    gn = _greek_rows(nai)
    L = min(g.shape[1], gn.shape[1])
    d = float(np.abs(g[:, :L] - gn[:, :L]).max())
    print(f"{case}: lengths {g.shape[1]} (PCW), {gn.shape[1]} (NAI-2); max |PCW - NAI-2| = {d:.3e} of {np.abs(gn).max():.3f}; "
          f"ω̃ {aero.ω̃ - nai.ω̃:.3e}, k {aero.k / nai.k - 1:.3e}")
    assert d <= 8 * 1.9e-13
    assert abs(aero.ω̃ - nai.ω̃) <= 8 * np.finfo(np.float64).eps and abs(aero.k / nai.k - 1) <= 8 * np.finfo(np.float64).eps
    assert abs(aero.greek_coefs.β[0] - 1) <= 8 * 1.9e-13
    # two calls are bitwise equal
    again = sc.compute_aerosol_optical_properties(model)
    assert np.array_equal(g, _greek_rows(again)) and aero.ω̃ == again.ω̃ and aero.k == again.k


def test_downstream_takes_the_result(rtamd):
    """truncate_phase takes the PCW optics unchanged; its β₀ is 1 and fᵗ the fit's"""
    sc = rtamd.scattering
    aero = sc.compute_aerosol_optical_properties(_model(rtamd, po.SMALL_CASES["n31"], sc.PCW()))
    tr = sc.truncate_phase(sc.δBGE(10, 2.0), aero)
    assert len(tr.greek_coefs.β) == 10 and abs(tr.greek_coefs.β[0] - 1) < 1e-12 and 0 < tr.fᵗ < 1
    # a scene built on either route: rt_run takes it, and the truncated optics agree by the criterion the reference holds the two
    # routes to (sqrt(eps)); the fit's normal equations amplify the routes' 1.9e-13, by how much is printed
    kw = dict(nStokes=3, l_trunc=10, Nz=3, S=4, seed=1)
    m_pcw, m_nai = rtamd.scenes.make_mie_scene(computation_type=sc.PCW(), **kw), rtamd.scenes.make_mie_scene(**kw)
    d = float(np.abs(_greek_rows(m_pcw.aerosol_optics[0]) - _greek_rows(m_nai.aerosol_optics[0])).max())
    print(f"make_mie_scene: max |PCW - NAI-2| of the truncated coefficients = {d:.3e}")
    assert d <= SQRT_EPS * float(np.abs(_greek_rows(m_nai.aerosol_optics[0])).max())
    R = rtamd.rt_run(m_pcw)[0]
    assert np.all(np.isfinite(R))


# ---- 4. the reference's test point ------------------------------------------------------------------------------------------------

REFERENCE_POINT = (30.0, 2500, 0.55, 1.3, 0.001, 0.3, 6.82)


def _norm_distance(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(a), np.linalg.norm(b)))


def test_reference_test_point(rtamd):
    """LogNormal(log 0.3, log 6.82), r_max = 30, 2500 radii, λ = 0.55, m = 1.3 + 0.001i: N_max = 381, 761 degrees.  Against the
    reference's stored PCW result by the reference's criterion, and against the device's NAI-2 run of the same model by the same
    criterion (the one the reference applies between its NAI-2 run and that file, test/test_Scattering.jl:115-117)."""
    sc = rtamd.scattering
    z = np.load(GOLDEN)
    aero = sc.compute_aerosol_optical_properties(_model(rtamd, REFERENCE_POINT, sc.PCW()))
    nai = sc.compute_aerosol_optical_properties(_model(rtamd, REFERENCE_POINT, sc.NAI2()))
    for name, key, a, n in zip(FIELDS, ("alpha", "beta", "gamma", "delta", "epsilon", "zeta"), _greek_rows(aero), _greek_rows(nai)):
        assert a.shape == z[key].shape == (761,)
        d_fix, d_nai = _norm_distance(a, z[key]), _norm_distance(a[:n.size], n[:a.size])
        print(f"{name}: PCW - fixture = {d_fix:.3e}, PCW - device NAI-2 = {d_nai:.3e} (criterion {SQRT_EPS:.3e})")
        assert d_fix <= SQRT_EPS and d_nai <= SQRT_EPS
    for name, got, want, other in (("ω̃", aero.ω̃, float(z["omega"]), nai.ω̃), ("k", aero.k, float(z["k"]), nai.k)):
        print(f"{name}: PCW = {got!r}, fixture = {want!r}, device NAI-2 = {other!r}")
        assert abs(got - want) <= SQRT_EPS * max(abs(got), abs(want)) and abs(got - other) <= SQRT_EPS * max(abs(got), abs(other))
    assert aero.fᵗ == float(z["f_t"]) == 1.0


# ---- 5. errors and neighbours ---------------------------------------------------------------------------------------------------

def test_argument_errors(rtamd):
    lib, EINVAL = rtamd._lib, rtamd._lib.MOM_EINVAL
    r, wx, N, _, _ = _inputs_and_oracle("n31")
    good = dict(r=r, w=wx, lam=0.55, n_r=1.3, n_i=0.001, N_max=N)
    bad = [dict(lam=0.0), dict(lam=-1.0), dict(n_i=-0.1), dict(n_r=float("nan")), dict(r=r[::-1].copy()), dict(r=np.concatenate([[0.0], r[1:]])),
           dict(N_max=N - 1), dict(N_max=0), dict(N_max=lib.MOM_PCW_MAX_ORDER + 1), dict(flags=1)]
    for change in bad:
        with pytest.raises(rtamd.MomError) as e:
            lib.mie_pcw(**{**good, **change})
        assert e.value.code == EINVAL and "mom_mie_pcw" in str(e.value), change
    with pytest.raises(rtamd.MomError) as e:
        lib.pcw_pair_averages(r, wx, 0.55, 1.3, 0.001, N - 1)
    assert e.value.code == EINVAL and "mom_pcw_pair_averages" in str(e.value)
    raw = lib.load()
    assert raw.mom_mie_pcw(0, len(r), lib.dp(r), None, 0.55, 1.3, 0.001, N, 0, None, None, None) == EINVAL
    assert raw.mom_mie_pcw(0, 0, lib.dp(r), lib.dp(wx), 0.55, 1.3, 0.001, N, 0, lib.dp(np.empty((6, 2 * N - 1))), lib.dp(np.empty(2)), None) == EINVAL
    # tables: a size below 1, a table above MOM_WIGNER_MAX_TABLE_BYTES (8 GiB here; refused before any allocation), null pointers
    for shape in ((0, 3, 3), (3, 0, 3), (3, 3, 0), (1024, 1024, 1024), (3, 1000, 1000), (200000, 30, 30)):
        with pytest.raises(rtamd.MomError) as e:
            lib.wigner_tables(*shape)
        assert e.value.code == EINVAL and "mom_wigner_tables" in str(e.value), shape
    assert "MOM_WIGNER_MAX_TABLE_BYTES" in str(e.value)             # 200000 x 30 x 30 doubles = 1.34 GiB
    assert raw.mom_wigner_tables(0, 3, 3, 3, None, None) == EINVAL
    with pytest.raises(TypeError):
        rtamd.compute_wigner_values(3, 3)


def test_autodiff_raises_and_nai2_is_unchanged(rtamd):
    sc = rtamd.scattering
    args = po.SMALL_CASES["n31"]
    pcw, nai2 = _model(rtamd, args, sc.PCW()), _model(rtamd, args, sc.NAI2())
    assert isinstance(nai2.computation_type, sc.NAI2) and nai2.wigner_A is None and nai2.wigner_B is None
    with pytest.raises(NotImplementedError):
        sc.compute_aerosol_optical_properties(pcw, autodiff=True)
    with pytest.raises(NotImplementedError):
        sc.make_mie_model(object(), pcw.aerosol, 0.55, None, None, 1.0, 10)
    with pytest.raises(ValueError):
        sc.make_mie_model(sc.NAI2(), pcw.aerosol, 0.55, None, None, 1.0, 10, wigner_A=np.zeros((1, 1, 1)))
    tables = rtamd.compute_wigner_values(3)
    with_tables = sc.make_mie_model(sc.PCW(), pcw.aerosol, 0.55, None, None, args[0], args[1], *tables)
    assert with_tables.wigner_A is tables[0]
    before = sc.compute_aerosol_optical_properties(nai2)
    a = sc.compute_aerosol_optical_properties(pcw)
    b = sc.compute_aerosol_optical_properties(with_tables)            # the tables are accepted and not needed
    after, partials = sc.compute_aerosol_optical_properties(nai2, autodiff=True)
    assert np.array_equal(_greek_rows(a), _greek_rows(b))
    # NAI-2 around the PCW calls: bitwise the direct device call's result, before and after
    inp = sc.mie_inputs(nai2)
    _, C, greek, _ = rtamd._lib.mie_nai2(inp.r, inp.w, nai2.λ, 1.3, 0.001, inp.w_μ, inp.π_, inp.τ_, inp.P, inp.P2, inp.R2, inp.T2)
    direct = sc.optics_from_sums(C, greek)[0]
    for o in (before, after):
        assert np.array_equal(_greek_rows(o), _greek_rows(direct)) and o.ω̃ == direct.ω̃ and o.k == direct.k
    assert len(partials) == 2
