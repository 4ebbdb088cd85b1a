"""The spectral Mie call on the device (mom_mie_tables, mom_mie_nai2_spectral, mom_mie_nai2_spectral_dual in csrc/mom_mie.hip, and
scattering.compute_spectral_aerosol_optical_properties): the device-built angle tables are bitwise the host's, every wavelength of
a batch is bitwise the single-wavelength call on the same grid and tables, its rows do not depend on what else is in the batch or
on how the batch is cut into sub-batches, and every wavelength passes the oracle at that wavelength.  Cases, conditions and the
oracle of a batch: tests/mie_spectral_cases.py; test_oracle_mie_spectral.py shows on the CPU that the conditions hold.

Tolerances (T4 only) are those of mie_shapes.compare: 8 x the oracle's Float64 / long-double distance, at least 2^-46.  Everything
else is compared with np.array_equal."""
import functools

import numpy as np
import pytest

import mie_shapes as ms
import mie_spectral_cases as sc

pytestmark = pytest.mark.gpu

FORMS = [("value", False, (1, 2, 3, 4)), ("dual", True, (1, 2, 3))]


def _fn(L, dual, spectral=True):
    if spectral:
        return L.mie_nai2_spectral_dual if dual else L.mie_nai2_spectral
    return L.mie_nai2_dual if dual else L.mie_nai2


def _spectral(L, case, nW, dual, flags=0, max_batch=0, order=None):
    """{bulk_f, C, greek} of one spectral call on the case's inputs with weight rows 0 .. nW - 1, the wavelengths in `order`"""
    inp = sc.device_inputs(case)
    o = np.arange(len(case.lam)) if order is None else np.asarray(order)
    out = _fn(L, dual)(inp["r"], inp["w"][:nW], inp["lam"][o], inp["n_r"][o], inp["n_i"][o], inp["mu"], inp["w_mu"], inp["n_max"],
                       inp["l_max"], flags=flags, max_batch=max_batch)
    assert out[3].shape == (4,) and np.all(out[3] >= 0)
    return dict(zip(ms.ARRAYS, out[:3]))


@functools.lru_cache(maxsize=None)
def _device_tables(case):
    """the tables mom_mie_tables returns for the case's grid, in numpy's orientation: what the single calls of T2 are given"""
    import rtamd
    inp = sc.device_inputs(case)
    return rtamd._lib.mie_tables(inp["mu"], inp["n_max"], inp["l_max"])


# ------------------------------------------------------------------------------------------------------------------------------
# T1: the tables, bitwise
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_mu", [1, 33, 65, 77])
def test_tables_are_bitwise_the_hosts(rtamd, n_mu):
    """pi, tau, P, P2, R2, T2 of k_mie_tables equal compute_mie_π_τ and compute_legendre_poly bit for bit: one and more than one
    wavefront of nodes, table heights at which the start values, the first recurrence step and the R2 / T2 recurrence begin"""
    S, L = rtamd.scattering, rtamd._lib
    mu, _ = S.gausslegendre(n_mu)
    for n_max in (1, 2, 31, 39):
        for l_max in (1, 2, 3, 7, 77):
            got = L.mie_tables(mu, n_max, l_max)
            want = S.compute_mie_π_τ(mu, n_max) + S.compute_legendre_poly(mu, l_max)
            for name, g, w in zip(("pi", "tau", "P", "P2", "R2", "T2"), got, want):
                assert g.shape == w.shape, (name, n_max, l_max)
                assert np.array_equal(g, w), (name, n_mu, n_max, l_max, float(np.abs(g - w).max()))


# ------------------------------------------------------------------------------------------------------------------------------
# T2: each wavelength is the single call, bitwise
# ------------------------------------------------------------------------------------------------------------------------------

def _assert_rows_are_the_single_calls(L, case, dual, nW, flags):
    inp, tabs = sc.device_inputs(case), _device_tables(case)
    got = _spectral(L, case, nW, dual, flags)
    nO = nW + 2 if dual else nW
    assert got["bulk_f"].shape == (len(case.lam), nO, 4, len(inp["mu"])) and got["C"].shape == (len(case.lam), nO, 2)
    assert got["greek"].shape == (len(case.lam), nO, 6, inp["l_max"])
    for j, lam in enumerate(case.lam):
        one = _fn(L, dual, False)(inp["r"], inp["w"][:nW], lam, *case.m[j], inp["w_mu"], *tabs, flags=flags)
        for q, a in zip(ms.ARRAYS, one[:3]):
            assert np.array_equal(got[q][j], a), (q, j, nW, flags)
    for j in range(1, len(case.lam)):           # the wavelengths do differ
        assert not np.array_equal(got["C"][j], got["C"][0])


@pytest.mark.parametrize("full_k", [False, True], ids=["tile_k_rule", "full_k"])
@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
@pytest.mark.parametrize("name", ["base", "tile_k"])
def test_each_wavelength_is_the_single_call(rtamd, name, form, full_k):
    """rows j of bulk_f, C and greek equal mom_mie_nai2(_dual) at wavelength j with the same radii, weight rows, grid and host
    tables (those mom_mie_tables returned, so this does not lean on T1), for every number of weight rows"""
    L = rtamd._lib
    _, dual, rows = form
    for nW in rows:
        _assert_rows_are_the_single_calls(L, sc.CASES[name], dual, nW, L.MOM_MIE_FULL_K if full_k else 0)


@pytest.mark.parametrize("dual", [False, True], ids=["value", "dual"])
def test_each_wavelength_is_the_single_call_on_the_chunk_walk(rtamd, dual):
    """G = 62 chunks over 129 tiles, per wavelength the single call's boustrophedon walk and chunk-order reduction"""
    _assert_rows_are_the_single_calls(rtamd._lib, sc.CHUNK_WALK, dual, 1, 0)


# ------------------------------------------------------------------------------------------------------------------------------
# T3: the batch does not matter
# ------------------------------------------------------------------------------------------------------------------------------

def _raw_spectral(L, case, nW, dual, order, max_batch):
    """the C entry itself on output buffers pre-filled with NaN"""
    inp = sc.device_inputs(case)
    lib, dp = L.load(), L.dp
    o = np.asarray(order)
    lam, n_r, n_i = (L.f64(inp[k][o]) for k in ("lam", "n_r", "n_i"))
    r, w, mu, w_mu = L.f64(inp["r"]), L.f64(inp["w"][:nW]), L.f64(inp["mu"]), L.f64(inp["w_mu"])
    nO, nL, n_mu, l_max = (nW + 2 if dual else nW), len(o), len(mu), inp["l_max"]
    bulk, C, greek = np.full((nL, nO, 4, n_mu), np.nan), np.full((nL, nO, 2), np.nan), np.full((nL, nO, 6, l_max), np.nan)
    fn = lib.mom_mie_nai2_spectral_dual if dual else lib.mom_mie_nai2_spectral
    rc = fn(0, len(r), dp(r), nW, dp(w), nL, dp(lam), dp(n_r), dp(n_i), n_mu, dp(mu), dp(w_mu), inp["n_max"], l_max, 0, max_batch,
            dp(bulk), dp(C), dp(greek), None)
    assert rc == L.MOM_OK, lib.mom_last_global_error().decode()
    return dict(bulk_f=bulk, C=C, greek=greek)


@pytest.mark.parametrize("dual", [False, True], ids=["value", "dual"])
def test_rows_do_not_depend_on_the_batch(rtamd, dual):
    """five wavelengths (0.35 and 2.1 twice, with other indices) in one launch, in sub-batches of 1 and of 2 + 2 + 1, and in
    reversed order: every wavelength's rows are bitwise the same.  Shortest first with max_batch = 1 reuses the workspace of
    the highest planes for wavelengths whose planes end lower: planes left from the sub-batch before would enter their sums."""
    L, case, nW = rtamd._lib, sc.BATCH5, 3
    nL = len(case.lam)
    fwd, rev = list(range(nL)), list(range(nL))[::-1]
    ref = _raw_spectral(L, case, nW, dual, fwd, 0)
    for q in ms.ARRAYS:
        assert np.all(np.isfinite(ref[q])), q
    three = _spectral(L, sc.BASE, nW, dual)
    for q in ms.ARRAYS:                         # the first three are the batch of three
        assert np.array_equal(ref[q][:3], three[q]), q
        assert not np.array_equal(ref[q][3], ref[q][0]) and not np.array_equal(ref[q][4], ref[q][2]), q
    for order in (fwd, rev):
        for max_batch in (0, 1, 2):
            got = _raw_spectral(L, case, nW, dual, order, max_batch)
            for q in ms.ARRAYS:
                assert np.all(np.isfinite(got[q])), (q, order, max_batch)
                for pos, j in enumerate(order):
                    assert np.array_equal(got[q][pos], ref[q][j]), (q, order, max_batch, j)


# ------------------------------------------------------------------------------------------------------------------------------
# T4: the oracle
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dual", [False, True], ids=["value", "dual"])
def test_every_wavelength_against_the_oracle(rtamd, dual):
    nW = 3 if dual else 4
    got = _spectral(rtamd._lib, sc.BASE, nW, dual)
    bad = sc.compare_batch(got, sc.oracle(sc.BASE, dual), dual_rows=nW if dual else 0)
    assert bad == [], bad


# ------------------------------------------------------------------------------------------------------------------------------
# T5: the public call
# ------------------------------------------------------------------------------------------------------------------------------

LAM = np.array([0.55, 0.35, 2.1])               # the shortest is not the first
N_R, N_I = np.array([1.3, 1.33, 1.45]), np.array([0.001, 0.01, 0.0])


def _model(rtamd, lam, n_r=1.3, n_i=0.001):
    S = rtamd.scattering
    aer = S.Aerosol(S.LogNormal(np.log(0.3), np.log(1.6)), float(n_r), float(n_i))
    return S.make_mie_model(S.NAI2(), aer, float(lam), rtamd.Stokes_IQUV(), S.δBGE(10, 2.0), 1.0, 37)


def _same_optics(a, b):
    ga, gb = vars(a.greek_coefs), vars(b.greek_coefs)
    assert len(ga) == 6 and set(ga) == set(gb)
    return all(np.array_equal(ga[f], gb[f]) for f in ga) and a.ω̃ == b.ω̃ and a.k == b.k and a.fᵗ == b.fᵗ


def test_public_call(rtamd):
    """each AerosolOptics is optics_from_sums of the library's rows cut to the wavelength's own length; at the shortest wavelength,
    where the shared grid is its own, it is the single public call bit for bit (the tables are bitwise, T1)"""
    S, L = rtamd.scattering, rtamd._lib
    model = _model(rtamd, 0.55)
    optics = S.compute_spectral_aerosol_optical_properties(model, LAM, N_R, N_I)
    inp = S.spectral_mie_inputs(model, LAM)
    _, C, greek, _ = L.mie_nai2_spectral(inp.r, inp.w, LAM, N_R, N_I, inp.μ, inp.w_μ, inp.n_top, inp.l_max)
    assert len(optics) == 3
    for j in range(3):
        n = 2 * int(inp.n_max[j]) - 1
        want, _ = S.optics_from_sums(C[j], greek[j][:, :, :n])
        assert len(optics[j].greek_coefs.β) == n and _same_optics(optics[j], want), j
        single = S.compute_aerosol_optical_properties(_model(rtamd, LAM[j], N_R[j], N_I[j]))
        assert len(single.greek_coefs.β) == n, j
    shortest = int(np.argmin(LAM))
    assert _same_optics(optics[shortest], S.compute_aerosol_optical_properties(_model(rtamd, LAM[shortest], N_R[shortest], N_I[shortest])))
    # the default index is the aerosol's
    default = S.compute_spectral_aerosol_optical_properties(model, LAM[[1]])
    assert _same_optics(default[0], S.compute_aerosol_optical_properties(_model(rtamd, LAM[1])))


@pytest.mark.parametrize("wrt", [("r_m", "σ_g"), ("nᵢ",), ("nᵢ", "σ_g", "nᵣ", "r_m"), None], ids=["size", "index", "mixed", "all"])
def test_public_call_partials_have_the_single_calls_order(rtamd, wrt):
    S = rtamd.scattering
    wrt = S.ALL_AEROSOL_PARAMETERS if wrt is None else wrt
    model = _model(rtamd, 0.55)
    optics, partials = S.compute_spectral_aerosol_optical_properties(model, LAM, N_R, N_I, autodiff=True, wrt=wrt)
    assert len(optics) == len(partials) == 3 and all(len(p) == len(wrt) for p in partials)
    shortest = int(np.argmin(LAM))
    one, one_partials = S.compute_aerosol_optical_properties(_model(rtamd, LAM[shortest], N_R[shortest], N_I[shortest]), autodiff=True, wrt=wrt)
    assert _same_optics(optics[shortest], one)
    for got, want in zip(partials[shortest], one_partials):
        assert _same_optics(got, want)
    for j in range(3):                          # the partials of a wavelength differ from each other: no column is repeated
        ks = [p.k for p in partials[j]]
        assert len(set(ks)) == len(ks), (j, ks)


# ------------------------------------------------------------------------------------------------------------------------------
# T6: rejected arguments
# ------------------------------------------------------------------------------------------------------------------------------

def _args(**over):
    inp = dict(sc.device_inputs(sc.BASE))
    a = dict(r=inp["r"], w=inp["w"][:1], lam=inp["lam"], n_r=inp["n_r"], n_i=inp["n_i"], mu=inp["mu"], w_mu=inp["w_mu"],
             n_max=inp["n_max"], l_max=inp["l_max"], flags=0, max_batch=0)
    a.update(over)
    return a


def _replaced(a, j, v):
    b = np.array(a, dtype=np.float64)
    b[j] = v
    return b


@pytest.mark.parametrize("dual", [False, True], ids=["value", "dual"])
def test_rejected_arguments(rtamd, dual):
    L = rtamd._lib
    fn = _fn(L, dual)
    base = sc.device_inputs(sc.BASE)
    name = "mom_mie_nai2_spectral_dual" if dual else "mom_mie_nai2_spectral"
    bad = {
        "nW": (_args(w=base["w"][:4] if dual else np.concatenate([base["w"], base["w"][:1]])), "nW must be"),
        "lambda": (_args(lam=_replaced(base["lam"], 1, 0.0)), "wavelength 1: lambda"),
        "lambda nan": (_args(lam=_replaced(base["lam"], 2, np.nan)), "wavelength 2: lambda"),
        "n_i": (_args(n_i=_replaced(base["n_i"], 2, -0.1)), "wavelength 2: n_i"),
        "n_r": (_args(n_r=_replaced(base["n_r"], 0, np.inf)), "wavelength 0: n_i"),
        "l_max": (_args(l_max=0), "l_max"),
        "n_max 0": (_args(n_max=0), "n_max"),
        "flag": (_args(flags=2), "unknown flag"),
        "max_batch": (_args(max_batch=-1), "max_batch"),
        "r[0]": (_args(r=_replaced(base["r"], 0, 0.0)), "r[0]"),
        "ascending": (_args(r=_replaced(base["r"], 5, base["r"][4])), "ascending"),
        # 31 rows serve wavelengths 1 and 2; wavelength 0 needs 39
        "n_max": (_args(n_max=31), "wavelength 0: n_max is smaller"),
        "n_max, last": (_args(n_max=31, lam=base["lam"][::-1].copy()), "wavelength 2: n_max is smaller"),
    }
    for what, (a, text) in bad.items():
        with pytest.raises(L.MomError) as e:
            fn(a["r"], a["w"], a["lam"], a["n_r"], a["n_i"], a["mu"], a["w_mu"], a["n_max"], a["l_max"], flags=a["flags"],
               max_batch=a["max_batch"])
        assert e.value.code == L.MOM_EINVAL and name + ":" in str(e.value) and text in str(e.value), (what, str(e.value))
    # through the C entry: no wavelength, no node, no radius, a null pointer
    lib, dp = L.load(), L.dp
    a = _args()
    r, w, lam, n_r, n_i, mu, w_mu = (L.f64(a[k]) for k in ("r", "w", "lam", "n_r", "n_i", "mu", "w_mu"))
    out = [np.zeros((3, 3, 4, len(mu))), np.zeros((3, 3, 2)), np.zeros((3, 3, 6, a["l_max"]))]
    raw = lib.mom_mie_nai2_spectral_dual if dual else lib.mom_mie_nai2_spectral

    def call(nR=len(r), nL=3, n_mu=len(mu), mu_p=dp(mu), lam_p=dp(lam)):
        return raw(0, nR, dp(r), 1, dp(w), nL, lam_p, dp(n_r), dp(n_i), n_mu, mu_p, dp(w_mu), a["n_max"], a["l_max"], 0, 0,
                   *[dp(o) for o in out], None)

    for kw, text in ((dict(nL=0), "nL"), (dict(n_mu=0), "n_mu"), (dict(nR=0), "nR"), (dict(mu_p=None), "null"), (dict(lam_p=None), "null")):
        assert call(**kw) == L.MOM_EINVAL, kw
        assert text in lib.mom_last_global_error().decode(), (kw, lib.mom_last_global_error().decode())
    assert call() == L.MOM_OK
    # mom_mie_tables
    for kw in (dict(n_max=0, l_max=3), dict(n_max=3, l_max=0)):
        with pytest.raises(L.MomError) as e:
            L.mie_tables(base["mu"], **kw)
        assert e.value.code == L.MOM_EINVAL and "mom_mie_tables" in str(e.value)
