"""The Dual run of the Voigt absorption path (k_voigt_dual, k_line_prefactors_profile<true> in csrc/voigt.hip; the
mom_voigt_*_dual / mom_absorption_get_partials entry points) against the forward-mode oracle tests/absdual_oracle.py:
sigma and its partials with respect to (p, T) as absorption_cross_section(...; autodiff = true) returns them."""
import dataclasses
from pathlib import Path

import numpy as np
import pytest

import absdual_oracle as ado
from oracle import absref
from test_oracle_absdual import CASES, GRID, hit_columns, lines24, oracle64  # noqa: F401  (oracle64: the shared fixture)

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).parent / "golden"


def assert_columns_close(got, ref, rtol, what):
    """|got - ref| <= rtol * max|ref| per column"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, what
    g2, r2 = got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1)
    for k in range(r2.shape[1]):
        scale = np.abs(r2[:, k]).max()
        err = np.abs(g2[:, k] - r2[:, k]).max()
        print(f"{what} column {k}: {err / scale if scale else err:.2e} of max (bar {rtol:.0e})")
        assert err <= rtol * scale, f"{what} column {k}: {err / scale if scale else err:.3e} > {rtol:.1e}"


def random_partials(rng, nu, gd, y, S):
    n = len(nu)
    return (1e-3 * rng.normal(size=(n, 2)), 0.01 * gd[:, None] * rng.normal(size=(n, 2)), 0.01 * y[:, None] * rng.normal(size=(n, 2)),
            0.01 * S[:, None] * rng.normal(size=(n, 2)))


# ---- 1. kernel against oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(3))
def test_kernel_against_oracle(rtamd, oracle64, case):
    sig_o, J_o, (nu, gd, y, S, i0, i1) = oracle64[case]
    args = (nu.v, gd.v, y.v, S.v, nu.d.T, gd.d.T, y.d.T, S.d.T, i0, i1, GRID)
    sig, J = rtamd._lib.voigt_xsec_dual(*args)
    assert J.shape == (GRID.size, 2) and np.abs(J_o[:, 0]).max() > 0 and np.abs(J_o[:, 1]).max() > 0
    assert_columns_close(sig, sig_o, 1e-13, "sigma vs oracle")
    assert_columns_close(J, J_o, 1e-13, "dsigma vs oracle")
    assert_columns_close(sig, rtamd.voigt_xsec(nu.v, gd.v, y.v, S.v, i0, i1, GRID), 1e-13, "sigma vs the value kernel")
    sig2, J2 = rtamd._lib.voigt_xsec_dual(*args)
    assert np.array_equal(sig, sig2) and np.array_equal(J, J2)      # no atomics: reproducible
    assert rtamd._lib.voigt_last_kernel_ms() > 0


# ---- 2. edges, on a 777-point grid (a ragged last workgroup) ------------------------------------------------------------
EDGE_GRID = np.linspace(100.0, 101.0, 777)


def test_no_lines(rtamd):
    e = np.zeros(0)
    sig, J = rtamd._lib.voigt_xsec_dual(e, e, e, e, np.zeros((0, 2)), None, None, None, [], [], EDGE_GRID)
    assert np.array_equal(sig, np.zeros(777)) and np.array_equal(J, np.zeros((777, 2)))


def test_window_edges_and_far_wings(rtamd):
    """a one-point window, an empty window (start > stop), a full window; far wings hit the humlicek2 branch"""
    nu = np.array([100.5, 100.2, 100.9]); gd = np.array([1e-3, 2e-3, 5e-4]); y = np.array([0.5, 2.0, 1e-3])
    S = np.array([1e-20, 2e-20, 3e-20]); i0 = [300, 500, 1]; i1 = [300, 499, 777]
    d = random_partials(np.random.default_rng(1), nu, gd, y, S)
    sig, J = rtamd._lib.voigt_xsec_dual(nu, gd, y, S, *d, i0, i1, EDGE_GRID)
    sig_o, J_o = ado.voigt_sum_dual(nu, gd, y, S, *d, i0, i1, EDGE_GRID)
    x = ado.C_SQRTLN2 / gd[2] * (EDGE_GRID - nu[2])
    assert np.any(np.abs(x) + y[2] >= 8) and np.any(np.abs(x) + y[2] < 8)
    assert_columns_close(sig, sig_o, 1e-13, "sigma")
    assert_columns_close(J, J_o, 1e-13, "dsigma")


def test_shuffled_line_order(rtamd, oracle64):
    """windows not monotone in the line index (the strided search): the sum in ITS line order"""
    nu, gd, y, S, i0, i1 = oracle64[0][2]
    perm = np.random.default_rng(0).permutation(nu.v.size)
    assert np.any(np.diff(i0[perm]) < 0)
    a = [np.ascontiguousarray(q[perm]) for q in (nu.v, gd.v, y.v, S.v, nu.d.T, gd.d.T, y.d.T, S.d.T, i0, i1)]
    sig, J = rtamd._lib.voigt_xsec_dual(*a, GRID)
    sig_o, J_o = ado.voigt_sum_dual(*a, GRID)
    assert_columns_close(sig, sig_o, 1e-13, "sigma")
    assert_columns_close(J, J_o, 1e-13, "dsigma")


def test_second_candidate_batch(rtamd):
    """300 lines whose windows all cover every workgroup's range: the candidate loop runs a second batch of 256"""
    rng = np.random.default_rng(7)
    n = 300
    nu = np.sort(rng.uniform(100.0, 101.0, n)); gd = rng.uniform(5e-3, 2e-2, n); y = rng.uniform(0.05, 1.5, n)
    S = 10.0 ** rng.uniform(-22, -20, n)
    i0, i1 = np.ones(n, dtype=np.int32), np.full(n, 777, dtype=np.int32)
    d = random_partials(rng, nu, gd, y, S)
    sig, J = rtamd._lib.voigt_xsec_dual(nu, gd, y, S, *d, i0, i1, EDGE_GRID)
    sig_o, J_o = ado.voigt_sum_dual(nu, gd, y, S, *d, i0, i1, EDGE_GRID)
    assert_columns_close(sig, sig_o, 1e-13, "sigma")
    assert_columns_close(J, J_o, 1e-13, "dsigma")


def test_null_partials_and_bad_window(rtamd, oracle64):
    nu, gd, y, S, i0, i1 = oracle64[0][2]
    sig, J = rtamd._lib.voigt_xsec_dual(nu.v, gd.v, y.v, S.v, None, None, None, None, i0, i1, GRID)
    assert sig.max() > 0 and np.array_equal(J, np.zeros((GRID.size, 2)))
    # one array given, the others NULL: only its term
    sig, J = rtamd._lib.voigt_xsec_dual(nu.v, gd.v, y.v, S.v, None, None, None, S.d.T, i0, i1, GRID)
    _, J_o = ado.voigt_sum_dual(nu.v, gd.v, y.v, S.v, None, None, None, S.d.T, i0, i1, GRID)
    assert_columns_close(J[:, 1], J_o[:, 1], 1e-13, "dsigma/dT from dS alone")
    bad = i0.copy()
    bad[0] = 0
    with pytest.raises(rtamd.MomError) as e:
        rtamd._lib.voigt_xsec_dual(nu.v, gd.v, y.v, S.v, None, None, None, None, bad, i1, GRID)
    assert "mom_voigt_xsec_dual" in str(e.value) and "outside the grid 1..777" in str(e.value)


# ---- 3. resident table -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1])
def test_resident_partials_table(rtamd, dtype):
    """Two absorbers by compute_absorption_profile(dual=True) on the host route: tau_abs as the value route's, dtau_abs
    bitwise the host accumulation of mom_voigt_xsec_dual columns times factor (same kernel, separately rounded product and
    sum).  Float64 and Float32 handles alike (the absorption table is Float64 on both)."""
    ab = rtamd.absorption
    S, Nz = 777, 3
    one, two = lines24(), ab.synthetic_o2a_lines(10, 12999.0, 13003.0, seed=12)
    p_full = np.array([5.0, 480.0, 930.0]); T = np.array([215.0, 262.25, 288.0]); vcd = np.array([1.1e23, 7.7e24, 1.3e25])
    absorbers = ((one, 0.21, 0.21), (two, np.array([4e-4, 4.1e-4, 4.2e-4]), 0.0))
    expect = np.zeros((2, S, Nz))
    for tab, vmr, mv in absorbers:
        for iz in range(Nz):
            v = vmr if np.ndim(vmr) == 0 else vmr[iz]
            _, J = ab.absorption_cross_section(tab, GRID, p_full[iz], T[iz], autodiff=True, vmr=mv, wing_cutoff=1.0)
            for k in range(2):
                expect[k][:, iz] += J[:, k] * (vcd[iz] * v)
    with rtamd.Handle(4, 1, S, 1, dtype=dtype) as h, rtamd.Handle(4, 1, S, 1, dtype=dtype) as hv:
        h.absorption_begin(Nz, GRID)
        with pytest.raises(rtamd.MomError) as e:
            h.absorption_get_partials()                     # no Dual call yet
        assert e.value.code == rtamd._lib.MOM_ESTATE
        for i, (tab, vmr, mv) in enumerate(absorbers):
            ab.compute_absorption_profile(h, tab, GRID, p_full, T, vcd, vmr, wing_cutoff=1.0, model_vmr=mv, begin=i == 0, dual=True)
            ab.compute_absorption_profile(hv, tab, GRID, p_full, T, vcd, vmr, wing_cutoff=1.0, model_vmr=mv, begin=i == 0)
        tau, tau_v, got = h.absorption_get(), hv.absorption_get(), h.absorption_get_partials()
        assert got.shape == (2, S, Nz)
        assert tau_v.max() > 1e-3
        assert_columns_close(tau, tau_v, 1e-13, "tau_abs, Dual route vs value route")
        assert np.abs(expect[0]).max() > 0 and np.abs(expect[1]).max() > 0
        assert np.array_equal(got, expect)
        with pytest.raises(rtamd.MomError) as e:
            h.voigt_tau_abs_dual(4, [1.0], [1.0], [1.0], [1.0], None, None, None, None, [1], [1], 1.0)   # layer out of range
        assert e.value.code == rtamd._lib.MOM_EINVAL and "mom_voigt_tau_abs_dual" in str(e.value)
        h.absorption_begin(Nz, GRID)
        assert np.array_equal(h.absorption_get_partials(), np.zeros((2, S, Nz)))
        h.absorption_set(tau_v)
        with pytest.raises(rtamd.MomError) as e:
            h.absorption_get_partials()
        assert e.value.code == rtamd._lib.MOM_ESTATE


# ---- 4. device-side prefactors -----------------------------------------------------------------------------------------
def line_set(ab, lines):
    """the "o2a", "shuffled" and "co2_file" line sets of test_gpu_voigt.test_device_side_line_prefactors"""
    if lines == "co2_file":
        tab = ab.hitran_table(ab.read_hitran(GOLD / "testCO2.data"))
        return tab, np.linspace(float(tab.νᵢ.min()) - 2.0, float(tab.νᵢ.max()) + 2.0, 3000), 4e-4, 5.0
    tab = ab.synthetic_o2a_lines(400, seed=5)
    if lines == "shuffled":
        perm = np.random.default_rng(3).permutation(tab.νᵢ.size)
        tab = ab.HitranTable(**{f.name: getattr(tab, f.name)[perm] for f in dataclasses.fields(tab)})
        tab.E_lower[::7] = -1.0
    return tab, np.linspace(12920.0, 13230.0, 4000), 0.21, 8.0


@pytest.mark.parametrize("lines", ["o2a", "shuffled", "co2_file"])
def test_device_side_prefactor_partials(rtamd, lines):
    ab = rtamd.absorption
    tab, grid, model_vmr, wing = line_set(ab, lines)
    p_full = np.array([5.0, 480.0, 930.0]); T = np.array([215.0, 262.25, 288.0]); vcd = np.array([1.1e23, 7.7e24, 1.3e25])
    S, Nz = grid.size, 3
    m = rtamd.scenes.make_scene(1, 3, Nz, S)
    with rtamd.corert.make_handle(m) as h_dev, rtamd.corert.make_handle(m) as h_host:
        ab.compute_absorption_profile(h_host, tab, grid, p_full, T, vcd, 0.3, wing_cutoff=wing, model_vmr=model_vmr, dual=True)
        ms = ab.compute_absorption_profile(h_dev, tab, grid, p_full, T, vcd, 0.3, wing_cutoff=wing, model_vmr=model_vmr,
                                           device_prefactors=True, dual=True)
        assert ms > 0
        dev = h_dev.absorption_get_prefactor_partials()
        val = h_dev.absorption_get_prefactors()
        a, da = h_dev.absorption_get(), h_dev.absorption_get_partials()
        b, db = h_host.absorption_get(), h_host.absorption_get_partials()
    hit = hit_columns(tab)
    # the prefactors of the last layer and their partials against the oracle
    nu, gd, y, Sl, i0, i1 = ado.line_parameters_dual(hit, grid, p_full[-1], T[-1], model_vmr, wing)
    assert val[0].size == nu.v.size and np.array_equal(val[4], i0) and np.array_equal(val[5], i1) and np.array_equal(val[0], nu.v)
    dnu, dgd, dy, dS = dev
    assert np.array_equal(dnu, nu.d.T)
    np.testing.assert_allclose(dgd, gd.d.T, rtol=1e-15)
    np.testing.assert_allclose(dy, y.d.T, rtol=4e-15)
    np.testing.assert_allclose(dS, Sl.d.T, rtol=1e-6)
    if lines == "shuffled":
        assert np.any(np.diff(i0) < 0) and np.any(dS[:, 1] == 0)
    # tau_abs and its partials of every layer
    np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-300)
    for k in range(2):
        assert_columns_close(da[k], db[k], 1e-9, f"dtau_abs[{k}] device vs host prefactors")
    for iz in range(Nz):
        sig_o, J_o = ado.cross_section_dual(hit, grid, p_full[iz], T[iz], model_vmr, wing)
        assert_columns_close(a[:, iz], sig_o * (vcd[iz] * 0.3), 1e-9, f"tau_abs layer {iz} vs oracle")
        assert_columns_close(da[:, :, iz].T, J_o * (vcd[iz] * 0.3), 1e-6, f"dtau_abs layer {iz} vs oracle")


def test_profile_dual_refuses_temperature_outside_tips(rtamd):
    ab = rtamd.absorption
    tab, grid, _, wing = line_set(ab, "o2a")
    with rtamd.corert.make_handle(rtamd.scenes.make_scene(1, 3, 1, grid.size)) as h:
        h.absorption_begin(1, grid)
        ab.resident_line_table(h, tab, grid, wing)
        with pytest.raises(rtamd.MomError) as e:
            h.voigt_tau_abs_profile_dual([500.0], [0.5], 0.0, wing, [1.0])
        assert "TIPS2017" in str(e.value)


# ---- 5. absorption_cross_section(autodiff=True) -------------------------------------------------------------------------
def test_absorption_cross_section_autodiff(rtamd):
    ab = rtamd.absorption
    tab = ab.hitran_table(ab.read_hitran(GOLD / "testCO2.data"))
    nu_s = float(tab.νᵢ[np.argmax(tab.Sᵢ)])
    grid = np.linspace(nu_s - 2.0, nu_s + 2.0, 900)
    p, T = 800.0, 270.0
    sig, J = ab.absorption_cross_section(tab, grid, p, T, autodiff=True)
    assert J.shape == (900, 2)
    assert np.array_equal(ab.absorption_cross_section(tab, grid, p, T), ab.compute_absorption_cross_section(tab, grid, p, T))
    ref = absref.absorption_cross_section(hit_columns(tab), grid, p, T)    # the route tests/golden/voigt_co2.npz was made by
    assert_columns_close(sig, ref, 1e-9, "sigma vs the golden route")
    sig_o, J_o = ado.cross_section_dual(hit_columns(tab), grid, p, T)
    assert_columns_close(J, J_o, 1e-6, "Jacobian vs oracle")


# ---- 6. end to end into the Dual run -----------------------------------------------------------------------------------
def test_temperature_jacobian_through_rt_run_dual(rtamd):
    """Parameter: a uniform temperature offset of all layers.  dtau_abs from the Dual profile call -> optics_partials ->
    scene_set_partials / rt_run_dual, against the central difference (dT = 0.02 K) of the value pipeline
    (compute_absorption_profile + rt_run).  Bar 1e-4 max|dR_SFI|: a sanity bar set by the difference, not by the kernels."""
    ab, rt = rtamd.absorption, rtamd.corert
    S, Nz, dT = 256, 3, 0.02
    grid = np.linspace(12999.5, 13002.5, S)
    base = rtamd.scenes.make_scene(1, 9, Nz, S, ν_lo=grid[0], ν_hi=grid[-1], absorption=False)
    assert len(base.quad_points.qp_μN) <= 12
    p_half = rtamd.scenes.pressure_grid(Nz)
    p_full = 0.5 * (p_half[1:] + p_half[:-1])
    T0 = np.array([220.0, 240.0, 280.0])
    vcd = 2.0e25 * np.diff(p_half) / p_half[-1]
    tab = lines24()

    def tables(T, dual):
        with rt.make_handle(base) as h:
            ab.compute_absorption_profile(h, tab, grid, p_full, T, vcd, 0.21, wing_cutoff=1.0, model_vmr=0.21,
                                          device_prefactors=True, dual=dual)
            return h.absorption_get(), (h.absorption_get_partials() if dual else None)

    tau_abs, dtau_abs = tables(T0, True)
    assert tau_abs.max() > 1.0
    models = [dataclasses.replace(base, τ_abs=t) for t in (tau_abs, tables(T0 + dT, False)[0], tables(T0 - dT, False)[0])]
    layers = [rt.construct_layer_inputs(m) for m in models]
    for L in layers[1:]:     # integer decisions of the three runs must agree for the difference to mean anything
        assert np.array_equal(L.ndoubl, layers[0].ndoubl) and np.array_equal(L.iface, layers[0].iface)
    partial = ab.optics_partials(layers[0].τ, layers[0].ϖ, dtau_abs[1])   # each layer's tau_abs depends on its own T only
    _, _, dR, _ = rtamd.rt_run_dual(models[0], [partial])
    Rp, Rm = rtamd.rt_run(models[1])[0], rtamd.rt_run(models[2])[0]
    fd = (Rp - Rm) / (2 * dT)
    scale = np.abs(dR[0]).max()
    err = np.abs(dR[0] - fd).max()
    print(f"dR_SFI/dT vs central difference: {err / scale:.2e} of max (bar 1e-4)")
    assert scale > 0 and err <= 1e-4 * scale
