"""The absorption path (csrc/voigt.hip; the mom_voigt_* / mom_absorption_* entry points) where its other tests do not look: the
accuracy of w and w' point by point on both branches, windows on the boundaries of the 256-point blocks, holes and further batches
in the ordered compaction, the interval search on non-uniform grids and at the TIPS knots, and the per-layer sortedness flag.
The cases come from tests/voigt_cases.py; tests/test_oracle_voigt_edges.py checks the same constructions without a GPU."""
import numpy as np
import pytest

import absdual_oracle as ado
import voigt_cases as vc

pytestmark = pytest.mark.gpu


def distance(got, ref, what, bar):
    """max |got - ref| / max |ref|, printed, asserted against bar"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, what
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max() / scale
    print(f"{what}: {err:.2e} of max (bar {bar:.0e})")
    assert scale > 0 and err <= bar, f"{what}: {err:.3e} > {bar:.1e}"
    return err


# ---- A. per-point accuracy of w and w' ---------------------------------------------------------------------------------
def test_pointwise_accuracy_of_w_and_its_derivative(rtamd, cref):
    """One line with b = cSqrtLn2 / gamma_d = 1 and nu = 0, so that x is the grid: 4095 points from 0 to 1e6 on both sides, nine
    values of y from 1e-8 to 1e4, |x| + y == 8 met exactly in three of them.  The arbiter is the forward-mode oracle in
    np.longdouble, the yardstick E_oracle64 the same oracle in Float64; per branch and quantity, pooled over the rows, the
    kernels may stand 4 times as far from the arbiter as the yardstick does (the rule of tests/test_gpu_precision.py) -- in the
    norms of voigt_cases.accuracy_errors: the far branch relative to the value at the point, the near branch relative to the
    size of the terms it adds up.  The kernels differ from the oracle's text by rcp_refined / div_refined for the IEEE division,
    one real reciprocal for Smith's complex division, and FMA contraction.

    Measured on an MI355X, pooled over the nine rows:
                      E_gpu value kernel   E_gpu Dual kernel   E_oracle64   C oracle
      near value           6.44e-15            6.44e-15         6.02e-15    6.02e-15
      far value            2.19e-15            2.19e-15         2.39e-15    2.04e-15
      near partial            -                8.88e-16         7.91e-16       -
      far partial             -                3.18e-15         3.61e-15       -
    """
    grid = vc.accuracy_grid()
    assert vc.ACC_GAMMA_D == ado.C_SQRTLN2 == vc.kernel_constant("cSqrtLn2")      # b = 1.0, x = grid, exactly
    rows = {"value kernel": [], "Dual kernel": [], "oracle64": [], "C oracle": []}
    for y in vc.ACC_Y:
        line = vc.accuracy_line(y)
        far = vc.accuracy_far(y)
        if y in vc.ACC_EXACT8:      # the branch decision itself: points with |x| + y == 8, a neighbour on either side
            exact = np.flatnonzero(np.abs(grid) + y == 8.0)
            assert exact.size == 2 and not far[exact[0] + 1] and far[exact[0] - 1] and not far[exact[1] - 1] and far[exact[1] + 1]
        _, (s64, J64) = vc.accuracy_reference(y)
        sig = rtamd.voigt_xsec(*line[:4], line[8], line[9], grid)
        sig_d, J = rtamd._lib.voigt_xsec_dual(*line, grid)
        rows["value kernel"].append(vc.accuracy_errors(y, sig))
        rows["Dual kernel"].append(vc.accuracy_errors(y, sig_d, J))
        rows["oracle64"].append(vc.accuracy_errors(y, s64, J64))
        rows["C oracle"].append(vc.accuracy_errors(y, cref.voigt_xsec(*line[:4], line[8], line[9], grid)))
        print(f"y = {y:g}: " + "; ".join(f"{who} " + ", ".join(f"{k} {v:.2e}" for k, v in r[-1].items()) for who, r in rows.items()))
    E = {who: vc.pool(r) for who, r in rows.items()}
    for norm, e64 in E["oracle64"].items():
        print(f"{norm}: E_gpu value kernel {E['value kernel'].get(norm, float('nan')):.2e}, Dual kernel {E['Dual kernel'][norm]:.2e}, "
              f"E_oracle64 {e64:.2e}, C oracle {E['C oracle'].get(norm, float('nan')):.2e} (bar {4 * e64:.2e})")
    assert set(E["oracle64"]) == {"near value", "far value", "near partial", "far partial"} and min(E["oracle64"].values()) > 0
    bad = [f"{who}, {norm}: {e:.2e} > 4 x {E['oracle64'][norm]:.2e}" for who in ("value kernel", "Dual kernel")
           for norm, e in E[who].items() if not e <= 4 * E["oracle64"][norm]]
    assert not bad, bad


# ---- B. windows on block boundaries, holes in the compaction, more than 256 candidates ---------------------------------
@pytest.mark.parametrize("name,order", vc.WINDOW_CASES)
def test_windows_on_block_boundaries(rtamd, cref, name, order):
    """Windows that end on, start on and straddle the boundaries of the blocks [1, 256], [257, 512], [513, 768], [769, 777], an
    empty one, stretches no window covers; 600 and 700 lines whose candidates fill three batches of 256, with a wave that has no
    hit and ragged masks in the others.  As listed (the monotone lists take the bisection) and shuffled (the strided pass);
    value and Dual kernel against the oracles in the same line order at 1e-13 of the maximum, exactly 0.0 wherever no window
    is and non-zero wherever one is."""
    a = vc.window_case(name, order)
    i0, i1 = a[8], a[9]
    assert vc.monotone(i0, i1) == (name in vc.MONOTONE_LISTS and (order == "listed" or name == "600_full"))
    sig_o, J_o = vc.window_reference(name, order)
    sig = rtamd.voigt_xsec(*a[:4], i0, i1, vc.EDGE_GRID)
    sig_d, J = rtamd._lib.voigt_xsec_dual(*a, vc.EDGE_GRID)
    distance(sig, cref.voigt_xsec(*a[:4], i0, i1, vc.EDGE_GRID), "sigma, value kernel vs the C oracle", 1e-13)
    distance(sig_d, sig_o, "sigma, Dual kernel vs oracle", 1e-13)
    for k in range(2):
        distance(J[:, k], J_o[:, k], f"dsigma[{k}] vs oracle", 1e-13)
    c = vc.covered(i0, i1)
    assert c.any() and (c.all() or name in ("monotone", "monotone_with_empty", "all"))
    for what, q in (("sigma", sig), ("sigma (Dual)", sig_d), ("dsigma[0]", J[:, 0]), ("dsigma[1]", J[:, 1])):
        assert np.all(q[~c] == 0.0), f"{what}: non-zero at points no window covers: {np.flatnonzero(q[~c] != 0.0)[:8]}"
        assert np.all(q[c] != 0.0), f"{what}: zero at covered points {np.flatnonzero(c)[q[c] == 0.0][:8] + 1}"


# ---- C. device-side prefactors on non-uniform grids --------------------------------------------------------------------
def run_profiles(rtamd, tab, grid, p, T, vcd, wing, layer_by_layer=True):
    """compute_absorption_profile(device_prefactors=True), value and Dual: (tau_abs, prefactors of the last layer) of the value
    run, (tau_abs, dtau_abs, prefactors, their partials) of the Dual run, tau_abs of the layer-by-layer entry"""
    ab = rtamd.absorption
    kw = dict(wing_cutoff=wing, model_vmr=vc.MODEL_VMR, device_prefactors=True)
    Nz = len(p)
    with rtamd.Handle(4, 1, grid.size, 1) as h, rtamd.Handle(4, 1, grid.size, 1) as hd:
        assert ab.compute_absorption_profile(h, tab, grid, p, T, vcd, vc.PROFILE_VMR, **kw) > 0
        value = h.absorption_get(), h.absorption_get_prefactors()
        assert ab.compute_absorption_profile(hd, tab, grid, p, T, vcd, vc.PROFILE_VMR, dual=True, **kw) > 0
        dual = hd.absorption_get(), hd.absorption_get_partials(), hd.absorption_get_prefactors(), hd.absorption_get_prefactor_partials()
        assert dual[1].shape == (2, grid.size, Nz)
        lbl = None
        if layer_by_layer:
            ab.compute_absorption_profile(h, tab, grid, p, T, vcd, vc.PROFILE_VMR, layer_by_layer=True, **kw)
            lbl = h.absorption_get()
    return value, dual, lbl


def check_prefactors(got, dgot, ref, dref):
    """the last layer's prefactors and partials against absref.line_parameters / ado.line_parameters_dual: identical windows, nu
    bitwise, the rest at the bars of test_device_side_line_prefactors and test_device_side_prefactor_partials"""
    nu, gd, y, S, i0, i1 = got
    onu, ogd, oy, oS, oi0, oi1 = ref
    assert nu.size == onu.size
    assert np.array_equal(i0, oi0), f"window starts differ at lines {np.flatnonzero(i0 != oi0)[:8]}: {i0[i0 != oi0][:8]} vs {oi0[i0 != oi0][:8]}"
    assert np.array_equal(i1, oi1), f"window stops differ at lines {np.flatnonzero(i1 != oi1)[:8]}: {i1[i1 != oi1][:8]} vs {oi1[i1 != oi1][:8]}"
    assert np.array_equal(nu, onu)
    np.testing.assert_allclose(gd, ogd, rtol=1e-15)
    np.testing.assert_allclose(y, oy, rtol=4e-15)
    np.testing.assert_allclose(S, oS, rtol=1e-9)
    if dgot is not None:
        dnu, dgd, dy, dS = dgot
        onu, ogd, oy, oS = dref[:4]
        assert np.array_equal(dnu, onu.d.T)
        np.testing.assert_allclose(dgd, ogd.d.T, rtol=1e-15)
        np.testing.assert_allclose(dy, oy.d.T, rtol=4e-15)
        np.testing.assert_allclose(dS, oS.d.T, rtol=1e-6)


def check_layers(cref, key, tab, grid, p, T, vcd, wing, tau, tau_d, dtau, what):
    """tau_abs (value and Dual run) of every layer within 1e-9 of absref + the C oracle's Voigt sum, dtau_abs within 1e-6 of the
    forward-mode oracle, each of its column's maximum; returns the largest distances"""
    worst = [0.0, 0.0]
    for iz in range(len(p)):
        prm, _, _, J_o = vc.layer_reference(key, tab, grid, p[iz], T[iz], vc.MODEL_VMR, wing)
        f = vcd[iz] * vc.PROFILE_VMR
        ref = cref.voigt_xsec(*prm, grid) * f
        worst[0] = max(worst[0], distance(tau[:, iz], ref, f"{what} tau_abs layer {iz}", 1e-9),
                       distance(tau_d[:, iz], ref, f"{what} tau_abs layer {iz}, Dual run", 1e-9))
        for k in range(2):
            worst[1] = max(worst[1], distance(dtau[k][:, iz], J_o[:, k] * f, f"{what} dtau_abs[{k}] layer {iz}", 1e-6))
    return worst


@pytest.mark.parametrize("name", vc.GRID_NAMES)
def test_device_prefactors_on_nonuniform_grids(rtamd, cref, name):
    """locate_interval guesses the interval from the mean spacing, walks three steps at the most and otherwise bisects: on a
    uniform grid the guess is right.  Geometric, two-band, jittered and quadratic grids, and grids of two and three points."""
    tab, grid = vc.o2a_lines(), vc.profile_grid(name)
    key = ("nonuniform", name)
    ref, dref, _, _ = vc.layer_reference(key, tab, grid, vc.P_FULL[-1], vc.T_FULL[-1], vc.MODEL_VMR, vc.WING)
    if name in vc.TIE_CHECKED:      # no interpolated index near a half-integer: identical windows are a fair demand
        for p in vc.P_FULL:
            nu = tab.νᵢ + p / 1013.25 * tab.δ_air
            assert vc.tie_distance(nu, grid, vc.WING) > 1e-6
        assert vc.tie_distance(ref[0], grid, vc.WING) > 1e-6
    (tau, pf), (tau_d, dtau, pf_d, dpf), lbl = run_profiles(rtamd, tab, grid, vc.P_FULL, vc.T_FULL, vc.VCD, vc.WING)
    check_prefactors(pf, None, ref, None)
    check_prefactors(pf_d, dpf, ref, dref)
    assert np.array_equal(tau, lbl)          # the profile entry against one call per layer: the same arithmetic
    check_layers(cref, key, tab, grid, vc.P_FULL, vc.T_FULL, vc.VCD, vc.WING, tau, tau_d, dtau, name)


def test_window_ends_on_grid_nodes(rtamd):
    """nu - wing exactly on an interior node, on grid[0], nu + wing exactly on grid[-1], and each one np.nextafter to either side"""
    tab = vc.node_lines()
    p, T, vcd = vc.P_FULL[-2:], vc.T_FULL[-2:], vc.VCD[-2:]
    key = ("nodes",)
    ref, dref, _, _ = vc.layer_reference(key, tab, vc.NODE_GRID, p[-1], T[-1], vc.MODEL_VMR, vc.NODE_WING)
    (tau, pf), (tau_d, dtau, pf_d, dpf), lbl = run_profiles(rtamd, tab, vc.NODE_GRID, p, T, vcd, vc.NODE_WING)
    assert np.array_equal(ref[4][:3], [1, 1, 1]) and np.array_equal(ref[5][-3:], [1281] * 3)
    check_prefactors(pf, None, ref, None)
    check_prefactors(pf_d, dpf, ref, dref)
    assert np.array_equal(tau, lbl)


# ---- D. TIPS knots -----------------------------------------------------------------------------------------------------
def test_tips_knots(rtamd):
    """The spline search starts at the second knot (the knots are 1, 20, 40, ...: uniform only from there on).  The first
    interval, T exactly on three knots and the last interval; S against absref at 1e-9, dS/dT against the forward-mode oracle at
    1e-6; T on or outside the ends of the table is refused."""
    ab = rtamd.absorption
    tab = vc.tips_lines()
    temps, knots = vc.tips_temperatures(tab)
    one = np.ones(1)
    with rtamd.Handle(4, 1, vc.TIPS_GRID.size, 1) as h, rtamd.Handle(4, 1, vc.TIPS_GRID.size, 1) as hd:
        for T in temps:
            ref, dref, _, _ = vc.layer_reference(("tips",), tab, vc.TIPS_GRID, 480.0, T, vc.MODEL_VMR, vc.TIPS_WING)
            assert np.all(np.isfinite(ref[3])) and np.all(ref[3] > 0) and ref[3].size == 40
            kw = dict(wing_cutoff=vc.TIPS_WING, model_vmr=vc.MODEL_VMR, device_prefactors=True)
            ab.compute_absorption_profile(h, tab, vc.TIPS_GRID, 480.0 * one, T * one, 1e24 * one, 0.3, **kw)
            ab.compute_absorption_profile(hd, tab, vc.TIPS_GRID, 480.0 * one, T * one, 1e24 * one, 0.3, dual=True, **kw)
            pf, pf_d, dpf = h.absorption_get_prefactors(), hd.absorption_get_prefactors(), hd.absorption_get_prefactor_partials()
            print(f"T = {T:g}: S vs absref {np.max(np.abs(pf[3] / ref[3] - 1)):.2e} (bar 1e-9), "
                  f"dS/dT vs oracle {np.max(np.abs(dpf[3][tab.E_lower != -1, 1] / dref[3].d[1][tab.E_lower != -1] - 1)):.2e} (bar 1e-6)")
            check_prefactors(pf, None, ref, None)
            check_prefactors(pf_d, dpf, ref, dref)
            assert np.array_equal(pf[3], pf_d[3]) and dpf[3][7, 1] == 0.0 and np.all(dpf[3][tab.E_lower != -1, 1] != 0.0)
        for T in (knots[0], knots[-1], 0.5, knots[-1] + 1.0):
            for dual in (False, True):
                with pytest.raises(rtamd.MomError) as e:
                    ab.compute_absorption_profile(h, tab, vc.TIPS_GRID, 480.0 * one, float(T) * one, 1e24 * one, 0.3, dual=dual, **kw)
                assert "TIPS2017" in str(e.value)


# ---- E. per-layer sortedness -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", ["as_given", "reversed"])
@pytest.mark.parametrize("lines", list(vc.SORT_LINES))
def test_window_order_flips_between_layers(rtamd, cref, lines, layers):
    """Pressure shifts of alternating sign: the windows are monotone in the line index at 5 hPa and not at 120, 480 and 930 hPa, so
    one profile launch holds layers that bisect and layers that scan -- a flag that wrongly says "sorted" drops lines.  "flipping":
    neighbours change places; "crossing": a line passes eighteen others and its window a whole block (measured with the flag forced
    to "sorted": the first list still passes at these bars, the second is off by 1e-6 of the maximum at 120 hPa and by 0.4 at
    930 hPa)."""
    tab = vc.SORT_LINES[lines]()
    order = slice(None) if layers == "as_given" else slice(None, None, -1)
    p, vcd = vc.P_FULL[order], vc.VCD[order]
    T = np.full(4, vc.SORT_T)
    key = (lines,)
    mono = [vc.monotone(*vc.layer_reference(key, tab, vc.SORT_GRID, q, vc.SORT_T, vc.MODEL_VMR, vc.SORT_WING)[0][4:]) for q in p]
    assert mono == [True, False, False, False][order]
    (tau, _), (tau_d, dtau, _, _), lbl = run_profiles(rtamd, tab, vc.SORT_GRID, p, T, vcd, vc.SORT_WING)
    assert np.array_equal(tau, lbl)
    check_layers(cref, key, tab, vc.SORT_GRID, p, T, vcd, vc.SORT_WING, tau, tau_d, dtau, f"{lines}, {layers}:")


@pytest.mark.parametrize("order", ["steady_first", "steady_last"])
@pytest.mark.parametrize("lines", list(vc.SORT_LINES))
def test_two_absorbers_of_different_order_on_one_handle(rtamd, cref, lines, order):
    """a list that is monotone in every layer and one that is not, accumulated on one handle (begin=False) in both orders"""
    ab = rtamd.absorption
    tabs = {"steady": vc.steady_lines(), lines: vc.SORT_LINES[lines]()}
    seq = ["steady", lines][::1 if order == "steady_first" else -1]
    T = np.full(4, vc.SORT_T)
    S = vc.SORT_GRID.size
    ref, dref = np.zeros((S, 4)), np.zeros((2, S, 4))
    for name in seq:
        for iz in range(4):
            prm, _, _, J_o = vc.layer_reference((name,), tabs[name], vc.SORT_GRID, vc.P_FULL[iz], vc.SORT_T, vc.MODEL_VMR, vc.SORT_WING)
            f = vc.VCD[iz] * vc.PROFILE_VMR
            ref[:, iz] += cref.voigt_xsec(*prm, vc.SORT_GRID) * f
            dref[:, :, iz] += J_o.T * f
    kw = dict(wing_cutoff=vc.SORT_WING, model_vmr=vc.MODEL_VMR, device_prefactors=True)
    with rtamd.Handle(4, 1, S, 1) as h, rtamd.Handle(4, 1, S, 1) as hd:
        for i, name in enumerate(seq):
            ab.compute_absorption_profile(h, tabs[name], vc.SORT_GRID, vc.P_FULL, T, vc.VCD, vc.PROFILE_VMR, begin=i == 0, **kw)
            ab.compute_absorption_profile(hd, tabs[name], vc.SORT_GRID, vc.P_FULL, T, vc.VCD, vc.PROFILE_VMR, begin=i == 0, dual=True, **kw)
        tau, tau_d, dtau = h.absorption_get(), hd.absorption_get(), hd.absorption_get_partials()
    for iz in range(4):
        distance(tau[:, iz], ref[:, iz], f"tau_abs layer {iz}, {seq[0]} then {seq[1]}", 1e-9)
        distance(tau_d[:, iz], ref[:, iz], f"tau_abs layer {iz}, Dual run", 1e-9)
        for k in range(2):
            distance(dtau[k][:, iz], dref[k][:, iz], f"dtau_abs[{k}] layer {iz}", 1e-6)


# ---- F. the handle's line buffers across entry points ------------------------------------------------------------------
def test_line_buffers_across_entry_points_on_one_handle(rtamd):
    """One handle per column (value, Dual) takes, in this order: a three-layer profile of 300 lines, the single-layer device
    entry, a host-prefactor call on one layer, a three-layer profile of 2500 lines (begin=False) -- so the resident line buffers
    change their layer count twice and outgrow their first capacity (2048 lines) -- and then the getters.  600 grid points: three
    workgroups, the last one partial.  Every call is repeated alone on a fresh handle; tau_abs and dtau_abs of the sequence equal
    the fresh tables added on the host in the same order, and the getters return the last layer of the last call, all bitwise."""
    ab = rtamd.absorption
    grid = np.linspace(12903.0, 13245.0, 600)
    small, big = ab.synthetic_o2a_lines(300), ab.synthetic_o2a_lines(2500, seed=4321)
    p, T, f = vc.P_FULL[1:], vc.T_FULL[1:], vc.VCD[1:] * vc.PROFILE_VMR
    wing, S = 3.0, grid.size
    kw = dict(wing_cutoff=wing, model_vmr=vc.MODEL_VMR, device_prefactors=True)
    pf, *dpf = ab.line_prefactors_dual(small, grid, p[0], T[0], vmr=vc.MODEL_VMR, wing_cutoff=wing, with_γ_l=True)
    assert pf.ν.size == 300
    line, dline = (pf.ν, pf.γ_d, pf.γ_l, pf.y, pf.S), (dpf[0], dpf[1], dpf[4], dpf[2], dpf[3])

    def calls(dual):
        """the four calls of a column, each a function of (handle, first call on it?)"""
        def layer(h, first):
            if first:
                h.absorption_begin(3, grid)
                assert ab.resident_line_table(h, small, grid, wing) == 300
            h.voigt_tau_abs_layer(2, p[1], T[1], vc.MODEL_VMR, wing, f[1])

        def host(h, first):
            if first:
                h.absorption_begin(3, grid)
            if dual:
                h.lineshape_tau_abs_dual(1, *line, *dline, pf.ind_start, pf.ind_stop, f[0])
            else:
                h.lineshape_tau_abs(1, *line, pf.ind_start, pf.ind_stop, f[0])

        def profile(tab):
            return lambda h, first: ab.compute_absorption_profile(h, tab, grid, p, T, vc.VCD[1:], vc.PROFILE_VMR, begin=first, dual=dual, **kw)
        return [profile(small), layer, host, profile(big)]

    def tables(h, dual, partials_exist=True):
        return h.absorption_get(), (h.absorption_get_partials() if dual and partials_exist else np.zeros((2, S, 3)))

    def getters(h, dual):
        out = h.absorption_get_prefactors() + [h.absorption_get_gamma_l()]
        if dual:
            g, dg = h.absorption_get_gamma_l(partials=True)
            out += h.absorption_get_prefactor_partials() + [g, dg]
        return out

    for dual in (False, True):
        seq = calls(dual)
        with rtamd.Handle(4, 1, S, 1) as h:
            for i, call in enumerate(seq):
                call(h, i == 0)
            tau, dtau = tables(h, dual)
            got = getters(h, dual)
        tau_ref, dtau_ref = np.zeros((S, 3)), np.zeros((2, S, 3))
        for i, call in enumerate(seq):
            with rtamd.Handle(4, 1, S, 1) as fresh:
                call(fresh, True)
                t, dt = tables(fresh, dual, partials_exist=i != 1)      # the single-layer device entry has no Dual run
                tau_ref, dtau_ref = tau_ref + t, dtau_ref + dt
                ref = getters(fresh, dual) if i == len(seq) - 1 else None
        assert tau.max() > 0 and np.all(tau[:, 0] > 0)
        assert np.array_equal(tau, tau_ref), f"tau_abs, dual={dual}: {np.flatnonzero((tau != tau_ref).any(axis=1))[:8]}"
        if dual:
            assert np.abs(dtau).max() > 0 and np.array_equal(dtau, dtau_ref)
        assert got[0].size == 2500 and len(got) == len(ref)
        for k, (a, b) in enumerate(zip(got, ref)):
            assert np.array_equal(a, b), f"getter array {k}, dual={dual}"
