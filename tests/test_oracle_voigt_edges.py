"""The constructions of tests/voigt_cases.py against the oracles alone, and the product's host route on the same grids: what makes
the bars of tests/test_gpu_voigt_edges.py fair demands.  No GPU."""
import numpy as np
import pytest

import absdual_oracle as ado
import voigt_cases as vc
from oracle import absref


# ---- A ------------------------------------------------------------------------------------------------------------------
def test_accuracy_grid_and_branches():
    g = vc.accuracy_grid()
    assert g.size == 4095 and np.all(np.diff(g) > 0) and np.array_equal(g, -g[::-1]) and g[-1] == 1e6
    assert vc.ACC_GAMMA_D == ado.C_SQRTLN2 == vc.kernel_constant("cSqrtLn2")
    assert ado.C_SQRTLN2 / vc.ACC_GAMMA_D == 1.0
    assert ado.C_SQRTLN2_DIV_SQRTPI == vc.kernel_constant("cSqrtLn2divSqrtPi")
    for y in vc.ACC_Y:
        far = vc.accuracy_far(y)
        assert far.any() and (y >= 8.0 or (~far).any())
        exact = np.flatnonzero(np.abs(g) + y == 8.0)
        if y in vc.ACC_EXACT8:     # on both sides of 0, a near-branch neighbour inside and a far-branch one outside
            assert exact.size == 2 and np.all(far[exact])
            assert not far[exact[0] + 1] and far[exact[0] - 1] and not far[exact[1] - 1] and far[exact[1] + 1]
            # the two approximations are far apart there, so `>` for `>=` would show: the near form evaluated on the far point
            (sa, _), _ = vc.accuracy_reference(y)
            z = ado.Dual(np.array([g[exact[1]] + 1j * y]), np.zeros((2, 1), dtype=complex))
            w_far = ado.w_hw32sd_dual(z, np.float64).v.real[0]
            w_near = ado.w_hw32sd_dual(ado.Dual(z.v - 1e-9, z.d), np.float64).v.real[0]
            assert abs(w_far - w_near) > 1e-7 * abs(w_far)


def test_float64_oracle_in_the_accuracy_norms(cref):
    """The Float64 oracle and the C oracle stay below 1e-14 of the arbiter in every norm of case A (measured: near value 7e-15,
    far value 2.2e-15, far partial 3.1e-15), and no partial of the far branch passes through zero."""
    rows, rows_c = [], []
    for y in vc.ACC_Y:
        (sa, Ja), (s64, J64) = vc.accuracy_reference(y)
        far = vc.accuracy_far(y)
        assert np.all(sa[far] > 0) and np.all(Ja[far] > 0)
        rows.append(vc.accuracy_errors(y, s64, J64))
        line = vc.accuracy_line(y)
        rows_c.append(vc.accuracy_errors(y, cref.voigt_xsec(*line[:4], line[8], line[9], vc.accuracy_grid())))
    E, Ec = vc.pool(rows), vc.pool(rows_c)
    print("E_oracle64:", {k: f"{v:.2e}" for k, v in E.items()}, " C oracle:", {k: f"{v:.2e}" for k, v in Ec.items()})
    assert set(E) == {"near value", "far value", "near partial", "far partial"}
    assert 0 < min(E.values()) and max(E.values()) <= 1e-14 and max(Ec.values()) <= 1e-14


# ---- B ------------------------------------------------------------------------------------------------------------------
def test_window_lists():
    for name in vc.MONOTONE_LISTS:
        a = vc.window_case(name, "listed")
        assert vc.monotone(a[8], a[9]), name
    for name in ("all", "wide", "700_ragged"):
        a = vc.window_case(name, "listed")
        assert not vc.monotone(a[8], a[9]), name
    every = {w for name in ("monotone", "monotone_with_empty") for w in vc.WINDOW_LISTS[name]}
    assert every == set(vc.WINDOWS)
    i0, i1 = vc.window_case("monotone_with_empty", "listed")[8:]
    k = int(np.flatnonzero(i1 < i0)[0])
    assert 0 < k < len(i0) - 1                                  # the empty window stands inside the list
    c = vc.covered(*vc.window_case("all", "listed")[8:])
    assert c.sum() == 2 + 255 + 1 + 10 and not c[:255].any() and not c[513:767].any()   # stretches no window covers
    # the ragged list: in the second block the second wave of the first batch has no hit, in the third every wave has holes
    i0, i1 = (np.array(q) for q in zip(*vc.WINDOW_LISTS["700_ragged"]))
    hit2 = (i0 <= 512) & (i1 >= 257)
    hit3 = (i0 <= 768) & (i1 >= 513)
    assert not hit2[64:128].any() and hit2[:64].all() and hit2[128:].all()
    for w in range(0, 700, 64):
        assert 0 < hit3[w:w + 64].sum() < min(64, 700 - w) or (w == 64 and hit3[w:w + 64].all())
    i0, i1 = (np.array(q) for q in zip(*vc.WINDOW_LISTS["700_monotone_hole"]))
    assert np.all(i1[64:128] < i0[64:128])


@pytest.mark.parametrize("name,order", vc.WINDOW_CASES)
def test_window_cases_two_oracles_agree(cref, name, order):
    """the forward-mode oracle and the C oracle, each in the case's line order: 1e-14 of the maximum, exact zeros where no window is"""
    a = vc.window_case(name, order)
    sig, J = vc.window_reference(name, order)
    if len(a[0]) < 20:      # the all-lines-at-once form of the oracle is the oracle, bit for bit
        sig_l, J_l = ado.voigt_sum_dual(*a, vc.EDGE_GRID)
        assert np.array_equal(sig, sig_l) and np.array_equal(J, J_l)
    ref = cref.voigt_xsec(*a[:4], a[8], a[9], vc.EDGE_GRID)
    assert np.max(np.abs(sig - ref)) <= 1e-14 * ref.max()
    c = vc.covered(a[8], a[9])
    assert np.all(ref[~c] == 0.0) and np.all(sig[~c] == 0.0) and np.all(J[~c] == 0.0)
    assert np.all(ref[c] != 0.0) and np.all(sig[c] != 0.0) and np.all(J[c] != 0.0)


# ---- C ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vc.GRID_NAMES)
def test_host_route_windows_on_nonuniform_grids(name):
    """absorption.line_prefactors against oracle/absref.line_parameters on the grids of case C: identical windows and nu in every
    layer; on the four long grids no interpolated index within 1e-6 of a half-integer."""
    import rtamd
    tab, grid = vc.o2a_lines(), vc.profile_grid(name)
    assert np.all(np.diff(grid) > 0)
    if name in vc.TIE_CHECKED:
        d = np.diff(grid)
        assert grid.size == 4000 and d.max() > 1.02 * d.min()
    for p, T in zip(vc.P_FULL, vc.T_FULL):
        pf = rtamd.absorption.line_prefactors(tab, grid, p, T, vmr=vc.MODEL_VMR, wing_cutoff=vc.WING)
        with vc.memoised_spline_setup():
            nu, gd, y, S, i0, i1 = absref.line_parameters(vc.hit_columns(tab), grid, p, T, vc.MODEL_VMR, vc.WING)
        assert np.array_equal(pf.ν, nu) and np.array_equal(pf.ind_start, i0) and np.array_equal(pf.ind_stop, i1)
        assert np.all(i0 >= 1) and np.all(i1 <= grid.size) and np.all(i0 <= i1)
        if name in vc.TIE_CHECKED:
            assert vc.tie_distance(nu, grid, vc.WING) > 1e-6


def test_host_route_window_ends_on_grid_nodes():
    import rtamd
    tab = vc.node_lines()
    pf = rtamd.absorption.line_prefactors(tab, vc.NODE_GRID, 480.0, 262.25, vmr=vc.MODEL_VMR, wing_cutoff=vc.NODE_WING)
    nu, _, _, _, i0, i1 = absref.line_parameters(vc.hit_columns(tab), vc.NODE_GRID, 480.0, 262.25, vc.MODEL_VMR, vc.NODE_WING)
    assert nu.size == 9 and np.array_equal(nu, tab.νᵢ)
    assert np.array_equal(pf.ind_start, i0) and np.array_equal(pf.ind_stop, i1)
    assert np.array_equal(i0[:3], [1, 1, 1]) and np.array_equal(i1[-3:], [1281] * 3) and np.array_equal(i0[3:6], [321] * 3)


# ---- D ------------------------------------------------------------------------------------------------------------------
def test_tips_knot_temperatures():
    """S(T) of the oracle is finite and positive at every temperature of case D; the host route agrees at the existing bars"""
    import rtamd
    ab = rtamd.absorption
    tab = vc.tips_lines()
    temps, knots = vc.tips_temperatures(tab)
    assert temps[-1] == knots[-1] - 10.0 and temps[0] < knots[1]
    hit = vc.hit_columns(tab)
    for T in temps:
        S = absref.line_parameters(hit, vc.TIPS_GRID, 480.0, T, vc.MODEL_VMR, vc.TIPS_WING)[3]
        assert S.size == 40 and np.all(np.isfinite(S)) and np.all(S > 0)
        pf, _, _, _, dS = ab.line_prefactors_dual(tab, vc.TIPS_GRID, 480.0, T, vmr=vc.MODEL_VMR, wing_cutoff=vc.TIPS_WING)
        Sd = ado.line_parameters_dual(hit, vc.TIPS_GRID, 480.0, T, vc.MODEL_VMR, vc.TIPS_WING)[3]
        np.testing.assert_allclose(pf.S, S, rtol=1e-9)
        np.testing.assert_allclose(dS[:, 1], Sd.d[1], rtol=1e-6)
        assert np.all(Sd.d[1][tab.E_lower != -1] != 0)
    for T in (knots[0], knots[-1], 0.5, knots[-1] + 1.0):
        with pytest.raises(AssertionError, match="TIPS2017"):
            absref.line_parameters(hit, vc.TIPS_GRID, 480.0, float(T), vc.MODEL_VMR, vc.TIPS_WING)


# ---- E ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lines", list(vc.SORT_LINES))
def test_window_order_flips_with_pressure(lines):
    hit, hit_s = vc.hit_columns(vc.SORT_LINES[lines]()), vc.hit_columns(vc.steady_lines())
    for p, mono in zip(vc.P_FULL, (True, False, False, False)):
        with vc.memoised_spline_setup():
            i0, i1 = absref.line_parameters(hit, vc.SORT_GRID, p, vc.SORT_T, vc.MODEL_VMR, vc.SORT_WING)[4:]
            i0s, i1s = absref.line_parameters(hit_s, vc.SORT_GRID, p, vc.SORT_T, vc.MODEL_VMR, vc.SORT_WING)[4:]
        assert i0.size == 200 and vc.monotone(i0, i1) == mono
        assert i0s.size == 150 and vc.monotone(i0s, i1s)
    if lines == "crossing":     # at 930 hPa a window stops more than a block before one of an earlier line
        assert np.max(np.maximum.accumulate(i1) - i1) > vc.BLOCK and np.max(np.maximum.accumulate(i0) - i0) > vc.BLOCK
