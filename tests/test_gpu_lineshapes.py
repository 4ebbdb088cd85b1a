"""The selectable absorption model on the GPU (csrc/voigt.hip: the Doppler, Lorentz and Voigt / HW32Voigt instantiations of the
line-shape block; mom_lineshape_xsec, mom_lineshape_tau_abs, mom_absorption_set_model and the device-prefactor entry points that
follow it) against tests/lineshape_oracle.py: block edges and compaction, accuracy point by point, the agreement of the routes,
and the defaults.  tests/test_oracle_lineshapes.py checks the oracle itself without a GPU."""
import functools

import numpy as np
import pytest

import lineshape_oracle as lso
import voigt_cases as vc

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3


def distance(got, ref, what, bar):
    """max |got - ref| / max |ref|, printed, asserted against bar"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, what
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max() / scale
    print(f"{what}: {err:.2e} of max (bar {bar:.0e})")
    assert scale > 0 and err <= bar, f"{what}: {err:.3e} > {bar:.1e}"
    return err


# ---- A. block edges and compaction -------------------------------------------------------------------------------------
EDGE_CASES = [(n, o) for n in ("all", "700_ragged", "700_monotone_hole") for o in ("listed", "shuffled")]


@functools.lru_cache(maxsize=None)
def edge_case(name, order):
    return lso.with_gamma_l(vc.window_case(name, order))


@pytest.mark.parametrize("name,order", EDGE_CASES)
@pytest.mark.parametrize("shape", lso.NEW_SHAPES)
def test_block_edges(rtamd, shape, name, order):
    """The windows of tests/voigt_cases.py on the boundaries of the 256-point blocks (777 grid points: four blocks, the last one
    partial), a wave without a hit, ragged masks, three batches of candidates, as listed (bisection where monotone) and shuffled
    (strided pass), with gamma_l = y gamma_d / sqrt(cLn2) as the fifth prefactor.  Value and Dual kernel against the Float64
    oracle in the same line order at 1e-13 of each column's maximum (the bar of test_gpu_voigt_edges.py); exactly 0.0 where no
    window is; non-zero where one is for Lorentz and HW32Voigt -- the Doppler shape underflows inside these windows, there it is
    finite, not negative, and its partials are finite."""
    a = edge_case(name, order)
    nu, gd, gl, y, S = a[:5]
    i0, i1 = a[10], a[11]
    L = rtamd._lib
    sig_o, J_o = lso.lineshape_sum_dual(shape, *a, vc.EDGE_GRID)
    sig = L.lineshape_xsec(*lso.CODES[shape], nu, gd, gl, y, S, i0, i1, vc.EDGE_GRID)
    sig_d, J = L.lineshape_xsec_dual(*lso.CODES[shape], *a, vc.EDGE_GRID)
    distance(sig, sig_o, f"{shape} sigma, value kernel vs oracle", 1e-13)
    distance(sig_d, sig_o, f"{shape} sigma, Dual kernel vs oracle", 1e-13)
    for k in range(2):
        distance(J[:, k], J_o[:, k], f"{shape} dsigma[{k}] vs oracle", 1e-13)
    c = vc.covered(i0, i1)
    assert c.any()
    for what, q in (("sigma", sig), ("sigma (Dual)", sig_d), ("dsigma[0]", J[:, 0]), ("dsigma[1]", J[:, 1])):
        assert np.all(q[~c] == 0.0), f"{what}: non-zero at points no window covers: {np.flatnonzero(q[~c] != 0.0)[:8]}"
        assert np.all(np.isfinite(q)), what
        if shape != "doppler":
            assert np.all(q[c] != 0.0), f"{what}: zero at covered points {np.flatnonzero(c)[q[c] == 0.0][:8] + 1}"
    assert np.all(sig >= 0.0) and np.all(sig_d >= 0.0) and sig.max() > 0


# ---- B. accuracy point by point ----------------------------------------------------------------------------------------
def pool_rule(E, kernels=("value kernel", "Dual kernel")):
    """per norm, pooled over the rows: the kernels at most 4 times as far from the arbiter as the Float64 oracle"""
    for norm, e64 in E["oracle64"].items():
        print(f"{norm}: " + ", ".join(f"E_gpu {k} {E[k][norm]:.2e}" for k in kernels if norm in E[k]) + f", E_oracle64 {e64:.2e} (bar {4 * e64:.2e})")
    assert min(E["oracle64"].values()) > 0
    bad = [f"{who}, {norm}: {e:.2e} > 4 x {E['oracle64'][norm]:.2e}" for who in kernels for norm, e in E[who].items()
           if not e <= 4 * E["oracle64"][norm]]
    assert not bad, bad


def hw_grid():
    """|x| = 0 .. 16 in steps of 2^-7, then 895 geometrically spaced points to 1e6; symmetric about 0, ascending"""
    near = np.arange(0, 16 * 128 + 1) / 128.0
    pos = np.concatenate([near, np.geomspace(16.0, 1e6, 896)[1:]])
    return np.concatenate([-pos[:0:-1], pos])


def hw_line(y, n):
    """the one line of voigt_cases.accuracy_line (b = cSqrtLn2 / gamma_d = 1, nu = 0: x is the grid), gamma_l as a fifth prefactor"""
    one = lambda v: np.array([float(v)])
    gl = y * vc.ACC_GAMMA_D / np.sqrt(lso.C_LN2)
    return (one(0.0), one(vc.ACC_GAMMA_D), one(gl), one(y), one(1.0), vc.ACC_DNU.copy(), vc.ACC_REL["gd"] * vc.ACC_GAMMA_D, vc.ACC_REL["y"] * gl,
            vc.ACC_REL["y"] * y, vc.ACC_REL["S"] * 1.0, np.array([1], dtype=np.int32), np.array([n], dtype=np.int32))


def hw_errors(y, x, far, arb, sigma, J=None):
    """the four norms of voigt_cases.accuracy_errors with far = region I, against the arbiter (sa, Ja) of the row"""
    sa, Ja = arb
    near = ~far
    xl = x.astype(np.longdouble)
    out = {}
    ds = np.abs(np.asarray(sigma).astype(np.longdouble) - sa)
    if far.any():
        out["far value"] = float(np.max(ds[far] / np.abs(sa[far])))
    if near.any():
        Lw = np.longdouble(np.sqrt(32 / np.sqrt(2)))
        a = np.longdouble(lso.C_SQRTLN2_DIV_SQRTPI) / np.longdouble(vc.ACC_GAMMA_D)
        size = a / np.sqrt((Lw + np.longdouble(y)) ** 2 + xl * xl) / np.sqrt(np.longdouble(np.pi))
        out["near value"] = float(np.max(ds[near] / size[near]))
    if J is not None:
        dJ = np.abs(np.asarray(J).astype(np.longdouble) - Ja)
        if far.any():
            out["far partial"] = float(np.max(dJ[far] / np.abs(Ja[far])))
        if near.any():
            out["near partial"] = float(np.max(dJ[near] / np.abs(Ja[near]).max(axis=0)))
    return out


def test_pointwise_accuracy_hw32voigt(rtamd):
    """w(::HumlicekWeidemann32VoigtErrorFunction, z) and its derivative point by point, by the rule of
    test_gpu_voigt_edges.py::test_pointwise_accuracy_of_w_and_its_derivative: one line with x = the grid (|x| from 0 to 16 in steps
    of 2^-7, then to 1e6), the nine rows y of voigt_cases.ACC_Y; |x| + y == 15 is met exactly for y = 0.5, 2.0, 7.5 and 8.0 and falls,
    with its inner neighbour, on the Weideman side, the next point outward on region I.  np.longdouble arbitrates; pooled over the
    rows, per norm (far = region I relative to the value at the point, near relative to the size of the terms added up), the
    kernels may stand 4 times as far from it as the Float64 oracle does.

    Measured on an MI355X, pooled over the nine rows:
                      E_gpu value kernel   E_gpu Dual kernel   E_oracle64
      near value           6.44e-15            6.44e-15         6.02e-15
      far value            9.70e-16            8.73e-16         9.62e-16
      near partial            -                8.88e-16         7.91e-16
      far partial             -                8.96e-16         1.23e-15
    """
    x = hw_grid()
    L = rtamd._lib
    rows = {"value kernel": [], "Dual kernel": [], "oracle64": []}
    ties = 0
    for y in vc.ACC_Y:
        line = hw_line(y, x.size)
        far = np.abs(x) + y > 15.0
        for t in np.flatnonzero(np.abs(x) + y == 15.0):
            s = 1 if x[t] > 0 else -1
            assert not far[t] and not far[t - s] and far[t + s]
            ties += 1
        arb = lso.lineshape_sum_dual("voigt15", *line, x, FT=np.longdouble)
        s64, J64 = lso.lineshape_sum_dual("voigt15", *line, x)
        sig = L.lineshape_xsec(0, 1, *line[:5], line[10], line[11], x)
        sig_d, J = L.lineshape_xsec_dual(0, 1, *line, x)
        rows["value kernel"].append(hw_errors(y, x, far, arb, sig))
        rows["Dual kernel"].append(hw_errors(y, x, far, arb, sig_d, J))
        rows["oracle64"].append(hw_errors(y, x, far, arb, s64, J64))
        print(f"y = {y:g}: " + "; ".join(f"{who} " + ", ".join(f"{k} {v:.2e}" for k, v in r[-1].items()) for who, r in rows.items()))
    assert ties == 8        # y = 0.5, 2.0, 7.5, 8.0 on either side
    E = {who: vc.pool(r) for who, r in rows.items()}
    assert set(E["oracle64"]) == {"near value", "far value", "near partial", "far partial"}
    pool_rule(E)


DOPPLER_ROWS = ((1.0, 0.0), (0.0123456, 13000.123))      # (gamma_d, nu), S = 1


def simple_errors(shape, g, line, arb, sigma, J=None):
    """value: relative to the arbiter's value; partials: relative to the sum of the magnitudes of the product-rule terms at the
    point (the partial itself crosses zero)"""
    nu, gd, gl, y, S, dnu, dgd, dgl, dy, dS = line[:10]
    sa, Ja = arb
    out = {"value": float(np.max(np.abs(np.asarray(sigma).astype(np.longdouble) - sa) / np.abs(sa)))}
    if J is not None:
        terms = lso.product_rule_terms(shape, g, nu[0], gd[0], gl[0], S[0], dnu, dgd, dgl, dS)
        assert np.all(terms > 0)
        out["partial"] = float(np.max(np.abs(np.asarray(J).astype(np.longdouble) - Ja) / terms))
    return out


def test_pointwise_accuracy_doppler(rtamd):
    """exp(-ln 2 q^2) point by point: q = (g - nu) / gamma_d from -31 to 31 in steps of 2^-6 (every value above 1e-290, none
    subnormal), for a line at 0 with gamma_d = 1 and one at 13000.123 cm^-1 with gamma_d = 0.0123456.  The value relative to the
    arbiter's, the partials relative to the sum of the magnitudes of the product-rule terms; pooled over the rows the kernels may
    stand 4 times as far from np.longdouble as the Float64 oracle does.  The kernel stages S c / gamma_d and 1 / gamma_d per line and
    multiplies where the reference divides: in numpy that form stands 1.2 times the as-written one (1.8e-13 against 1.5e-13, both
    the rounding of the exponent's argument, 666 at the ends).  At |q| = 33, 40, 1e3, 1e6 the exponential underflows: value and
    partials are finite, not negative, below 1e-300.

    Measured on an MI355X, pooled over the two rows:
                 E_gpu value kernel   E_gpu Dual kernel   E_oracle64
      value           1.82e-13            1.82e-13         1.48e-13
      partial            -                1.82e-13         1.48e-13
    """
    L = rtamd._lib
    q = np.arange(-31 * 64, 31 * 64 + 1) / 64.0
    one = lambda v: np.array([float(v)])
    rows = {"value kernel": [], "Dual kernel": [], "oracle64": []}
    for gd, nu in DOPPLER_ROWS:
        g = nu + q * gd
        assert np.all(np.diff(g) > 0)
        line = (one(nu), one(gd), None, None, one(1.0), vc.ACC_DNU.copy(), vc.ACC_REL["gd"] * gd, None, None, vc.ACC_REL["S"] * 1.0,
                np.array([1], dtype=np.int32), np.array([g.size], dtype=np.int32))
        oline = (line[0], line[1], one(0.045), one(0.3)) + line[4:]
        arb = lso.lineshape_sum_dual("doppler", *oline, g, FT=np.longdouble)
        assert arb[0].min() > 1e-290
        s64, J64 = lso.lineshape_sum_dual("doppler", *oline, g)
        sig = L.lineshape_xsec(1, 0, *line[:5], line[10], line[11], g)
        sig_d, J = L.lineshape_xsec_dual(1, 0, *line, g)
        rows["value kernel"].append(simple_errors("doppler", g, oline, arb, sig))
        rows["Dual kernel"].append(simple_errors("doppler", g, oline, arb, sig_d, J))
        rows["oracle64"].append(simple_errors("doppler", g, oline, arb, s64, J64))
        print(f"gamma_d = {gd:g}: " + "; ".join(f"{who} " + ", ".join(f"{k} {v:.2e}" for k, v in r[-1].items()) for who, r in rows.items()))
    pool_rule({who: vc.pool(r) for who, r in rows.items()})
    far = np.array([-1e6, -1e3, -40.0, -33.0, 33.0, 40.0, 1e3, 1e6])
    line = (one(0.0), one(1.0), None, None, one(1.0), vc.ACC_DNU.copy(), vc.ACC_REL["gd"] * 1.0, None, None, vc.ACC_REL["S"] * 1.0,
            np.array([1], dtype=np.int32), np.array([far.size], dtype=np.int32))
    sig = L.lineshape_xsec(1, 0, *line[:5], line[10], line[11], far)
    sig_d, J = L.lineshape_xsec_dual(1, 0, *line, far)
    print("Doppler far wing:", sig, sig_d, J.T)
    for v in (sig, sig_d):
        assert np.all(np.isfinite(v)) and np.all(v >= 0.0) and np.all(v < 1e-300)
    assert np.all(np.isfinite(J)) and np.all(np.abs(J) < 1e-300)


def test_pointwise_accuracy_lorentz(rtamd):
    """S gamma_l / (pi (gamma_l^2 + D^2)) point by point: gamma_l = 0.045, S = 1, |D| = 0 and 1e-6 .. 1e2 geometrically, on both
    sides.  Value relative to the arbiter's value, partials relative to the sum of the magnitudes of the product-rule terms;
    the kernels at most 4 times as far from np.longdouble as the Float64 oracle (which stands at 2.7e-16 in the value).

    Measured on an MI355X:
                 E_gpu value kernel   E_gpu Dual kernel   E_oracle64
      value           2.61e-16            2.61e-16         2.61e-16
      partial            -                4.51e-16         4.61e-16
    """
    L = rtamd._lib
    pos = np.geomspace(1e-6, 1e2, 801)
    g = np.concatenate([-pos[::-1], [0.0], pos])
    one = lambda v: np.array([float(v)])
    gl = 0.045
    line = (one(0.0), None, one(gl), None, one(1.0), vc.ACC_DNU.copy(), None, vc.ACC_REL["y"] * gl, None, vc.ACC_REL["S"] * 1.0,
            np.array([1], dtype=np.int32), np.array([g.size], dtype=np.int32))
    oline = (line[0], one(0.01), line[2], one(0.3)) + line[4:]
    arb = lso.lineshape_sum_dual("lorentz", *oline, g, FT=np.longdouble)
    s64, J64 = lso.lineshape_sum_dual("lorentz", *oline, g)
    sig = L.lineshape_xsec(2, 0, *line[:5], line[10], line[11], g)
    sig_d, J = L.lineshape_xsec_dual(2, 0, *line, g)
    E = {"value kernel": simple_errors("lorentz", g, oline, arb, sig), "Dual kernel": simple_errors("lorentz", g, oline, arb, sig_d, J),
         "oracle64": simple_errors("lorentz", g, oline, arb, s64, J64)}
    pool_rule(E)


# ---- C. the routes agree -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def profile_lines(iz):
    """the oracle's Dual line parameters of layer iz of the profile case (shared by the shapes)"""
    return lso.line_parameters_dual(vc.hit_columns(vc.o2a_lines()), vc.profile_grid("jittered"), vc.P_FULL[iz], vc.T_FULL[iz], vc.MODEL_VMR,
                                    vc.WING)


@functools.lru_cache(maxsize=None)
def profile_reference(shape, iz):
    """(sigma, J) of the oracle for layer iz"""
    nu, gd, gl, y, S, i0, i1 = profile_lines(iz)
    return lso.lineshape_sum_dual(shape, nu.v, gd.v, gl.v, y.v, S.v, nu.d.T, gd.d.T, gl.d.T, y.d.T, S.d.T, i0, i1, vc.profile_grid("jittered"))


def check_table(shape, tau, dtau, bar_v, bar_d, what):
    f = vc.VCD * vc.PROFILE_VMR
    for iz in range(len(vc.P_FULL)):
        sig, J = profile_reference(shape, iz)
        distance(tau[:, iz], sig * f[iz], f"{what}: tau_abs, layer {iz + 1}", bar_v)
        for k in range(2):
            if dtau is not None:
                distance(dtau[k][:, iz], J[:, k] * f[iz], f"{what}: dtau_abs[{k}], layer {iz + 1}", bar_d)


@pytest.mark.parametrize("shape", lso.NEW_SHAPES)
def test_routes_agree(rtamd, shape):
    """One absorber (400 O2-A-like lines) on a jittered grid of 4000 points, four layers, per new shape: the device-prefactor route
    as a profile (value and Dual) and layer by layer -- bitwise the profile --, tau_abs within 1e-9 and dtau_abs within 1e-6 of the
    oracle's column maximum (the bars of test_gpu_voigt_edges.py::check_layers: device exp / pow in S); gamma_l and its partials
    as the device formed them at rtol 4e-15 (y's bar: the same pow); the host-prefactor route fed with the oracle's own line
    parameters within 1e-13; absorption_cross_section(autodiff=True, broadening=...) within 1e-13 of the line-shape oracle on the
    host prefactors it is built from, and within 1e-9 / 1e-6 of the oracle of the whole function."""
    ab = rtamd.absorption
    tab, grid = vc.o2a_lines(), vc.profile_grid("jittered")
    b, c = lso.NAMES[shape]
    kw = dict(wing_cutoff=vc.WING, model_vmr=vc.MODEL_VMR, device_prefactors=True, broadening=b, cef=c)
    Nz = len(vc.P_FULL)
    f = vc.VCD * vc.PROFILE_VMR
    with rtamd.Handle(4, 1, grid.size, 1) as h, rtamd.Handle(4, 1, grid.size, 1) as hd:
        assert ab.compute_absorption_profile(h, tab, grid, vc.P_FULL, vc.T_FULL, vc.VCD, vc.PROFILE_VMR, **kw) > 0
        tau = h.absorption_get()
        assert ab.compute_absorption_profile(hd, tab, grid, vc.P_FULL, vc.T_FULL, vc.VCD, vc.PROFILE_VMR, dual=True, **kw) > 0
        tau_d, dtau = hd.absorption_get(), hd.absorption_get_partials()
        n = profile_lines(Nz - 1)[0].v.size
        gl_dev, dgl_dev = hd.absorption_get_gamma_l(n, partials=True)
        ab.compute_absorption_profile(h, tab, grid, vc.P_FULL, vc.T_FULL, vc.VCD, vc.PROFILE_VMR, layer_by_layer=True, **kw)
        tau_lbl = h.absorption_get()
        gl_lbl = h.absorption_get_gamma_l(n)
        # host prefactors: the oracle's own line parameters through mom_lineshape_tau_abs / _dual
        h.absorption_begin(Nz, grid)
        hd.absorption_begin(Nz, grid)
        for iz in range(Nz):
            nu, gd, gl, y, S, i0, i1 = profile_lines(iz)
            h.lineshape_tau_abs(iz + 1, nu.v, gd.v, gl.v, y.v, S.v, i0, i1, f[iz])
            hd.lineshape_tau_abs_dual(iz + 1, nu.v, gd.v, gl.v, y.v, S.v, nu.d.T, gd.d.T, gl.d.T, y.d.T, S.d.T, i0, i1, f[iz])
        tau_h, tau_hd, dtau_h = h.absorption_get(), hd.absorption_get(), hd.absorption_get_partials()
    assert np.array_equal(tau, tau_lbl)
    distance(tau_d, tau, f"{shape}: tau_abs, Dual run vs value run", 1e-13)
    check_table(shape, tau, None, 1e-9, None, f"{shape}, device prefactors")
    check_table(shape, tau_d, dtau, 1e-9, 1e-6, f"{shape}, device prefactors, Dual run")
    gl_o = profile_lines(Nz - 1)[2]
    np.testing.assert_allclose(gl_dev, gl_o.v, rtol=4e-15)
    np.testing.assert_allclose(dgl_dev, gl_o.d.T, rtol=4e-15)
    assert np.array_equal(gl_lbl, gl_dev)
    check_table(shape, tau_h, None, 1e-13, None, f"{shape}, host prefactors")
    check_table(shape, tau_hd, dtau_h, 1e-13, 1e-13, f"{shape}, host prefactors, Dual run")
    # absorption_cross_section(autodiff=True): (sigma, J [nGrid, 2])
    iz = 2
    sig, J = ab.absorption_cross_section(tab, grid, vc.P_FULL[iz], vc.T_FULL[iz], autodiff=True, vmr=vc.MODEL_VMR, wing_cutoff=vc.WING,
                                         broadening=b, cef=c)
    assert sig.shape == (grid.size,) and J.shape == (grid.size, 2)
    pf, dnu, dgd, dy, dS, dgl = ab.line_prefactors_dual(tab, grid, vc.P_FULL[iz], vc.T_FULL[iz], vc.MODEL_VMR, vc.WING, with_γ_l=True)
    sig_o, J_o = lso.lineshape_sum_dual(shape, pf.ν, pf.γ_d, pf.γ_l, pf.y, pf.S, dnu, dgd, dgl, dy, dS, pf.ind_start, pf.ind_stop, grid)
    distance(sig, sig_o, f"{shape}: absorption_cross_section sigma vs the line-shape oracle", 1e-13)
    for k in range(2):
        distance(J[:, k], J_o[:, k], f"{shape}: absorption_cross_section J[{k}] vs the line-shape oracle", 1e-13)
    sig_f, J_f = profile_reference(shape, iz)
    distance(sig, sig_f, f"{shape}: absorption_cross_section sigma vs the oracle of the function", 1e-9)
    for k in range(2):
        distance(J[:, k], J_f[:, k], f"{shape}: absorption_cross_section J[{k}] vs the oracle of the function", 1e-6)
    distance(ab.absorption_cross_section(tab, grid, vc.P_FULL[iz], vc.T_FULL[iz], vmr=vc.MODEL_VMR, wing_cutoff=vc.WING, broadening=b, cef=c),
             sig, f"{shape}: absorption_cross_section, value run vs Dual run", 1e-13)


# ---- D. defaults and the selector --------------------------------------------------------------------------------------
def test_default_model_is_the_voigt_kernel(rtamd):
    """mom_lineshape_xsec(VOIGT, HW32SD) is mom_voigt_xsec and, under Voigt, mom_lineshape_tau_abs is mom_voigt_tau_abs: bitwise,
    the same kernel instantiation runs (with and without gamma_l, which Voigt does not read)."""
    L = rtamd._lib
    a = edge_case("700_ragged", "shuffled")
    nu, gd, gl, y, S, dnu, dgd, dgl, dy, dS, i0, i1 = a
    ref = L.voigt_xsec(nu, gd, y, S, i0, i1, vc.EDGE_GRID)
    assert ref.max() > 0
    assert np.array_equal(L.lineshape_xsec(0, 0, nu, gd, gl, y, S, i0, i1, vc.EDGE_GRID), ref)
    assert np.array_equal(L.lineshape_xsec(0, 0, nu, gd, None, y, S, i0, i1, vc.EDGE_GRID), ref)
    ref_d = L.voigt_xsec_dual(nu, gd, y, S, dnu, dgd, dy, dS, i0, i1, vc.EDGE_GRID)
    got_d = L.lineshape_xsec_dual(0, 0, *a, vc.EDGE_GRID)
    assert np.array_equal(got_d[0], ref_d[0]) and np.array_equal(got_d[1], ref_d[1])
    n = vc.EDGE_GRID.size
    with rtamd.Handle(4, 1, n, 1) as h:
        tabs = []
        for call in (lambda: h.voigt_tau_abs(1, nu, gd, y, S, i0, i1, 2.5e20), lambda: h.lineshape_tau_abs(1, nu, gd, gl, y, S, i0, i1, 2.5e20),
                     lambda: h.lineshape_tau_abs(1, nu, gd, None, y, S, i0, i1, 2.5e20)):
            h.absorption_begin(1, vc.EDGE_GRID)
            call()
            tabs.append(h.absorption_get())
        assert tabs[0].max() > 0 and np.array_equal(tabs[0], tabs[1]) and np.array_equal(tabs[0], tabs[2])
        for call in (lambda: h.voigt_tau_abs_dual(1, nu, gd, y, S, dnu, dgd, dy, dS, i0, i1, 2.5e20),
                     lambda: h.lineshape_tau_abs_dual(1, *a, 2.5e20)):
            h.absorption_begin(1, vc.EDGE_GRID)
            call()
            tabs.append((h.absorption_get(), h.absorption_get_partials()))
        assert np.array_equal(tabs[3][0], tabs[4][0]) and np.array_equal(tabs[3][1], tabs[4][1]) and np.abs(tabs[3][1]).max() > 0


def code_of(exc):
    return exc.value.code


def test_selector_errors(rtamd):
    """After set_model(DOPPLER, .) the four-array entry points return MOM_ESTATE and name mom_lineshape_tau_abs; unknown codes return
    MOM_EINVAL with the code in the text; an array the broadening does not read may be NULL, one it reads may not."""
    L = rtamd._lib
    nu, gd, gl, y, S, dnu, dgd, dgl, dy, dS, i0, i1 = edge_case("all", "listed")
    n = vc.EDGE_GRID.size
    with rtamd.Handle(4, 1, n, 1) as h:
        h.absorption_begin(1, vc.EDGE_GRID)
        h.absorption_set_model(L.BROADENING_DOPPLER, L.CEF_HW32SD)
        with pytest.raises(L.MomError, match="mom_lineshape_tau_abs") as e:
            h.voigt_tau_abs(1, nu, gd, y, S, i0, i1, 1.0)
        assert code_of(e) == ESTATE
        with pytest.raises(L.MomError, match="mom_lineshape_tau_abs_dual") as e:
            h.voigt_tau_abs_dual(1, nu, gd, y, S, dnu, dgd, dy, dS, i0, i1, 1.0)
        assert code_of(e) == ESTATE
        assert np.all(h.absorption_get() == 0.0)
        h.lineshape_tau_abs(1, nu, gd, None, None, S, i0, i1, 1.0)            # Doppler reads neither gamma_l nor y
        dop = h.absorption_get()
        assert np.array_equal(dop[:, 0], L.lineshape_xsec(1, 0, nu, gd, None, None, S, i0, i1, vc.EDGE_GRID)) and dop.max() > 0
        with pytest.raises(L.MomError) as e:
            h.lineshape_tau_abs(1, nu, None, gl, y, S, i0, i1, 1.0)             # ... but gamma_d
        assert code_of(e) == EINVAL
        h.absorption_set_model(L.BROADENING_LORENTZ, L.CEF_HW32VOIGT)             # the CEF is ignored, not refused
        h.lineshape_tau_abs(1, nu, None, gl, None, S, i0, i1, 1.0)
        with pytest.raises(L.MomError) as e:
            h.lineshape_tau_abs(1, nu, gd, None, y, S, i0, i1, 1.0)
        assert code_of(e) == EINVAL
        for b, c, text in ((3, 0, "broadening code 3 "), (-1, 0, "broadening code -1 "), (0, 2, "CEF code 2 "), (0, -1, "CEF code -1 ")):
            with pytest.raises(L.MomError, match=text) as e:
                h.absorption_set_model(b, c)
            assert code_of(e) == EINVAL
        h.absorption_set_model(L.BROADENING_VOIGT, L.CEF_HW32VOIGT)               # Voigt again: the four-array entry point runs, with the handle's CEF
        h.absorption_begin(1, vc.EDGE_GRID)
        h.voigt_tau_abs(1, nu, gd, y, S, i0, i1, 1.0)
        assert np.array_equal(h.absorption_get()[:, 0], L.lineshape_xsec(0, 1, nu, gd, None, y, S, i0, i1, vc.EDGE_GRID))
    with pytest.raises(L.MomError, match="broadening code 7 ") as e:
        L.lineshape_xsec(7, 0, nu, gd, gl, y, S, i0, i1, vc.EDGE_GRID)
    assert code_of(e) == EINVAL
    with pytest.raises(L.MomError, match="CEF code 5 ") as e:
        L.lineshape_xsec_dual(0, 5, nu, gd, gl, y, S, dnu, dgd, dgl, dy, dS, i0, i1, vc.EDGE_GRID)
    assert code_of(e) == EINVAL
    with pytest.raises(L.MomError) as e:
        L.lineshape_xsec(2, 0, nu, gd, None, y, S, i0, i1, vc.EDGE_GRID)          # Lorentz reads gamma_l
    assert code_of(e) == EINVAL
    assert np.array_equal(L.lineshape_xsec(2, 0, nu, None, gl, None, S, i0, i1, vc.EDGE_GRID),
                          L.lineshape_xsec(2, 0, nu, gd, gl, y, S, i0, i1, vc.EDGE_GRID))


def test_two_absorbers_two_models_and_float32_handle(rtamd):
    """A Lorentz absorber and a Voigt / HW32SD absorber accumulated into one table (begin=False, mom_absorption_set_model between
    them) equal the sum of their separate references at 1e-9 of the column maximum; a Float32 handle gives the Float64 handle's
    tau_abs bitwise (the absorption table is Float64 on both)."""
    ab = rtamd.absorption
    grid = vc.SORT_GRID
    tabs = (vc.steady_lines(), ab.synthetic_o2a_lines(120, 12990.0, 13010.0, seed=9))
    p, T, vcd = vc.P_FULL[2:], vc.T_FULL[2:], vc.VCD[2:]
    kw = dict(wing_cutoff=vc.SORT_WING, model_vmr=vc.MODEL_VMR, device_prefactors=True)
    ref = np.zeros((grid.size, 2))
    for tab, shape in zip(tabs, ("lorentz", "voigt_sd")):
        for iz in range(2):
            sig, _ = lso.cross_section_dual(shape, vc.hit_columns(tab), grid, p[iz], T[iz], vc.MODEL_VMR, vc.SORT_WING)
            ref[:, iz] += sig * (vcd[iz] * vc.PROFILE_VMR)
    out = []
    for dtype in (0, 1):
        with rtamd.Handle(4, 1, grid.size, 1, dtype=dtype) as h:
            ab.compute_absorption_profile(h, tabs[0], grid, p, T, vcd, vc.PROFILE_VMR, broadening="Lorentz()", **kw)
            first = h.absorption_get()
            ab.compute_absorption_profile(h, tabs[1], grid, p, T, vcd, vc.PROFILE_VMR, begin=False, **kw)
            out.append((first, h.absorption_get()))
    for iz in range(2):
        distance(out[0][1][:, iz], ref[:, iz], f"two absorbers, layer {iz + 1}", 1e-9)
    assert np.all(out[0][1] >= out[0][0]) and np.any(out[0][1] > out[0][0]) and out[0][0].max() > 0
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
