"""The Dual run of the device-side layer optics (k_optics_dual in csrc/mom_optics.hip; mom_scene_set_optics_partials,
mom_scene_get_partials): the scene's partials formed on the GPU from the partials of the ingredients, against the numpy twin
absorption.optics_partials_host (itself checked against the Dual oracle in test_oracle_optics_dual.py), through mom_rt_run_dual,
and against central differences of the value pipeline.  S = 300 is no multiple of 64 or 256: the last wavefront and the last block
are partly live."""
import dataclasses

import numpy as np
import pytest

import helpers
import optics_dual_cases as oc
import rtamd
from test_oracle_absdual import lines24

pytestmark = pytest.mark.gpu
rt, ab, lib = rtamd.corert, rtamd.absorption, rtamd._lib
S, NZ = 300, 3
GRID = np.linspace(12999.5, 13002.5, S)
T0 = np.array([220.0, 240.0, 280.0])


def profile(Nz=NZ):
    p_half = rtamd.scenes.pressure_grid(Nz)
    return 0.5 * (p_half[1:] + p_half[:-1]), 2.0e25 * np.diff(p_half) / p_half[-1]


def dual_tables(h, grid=GRID, T=T0, dual=True):
    """24 lines -> the handle's resident τ_abs and (dual) dτ_abs tables, all layers in two launches"""
    p_full, vcd = profile()
    ab.compute_absorption_profile(h, lines24(), grid, p_full, T, vcd, 0.21, wing_cutoff=1.0, model_vmr=0.21, device_prefactors=True, dual=dual)
    return h.absorption_get(), (h.absorption_get_partials() if dual else None)


def scene(nAer, grid=GRID):
    base = rtamd.scenes.make_scene(1, 9, NZ, grid.size, ν_lo=grid[0], ν_hi=grid[-1], absorption=False, aerosol_total=0.2 if nAer else 0.0)
    assert len(base.quad_points.qp_μN) <= 12
    if nAer != 2:
        return base
    m = oc.three_mode_model(base, seed=4)
    md = oc.modes(m)
    assert np.all(md[:, 1] == 0) and np.all(md[0, [0, 2]] == 2) and np.all(md[1, [0, 2]] == 1)   # the three modes are present
    return m


def parameters(model, P):
    six = oc.six_parameters(model)                       # four of them without aerosols
    if P == 1:
        return [oc.combined(six)]                        # every ingredient depends on the one parameter
    ps = [oc.combined(six[:2])] + six[2:] if len(six) == 6 else six + [oc.combined(six)]
    assert len(ps) == P
    return ps


# ---- 1. device against the host twin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("nAer", [0, 2])
def test_device_partials_match_the_host_twin(nAer, P):
    m0 = scene(nAer)
    with rt.make_handle(m0) as h:
        tau_abs, dtau_abs = dual_tables(h)
        model = dataclasses.replace(m0, τ_abs=tau_abs)
        ps = parameters(model, P)
        rt.rt_run_dual_device_optics(h, model, ps, upload_tau_abs=False)
        got = h.scene_get_partials()
    ref = oc.stack(ab.optics_partials_host(model, ps, dtau_abs), 1 + nAer, S, NZ)
    assert tau_abs.max() > 1.0 and np.abs(dtau_abs[0]).max() > 0 and np.abs(dtau_abs[1]).max() > 0
    for k, name in enumerate(("dτ", "dϖ", "dzw")):
        assert got[k].shape == ref[k].shape
        oc.assert_columns(got[k], ref[k], 1e-13, f"{name} device vs host twin (nAer {nAer}, P {P})")
    assert np.abs(ref[0]).max() > 0 and np.abs(ref[1]).max() > 0
    if nAer == 0:
        assert not np.any(got[2])                        # the buffer is absent: zeros
    else:
        assert np.abs(got[2]).max() > 0


# ---- 2. wiring, exact ------------------------------------------------------------------------------------------------------
def test_device_partials_reach_the_sweep_bitwise():
    """The device-formed partials, read back and fed to a second handle through mom_scene_set + mom_scene_set_partials: after
    rt_run_dual both handles hold bitwise the same R, T and partials."""
    m0 = scene(2)
    with rt.make_handle(m0) as h, rt.make_handle(m0) as h2:
        tau_abs, _ = dual_tables(h)
        model = dataclasses.replace(m0, τ_abs=tau_abs)
        ps = parameters(model, 5)
        R, T, dR, dT = rt.rt_run_dual_device_optics(h, model, ps, upload_tau_abs=False)
        dτ, dϖ, dzw = h.scene_get_partials()
        nd, iface, tau, varpi, zw, tau_sum = h.scene_get_layers(NZ, 3)
        sc = dataclasses.replace(rt.prepare_scene(model), tau=tau, varpi=varpi, zw=zw, ndoubl=nd, iface=iface, tau_sum=tau_sum)
        rt.scene_set(h2, sc)
        rt.scene_set_partials(h2, sc, [rt.ScenePartial(dτ=dτ[k], dϖ=dϖ[k], dzw=dzw[k]) for k in range(5)])
        h2.rt_run_dual()
        R2, T2 = h2.get_RT()
        dR2, dT2 = h2.get_RT_partials()
        again = h2.scene_get_partials()                  # the getter serves the host setter's partials as well
    assert np.abs(dR).max() > 0 and np.all(np.isfinite(dR)) and np.all(np.isfinite(dT))
    for x, y in ((R, R2), (T, T2), (dR, dR2), (dT, dT2), (dτ, again[0]), (dϖ, again[1]), (dzw, again[2])):
        assert np.array_equal(x, y)


# ---- 3. end to end against central differences -----------------------------------------------------------------------------
def test_jacobians_through_the_device_pipeline():
    """The scene of test_gpu_voigt_dual.test_temperature_jacobian_through_rt_run_dual (S = 256, 24 lines, wing 1.0), on the device
    route: compute_absorption_profile(device_prefactors, dual) -> scene_set_optics -> scene_set_optics_partials -> rt_run_dual.
    Parameter 1: a uniform temperature offset (w_T ≡ 1), central difference dT = 0.02 K.  Parameter 2: a scaling of the aerosol
    type's τ_aer, relative step 1e-4.  Bar 1e-4 max|dR_SFI|: that test's sanity bar, set by the difference, not by the kernels."""
    Sx, dT, hx = 256, 0.02, 1e-4
    grid = np.linspace(12999.5, 13002.5, Sx)
    base = scene(1, grid)
    assert base.τ_aer.shape == (1, NZ)

    def tau_table(T):
        with rt.make_handle(base) as h:
            return dual_tables(h, grid, T, dual=False)[0]

    with rt.make_handle(base) as h:
        tau_abs, _ = dual_tables(h, grid)
        ps = [rt.OpticsPartial(w_T=np.ones(NZ)), rt.OpticsPartial(dτ_aer=base.τ_aer.copy())]
        _, _, dR, _ = rt.rt_run_dual_device_optics(h, base, ps, upload_tau_abs=False)
    assert tau_abs.max() > 1.0
    centre = dataclasses.replace(base, τ_abs=tau_abs)
    stepped = [[dataclasses.replace(base, τ_abs=tau_table(T0 + s * dT)) for s in (1, -1)],
               [dataclasses.replace(centre, τ_aer=base.τ_aer * (1 + s * hx)) for s in (1, -1)]]
    L0 = rt.construct_layer_inputs(centre)
    for k, (pair, step) in enumerate(zip(stepped, (dT, hx))):
        for m in pair:     # integer decisions of the stepped runs must agree for the difference to mean anything
            L = rt.construct_layer_inputs(m)
            assert np.array_equal(L.ndoubl, L0.ndoubl) and np.array_equal(L.iface, L0.iface)
        fd = (rtamd.rt_run(pair[0])[0] - rtamd.rt_run(pair[1])[0]) / (2 * step)
        scale = np.abs(dR[k]).max()
        err = np.abs(dR[k] - fd).max()
        print(f"dR_SFI/dx_{k} vs central difference: {err / scale:.2e} of max (bar 1e-4)")
        assert scale > 0 and err <= 1e-4 * scale


# ---- 4. the gas column -----------------------------------------------------------------------------------------------------
def test_gas_column_weight_needs_no_dual_absorption_call():
    """w_gas ≡ 1 on a table that came from the host (no dτ_abs resident): dτ = τ_abs, dϖ = -ϖ τ_abs / τ"""
    model = scene(2)
    with rt.make_handle(model) as h:
        rt.run_scene_device_optics(h, model)             # uploads model.τ_abs: mom_absorption_set drops any partial table
        with pytest.raises(rtamd.MomError):
            h.absorption_get_partials()
        rt.scene_set_optics_partials(h, model, [rt.OpticsPartial(w_gas=np.ones(NZ))])
        dτ, dϖ, dzw = h.scene_get_partials()
        tau_abs = h.absorption_get()
        _, _, tau, varpi, _, _ = h.scene_get_layers(NZ, 3)
    τ, ϖ = tau.reshape(NZ, S).T, varpi.reshape(NZ, S).T
    assert np.array_equal(tau_abs, model.τ_abs) and tau_abs.min() > 0
    oc.assert_columns(dτ, tau_abs[None], 1e-13, "dτ vs τ_abs")
    oc.assert_columns(dϖ, (-ϖ * tau_abs / τ)[None], 1e-13, "dϖ vs -ϖ τ_abs / τ")
    assert not np.any(dzw)


# ---- 5. states and arguments -----------------------------------------------------------------------------------------------
def refused(code, call, *a, name="mom_scene_set_optics_partials", **kw):
    with pytest.raises(rtamd.MomError) as e:
        call(*a, **kw)
    assert e.value.code == code and name in str(e.value), str(e.value)
    return e.value


def test_states_and_arguments():
    model = scene(2)
    N, K, M = len(model.quad_points.qp_μN), 3, model.params.max_m
    w_p = np.zeros((1, 3, NZ))
    w_p[0, 0, 1] = 1.0
    with rt.make_handle(model) as h:
        refused(lib.MOM_ESTATE, h.scene_set_optics_partials, 1)                     # no scene
        refused(lib.MOM_ESTATE, h.scene_get_partials, name="mom_scene_get_partials")
        rt.scene_set(h, rt.prepare_scene(model))
        refused(lib.MOM_ESTATE, h.scene_set_optics_partials, 1)                     # host optics
        rt.run_scene_device_optics(h, model)
        R0, _ = h.get_RT()
        refused(lib.MOM_ESTATE, h.scene_get_partials, name="mom_scene_get_partials")   # a scene, no partials yet
        refused(lib.MOM_ESTATE, h.scene_set_optics_partials, 1, w_abs=w_p)          # a pressure weight, no dτ_abs table
        refused(lib.MOM_EINVAL, h.scene_set_optics_partials, 65)
        refused(lib.MOM_EINVAL, h.scene_set_optics_partials, 1, dZpp=np.zeros(N * N * K * M))
        h.scene_set_optics_partials(1, w_rayl=np.ones(NZ))
        assert np.abs(h.scene_get_partials()[0]).max() > 0
        h.scene_set_optics_partials(0)                                              # P = 0 clears the partials ...
        refused(lib.MOM_ESTATE, h.scene_get_partials, name="mom_scene_get_partials")
        h.rt_run_dual()                                                             # ... and the Dual run still gives the values
        R1, _ = h.get_RT()
        helpers.assert_stokes_close(R1, R0, what="P = 0 after clearing")
        refused(lib.MOM_ESTATE, h.get_RT_partials, name="mom_get_RT_partials")
        h.absorption_begin(NZ, GRID)
        refused(lib.MOM_ESTATE, h.scene_set_optics_partials, 1)                     # the table is no longer the scene's
    with rt.make_handle(model, float_type="Float32") as h:
        rt.run_scene_device_optics(h, model)
        want = refused(lib.MOM_EINVAL, h.scene_set_partials, 1, name="mom_scene_set_partials")
        got = refused(want.code, h.scene_set_optics_partials, 1)
        assert "Float32" in str(got)
