"""Band-resolved aerosol optics on the device (k_optics_bands, k_optics_bands_dual in csrc/mom_optics.hip;
mom_scene_set_optics_bands, mom_scene_set_optics_bands_partials): against the host twin (corert.construct_layer_inputs,
absorption.optics_partials_host, themselves checked in test_oracle_bands.py), against the literal restatement of the reference's
per-band algebra run through the oracle's rt loop (bands_oracle.py), and through mom_rt_run / mom_rt_run_dual.  Band lengths
5 + 70 + 3 and 130 + 127 + 43: band edges inside a wavefront, one workgroup edge inside a band, a partly live last wavefront."""
import dataclasses

import numpy as np
import pytest

import bands_cases as bc
import bands_oracle as bo
import helpers
import optics_dual_cases as oc
import rtamd

pytestmark = pytest.mark.gpu
rt, ab, lib = rtamd.corert, rtamd.absorption, rtamd._lib
NZ = bc.NZ


@pytest.fixture(scope="module")
def models():
    return {(S, nAer): bc.banded(S, nAer) for S in (78, 300) for nAer in (0, 2)}


@pytest.fixture(scope="module")
def oracle_RT(models):
    """R_SFI, T_SFI of the restatement, computed once per scene"""
    return {S: bo.rt_run(bo.band_scene(models[S, 2])) for S in (78, 300)}


def layers_of(h, K):
    nd, iface, tau, varpi, zw, tau_sum = h.scene_get_layers(NZ, K)
    S = h.S
    return nd, iface, tau.reshape(NZ, S).T, varpi.reshape(NZ, S).T, zw.reshape(NZ, S, K).transpose(2, 1, 0), tau_sum.reshape(NZ + 1, S).T


# ---- 1. device against the host twin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nAer", [0, 2])
@pytest.mark.parametrize("S", [78, 300])
def test_device_layers_are_the_host_twins_bitwise(models, S, nAer):
    model = models[S, nAer]
    bc.assert_input_conditions(model, S, nAer)
    L = rt.construct_layer_inputs(model)
    K = 1 + 3 * nAer
    with rt.make_handle(model) as h:
        rt.scene_set_device_optics(h, model, upload_tau_abs=True)
        nd, iface, τ, ϖ, zw, τ_sum = layers_of(h, K)
    assert np.array_equal(nd, L.ndoubl) and np.array_equal(iface, L.iface)
    assert np.array_equal(τ, L.τ) and np.array_equal(ϖ, L.ϖ) and np.array_equal(τ_sum, L.τ_sum)
    assert zw.shape == L.zw.shape and np.array_equal(zw, L.zw)
    band_of = model.bands.band_of()
    for k in range(1, K):
        outside = band_of != (k - 1) // nAer
        assert not np.any(zw[k, outside]) and not np.any(np.signbit(zw[k, outside]))   # 0.0, not -0.0 and not stale memory
    if nAer:   # every band has a live aerosol basis (a type with ω̃ = 0 never gets weight: its basis stays at zero)
        assert all(np.abs(zw[1 + nAer * b:1 + nAer * (b + 1)]).max() > 0 for b in range(3))


@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("nAer", [0, 2])
@pytest.mark.parametrize("S", [78, 300])
def test_device_partials_match_the_host_twin(models, S, nAer, P):
    model = models[S, nAer]
    ps = bc.parameters(model, P)
    K = 1 + 3 * nAer
    with rt.make_handle(model) as h:
        kind = rt.scene_set_device_optics(h, model, upload_tau_abs=True)
        rt.scene_set_optics_partials(h, model, ps, surf_kind=kind)
        got = h.scene_get_partials()
    ref = oc.stack(ab.optics_partials_host(model, ps), K, S, NZ)
    for k, name in enumerate(("dτ", "dϖ", "dzw")):
        oc.assert_columns(got[k], ref[k], 1e-13, f"{name} device vs host twin (S {S}, nAer {nAer}, P {P})")
    assert np.abs(ref[0]).max() > 0 and np.abs(ref[1]).max() > 0
    if nAer == 0:
        assert not np.any(got[2])
    else:
        band_of = model.bands.band_of()
        assert np.abs(got[2]).max() > 0
        for k in range(1, K):
            assert not np.any(got[2][:, k][:, band_of != (k - 1) // nAer])


# ---- 2. against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [78, 300])
def test_device_and_host_route_against_the_oracle(models, oracle_RT, S):
    model = models[S, 2]
    Rr, Tr = oracle_RT[S]
    with rt.make_handle(model) as h:
        R1, T1 = rt.run_scene_device_optics(h, model)
    with rt.make_handle(model) as h:
        R0, T0 = rt.run_scene(h, rt.prepare_scene(model))
    assert np.abs(Rr).max() > 0
    for R, T, route in ((R1, T1, "device route"), (R0, T0, "host route")):
        helpers.assert_stokes_close(R, Rr, what=f"banded {route} R vs oracle (S {S})")
        helpers.assert_stokes_close(T, Tr, what=f"banded {route} T vs oracle (S {S})")


def test_headline_image_against_the_oracle():
    """the streams of scene_C2 (N = 60), S = 16 in two bands of 9 + 7 points, one aerosol type: K = 3 bases"""
    m = rtamd.scenes.scene_C2(S=16, Nz=NZ, aerosol_total=0.05)   # ndoubl <= 15: the 1e-10 bar is the oracle's own up to there
    assert len(m.quad_points.qp_μN) == 60
    other = rt.AerosolOptics(rtamd.scenes.hg_like_greek(0.6, m.params.l_trunc), 0.9, 0.1)
    model = rt.with_bands(m, rt.Bands(np.array([0, 9, 16]), np.array([m.τ_aer, 0.5 * m.τ_aer]), [[m.aerosol_optics[0]], [other]],
                                      np.array([1.0, 0.96])))
    Rr, Tr = bo.rt_run(bo.band_scene(model))
    with rt.make_handle(model) as h:
        R, T = rt.run_scene_device_optics(h, model)
        assert h.scene_get_layers(NZ, 3, arrays=False)[0].max() <= 15
    helpers.assert_stokes_close(R, Rr, what="banded C2 streams R vs oracle")
    helpers.assert_stokes_close(T, Tr, what="banded C2 streams T vs oracle")


def test_float32_handle_device_route_is_the_host_routes_run(models):
    model = models[78, 2]
    sc = rt.prepare_scene(model)
    with rt.make_handle(model, float_type="Float32") as h:
        R0, T0 = rt.run_scene(h, sc)
    with rt.make_handle(model, float_type="Float32") as h:
        R1, T1 = rt.run_scene_device_optics(h, model)
        with pytest.raises(rtamd.MomError) as e:
            h.scene_set_optics_bands_partials(1)
        assert e.value.code == lib.MOM_EINVAL and "Float32" in str(e.value) and "mom_scene_set_optics_bands_partials" in str(e.value)
    assert np.abs(R0).max() > 0 and np.array_equal(R1, R0) and np.array_equal(T1, T0)


# ---- 3. no leakage between bands -------------------------------------------------------------------------------------------
def test_another_aerosol_in_one_band_leaves_the_other_bands_alone(models):
    a = models[300, 2]
    b = bc.other_band_1(a)
    La, Lb = rt.construct_layer_inputs(a), rt.construct_layer_inputs(b)
    assert np.array_equal(La.ndoubl, Lb.ndoubl) and np.array_equal(La.iface, Lb.iface)
    out = []
    for model in (a, b):
        with rt.make_handle(model) as h:
            R, T = rt.run_scene_device_optics(h, model)
            out.append((R, T) + layers_of(h, 7)[2:5])
    others = a.bands.band_of() != 1
    (Ra, Ta, τa, ϖa, zwa), (Rb, Tb, τb, ϖb, zwb) = out
    assert np.array_equal(τa[others], τb[others]) and np.array_equal(ϖa[others], ϖb[others]) and np.array_equal(zwa[:, others], zwb[:, others])
    assert np.abs(Ra[..., ~others] - Rb[..., ~others]).max() > 1e-6 * np.abs(Ra).max()     # band 1 itself did change
    helpers.assert_stokes_close(Rb[..., others], Ra[..., others], rtol=1e-13, atol=0.0, what="R of bands 0 and 2")
    helpers.assert_stokes_close(Tb[..., others], Ta[..., others], rtol=1e-13, atol=0.0, what="T of bands 0 and 2")


def test_a_partial_of_one_band_has_zero_partials_in_the_others(models):
    model = models[300, 2]
    ps = [bc.band_only(model, 1, dτ_aer=True), bc.band_only(model, 1, dω̃=True), bc.band_only(model, 1, dZ=True)]
    with rt.make_handle(model) as h:
        _, _, dR, dT = rt.rt_run_dual_device_optics(h, model, ps)
    others = model.bands.band_of() != 1
    for k in range(3):
        assert not np.any(dR[k][..., others]) and not np.any(dT[k][..., others]), k
        assert np.abs(dR[k][..., ~others]).max() > 0 and np.abs(dT[k][..., ~others]).max() > 0, k
    assert np.all(np.isfinite(dR)) and np.all(np.isfinite(dT))


# ---- 4. the Jacobian end to end --------------------------------------------------------------------------------------------
def test_jacobians_against_central_differences(models):
    """dR_SFI with respect to a scaling of band 1's τ_aer and of band 2's ω̃ against central differences of the banded value run,
    relative step 1e-4.  Bar 1e-4 max|dR_SFI|: the sanity bar of test_gpu_optics_dual.test_jacobians_through_the_device_pipeline,
    set by the difference, not by the kernels."""
    model, hx = models[78, 2], 1e-4
    bd = model.bands
    ps = [bc.band_only(model, 1, dτ_aer=True), rt.OpticsPartial(dω̃=np.array([[0.0, 0.0], [0.0, 0.0], [a.ω̃ for a in bd.aerosol_optics[2]]]))]
    with rt.make_handle(model) as h:
        _, _, dR, _ = rt.rt_run_dual_device_optics(h, model, ps)

    def stepped(k, s):
        τ_aer, optics = bd.τ_aer.copy(), [list(band) for band in bd.aerosol_optics]
        if k == 0:
            τ_aer[1] *= 1 + s * hx
        else:
            optics[2] = [dataclasses.replace(a, ω̃=a.ω̃ * (1 + s * hx)) for a in optics[2]]
        return rt.with_bands(model, rt.Bands(bd.band_start, τ_aer, optics, bd.ϖ_Cabannes))

    L0 = rt.construct_layer_inputs(model)
    for k in range(2):
        runs = []
        for s in (1, -1):
            m = stepped(k, s)
            L = rt.construct_layer_inputs(m)   # equal integer decisions, or the difference means nothing
            assert np.array_equal(L.ndoubl, L0.ndoubl) and np.array_equal(L.iface, L0.iface)
            assert np.array_equal(bc.band_modes(m), bc.band_modes(model))
            with rt.make_handle(m) as h:
                runs.append(rt.run_scene_device_optics(h, m)[0])
        fd = (runs[0] - runs[1]) / (2 * hx)
        scale, err = np.abs(dR[k]).max(), np.abs(dR[k] - fd).max()
        print(f"banded dR_SFI/dx_{k} vs central difference: {err / scale:.2e} of max (bar 1e-4)")
        assert scale > 0 and err <= 1e-4 * scale


# ---- 5. wiring -------------------------------------------------------------------------------------------------------------
def test_device_partials_reach_the_sweep_bitwise(models):
    """the device-formed layers and partials, read back and fed to a second handle through mom_scene_set + mom_scene_set_partials"""
    model = models[78, 2]
    ps = bc.parameters(model, 5)
    with rt.make_handle(model) as h, rt.make_handle(model) as h2:
        R, T, dR, dT = rt.rt_run_dual_device_optics(h, model, ps)
        dτ, dϖ, dzw = h.scene_get_partials()
        nd, iface, tau, varpi, zw, tau_sum = h.scene_get_layers(NZ, 7)
        sc = dataclasses.replace(rt.prepare_scene(model), tau=tau, varpi=varpi, zw=zw, ndoubl=nd, iface=iface, tau_sum=tau_sum)
        rt.scene_set(h2, sc)
        rt.scene_set_partials(h2, sc, [rt.ScenePartial(dτ=dτ[k], dϖ=dϖ[k], dzw=dzw[k]) for k in range(5)])
        h2.rt_run_dual()
        R2, T2 = h2.get_RT()
        dR2, dT2 = h2.get_RT_partials()
    assert np.abs(dR).max() > 0 and np.all(np.isfinite(dR)) and np.all(np.isfinite(dT))
    for x, y in ((R, R2), (T, T2), (dR, dR2), (dT, dT2)):
        assert np.array_equal(x, y)


def test_host_route_split_inside_a_band_equals_the_unsplit_run(models):
    """sharding's host route: SceneInputs.spectral_slice on the shard bounds of a world of two; 39 lies inside band 1 (5 .. 75)"""
    model = models[78, 2]
    sc = rt.prepare_scene(model)
    bounds = [rtamd.sharding.shard_bounds(78, 2, r) for r in range(2)]
    assert bounds == [(0, 39), (39, 78)] and model.bands.band_start[1] < 39 < model.bands.band_start[2]
    with rt.make_handle(model) as h:
        R, T = rt.run_scene(h, sc)
    parts = []
    for lo, hi in bounds:
        with rt.make_handle(model, S=hi - lo) as h:
            parts.append(rt.run_scene(h, sc.spectral_slice(lo, hi)))
    assert np.array_equal(np.concatenate([p[0] for p in parts], axis=2), R)
    assert np.array_equal(np.concatenate([p[1] for p in parts], axis=2), T)


# ---- 6. the glue from spectral Mie -----------------------------------------------------------------------------------------
def test_band_aerosol_optics_is_one_spectral_call():
    sc = rtamd.scattering
    l_trunc, λ_bands, λ_ref, τ_ref = 5, np.array([0.76, 1.6]), 0.55, 0.3
    aerosol = sc.Aerosol(sc.LogNormal(np.log(0.3), np.log(1.6)), 1.3, 0.001)
    mie = sc.make_mie_model(sc.NAI2(), aerosol, λ_ref, rt.Stokes_IQU(), sc.δBGE(l_trunc, 2.0), 1.0, 37)
    profile = np.array([0.1, 0.3, 0.6])
    optics, τ_aer = sc.band_aerosol_optics(mie, λ_bands, λ_ref, τ_ref, profile)
    raw = sc.compute_spectral_aerosol_optical_properties(mie, np.append(λ_bands, λ_ref))
    assert len(optics) == 2 and τ_aer.shape == (2, 3)
    for b in range(2):
        want = sc.truncate_phase(mie.truncation_type, raw[b])
        six = lambda g: (g.α, g.β, g.γ, g.δ, g.ϵ, g.ζ)
        assert all(np.array_equal(x, y) for x, y in zip(six(optics[b].greek_coefs), six(want.greek_coefs))), b
        assert (optics[b].ω̃, optics[b].fᵗ, optics[b].k) == (want.ω̃, want.fᵗ, want.k) and optics[b].fᵗ != 0.0
        assert np.array_equal(τ_aer[b], τ_ref * (raw[b].k / raw[2].k) * profile)
    assert optics[0].k != optics[1].k
    model = rtamd.scenes.make_mie_band_scene(3, l_trunc, NZ, [0, 5, 12], λ_bands, λ_ref, vza=(0.0, 60.0), vaz=(0.0, 45.0))
    assert model.bands.nBand == 2 and rt.prepare_scene(model).K == 3


# ---- 7. states and arguments -----------------------------------------------------------------------------------------------
def refused(code, call, *a, name, text=None, **kw):
    with pytest.raises(rtamd.MomError) as e:
        call(*a, **kw)
    assert e.value.code == code and name in str(e.value) and (text is None or text in str(e.value)), str(e.value)
    return e.value


def test_states_and_arguments(models):
    model = models[78, 2]
    flat = bc.unbanded(78, 2)
    bd = model.bands
    M, S = model.params.max_m, 78
    Zpp, Zmp = [rt._abi_mats(Z) for Z in rt.z_bases(model)]
    VAL, PAR = "mom_scene_set_optics_bands", "mom_scene_set_optics_bands_partials"
    ω̃ = [[a.ω̃ for a in band] for band in bd.aerosol_optics]
    fᵗ = [[a.fᵗ for a in band] for band in bd.aerosol_optics]
    cm, sm = np.ones((M, 2)).reshape(-1), np.zeros((M, 2)).reshape(-1)

    def set_bands(h, band_start, τ_aer=bd.τ_aer, om=ω̃, ft=fᵗ, ϖ_Cab=None, zp=Zpp, zm=Zmp):
        nB = len(band_start) - 1
        h.scene_set_optics_bands(NZ, M, band_start, model.τ_rayl, np.ones(max(nB, 1)) if ϖ_Cab is None else ϖ_Cab, τ_aer, om, ft, zp, zm, 0.2,
                                 rt.view_nodes(model), cm, sm)

    with rt.make_handle(model) as h:
        refused(lib.MOM_ESTATE, set_bands, h, bd.band_start, name=VAL, text="tau_abs")          # no resident τ_abs table
        refused(lib.MOM_ESTATE, h.scene_set_optics_bands_partials, 1, name=PAR, text="first")     # no scene
        h.absorption_set(model.τ_abs)
        refused(lib.MOM_EINVAL, set_bands, h, [0], τ_aer=np.zeros((0, 0, NZ)), name=VAL, text="at least one band")
        refused(lib.MOM_EINVAL, set_bands, h, [1, 5, 75, S], name=VAL, text="band_start[0] = 1")
        refused(lib.MOM_EINVAL, set_bands, h, [0, 5, 75, S - 1], name=VAL, text="band_start[nBand] = 77, not nSpec = 78")
        refused(lib.MOM_EINVAL, set_bands, h, [0, 75, 75, S], name=VAL, text="not strictly ascending: band 2 is [75, 75)")
        refused(lib.MOM_EINVAL, set_bands, h, [0, 75, 5, S], name=VAL, text="not strictly ascending")
        many = np.arange(11) * 7
        many[-1] = S
        refused(lib.MOM_EINVAL, set_bands, h, many, τ_aer=np.zeros((10, 7, NZ)), om=np.zeros((10, 7)), ft=np.zeros((10, 7)), name=VAL,
                text="1 + 7 x 10 phase-matrix bases, at most 64")
        refused(lib.MOM_EINVAL, set_bands, h, [0, S], τ_aer=np.zeros((1, 8, NZ)), om=np.zeros((1, 8)), ft=np.zeros((1, 8)), name=VAL,
                text="bad argument")
        rt.scene_set(h, rt.prepare_scene(model))
        refused(lib.MOM_ESTATE, h.scene_set_optics_bands_partials, 1, name=PAR, text="host optics")
        rt.run_scene_device_optics(h, flat)                                                         # a scene without bands
        refused(lib.MOM_ESTATE, h.scene_set_optics_bands_partials, 1, name=PAR, text="mom_scene_set_optics_partials")
        rt.run_scene_device_optics(h, model)
        R0, _ = h.get_RT()
        refused(lib.MOM_ESTATE, h.scene_set_optics_partials, 1, name="mom_scene_set_optics_partials", text=PAR)   # ... and the reverse
        w_p = np.zeros((1, 3, NZ))
        w_p[0, 0, 1] = 1.0
        refused(lib.MOM_ESTATE, h.scene_set_optics_bands_partials, 1, w_abs=w_p, name=PAR, text="dtau_abs")
        refused(lib.MOM_EINVAL, h.scene_set_optics_bands_partials, 65, name=PAR)
        refused(lib.MOM_EINVAL, h.scene_set_optics_bands_partials, 1, dZpp=np.zeros(Zpp.size), name=PAR)
        h.scene_set_optics_bands_partials(1, w_rayl=np.ones(NZ))
        assert np.abs(h.scene_get_partials()[0]).max() > 0
        h.scene_set_optics_bands_partials(0)                                                        # P = 0 clears the partials
        refused(lib.MOM_ESTATE, h.scene_get_partials, name="mom_scene_get_partials")
        h.rt_run_dual()
        helpers.assert_stokes_close(h.get_RT()[0], R0, what="P = 0 after clearing")
        h.absorption_begin(NZ, np.linspace(13000.0, 13001.0, S))
        refused(lib.MOM_ESTATE, h.scene_set_optics_bands_partials, 1, name=PAR, text="not the scene's")
    with rt.make_handle(model) as h:
        h.absorption_set(model.τ_abs)
        h.comm_init(0, 1, lib.comm_unique_id())
        refused(lib.MOM_EUNSUPPORTED, set_bands, h, bd.band_start, name=VAL, text="communicator")
        h.comm_destroy()
        set_bands(h, bd.band_start, ϖ_Cab=bd.ϖ_Cabannes)                                            # without it the call goes through
