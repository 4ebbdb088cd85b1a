"""Scenes from Greek coefficients: the Z bases formed in the handle's memory (mom_scene_stage_greeks / _greek_partials, the staged
branches of scene_common and mom_partials_rest, csrc/mom_zmom.hip) against the round-trip device route (mom_z_moments, then the host
setter: params.z_moments_on_device).

The bar is bitwise (np.array_equal), not a tolerance: the staged route runs the very arithmetic of mom_z_moments, the host's pad
(mom_pad_blocks) and cut (mom_m0_cut) move values without touching them, and the reduction decision is a Boolean of those values.
So everything the staged route leaves on the device (read with mom_scene_get_bases) and every result of a run equals the round-trip
route's.  The accuracy of Z itself against the extended-precision oracle is test_gpu_zmoments.py's.

The kernels' edges (strip_pad over mom_find_image, and the quad-block rule of scene_common) are never written down here: they are what
the library reports (mom_scene_get_bases' edge) after the uploaded route, and the numpy restatements of the pad and the cut are
built for those edges."""
import dataclasses
import math
import unicodedata

import numpy as np
import pytest

import bands_cases as bc
import rtamd

pytestmark = pytest.mark.gpu
rt, L = rtamd.corert, rtamd._lib


def rows(g):
    return (g.α, g.β, g.γ, g.δ, g.ϵ, g.ζ)


def with_epsilon(g):
    """hg_like_greek with an ϵ row of the size of the others: the (3,4) / (4,3) entries of B carry weight"""
    hi = (np.arange(len(g.β)) >= 2).astype(np.float64)
    return dataclasses.replace(g, ϵ=0.3 * g.β * hi)


def route(model, resident):
    """`model` on the staged route (resident) or on the round-trip device route"""
    return dataclasses.replace(model, params=dataclasses.replace(model.params, z_moments_on_device=not resident, z_resident=resident))


def layout_model(nS, l_trunc, pol=None, nan=False):
    """Nz = 3, S = 8, K = 3 bases of ragged length -- Rayleigh's 3, 33 (with ϵ) and 9 -- M = 3; (l_trunc + 1) // 2 + 3 streams"""
    m = rtamd.scenes.make_scene(nS, l_trunc, 3, 8, seed=4)
    a0 = m.aerosol_optics[0]
    g33, g9 = with_epsilon(rtamd.scenes.hg_like_greek(0.7, 33)), rtamd.scenes.hg_like_greek(0.5, 9)
    if nan:
        γ = g9.γ.copy()
        γ[2] = np.nan
        g9 = dataclasses.replace(g9, γ=γ)
    m = dataclasses.replace(m, τ_aer=np.vstack([0.6 * m.τ_aer[0], 0.4 * m.τ_aer[0]]),
                            aerosol_optics=[rt.AerosolOptics(g33, a0.ω̃, a0.fᵗ), rt.AerosolOptics(g9, 0.9, 0.1)])
    if pol is not None:
        m = dataclasses.replace(m, params=dataclasses.replace(m.params, polarization_type=pol))
    return m


CASES = {"a": (3, 27, 17), "b": (4, 15, 11), "c": (1, 133, 70), "d": (3, 3, 5)}   # nS, l_trunc, streams


def resident_arrays(model, resident):
    """(edge, Zpp, Zmp) of which = 0 and which = 1 after the scene is set on `model`'s route"""
    sc = rt.prepare_scene(route(model, resident))
    assert (sc.Zpp is None) == resident
    with rt.make_handle(model) as h:
        rt.scene_set(h, sc)
        return h.scene_get_bases(0), h.scene_get_bases(1), sc


def same(a, b):
    return a[0] == b[0] and a[1].shape == b[1].shape and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ---- 1. the resident layout, every form ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_resident_layout(case):
    nS, l_trunc, streams = CASES[case]
    m = layout_model(nS, l_trunc)
    N, K, M = nS * streams, 3, m.params.max_m
    assert len(m.quad_points.qp_μN) == N and len(rt.z_greeks(m)) == K
    up0, up1, sc = resident_arrays(m, False)
    st0, st1, _ = resident_arrays(m, True)
    assert same(st0, up0), f"case {case}: bases, staged vs uploaded (edges {st0[0]}, {up0[0]})"
    assert same(st1, up1), f"case {case}: (I,Q) sub-problem, staged vs uploaded (edges {st1[0]}, {up1[0]})"
    # numpy restatements of mom_pad_blocks / mom_m0_cut on mom_z_moments' output, for the edges the library chose
    Nk, N0 = up0[0], up1[0]
    assert N <= Nk <= N + 4
    Z = [z.reshape(M * K, N, N) for z in (sc.Zpp, sc.Zmp)]          # the ABI buffer: C array [m K + k, j, i]
    for got, z in zip(st0[1:], Z):
        pad = np.zeros((M * K, Nk, Nk))
        pad[:, :N, :N] = z
        assert got.shape == pad.shape and np.array_equal(got, pad)
        assert not np.any(got[:, N:, :]) and not np.any(got[:, :, N:])   # pad entries: 0.0
    if case == "c":
        assert N0 == 0 and st1[1].size == 0      # one Stokes component: no reduction
        return
    N0r = 2 * streams
    assert N0r <= N0 <= N0r + 4
    full = np.array([(i // 2) * nS + i % 2 for i in range(N0r)])
    for got, z in zip(st1[1:], Z):
        cut = np.zeros((K, N0, N0))
        cut[:, :N0r, :N0r] = z[:K][:, full][:, :, full]
        assert got.shape == cut.shape and np.array_equal(got, cut)
        assert not np.any(got[:, N0r:, :]) and not np.any(got[:, :, N0r:])
    if case == "a":
        assert Nk != N and N0 != N0r        # strip_pad changes both edges
    if case == "b":
        assert N0r == 22 and N0 == N0r + 2   # the quad-block rule of scene_common
    if case == "d":
        assert Nk == N                       # the wave route: unpadded but reduced


# ---- 2. runs -------------------------------------------------------------------------------------------------------------------
def assert_same_run(got, ref, names):
    for g, r, what in zip(got, ref, names):
        assert np.asarray(g).shape == np.asarray(r).shape and np.array_equal(g, r), f"{what}: staged vs round trip"


@pytest.mark.parametrize("which", ["small", "a"])
def test_rt_run(which):
    m = rtamd.scenes.make_scene(1, 3, 6, 24, seed=4) if which == "small" else layout_model(*CASES["a"][:2])
    got, ref = rt.rt_run(route(m, True)), rt.rt_run(route(m, False))
    assert np.abs(ref[0]).max() > 0
    assert_same_run(got, ref, ("R", "T", "ieR", "ieT", "hdr", "bhr_uw", "bhr_dw"))


def device_optics_run(model):
    with rt.make_handle(model) as h:
        R, T = rt.run_scene_device_optics(h, model)
        return (R, T) + tuple(h.get_hdr())


@pytest.mark.parametrize("banded", [False, True])
def test_run_scene_device_optics(banded):
    m = bc.banded(78, 2) if banded else layout_model(*CASES["a"][:2])
    assert not banded or len(rt.z_greeks(m)) == 7
    assert_same_run(device_optics_run(route(m, True)), device_optics_run(route(m, False)), ("R", "T", "hdr", "bhr_uw", "bhr_dw"))


def test_rt_run_rrs():
    """the case of test_gpu_zmoments.py::test_rt_run_rrs_with_device_z: elastic bases and the Raman set both staged"""
    m = rtamd.scenes.make_scene(1, 3, 3, 24, seed=1 + 3 + 24, aerosol_total=0.1)
    vp = 0.02 * (1.0 + 0.1 * np.arange(5))
    RS = rt.RRS(greek_raman=rt.get_greek_rayleigh(0.2), ϖ_Cabannes=0.96, ϖ_λ1λ0=vp, i_λ1λ0=np.asarray([-4, -1, 2, 7, 3]), rrs_strict_reference=False)
    got, ref = rt.rt_run_rrs(RS, route(m, True)), rt.rt_run_rrs(RS, route(m, False))
    assert np.abs(ref[2]).max() > 0
    assert_same_run(got, ref, ("R", "T", "ieR", "ieT", "hdr", "bhr_uw", "bhr_dw"))


def test_rt_run_test_ms():
    m = rtamd.scenes.make_scene(1, 3, 6, 24, seed=4)
    got, ref = rt.rt_run_test_ms([1, 3], route(m, True)), rt.rt_run_test_ms([1, 3], route(m, False))
    for s in range(2):
        assert_same_run((got[0][s], got[1][s]), (ref[0][s], ref[1][s]), (f"uwJ sensor {s}", f"dwJ sensor {s}"))


# ---- 3. Dual -------------------------------------------------------------------------------------------------------------------
def test_chain_to_rt_run_dual():
    """the chain of test_gpu_zmoments.py::test_chain_to_rt_run_dual_with_device_z with the bases and their partials formed in the handle"""
    sc = rtamd.scattering
    kw_r, kw_i = (unicodedata.normalize("NFKC", s) for s in ("nᵣ", "nᵢ"))
    base = {"r_m": 0.3, "σ_g": 1.6, kw_r: 1.3, kw_i: 0.001, "λ": 0.55, "r_max": 1.0, "nquad_radius": 37, "truncation": sc.δBGE(10, 2.0)}
    m = rtamd.scenes.make_mie_scene(1, 3, 6, 24, seed=4, **base)
    md, mr = route(m, False), route(m, True)
    aer = sc.Aerosol(sc.LogNormal(math.log(0.3), math.log(1.6)), 1.3, 0.001)
    mie = sc.make_mie_model(sc.NAI2(), aer, 0.55, rtamd.Stokes_I(), sc.δBGE(10, 2.0), 1.0, 37)
    aero, partials = sc.compute_aerosol_optical_properties(mie, autodiff=True, wrt=("nᵣ", "nᵢ"))
    _, d_trunc = sc.truncate_phase(mie.truncation_type, aero, partials=partials)
    items = [(0, d, None, None) for d in d_trunc]
    ops_d = sc.aerosol_optics_partials(md, items, device=md.params.architecture.device)
    ops_r = sc.aerosol_optics_partials(mr, items, resident=True)
    assert all(p.dZpp is None and p.dZmp is None and len(p.d_greeks) == 1 and p.d_greeks[0][0] == 1 for p in ops_r)
    with rt.make_handle(md) as h:
        v0, d0 = rt.rt_run_dual_device_optics(h, md, ops_d, full=True)
    with rt.make_handle(mr) as h:
        v1, d1 = rt.rt_run_dual_device_optics(h, mr, ops_r, full=True)
    assert np.abs(d0[0]).max() > 0
    assert_same_run(v1, v0, ("R", "T", "hdr", "bhr_uw", "bhr_dw"))
    assert_same_run(d1, d0, ("dR", "dT", "dhdr", "dbhr_uw", "dbhr_dw"))


def test_resident_partials_layout():
    """case (a), P = 3, nD = 2: the pairs (k = 1, p = 0) and (k = 2, p = 2) hold mom_z_moments of their sets, padded; every other
    block of [Nk, Nk, K, M, P], all of p = 1 included, is exactly zero"""
    nS, l_trunc, streams = CASES["a"]
    m = route(layout_model(nS, l_trunc), True)
    N, K, M, P = nS * streams, 3, m.params.max_m, 3
    gA, gB = with_epsilon(rtamd.scenes.hg_like_greek(0.6, 21)), rt.get_greek_rayleigh(0.1)
    partials = [rt.ScenePartial(d_greeks=[(1, gA)]), rt.ScenePartial(), rt.ScenePartial(d_greeks=[(2, gB)])]
    sc = rt.prepare_scene(m)
    with rt.make_handle(m) as h:
        rt.scene_set(h, sc)
        Nk = h.scene_get_bases(0)[0]
        rt.scene_set_partials(h, sc, partials)
        edge, dZpp, dZmp = h.scene_get_bases(2)
    assert edge == Nk and dZpp.shape == (P * M * K, Nk, Nk)
    named = {(1, 0): gA, (2, 2): gB}
    for got, sign in ((dZpp.reshape(P, M, K, Nk, Nk), 0), (dZmp.reshape(P, M, K, Nk, Nk), 1)):
        for p in range(P):
            for k in range(K):
                blk = got[p, :, k]
                if (k, p) in named:
                    Z = L.z_moments(nS, m.quad_points.qp_μ, [rows(named[(k, p)])], M)[sign][:, 0]   # [M, N(j), N(i)]
                    assert np.abs(Z).max() > 0 and np.array_equal(blk[:, :N, :N], Z), (k, p)
                    assert not np.any(blk[:, N:, :]) and not np.any(blk[:, :, N:]), (k, p)
                else:
                    assert not np.any(blk), (k, p)


# ---- 4. the reduction decision, both outcomes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("situation", ["physical", "source with U", "NaN in γ"])
def test_reduction_decision(situation):
    """the edge of the (I,Q) sub-problem (0: not reduced) is the uploaded route's: reduced for a physical set; not reduced by the host
    half of the condition when I0 has a U component; not reduced by the device flag when the m = 0 coupling entries are NaN (one set
    with a NaN in γ at l = 2).  Getter only: no run is made."""
    nS, l_trunc, _ = CASES["a"]
    pol = rt.PolarizationType(3, (1.0, 1.0, -1.0), (1.0, 0.0, 0.25)) if situation == "source with U" else None
    m = layout_model(nS, l_trunc, pol=pol, nan=situation == "NaN in γ")
    up1, st1 = resident_arrays(m, False)[1], resident_arrays(m, True)[1]
    assert st1[0] == up1[0]
    assert (up1[0] > 0) == (situation == "physical")
    if situation == "physical":
        assert same(st1, up1)


# ---- 5. handle reuse and state ---------------------------------------------------------------------------------------------------
def run_full(h, sc):
    R, T = rt.run_scene(h, sc)
    return (R, T) + tuple(h.get_hdr())


def test_handle_reuse():
    """host-uploaded, staged, host-uploaded again on ONE handle: each run is bitwise the fresh-handle run of its route"""
    m = layout_model(*CASES["a"][:2])
    sc_h, sc_r = rt.prepare_scene(m), rt.prepare_scene(route(m, True))
    fresh = []
    for sc in (sc_h, sc_r):
        with rt.make_handle(m) as h:
            fresh.append(run_full(h, sc))
    with rt.make_handle(m) as h:
        for sc, ref, what in ((sc_h, fresh[0], "host, first"), (sc_r, fresh[1], "staged, second"), (sc_h, fresh[0], "host, third")):
            assert_same_run(run_full(h, sc), ref, tuple(f"{x} ({what})" for x in ("R", "T", "hdr", "bhr_uw", "bhr_dw")))


def refused(code, call, *a, text=None, **kw):
    with pytest.raises(rtamd.MomError) as e:
        call(*a, **kw)
    assert e.value.code == code and (text is None or text in str(e.value)), str(e.value)


def test_states_and_arguments():
    m = route(layout_model(*CASES["d"][:2]), True)
    sc = rt.prepare_scene(m)
    greeks = [rows(g) for g in sc.greeks]
    set_null = lambda h, K=sc.K, M=sc.M: h.scene_set(sc.Nz, K, M, sc.tau, sc.varpi, sc.zw, None, None, sc.ndoubl, sc.iface, sc.tau_sum,
                                                     sc.albedo, sc.node, sc.cos_mphi, sc.sin_mphi)
    with rt.make_handle(m) as h:
        refused(L.MOM_EINVAL, set_null, h, text="mom_scene_set")                 # no stage: NULL is what it always was
        h.scene_stage_greeks(greeks, sc.M)
        set_null(h)
        refused(L.MOM_EINVAL, set_null, h, text="mom_scene_set")                 # the stage is consumed
        h.scene_stage_greeks(greeks, sc.M)
        refused(L.MOM_EINVAL, set_null, h, M=sc.M - 1, text=f"M = {sc.M}")       # both values in the text
        refused(L.MOM_EINVAL, set_null, h, M=sc.M - 1, text=f"M = {sc.M - 1}")
        h.scene_stage_greeks(greeks[:2], sc.M)
        refused(L.MOM_EINVAL, set_null, h, text="K = 2")
        refused(L.MOM_EINVAL, set_null, h, text=f"K = {sc.K}")
        h.scene_stage_greeks(greeks, sc.M)
        set_null(h)
        # partial stages: a duplicate pair, a disagreeing P, and a new scene drops a pending one
        pair = lambda k, p: ((k, p), greeks[1])
        refused(L.MOM_EINVAL, h.scene_stage_greek_partials, 2, [pair(1, 0), pair(1, 0)], text="twice")
        h.scene_stage_greek_partials(2, [pair(1, 0), pair(1, 1)])
        refused(L.MOM_EINVAL, h.scene_set_partials, 3, text="P = 2")
        h.scene_set_partials(2)
        assert h.scene_get_bases(2)[1].shape[0] == 2 * sc.M * sc.K
        h.scene_stage_greek_partials(2, [pair(2, 1)])
        h.scene_stage_greeks(greeks, sc.M)
        set_null(h)                                                              # a new scene: the partial stage is gone
        h.scene_set_partials(2)                                                  # NULL means "no dependence" again
        assert h.scene_get_bases(2)[1].size == 0
    with rt.make_handle(m, float_type="Float32") as h:
        refused(L.MOM_EUNSUPPORTED, h.scene_stage_greeks, greeks, sc.M, text="mom_scene_stage_greeks")
        refused(L.MOM_EUNSUPPORTED, h.scene_stage_greek_partials, 1, [((1, 0), greeks[1])], text="mom_scene_stage_greek_partials")
    h = L.Handle(len(m.quad_points.qp_μN), 3, 8, sc.M)
    try:
        refused(L.MOM_ESTATE, h.scene_stage_greeks, greeks, sc.M, text="mom_set_streams")
    finally:
        h.close()
