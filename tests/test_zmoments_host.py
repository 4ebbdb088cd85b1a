"""The host side of the device phase-matrix moments, without a GPU: the extended-precision arbiter (zmom_oracle.py) validated against
the oracle it restates, the batched host twin and the once-per-pair z_bases against the per-call function, and the argument checks of
mom_z_moments, which all come before the first HIP call."""
import dataclasses

import numpy as np
import pytest

import zmom_oracle as zo
from oracle import momref as mr

POLS = {1: "Stokes_I", 3: "Stokes_IQU", 4: "Stokes_IQUV"}


def rows(g):
    return (g.α, g.β, g.γ, g.δ, g.ϵ, g.ζ)


@pytest.mark.parametrize("n", [1, 3, 4])
def test_float64_twin_is_the_oracle_bitwise(rtamd, n):
    """zmom_oracle with dtype float64 performs momref's operations: its own validation.  mu = 1 and a node below 1e-2 included, every
    m up to l_max (the last one: zeros)."""
    μ = np.array([1.0, 0.83, 0.41, 0.0071, 0.2])
    for g in (rtamd.scenes.hg_like_greek(0.7, 9), rtamd.corert.get_greek_rayleigh(0.03)):
        for m in range(len(g.β) + 1):
            a = mr.compute_Z_moments(n, μ, mr.GreekCoefs(*rows(g)), m)
            b = zo.compute_Z_moments(n, μ, rows(g), m, dtype=np.float64)
            assert b[0].dtype == np.float64 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            ld = zo.compute_Z_moments(n, μ, rows(g), m)
            assert ld[0].dtype == np.longdouble
            # the triangle inequality: |Z| = 2 fact |A| <= 2 A_abs
            assert float(ld[2][0].min()) >= 0.0 and float(ld[2][1].min()) >= 0.0
            assert float(np.abs(ld[0]).max()) <= 2.0 * float(ld[2][0].max()) and float(np.abs(ld[1]).max()) <= 2.0 * float(ld[2][1].max())


def test_batch_on_the_host_is_the_per_call_function_bitwise(rtamd):
    rt = rtamd.corert
    μ = rtamd.scenes.scene_C2(S=8, Nz=2).quad_points.qp_μ
    greeks = [rt.get_greek_rayleigh(0.03), rtamd.scenes.hg_like_greek(0.7, 33)]
    for n in (1, 3, 4):
        pol = getattr(rt, POLS[n])()
        Zpp, Zmp = rtamd.compute_Z_moments_batch(pol, μ, greeks, 3, m_first=1)
        assert Zpp.shape == Zmp.shape == (3, 2, n * 20, n * 20)
        for mi in range(3):
            for k, g in enumerate(greeks):
                a = rt.compute_Z_moments(pol, μ, g, 1 + mi)
                assert np.array_equal(Zpp[mi, k], a[0]) and np.array_equal(Zmp[mi, k], a[1])


def _old_z_bases(rt, model):
    """z_bases of an unbanded model as it stood: every (m, Greek set) pair computed twice, once per output"""
    pol, μ = model.params.polarization_type, model.quad_points.qp_μ
    greeks = [model.greek_rayleigh] + [a.greek_coefs for a in model.aerosol_optics]
    Zpp = np.array([[rt.compute_Z_moments(pol, μ, g, m)[0] for g in greeks] for m in range(model.params.max_m)])
    Zmp = np.array([[rt.compute_Z_moments(pol, μ, g, m)[1] for g in greeks] for m in range(model.params.max_m)])
    return Zpp, Zmp


def test_z_bases_once_per_pair_is_bitwise_the_old_result(rtamd, monkeypatch):
    import bands_cases as bc
    rt = rtamd.corert
    m = rtamd.scenes.scene_C2(S=8, Nz=2)
    old = _old_z_bases(rt, m)
    calls = []
    real = rt.compute_Z_moments
    monkeypatch.setattr(rt, "compute_Z_moments", lambda *a: (calls.append(a[-1]), real(*a))[1])
    new = rt.z_bases(m)
    assert len(calls) == m.params.max_m * 2   # K = 2 sets, each (m, set) pair once
    assert new[0].shape == old[0].shape and np.array_equal(new[0], old[0]) and np.array_equal(new[1], old[1])
    b = bc.banded(78, 2)
    pol, μ = b.params.polarization_type, b.quad_points.qp_μ
    greeks = [b.greek_rayleigh] + [a.greek_coefs for band in b.bands.aerosol_optics for a in band]
    Z = rt.z_bases(b)
    assert Z[0].shape == (b.params.max_m, 7, 15, 15)
    for mm in range(b.params.max_m):
        for k, g in enumerate(greeks):
            ref = real(pol, μ, g, mm)
            assert np.array_equal(Z[0][mm, k], ref[0]) and np.array_equal(Z[1][mm, k], ref[1])


def test_flag_defaults_off_and_partials_twin(rtamd):
    import bands_cases as bc
    rt = rtamd.corert
    m = rtamd.scenes.scene_C2(S=8, Nz=2)
    assert m.params.z_moments_on_device is False and dataclasses.fields(m.params)[-1].name == "z_moments_on_device"
    assert rtamd.scenes.make_scene(1, 3, 2, 4, z_moments_on_device=True).params.z_moments_on_device is True
    b = bc.banded(78, 2)
    d = rt.AerosolOptics(rtamd.scenes.hg_like_greek(0.6, b.params.l_trunc), 0.1, 0.05)
    items = [(0, d, None, 0), (1, d, None, 2)]
    many = rtamd.aerosol_optics_partials(b, items)
    for it, p in zip(items, many):
        one = rtamd.aerosol_optics_partial(b, *it)
        assert np.array_equal(p.dZpp, one.dZpp) and np.array_equal(p.dZmp, one.dZmp) and np.array_equal(p.dω̃, one.dω̃)
        k = 1 + it[0] + 2 * it[3]
        for mm in range(b.params.max_m):
            assert np.array_equal(p.dZpp[mm, k], rt.compute_Z_moments(b.params.polarization_type, b.quad_points.qp_μ, d.greek_coefs, mm)[0])


def test_rejected_arguments(rtamd):
    """every MOM_EINVAL of mom_z_moments with its message; the checks run before any HIP call, so they need no GPU"""
    lib, L = rtamd.load(), rtamd._lib
    μ = L.f64([1.0, 0.5, 0.1])
    greek = L.f64(np.ones((2, 6, 5)))
    l_max = L.i32([5, 3])
    Z = [np.zeros((2, 2, 12, 12)) for _ in range(2)]
    ms = np.zeros(1)

    def call(n=4, n_mu=3, mu=μ, nG=2, l_pad=5, lm=l_max, gr=greek, m_first=0, M=2, inner=0, null=None):
        ptr = {"mu": L.dp(mu), "l_max": L.ip(lm), "greek": L.dp(gr), "Zpp": L.dp(Z[0]), "Zmp": L.dp(Z[1])}
        if null:
            ptr[null] = None
        return lib.mom_z_moments(0, n, n_mu, ptr["mu"], nG, l_pad, ptr["l_max"], ptr["greek"], m_first, M, inner, ptr["Zpp"], ptr["Zmp"], L.dp(ms))

    cases = [(dict(n=2), b"nStokes"), (dict(n=0), b"nStokes"), (dict(n_mu=0), b"n_mu"), (dict(nG=0), b"nG"), (dict(M=0), b"M must"),
             (dict(m_first=-1), b"m_first"), (dict(lm=L.i32([5, 0])), b"l_max"), (dict(lm=L.i32([6, 3])), b"l_max"),
             (dict(l_pad=0), b"l_pad"), (dict(mu=L.f64([1.0, 0.0, 0.1])), b"]0,1]"), (dict(mu=L.f64([1.0, 0.5, 1.0000001])), b"]0,1]"),
             (dict(mu=L.f64([1.0, -0.5, 0.1])), b"]0,1]"), (dict(mu=L.f64([1.0, np.nan, 0.1])), b"]0,1]"), (dict(inner=-1), b"set_inner"),
             (dict(nG=2, inner=3), b"set_inner")] + [(dict(null=k), b"null pointer") for k in ("mu", "l_max", "greek", "Zpp", "Zmp")]
    for kw, text in cases:
        assert call(**kw) == L.MOM_EINVAL, kw
        msg = lib.mom_last_global_error()
        assert b"mom_z_moments" in msg and text in msg, (kw, msg)
    with pytest.raises(L.MomError, match="mom_z_moments"):
        L.z_moments(2, μ, [tuple(np.ones(3) for _ in range(6))], 1)
    with pytest.raises(ValueError):
        L.z_moments(3, μ, [tuple(np.ones(3 + q) for q in range(6))], 1)


def test_fails_loudly_without_gpu(rtamd):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    rt = rtamd.corert
    with pytest.raises(rtamd.MomError) as e:
        rtamd.compute_Z_moments_batch(rt.Stokes_IQU(), np.array([1.0, 0.5]), [rt.get_greek_rayleigh(0.03)], 2, device=0)
    assert e.value.code == rtamd._lib.MOM_EHIP and "HIP device" in str(e.value)
    m = rtamd.scenes.make_scene(1, 3, 2, 4, z_moments_on_device=True)
    with pytest.raises(rtamd.MomError):
        rt.z_bases(m)   # no quiet fall-back to the host loop
