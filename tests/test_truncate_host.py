"""The host side of the device δ-BGE truncation, without a GPU: the argument checks of mom_truncate_phase, which all come before the
first HIP call, and the fallbacks of the public layer (device=None is bitwise the numpy text, l_max > 128 and Float32 coefficients
take the host path with one warning per process)."""
import warnings

import numpy as np
import pytest

import trunc_cases as tc


def _call(rtamd, **kw):
    lib, L = rtamd.load(), rtamd._lib
    a = dict(n_mu=5, nG=2, nP=1, l_full=6, l_tr=4, null=None, mu=None, w_mu=None, greek=None)
    a.update(kw)
    μ, w = rtamd.scattering.gausslegendre(5)
    mu = L.f64(μ if a["mu"] is None else a["mu"])
    w_mu = L.f64(w if a["w_mu"] is None else a["w_mu"])
    R, nG, lf, lt = max(1 + a["nP"], 1), max(a["nG"], 1), max(a["l_full"], 1), max(a["l_tr"], 1)
    greek = L.f64(np.ones((nG, R, 6, lf)) if a["greek"] is None else a["greek"])
    out, c0, status, ms = np.zeros((nG, R, 6, lt)), np.zeros((nG, R)), np.zeros(nG, dtype=np.int32), np.zeros(1)
    ptr = {"mu": L.dp(mu), "w_mu": L.dp(w_mu), "greek": L.dp(greek), "greek_t": L.dp(out), "c0": L.dp(c0), "status": L.ip(status)}
    if a["null"]:
        ptr[a["null"]] = None
    rc = lib.mom_truncate_phase(0, a["n_mu"], ptr["mu"], ptr["w_mu"], a["nG"], a["nP"], a["l_full"], a["l_tr"], ptr["greek"],
                                ptr["greek_t"], ptr["c0"], ptr["status"], L.dp(ms))
    return rc, lib.mom_last_global_error()


def test_rejected_arguments(rtamd):
    L = rtamd._lib
    bad = np.ones((2, 2, 6, 6))
    bad[1, 1, 4, 5] = np.inf
    nan = np.ones((2, 2, 6, 6))
    nan[0, 0, 0, 0] = np.nan
    cases = [(dict(n_mu=0), b"n_mu"), (dict(nG=0), b"nG"), (dict(l_full=0), b"l_full"), (dict(l_tr=0), b"l_tr"), (dict(nP=-1), b"nP"),
             (dict(l_tr=7), b"l_tr must not exceed l_full"), (dict(mu=[-1.0000001, -0.5, 0.0, 0.5, 1.0]), b"[-1, 1]"),
             (dict(mu=[-1.0, -0.5, 0.0, 0.5, 1.5]), b"[-1, 1]"), (dict(mu=[-1.0, np.nan, 0.0, 0.5, 1.0]), b"[-1, 1]"),
             (dict(w_mu=[0.1, 0.2, np.inf, 0.2, 0.1]), b"not finite"), (dict(greek=bad), b"not finite"), (dict(greek=nan), b"not finite")]
    cases += [(dict(null=k), b"null pointer") for k in ("mu", "w_mu", "greek", "greek_t", "c0", "status")]
    for kw, text in cases:
        rc, msg = _call(rtamd, **kw)
        assert rc == L.MOM_EINVAL, (kw, rc, msg)
        assert b"mom_truncate_phase" in msg and text in msg, (kw, msg)
    # mu = -1 and mu = 1 are nodes like any other: the checks pass and the call goes on to look for a device


def test_order_above_128_is_unsupported(rtamd):
    L = rtamd._lib
    rc, msg = _call(rtamd, l_full=129, l_tr=129)
    assert rc == L.MOM_EUNSUPPORTED and b"mom_truncate_phase" in msg and b"128" in msg, (rc, msg)
    rc, msg = _call(rtamd, l_full=130, l_tr=129, nP=-1)   # a bad argument is reported first
    assert rc == L.MOM_EINVAL
    with pytest.raises(L.MomError) as e:
        L.truncate_phase(*rtamd.scattering.gausslegendre(5), np.ones((1, 1, 6, 130)), 129)
    assert e.value.code == L.MOM_EUNSUPPORTED
    with pytest.raises(ValueError):
        L.truncate_phase(*rtamd.scattering.gausslegendre(5), np.ones((1, 6, 130)), 3)


def _same(a, b):
    return np.array_equal(tc.stack(a), tc.stack(b)) and (a.ω̃, a.fᵗ, a.k) == (b.ω̃, b.fᵗ, b.k)


def test_host_route_is_unchanged_and_fallbacks_take_it(rtamd):
    sc = rtamd.scattering
    g, dirs = tc.greek_set("case2")
    aero, parts = tc.optics(rtamd, g), [tc.optics(rtamd, d) for d in dirs[:2]]
    mod = sc.δBGE(10, 2.0)
    a = sc.truncate_phase(mod, aero)
    assert _same(a, sc.truncate_phase(mod, aero, device=None)) and _same(a, sc.truncate_phase(mod, aero, None, None))
    v, d = sc.truncate_phase(mod, aero, parts)
    batch = rtamd.truncate_phase_batch(mod, [aero, aero], [parts, parts[:1]], device=None)
    assert _same(batch[0][0], v) and all(_same(x, y) for x, y in zip(batch[0][1], d)) and len(batch[1][1]) == 1 and _same(batch[1][1][0], d[0])
    assert [_same(x, a) for x in rtamd.truncate_phase_batch(mod, [aero], device=None)] == [True]
    assert rtamd.truncate_phase_batch(mod, [], device=0) == []
    with pytest.raises(ValueError):
        rtamd.truncate_phase_batch(mod, [aero], [parts, parts], device=0)
    # l_max > 128 and Float32 coefficients: the host path, whatever the device, with ONE warning for all of them
    gb, _ = tc.greek_set("bigger")
    big = tc.optics(rtamd, gb)
    f32 = rtamd.corert.AerosolOptics(rtamd.corert.GreekCoefs(*(np.asarray(r, dtype=np.float32) for r in g)), 0.9, 0.0, 2.0)
    sc._warned_host_truncation = False
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        b129 = sc.truncate_phase(sc.δBGE(129, 2.0), big, device=0)
        again = rtamd.truncate_phase_batch(sc.δBGE(129, 2.0), [big, big], device=0)
        lo = sc.truncate_phase(mod, f32, device=0)
    assert len([w for w in seen if issubclass(w.category, RuntimeWarning) and "host path" in str(w.message)]) == 1
    assert _same(b129, sc.truncate_phase(sc.δBGE(129, 2.0), big)) and _same(again[1], b129) and _same(lo, sc.truncate_phase(mod, f32))


def test_fails_loudly_without_gpu(rtamd):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    sc = rtamd.scattering
    g, _ = tc.greek_set("absorbing")
    with pytest.raises(rtamd.MomError) as e:
        sc.truncate_phase(sc.δBGE(10, 2.0), tc.optics(rtamd, g), device=0)   # no quiet fall-back to the host text
    assert e.value.code == rtamd._lib.MOM_EHIP and "HIP device" in str(e.value)
