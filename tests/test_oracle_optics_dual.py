"""absorption.optics_partials_host -- the numpy twin of the device kernel k_optics_dual (mom_scene_set_optics_partials) -- against
the independent Dual oracle tests/optics_dual_oracle.py, against central differences of corert.construct_layer_inputs, and
against the existing absorption.optics_partials where that one applies.  No GPU."""
import dataclasses

import numpy as np
import pytest

import optics_dual_cases as oc
import optics_dual_oracle as odo
import rtamd

rt, ab = rtamd.corert, rtamd.absorption
S, NZ = 7, 4


@pytest.fixture(scope="module")
def case():
    """the scene (S = 7, Nz = 4, two aerosol types, all three modes), synthetic dτ_abs, the six parameters, the oracle's result"""
    model = oc.three_mode_model(rtamd.scenes.make_scene(1, 3, NZ, S, absorption=False), seed=2)
    md = oc.modes(model)
    assert np.all(md[:, 1] == 0) and np.all(md[0, [0, 2, 3]] == 2) and np.all(md[1, [0, 2, 3]] == 1) and model.τ_abs.min() > 0
    rng = np.random.default_rng(3)
    dtau_abs = model.τ_abs[None] * rng.uniform(-1.0, 1.0, (2, S, NZ))
    ps = oc.six_parameters(model)
    assert len(ps) == 6
    return model, dtau_abs, ps, odo.layer_optics_dual(model, oc.seeds(model, ps), dtau_abs)


def test_host_twin_matches_the_dual_oracle(case):
    """1e-13 of each column's maximum: every entry is a chain of a few tens of IEEE operations on terms bounded by that maximum,
    which leaves more than an order of magnitude over the rounding bound."""
    model, dtau_abs, ps, ((τ, ϖ, zw), (dτ, dϖ, dzw)) = case
    L = rt.construct_layer_inputs(model)
    assert np.array_equal(τ, L.τ) and np.array_equal(ϖ, L.ϖ) and np.array_equal(zw, L.zw)   # the oracle runs the same value statements
    got = oc.stack(ab.optics_partials_host(model, ps, dtau_abs), 3, S, NZ)
    for k in range(6):
        assert np.abs(dτ[k]).max() > 0 and np.abs(dϖ[k]).max() > 0
    assert np.abs(dzw[3]).max() > 0 and np.abs(dzw[4]).max() > 0 and np.abs(dzw[5]).max() > 0 and not np.any(dzw[:3])
    oc.assert_columns(got[0], dτ, 1e-13, "dτ host twin vs Dual oracle")
    oc.assert_columns(got[1], dϖ, 1e-13, "dϖ host twin vs Dual oracle")
    oc.assert_columns(got[2], dzw, 1e-13, "dzw host twin vs Dual oracle")


def stepped(model, dtau_abs, q, x):
    """the model with the parameter of OpticsPartial q at the value x (0 = the model itself)"""
    one = lambda w: 1.0 if w is None else 1.0 + x * np.asarray(w)[None, :]
    τ_abs = model.τ_abs * one(q.w_gas)
    for k, w in enumerate((q.w_p, q.w_T)):
        if w is not None:
            τ_abs = τ_abs + x * dtau_abs[k] * np.asarray(w)[None, :]
    aer = [dataclasses.replace(a, ω̃=a.ω̃ + (0.0 if q.dω̃ is None else x * q.dω̃[i]), fᵗ=a.fᵗ + (0.0 if q.dfᵗ is None else x * q.dfᵗ[i]))
           for i, a in enumerate(model.aerosol_optics)]
    return dataclasses.replace(model, τ_rayl=model.τ_rayl * one(q.w_rayl), τ_abs=τ_abs,
                               τ_aer=model.τ_aer + (0.0 if q.dτ_aer is None else x * q.dτ_aer), aerosol_optics=aer)


def test_host_twin_against_central_differences(case):
    """A sanity check: every parameter is a relative change (oc.six_parameters), stepped by 1e-6; bar 1e-7 of the column maximum."""
    model, dtau_abs, ps, _ = case
    got = oc.stack(ab.optics_partials_host(model, ps, dtau_abs), 3, S, NZ)
    L0 = rt.construct_layer_inputs(model)
    h = 1e-6
    fd = [[], [], []]
    for q in ps:
        Lp, Lm = (rt.construct_layer_inputs(stepped(model, dtau_abs, q, x)) for x in (h, -h))
        for L in (Lp, Lm):
            assert np.array_equal(L.ndoubl, L0.ndoubl) and np.array_equal(L.iface, L0.iface)
        for k, f in enumerate((lambda L: L.τ, lambda L: L.ϖ, lambda L: L.zw)):
            fd[k].append((f(Lp) - f(Lm)) / (2 * h))
    for k, name in enumerate(("dτ", "dϖ", "dzw")):
        oc.assert_columns(got[k], np.array(fd[k]), 1e-7, f"{name} host twin vs central differences")


def test_temperature_only_equals_optics_partials(case):
    model, dtau_abs, _, _ = case
    L = rt.construct_layer_inputs(model)
    new = ab.optics_partials_host(model, [rt.OpticsPartial(w_T=np.ones(NZ))], dtau_abs)[0]
    old = ab.optics_partials(L.τ, L.ϖ, dtau_abs[1])
    assert new.dzw is None and old.dzw is None
    oc.assert_columns(new.dτ[None], old.dτ[None], 1e-13, "dτ vs optics_partials")
    oc.assert_columns(new.dϖ[None], old.dϖ[None], 1e-13, "dϖ vs optics_partials")


def test_w_p_without_dtau_abs_is_refused(case):
    model, _, ps, _ = case
    with pytest.raises(ValueError):
        ab.optics_partials_host(model, ps[:1])
    assert len(ab.optics_partials_host(model, ps[2:])) == 4   # w_gas, w_rayl and the aerosol partials need no dτ_abs
