"""Test helper (not a test file): the scenes, parameters and comparisons the layer-optics Dual tests share
(test_oracle_optics_dual.py, test_gpu_optics_dual.py)."""
import dataclasses

import numpy as np

import rtamd

rt = rtamd.corert


def three_mode_model(base, seed=0, tau_abs=None):
    """`base` with two aerosol types such that every case of the `+` of types.jl:641-661 occurs: layer 1 has τ_rayl ≡ 0 (the left
    operand is all zero: mode 0, for both types, since the first has w_y = 0), aerosol type 1 has ω̃ = 0 (w_y = 0: mode 2 in the
    other layers), type 2 mixes there (mode 1).  τ_abs > 0.  Every ingredient of a layer is within two orders of magnitude of the
    others (the Rayleigh columns keep their spectral shape, rescaled): a central difference of τ, ϖ, zw with step h carries a
    rounding error of eps |value| / h, so a 1e-7 comparison at h = 1e-6 needs |partial| > 2e-3 |value| in every column."""
    rng = np.random.default_rng(seed)
    S, Nz = base.τ_rayl.shape
    τ_rayl = base.τ_rayl * (rng.uniform(0.05, 0.3, Nz) / base.τ_rayl.mean(axis=0))[None, :]
    τ_rayl[:, 1] = 0.0
    greek = rtamd.scenes.hg_like_greek(0.7, base.params.l_trunc)
    aer = [rt.AerosolOptics(greek, 0.0, 0.1), rt.AerosolOptics(greek, 0.93, 0.2)]
    τ_aer = rng.uniform(0.02, 0.2, (2, Nz))
    τ_abs = rng.uniform(0.01, 1.0, (S, Nz)) if tau_abs is None else tau_abs
    return dataclasses.replace(base, τ_rayl=τ_rayl, τ_abs=τ_abs, τ_aer=τ_aer, aerosol_optics=aer)


def modes(model):
    """the case of the `+` each (aerosol type, layer) takes, by construct_layer_inputs' own tests on the values"""
    S, Nz = model.τ_rayl.shape
    out = np.zeros((len(model.aerosol_optics), Nz), dtype=int)
    for z in range(Nz):
        x_zero = model.ϖ_Cabannes == 0.0 or not np.any(model.τ_rayl[:, z] != 0.0)
        for a, aer in enumerate(model.aerosol_optics):
            wy = (1 - aer.fᵗ * aer.ω̃) * model.τ_aer[a, z] * ((1 - aer.fᵗ) * aer.ω̃ / (1 - aer.fᵗ * aer.ω̃))
            out[a, z] = 0 if x_zero else (1 if wy != 0.0 else 2)
            x_zero = x_zero and wy == 0.0
    return out


def six_parameters(model, seed=1):
    """one OpticsPartial each for w_p, w_T, w_gas, w_rayl, dτ_aer, and dω̃ + dfᵗ together.  Every weight is O(1) and every absolute
    partial is O(its value): a parameter is a relative change.  dω̃ of the type with ω̃ = 0 stays 0: there the reference's value-side
    test `all(w_y .== 0)` makes the Dual run differ from a difference quotient by design."""
    rng = np.random.default_rng(seed)
    nAer, Nz = model.τ_aer.shape
    u = lambda: rng.uniform(0.5, 1.5, Nz)
    ps = [rt.OpticsPartial(w_p=u()), rt.OpticsPartial(w_T=u()), rt.OpticsPartial(w_gas=u()), rt.OpticsPartial(w_rayl=u())]
    if nAer:
        ps.append(rt.OpticsPartial(dτ_aer=model.τ_aer * rng.uniform(0.5, 1.5, (nAer, Nz))))
        ω̃ = np.array([a.ω̃ for a in model.aerosol_optics])
        ps.append(rt.OpticsPartial(dω̃=-0.5 * ω̃, dfᵗ=rng.uniform(0.1, 0.3, nAer)))
    return ps


def combined(ps):
    """one parameter that carries every field of `ps` at once"""
    out = rt.OpticsPartial()
    for p in ps:
        for f in dataclasses.fields(p):
            v = getattr(p, f.name)
            if v is not None and not (f.name == "dalbedo" and v == 0.0):
                setattr(out, f.name, v)
    return out


def seeds(model, ps):
    """OpticsPartials -> the arrays optics_dual_oracle.layer_optics_dual takes (parameter index first, None = zeros)"""
    nAer, Nz = model.τ_aer.shape
    P = len(ps)
    get = lambda f, shape: np.array([np.zeros(shape) if f(p) is None else np.asarray(f(p), dtype=np.float64) for p in ps]).reshape((P,) + shape)
    return {"w_p": get(lambda p: p.w_p, (Nz,)), "w_T": get(lambda p: p.w_T, (Nz,)), "w_gas": get(lambda p: p.w_gas, (Nz,)),
            "w_rayl": get(lambda p: p.w_rayl, (Nz,)), "dτ_aer": get(lambda p: p.dτ_aer, (nAer, Nz)), "dω̃": get(lambda p: p.dω̃, (nAer,)),
            "dfᵗ": get(lambda p: p.dfᵗ, (nAer,))}


def stack(scene_partials, K, S, Nz):
    """a list of ScenePartials -> dτ, dϖ [P, S, Nz], dzw [P, K, S, Nz] (an absent dzw: zeros)"""
    z = np.zeros((K, S, Nz))
    return (np.array([p.dτ for p in scene_partials]), np.array([p.dϖ for p in scene_partials]),
            np.array([z if p.dzw is None else p.dzw for p in scene_partials]))


def assert_columns(got, ref, bar, what):
    """got, ref [P, ..., Nz]: every column (one layer, one partial) within `bar` of that column's maximum magnitude in ref"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    worst = 0.0
    for k in range(ref.shape[0]):
        for z in range(ref.shape[-1]):
            scale = np.abs(ref[k, ..., z]).max()
            err = np.abs(got[k, ..., z] - ref[k, ..., z]).max()
            worst = max(worst, err / scale if scale else err)
            assert err <= bar * scale, f"{what}: partial {k}, layer {z}: {err / scale if scale else err:.3e} of the column maximum > {bar:.0e}"
    print(f"{what}: worst column {worst:.2e} of its maximum (bar {bar:.0e})")
