"""Test helper (not a test file): the reference's layer algebra on Dual numbers.

The reference gets the partials of the layer optics by running constructCoreOpticalProperties / createAero
(compEffectiveLayerProperties.jl:1-85) and the `+` of types.jl:632-678 on ForwardDiff.Dual element types.  This file runs the
statements of corert.construct_layer_inputs on the `Dual` class of tests/absdual_oracle.py (a value and P partials, ForwardDiff's
rules per operation), seeded from the partials of the ingredients.  It shares no code with absorption.optics_partials_host or the
device kernel: there the product and quotient rules are written out per statement, here the operators of `Dual` apply them.

Boolean decisions (the all-zero tests of types.jl:641-661) are taken on the values, as ForwardDiff takes them.
"""
import numpy as np

from absdual_oracle import Dual


def const(v, P):
    v = np.asarray(v, dtype=np.float64)
    return Dual(v, np.zeros((P,) + v.shape))


def layer_optics_dual(model, seeds, dtau_abs=None):
    """`seeds`: the partials of the ingredients with the parameter index first -- w_p, w_T, w_gas, w_rayl [P, Nz], dτ_aer
    [P, nAer, Nz], dω̃, dfᵗ [P, nAer]; dtau_abs [2, S, Nz].  Returns (τ, ϖ [S, Nz], zw [K, S, Nz]) and their partials
    (dτ, dϖ [P, S, Nz], dzw [P, K, S, Nz])."""
    S, Nz = model.τ_rayl.shape
    K = 1 + len(model.aerosol_optics)
    P = seeds["w_rayl"].shape[0]
    if dtau_abs is None:
        dtau_abs = np.zeros((2, S, Nz))
    τ, ϖ, zw = np.empty((S, Nz)), np.empty((S, Nz)), np.empty((K, S, Nz))
    dτ, dϖ, dzw = np.empty((P, S, Nz)), np.empty((P, S, Nz)), np.empty((P, K, S, Nz))
    for z in range(Nz):
        # the Dual inputs of this layer: each ingredient with the partials its parameters give it
        τr = model.τ_rayl[:, z]
        τz = Dual(τr.copy(), seeds["w_rayl"][:, z][:, None] * τr[None, :])
        τa = model.τ_abs[:, z]
        τ_abs = Dual(τa.copy(), seeds["w_p"][:, z][:, None] * dtau_abs[0][:, z][None, :] + seeds["w_T"][:, z][:, None] * dtau_abs[1][:, z][None, :]
                     + seeds["w_gas"][:, z][:, None] * τa[None, :])
        ϖz = const(np.full(S, float(model.ϖ_Cabannes)), P)
        w = [const(np.full(S, 1.0 if k == 0 else 0.0), P) for k in range(K)]
        for a, aer in enumerate(model.aerosol_optics, start=1):
            ω̃ = Dual(np.array([aer.ω̃], dtype=np.float64), seeds["dω̃"][:, a - 1][:, None].copy())
            fᵗ = Dual(np.array([aer.fᵗ], dtype=np.float64), seeds["dfᵗ"][:, a - 1][:, None].copy())
            τ_aer = Dual(np.array([model.τ_aer[a - 1, z]], dtype=np.float64), seeds["dτ_aer"][:, a - 1, z][:, None].copy())
            τy = (1 - fᵗ * ω̃) * τ_aer
            ϖy = (1 - fᵗ) * ω̃ / (1 - fᵗ * ω̃)
            wx, wy = τz * ϖz, τy * ϖy
            tot = wx + wy
            τn = τz + τy
            ϖn = tot / τn
            if np.all(wx.v == 0.0):
                w = [const(np.zeros(S), P) for _ in range(K)]
                w[a] = const(np.ones(S), P)
            elif not np.all(wy.v == 0.0):
                f = wx / tot
                w = [wk * f for wk in w]
                w[a] = wy / tot
            τz, ϖz = τn, ϖn
        τn = τz + τ_abs
        ϖz = (τz * ϖz) / τn
        τ[:, z], ϖ[:, z], dτ[:, :, z], dϖ[:, :, z] = τn.v, ϖz.v, τn.d, ϖz.d
        for k in range(K):
            zw[k, :, z], dzw[:, k, :, z] = np.broadcast_to(w[k].v, (S,)), np.broadcast_to(w[k].d, (P, S))
    return (τ, ϖ, zw), (dτ, dϖ, dzw)
