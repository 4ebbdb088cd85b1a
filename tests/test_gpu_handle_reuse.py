"""A handle owns its device buffers (csrc/mom_host.hpp: MomDevBuf) and reallocates or grows them as the calls it serves change
shape.  The property tested here is always the same: a handle that has been through a sequence of differently shaped calls
gives results BITWISE equal to those of a fresh handle -- nothing of an earlier call survives in a buffer that was reused,
regrown or replaced.  S = 16 and Nz <= 3 throughout; every fresh-handle reference is computed once per case."""
import dataclasses

import numpy as np
import pytest

S = 16
WHAT = ("R", "T", "hdr", "bhr_uw", "bhr_dw")


def _scenes(rtamd, nS, lt):
    """Scene A: Nz = 3, three view angles, all moments, Lambertian surface.  Scene B on the same streams: Nz = 2, ONE view
    angle, two of the three moments, an RPV BRDF surface (d_hdrJm, d_Rsurf, d_Rsurf0)."""
    mA = rtamd.scenes.make_scene(nS, lt, 3, S, seed=11 * nS + lt)
    mB = rtamd.scenes.make_scene(nS, lt, 2, S, max_m=2, seed=13 * nS + lt, aerosol_total=0.4)
    mB.params.brdf = rtamd.corert.rpvSurfaceScalar(0.1, 0.8, 0.7, -0.1)
    A, B = rtamd.prepare_scene(mA), rtamd.prepare_scene(mB)
    nV = len(B.node)
    B = dataclasses.replace(B, node=B.node[:1].copy(), cos_mphi=B.cos_mphi.reshape(B.M, nV)[:, :1].reshape(-1).copy(),
                            sin_mphi=B.sin_mphi.reshape(B.M, nV)[:, :1].reshape(-1).copy())
    assert (A.Nz, len(A.node), A.M, A.surf_kind) == (3, 3, 3, 0) and (B.Nz, len(B.node), B.M, B.surf_kind) == (2, 1, 2, 1)
    return mA, A, B


def _outputs(rtamd, h, sc):
    R, T = rtamd.corert.run_scene(h, sc)
    return (R, T) + tuple(h.get_hdr())


@pytest.mark.gpu
@pytest.mark.parametrize("nS,lt,N,float_type", [
    (1, 1, 4, "Float64"),     # scene A on the lane kernel (d_smtab, d_ndif, d_smpart), scene B (BRDF) on the general path
    (3, 1, 12, "Float64"),    # wave kernel
    (3, 15, 33, "Float64"),   # padded to 36, with the (I,Q) sub-problem: every *0 buffer, the resume table
    (4, 27, 68, "Float64"),   # generic mode: scratch slabs
    (3, 1, 12, "Float32"), (3, 15, 33, "Float32")])   # momf_scene and its sub-scene
def test_scene_sequence_equals_fresh_handles(rtamd, nS, lt, N, float_type):
    mA, A, B = _scenes(rtamd, nS, lt)
    assert A.N == N and B.N == N
    fresh = {}
    for name, sc in (("A", A), ("B", B)):
        with rtamd.corert.make_handle(mA, float_type=float_type) as h:
            fresh[name] = _outputs(rtamd, h, sc)
    with rtamd.corert.make_handle(mA, float_type=float_type) as h:
        for step, (name, sc) in enumerate((("A", A), ("B", B), ("A", A))):
            got = _outputs(rtamd, h, sc)
            for k, what in enumerate(WHAT):
                assert got[k].shape == fresh[name][k].shape
                assert np.array_equal(got[k], fresh[name][k]), f"step {step} (scene {name}) on the reused handle: {what}"


@pytest.mark.gpu
@pytest.mark.parametrize("float_type", ["Float64", "Float32"])
def test_operator_calls_equal_fresh_handles(rtamd, float_type):
    """batch_inv / batched_mul with batch 4, 32, 4 and elemental with z_batch 1, S, 1 on ONE handle (n = 8): the grow-only
    workspaces and the Z buffers grow in the middle call and are reused, larger than needed, in the last."""
    n = 8
    m = rtamd.scenes.make_scene(1, 9, 3, S)
    sc = rtamd.prepare_scene(m)
    assert sc.N == n
    rng = np.random.default_rng(5)
    mats = {b: (rng.standard_normal((b, n, n)) + 4.0 * np.eye(n), rng.standard_normal((b, n, n))) for b in (4, 32)}
    ts, dt, w = rng.uniform(0.1, 1.0, S), rng.uniform(1e-3, 1e-2, S), rng.uniform(0.5, 1.0, S)
    Z = {zb: (rng.uniform(0.0, 1.0, (zb, n, n)), rng.uniform(0.0, 1.0, (zb, n, n))) for zb in (1, S)}

    def blas(h, b):
        return h.batch_inv(n, b, mats[b][0]), h.batched_mul(n, b, mats[b][0], mats[b][1])

    def elemental(h, zb):
        h.elemental(0, 2, ts, dt, w, Z[zb][0], Z[zb][1], zb)
        return tuple(h.download(k) for k in range(6))          # the added layer: r-+, r+-, t--, t++, j0+, j0-

    fresh_blas, fresh_el = {}, {}
    for b in (4, 32):
        with rtamd.corert.make_handle(m, float_type=float_type) as h:
            fresh_blas[b] = blas(h, b)
    for zb in (1, S):
        with rtamd.corert.make_handle(m, float_type=float_type) as h:
            fresh_el[zb] = elemental(h, zb)
    with rtamd.corert.make_handle(m, float_type=float_type) as h:
        for step, (b, zb) in enumerate(((4, 1), (32, S), (4, 1))):
            for got, ref, what in zip(blas(h, b), fresh_blas[b], ("batch_inv", "batched_mul")):
                assert np.array_equal(got, ref), f"step {step}: {what}, batch {b}"
            for k, (got, ref) in enumerate(zip(elemental(h, zb), fresh_el[zb])):
                assert np.array_equal(got, ref), f"step {step}: elemental, z_batch {zb}, added array {k}"


@pytest.mark.gpu
def test_multisensor_sequence_equals_fresh_handles(rtamd):
    """One sensor, three sensors at distinct levels, one sensor again on ONE handle (Float64, IQU N = 12): the composite sets
    and the output buffer grow in the middle call."""
    m = rtamd.scenes.make_scene(3, 1, 3, S, seed=3)
    sc = rtamd.prepare_scene(m)
    assert sc.N == 12 and sc.Nz == 3
    calls = ((1,), (0, 1, 2), (1,))
    fresh = {}
    for lv in set(calls):
        with rtamd.corert.make_handle(m) as h:
            rtamd.corert.scene_set(h, sc)
            fresh[lv] = h.rt_run_multisensor(lv)
    with rtamd.corert.make_handle(m) as h:
        rtamd.corert.scene_set(h, sc)
        for step, lv in enumerate(calls):
            uw, dw = h.rt_run_multisensor(lv)
            assert uw.shape == (len(lv), 3, 3, S)
            assert np.array_equal(uw, fresh[lv][0]), f"step {step}, sensor levels {lv}: uwJ"
            assert np.array_equal(dw, fresh[lv][1]), f"step {step}, sensor levels {lv}: dwJ"
