"""The second and later units of a persistent workgroup.  Almost every layer kernel creates a workgroup once, sets up LDS state (the
stream tables, c.ptab, the strip slots, the lay[] batch, c.tabE / c.tabZS, the held th[] registers, *c.bad, the scratch slabs of the
generic mode, the resume tables) and then walks `for (pt = blockIdx.x; pt < units; pt += gridDim.x)` (the two-buffer image: tickets of
its queue).  Every case here gives each workgroup of the launch under test two whole rounds and a partial third (the quad-block
image: more units than the device holds wavefronts) and compares three ways:

  1. with the C oracle on ALL points (R, T, hdr, bhr), at the suite's bars;
  2. bitwise with the same handle options on the permuted spectral axis (reversed in the first case of a group, rotated by an odd
     offset in the others): every unit gets another predecessor in its workgroup.  Units are independent and own their composite
     blocks (tests/test_gpu_strip2_sched.py), so the bar is exact;
  3. bitwise with the last CUs // moments points run alone on a fresh handle, where no workgroup of any image has a second unit:
     state that is wrong for every later unit whatever its predecessor.

The grid bounds are read from the sources (later_units.grid_constants), S is derived from them and the device's CU count."""
import subprocess
import sys

import numpy as np
import pytest

import helpers
from later_units import grid_constants, points_for, take, take_model
from oracle import momref as mr
from test_gpu_strip_row_blocks import NAMES, THICK

gpu = pytest.mark.gpu
WAVES_PER_CU = 32     # the quad-block image's workgroup is one wavefront: the hardware holds 8 per SIMD, 32 per CU, whatever its occupancy
M = 3                 # Fourier moments of scenes.make_scene
LEVELS = [2, 0, 1]    # sensors of the multi-target cases (unsorted: the library orders the slabs itself)

_SCENES = {}


def _scene(rtamd, nS, lt, Nz, S, kw):
    """(model, prepared scene, oracle result or None) of one seeded scene, made once"""
    key = (nS, lt, Nz, S, tuple(sorted(kw.items())))
    if key not in _SCENES:
        m = rtamd.scenes.make_scene(nS, lt, Nz, S, seed=11 * nS + lt, **kw)
        _SCENES[key] = [m, rtamd.prepare_scene(m), None, None]
    return _SCENES[key]


def _oracle(cref, entry):
    if entry[2] is None:
        out = cref.rt_run_full(cref.pack_scene(helpers.oracle_scene(entry[0])))
        assert out[5] == 0
        for a in out[:5]:
            a.setflags(write=False)
        entry[2] = out[:5]
    return entry[2]


@pytest.fixture(scope="module")
def cus():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked once in a process of its own: with the whole suite in one
    process the library has initialised the device long before, and torch, which brings its own HIP runtime, then reports no GPU."""
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return int(out.stdout.split()[-1])


def _run(rtamd, m, sc, opts, float_type="Float64"):
    """One run on a fresh handle of sc.S points: (R, T, hdr, bhr_uw, bhr_dw), the timers, strip2_resumed()"""
    with rtamd.corert.make_handle(m, S=sc.S, float_type=float_type) as h:
        for name, v in opts.items():
            h.set_option(getattr(rtamd._lib, name), v)
        R, T = rtamd.corert.run_scene(h, sc)
        out = (R, T) + tuple(h.get_hdr())
        return out, h.timers(), (h.strip2_resumed() if float_type == "Float64" else (0, 0))


def _run_ms(rtamd, m, sc, opts):
    with rtamd.corert.make_handle(m, S=sc.S) as h:
        for name, v in opts.items():
            h.set_option(getattr(rtamd._lib, name), v)
        rtamd.corert.scene_set(h, sc)
        return tuple(h.rt_run_multisensor(LEVELS))


def _order(first, S):
    """S-1 ... 0 in the first case of a group, elsewhere a rotation by an odd offset"""
    return np.arange(S)[::-1].copy() if first else np.roll(np.arange(S), -((S // 3) | 1))


def _same(a, b, names, what):
    for k, name in enumerate(names):
        if not np.array_equal(a[k], b[k]):
            pts = np.nonzero(np.any((a[k] != b[k]).reshape(-1, a[k].shape[-1]), axis=0))[0]
            raise AssertionError(f"{what}: {name} differs at {pts.size} of {a[k].shape[-1]} points, first {pts[:8]}, "
                                 f"max |Δ| = {np.nanmax(np.abs(a[k] - b[k])):.3e}")


def _order_and_tail(run, sc, big, first, tail_n, names=NAMES):
    """Comparisons 2 and 3 of the module docstring; run(scene) -> the outputs, spectral axis last"""
    S = sc.S
    perm = _order(first, S)
    got = run(take(sc, perm))
    back = np.argsort(perm)
    _same([x[..., back] for x in got], big, names, "permuted spectral axis against the first run")
    assert 0 < tail_n < S
    tail = np.arange(S - tail_n, S)
    alone = run(take(sc, tail))
    _same(alone, [x[..., tail] for x in big], names, f"the last {tail_n} points alone against their columns of the first run")


def _against_oracle(out, ref, sc, what):
    Rr, Tr, Hr, upr, dwr = ref
    tol = helpers.stokes_rtol(sc.ndoubl)
    d = max(helpers.assert_stokes_close(out[0], Rr, rtol=tol, what=f"{what}: R"),
            helpers.assert_stokes_close(out[1], Tr, rtol=tol, what=f"{what}: T"),
            helpers.assert_stokes_close(out[2], Hr, rtol=tol, what=f"{what}: hdr"))
    np.testing.assert_allclose(out[4], dwr, rtol=max(tol, 1e-10), atol=helpers.ATOL_STOKES)
    return d


def _rounds(units, bound, exact=True):
    """two whole rounds and part of a third for every workgroup of a grid of `bound`"""
    assert units >= 2 * bound + bound // 2 + 1, (units, bound)
    if exact:
        assert units % bound != 0, (units, bound)
    return units / bound


def _report(what, N, bound, S, units, d):
    print(f"later units, {what}: N = {N}, grid bound {bound}, S = {S}, {units} units, {units / bound:.2f} rounds, "
          f"oracle distance {d:.2e}")


# ---- the harness itself (CPU) ---------------------------------------------------------------------------------------------
def test_take_and_the_oracle_on_a_permuted_axis(rtamd, cref):
    """take() is spectral_slice for an index array, the gather commutes with the host preparation, and the C oracle -- which
    treats the points independently -- returns the permuted columns of its answer for the permuted scene, bit for bit: what the
    order comparison needs of the harness, shown without the GPU."""
    m = rtamd.scenes.make_scene(3, 9, 4, 23, seed=5)
    sc = rtamd.prepare_scene(m)
    arrays = ("tau", "varpi", "zw", "Zpp", "Zmp", "ndoubl", "iface", "tau_sum", "node", "cos_mphi", "sin_mphi")
    for lo, hi in ((0, 23), (4, 17), (22, 23)):
        a, b = take(sc, np.arange(lo, hi)), sc.spectral_slice(lo, hi)
        for name in arrays:
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
        assert (a.N, a.nStokes, a.S, a.Nz, a.K, a.M, a.albedo, a.surf_kind) == (b.N, b.nStokes, b.S, b.Nz, b.K, b.M, b.albedo, b.surf_kind)
        assert a.Rsurf is b.Rsurf is None and a.albedo_spec is b.albedo_spec is None
    m2 = rtamd.scenes.make_scene(3, 9, 4, 23, seed=5)
    m2.params.brdf = rtamd.corert.LambertianSurfaceLegendre((0.2, 0.05, -0.02))        # a surface with a spectral axis
    sc2 = rtamd.prepare_scene(m2)
    assert np.array_equal(take(sc2, np.arange(3, 9)).albedo_spec, sc2.spectral_slice(3, 9).albedo_spec)
    for first in (True, False):
        perm = _order(first, sc.S)
        assert np.array_equal(np.sort(perm), np.arange(sc.S)) and perm[0] != 0
        mp = take_model(m, perm)
        a, b = take(sc, perm), rtamd.prepare_scene(mp)
        for name in arrays:
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
        assert np.array_equal(a.tau.reshape(sc.Nz, sc.S)[:, 0], sc.tau.reshape(sc.Nz, sc.S)[:, perm[0]])
        ref = cref.rt_run_full(cref.pack_scene(helpers.oracle_scene(m)))
        got = cref.rt_run_full(cref.pack_scene(helpers.oracle_scene(mp)))
        assert ref[5] == 0 and got[5] == 0
        _same(got[:5], [x[..., perm] for x in ref[:5]], NAMES, "oracle on the permuted scene")
        assert not np.array_equal(got[0], ref[0])


def test_unit_counts_from_the_sources():
    """The constants the cases derive S from are where the sources had them (CPU: a changed launch rule shows here first)."""
    g = grid_constants()
    assert all(v >= 1 for v in g.values()), g
    for cu in (64, 256, 304):
        for per in (g["strip8"], g["strip4"], g["strip2"], g["lean"], g["lean6"]):
            for mom in (2, 3):
                assert points_for(per * cu, mom) * mom >= 2 * per * cu + (per * cu) // 2 + 1
                assert (points_for(per * cu, mom) - 1) * mom < 2 * per * cu + (per * cu) // 2 + 1


# ---- lean images and the 4-wave strip finisher, edges 36 / 40 / 44 ---------------------------------------------------------
LEAN_CASES = [(4, 11, 36, 1, False), (4, 11, 36, 2, False), (4, 11, 36, 0, False),
              (4, 13, 40, 1, False), (4, 13, 40, 2, False), (4, 13, 40, 0, False),
              (4, 13, 40, 1, True), (4, 13, 40, 2, True), (4, 13, 40, 0, True),
              (4, 15, 44, 0, False)]


@gpu
@pytest.mark.parametrize("nS,lt,N,lean,thick", LEAN_CASES)
def test_lean_images_later_units(rtamd, cref, cus, nS, lt, N, lean, thick):
    """MOM_OPT_LEAN = 1: the lean image, three workgroups per CU; 2: the six-wave lean image, two per CU; 0: the 4-wave strip
    finisher alone, two per CU.  The full problem's launch holds the moments 1 .. M - 1.  Thick layers: units leave the first
    stage and the finisher's workgroups meet finished and resumed units in turn (a resumed one enters lay[] in mid-batch)."""
    g = grid_constants()
    bound = {1: g["lean"], 2: g["lean6"], 0: g["strip4"]}[lean] * cus
    S = points_for(bound, M - 1)
    entry = _scene(rtamd, nS, lt, 4, S, THICK if thick else {})
    m, sc = entry[:2]
    assert sc.N == N and sc.M == M and sc.S == S
    units = S * (M - 1)
    _rounds(units, bound)
    opts = dict(MOM_OPT_LEAN=lean)
    big, t, _ = _run(rtamd, m, sc, opts)
    off, t0, _ = (big, t, None) if lean == 0 else _run(rtamd, m, sc, dict(MOM_OPT_LEAN=0))
    assert t0["full_launches"] == 1 and t["full_launches"] == 1                     # the sweep: one launch for all layers
    if lean:
        assert t["layer_launches"] > t0["layer_launches"], (t, t0)                  # the first stage, and the finisher behind it
    if lean == 1:
        _same(big, off, NAMES, "the four-wave lean image against the strip finisher alone")
    d = _against_oracle(big, _oracle(cref, entry), sc, f"MOM_OPT_LEAN = {lean}")
    _order_and_tail(lambda s: _run(rtamd, m, s, opts)[0], sc, big, (N, lean, thick) == (36, 1, False), cus // (M - 1))
    _report(f"MOM_OPT_LEAN = {lean}{' thick' if thick else ''}", N, bound, S, units, d)


# ---- the 8-wave strip finisher, one workgroup per CU ------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("thick", [False, True])
def test_strip8_finisher_later_units(rtamd, cref, cus, thick):
    """Edge 52.  Thin with MOM_OPT_STRIP2 = 0: every unit runs on the 8-wave image.  Thick with the two-buffer image in front: the
    units it leaves (0 < left < units) are finished by 8-wave workgroups that skip the finished ones between them."""
    g = grid_constants()
    bound8, bound2 = g["strip8"] * cus, g["strip2"] * cus
    bound = bound2 if thick else bound8
    S = points_for(bound, M - 1)
    entry = _scene(rtamd, 4, 19, 4, S, THICK if thick else {})
    m, sc = entry[:2]
    assert sc.N == 52 and sc.M == M
    units = S * (M - 1)
    _rounds(units, bound)
    _rounds(units, bound8)
    opts = dict(MOM_OPT_STRIP2=1 if thick else 0)
    big, t, (ru, left) = _run(rtamd, m, sc, opts)
    other, t1, (ru1, left1) = _run(rtamd, m, sc, dict(MOM_OPT_STRIP2=0 if thick else 1))
    _same(big, other, NAMES, "the 8-wave image alone against the two-buffer image in front of it")
    if thick:
        assert ru == units and 0 < left < units, (ru, left, units)
        assert ru1 == 0 and t["layer_launches"] == t1["layer_launches"] + 1
    else:
        assert ru == 0 and ru1 == units, (ru, ru1, units)                           # no two-buffer launch on this handle
        assert t["layer_launches"] == t1["layer_launches"] - 1
    d = _against_oracle(big, _oracle(cref, entry), sc, "8-wave strip finisher")
    _order_and_tail(lambda s: _run(rtamd, m, s, opts)[0], sc, big, not thick, cus // (M - 1))
    _report(f"8-wave strip finisher{' thick' if thick else ''}", 52, bound, S, units, d)


# ---- the quad-block image ------------------------------------------------------------------------------------------------------
# nS, l_trunc, N (or N0 of the sub-problem), Nz, handle options, moments of the launch under test, scene keywords
Q4_FULL = [
    pytest.param(4, 11, 36, 4, dict(MOM_OPT_M0_REDUCTION=0), M, {}, id="KS9-N36"),
    pytest.param(4, 13, 40, 4, dict(MOM_OPT_M0_REDUCTION=0), M, {}, id="KS10-N40"),
    pytest.param(4, 3, 20, 4, dict(MOM_OPT_SMALL_N=0), M - 1, {}, id="KS5-N20"),
    pytest.param(4, 9, 32, 4, dict(MOM_OPT_SMALL_N=0), M - 1, {}, id="KS8-N32"),
    pytest.param(4, 13, 40, 4, dict(MOM_OPT_M0_REDUCTION=0), M, THICK, id="KS10-N40-thick"),
]


def _quad_block_case(rtamd, cref, cus, nS, lt, N, Nz, opts, moments, kw, elemental, first, what, sub_of=None):
    bound = WAVES_PER_CU * cus
    S = bound // moments + 1
    entry = _scene(rtamd, nS, lt, Nz, S, kw)
    m, sc = entry[:2]
    assert sc.N == (sub_of or N) and sc.M == M and sc.K == 2
    assert sub_of is None or 2 * (sc.N // sc.nStokes) == N          # the (I,Q) entries of every stream
    units = S * moments
    assert units > bound, (units, bound)        # the real grid is the runtime's occupancy x CUs <= this: that only adds rounds
    opts = dict(opts, MOM_OPT_ELEMENTAL=elemental)
    big, t, resumed = _run(rtamd, m, sc, opts)
    _, t0, _ = _run(rtamd, m, sc, dict(opts, MOM_OPT_LEAN=0))
    assert t["layer_launches"] > t0["layer_launches"], (t, t0)      # the quad-block launch in front of the finishing launch
    if not elemental:                                               # the two forms of the elemental layer: bit for bit
        _same(big, _run(rtamd, m, sc, dict(opts, MOM_OPT_ELEMENTAL=1))[0], NAMES, "MOM_OPT_ELEMENTAL = 0 against 1")
    d = _against_oracle(big, _oracle(cref, entry), sc, what)
    _order_and_tail(lambda s: _run(rtamd, m, s, opts)[0], sc, big, first, cus // moments)
    _report(f"{what}, MOM_OPT_ELEMENTAL = {elemental}", N, bound, S, units, d)
    return S, resumed


@gpu
@pytest.mark.parametrize("elemental", [1, 0])
@pytest.mark.parametrize("nS,lt,N,Nz,opts,moments,kw", Q4_FULL)
def test_quad_block_full_problem_later_units(rtamd, cref, cus, nS, lt, N, Nz, opts, moments, kw, elemental):
    """One wavefront per unit, and more units than the device holds wavefronts.  Edges 36 / 40 with every moment on the full
    problem, edges 20 / 32 on the general route; the table form of the elemental layer (c.tabE / c.tabZS, kept across units) and
    elemental_build; thick layers at edge 40 (the finishing launch meets finished and resumed units)."""
    _quad_block_case(rtamd, cref, cus, nS, lt, N, Nz, opts, moments, kw, elemental, (N, elemental, bool(kw)) == (36, 1, False),
                     "quad-block image, full problem")


@gpu
def test_quad_block_sources_only_later_units(rtamd, cref, cus):
    """Edge 40 with the default MOM_OPT_M0_REDUCTION: the full problem's launch starts behind moment 0 and takes the sources-only
    form (no composite R-+ and T++)."""
    _quad_block_case(rtamd, cref, cus, 4, 13, 40, 4, {}, M - 1, {}, 1, False, "quad-block image, sources-only form")


@gpu
@pytest.mark.parametrize("elemental", [1, 0])
def test_quad_block_sub_problem_later_units(rtamd, cref, cus, elemental):
    """N0 = 28 under N = 56, default options: the (I,Q) sub-problem's launch has one moment, S units.  The same run gives the
    two-buffer strip image at edge 56 twice as many (two layers: the oracle's time goes with S, and S is the point)."""
    S, (ru, left) = _quad_block_case(rtamd, cref, cus, 4, 21, 28, 2, {}, 1, {}, elemental, False,
                                     "quad-block image, (I,Q) sub-problem", sub_of=56)
    g = grid_constants()
    assert ru == S * (M - 1) and ru > 2 * g["strip2"] * cus and ru % (g["strip2"] * cus) != 0, (ru, left)


# ---- LDS-resident general kernels: one workgroup per point from S = 2048 on, looping over the moments ------------------------
@gpu
@pytest.mark.parametrize("nS,lt,N,Nz,opts", [
    (3, 9, 24, 4, dict(MOM_OPT_SMALL_N=0, MOM_OPT_LEAN=0, MOM_OPT_STRIP_PAD=0)),
    (3, 29, 54, 3, dict(MOM_OPT_STRIP_PAD=0))])
def test_general_kernels_one_workgroup_per_point(rtamd, cref, cus, nS, lt, N, Nz, opts):
    S = grid_constants()["point_rule"]
    entry = _scene(rtamd, nS, lt, Nz, S, {})
    m, sc = entry[:2]
    assert sc.N == N and sc.M == M and sc.S >= S
    units = S * (M - 1)
    assert units > S                                                # grid = S: every workgroup takes the moments 1 and 2 in turn
    big, t, _ = _run(rtamd, m, sc, opts)
    assert t["full_launches"] == 1 and t["reduced_launches"] == 1, t     # one layer launch per problem size (the sweep)
    if N == 24:
        assert t["layer_launches"] == 2, t                          # and no first-stage image in front of either
    d = _against_oracle(big, _oracle(cref, entry), sc, f"general image N = {N}")
    _order_and_tail(lambda s: _run(rtamd, m, s, opts)[0], sc, big, N == 24, cus // (M - 1))
    _report("general LDS image, one workgroup per point", N, S, S, units, d)


# ---- generic mode: grid = min(units, G) -------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nS,lt,N,Nz,opts", [(3, 9, 24, 4, dict(MOM_OPT_FORCE_GENERIC=1)), (4, 43, 100, 2, {}), (3, 37, 66, 2, {})])
def test_generic_mode_later_units(rtamd, cref, cus, nS, lt, N, Nz, opts):
    """k_layer on the per-workgroup scratch slabs (N = 24 forced, N = 100: panel GEMM) and the register-resident doubling (N = 66);
    k_surface has its own min(S, G) grid and loops as well."""
    G = grid_constants()["G"]
    S = points_for(G, M - 1)
    entry = _scene(rtamd, nS, lt, Nz, S, {})
    m, sc = entry[:2]
    assert sc.N == N and sc.M == M
    units = S * (M - 1)
    _rounds(units, G)
    assert 3 * S > G and S > G
    big, t, _ = _run(rtamd, m, sc, opts)
    assert t["full_launches"] == 1, t
    if opts:                                                        # without the option the wave-per-point kernel: one launch
        assert t["layer_launches"] > _run(rtamd, m, sc, {})[1]["layer_launches"]
    d = _against_oracle(big, _oracle(cref, entry), sc, f"generic mode N = {N}")
    _order_and_tail(lambda s: _run(rtamd, m, s, opts)[0], sc, big, N == 24, cus // (M - 1))
    _report("generic mode", N, G, S, units, d)


# ---- multi-target images (mom_rt_run_multisensor) --------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nS,lt,N,generic", [(3, 33, 60, False), (4, 31, 76, True)])
def test_multi_target_later_units(rtamd, cref, cus, nS, lt, N, generic):
    """Edge 60: the 8-wave multi-target image, one workgroup per CU, every moment on the full problem.  Edge 76: the generic k_layer
    with targets, k_interlayer and k_combine on min(units, G) workgroups."""
    g = grid_constants()
    bound = g["G"] if generic else g["strip8"] * cus
    S = points_for(bound, M)
    entry = _scene(rtamd, nS, lt, 4, S, {})
    m, sc = entry[:2]
    assert sc.N == N and sc.M == M
    units = S * M
    _rounds(units, bound)
    assert 3 * S > (bound if generic else 2.5 * cus)
    big = _run_ms(rtamd, m, sc, {})
    if entry[3] is None:
        uwr, dwr, info = cref.rt_run_multisensor(cref.pack_scene(helpers.oracle_scene(m)), LEVELS)
        assert info == 0
        entry[3] = (uwr, dwr)
    tol = helpers.stokes_rtol(sc.ndoubl)
    d = 0.0
    for ims, lev in enumerate(LEVELS):
        d = max(d, helpers.assert_stokes_close(big[0][ims], entry[3][0][ims], rtol=tol, what=f"uwJ level {lev}"),
                helpers.assert_stokes_close(big[1][ims], entry[3][1][ims], rtol=tol, what=f"dwJ level {lev}"))
    _order_and_tail(lambda s: _run_ms(rtamd, m, s, {}), sc, big, not generic, cus // M, names=("uwJ", "dwJ"))
    _report("multi-target", N, bound, S, units, d)


# ---- Float32: the same rule, grid = S from 2048 points on --------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nS,lt,N,opts", [(3, 33, 60, {}), (3, 9, 24, dict(MOM_OPT_SMALL_N=0))])
def test_float32_later_units(rtamd, cus, nS, lt, N, opts):
    """Comparisons 2 and 3 on a Float32 handle (strip image at edge 60, general image at 24); the accuracy against the Float32
    oracle stays with test_float32_* of test_gpu_rt_run.py."""
    S = grid_constants()["point_rule"]
    m, sc = _scene(rtamd, nS, lt, 4, S, {})[:2]
    assert sc.N == N and sc.M == M and S * (M - 1) > S
    big, t, _ = _run(rtamd, m, sc, opts, "Float32")
    assert t["layer_launches"] >= 2, t                             # the full problem and the (I,Q) sub-scene
    for k, name in enumerate(NAMES):
        assert np.all(np.isfinite(big[k])), name
    assert np.abs(big[0]).max() > 0
    _order_and_tail(lambda s: _run(rtamd, m, s, opts, "Float32")[0], sc, big, N == 60, cus // (M - 1))


# ---- operator level -----------------------------------------------------------------------------------------------------------------
@gpu
def test_batched_operators_later_units(rtamd, cref):
    """k_batch_inv / k_batched_mul above edge 64: min(batch, 1024) workgroups on global slabs, 76 of them with a second matrix.
    Against the oracle at the bars of test_batch_inv_and_mul, and bitwise against the run on the reversed batch."""
    n, batch = 65, 1100
    assert batch > grid_constants()["ops"] and batch % grid_constants()["ops"] != 0 and n > 64
    rng = np.random.default_rng(n)
    A = rng.normal(size=(batch, n, n)) + 3 * np.eye(n)
    B = rng.normal(size=(batch, n, n))
    rev = lambda flat: flat.reshape(batch, n * n)[::-1].reshape(-1)
    with rtamd.Handle(4, 1, 1, 1) as h:
        X = h.batch_inv(n, batch, mr.to_abi(A))
        Cg = h.batched_mul(n, batch, mr.to_abi(A), mr.to_abi(B))
        Xv = h.batch_inv(n, batch, mr.to_abi(A[::-1]))
        Cv = h.batched_mul(n, batch, mr.to_abi(A[::-1]), mr.to_abi(B[::-1]))
    Xr, info = cref.batch_inv(n, batch, mr.to_abi(A))
    assert info == 0
    helpers.assert_op_close(X, Xr, rtol=1e-11, what="batch_inv")
    helpers.assert_op_close(Cg, cref.batched_mul(n, batch, mr.to_abi(A), mr.to_abi(B)), rtol=1e-13, what="⊠")
    assert np.array_equal(rev(Xv), X), "batch_inv: reversed batch"
    assert np.array_equal(rev(Cv), Cg), "⊠: reversed batch"


@gpu
def test_interaction_operator_later_units(rtamd, cref):
    """k_op_interaction (interface code 3) at N = 72: generic mode, min(S, G) workgroups, S = 1100."""
    N, S, iface = 72, 1100, 3
    assert S > grid_constants()["G"] and S % grid_constants()["G"] != 0
    rng = np.random.default_rng(iface + N)
    mk = lambda s: rng.random((S, N, N)) * s / N
    added = [mk(0.6), mk(0.6), mk(0.9) + 0.3 * np.eye(N), mk(0.9) + 0.3 * np.eye(N), rng.random((S, N)), rng.random((S, N))]
    comp = [mk(0.6), mk(0.6), mk(0.9), mk(0.9), rng.random((S, N)), rng.random((S, N))]
    pol = rtamd.corert.Stokes_I()
    mu = np.linspace(0.1, 1.0, N)
    got = {}
    for flip in (False, True):
        sl = slice(None, None, -1) if flip else slice(None)
        with rtamd.Handle(N, 1, S, 1) as h:
            h.set_streams(mu, np.full(N, 1.0 / N), 1, mu[0], pol.I0, pol.D, True)
            for k in range(6):
                h.upload(k, mr.to_abi(added[k][sl]))
                h.upload(6 + k, mr.to_abi(comp[k][sl]))
            h.interaction(iface)
            got[flip] = [h.download(6 + k).reshape(S, -1) for k in range(6)]
    c_add = [mr.to_abi(x).copy() for x in added]
    c_comp = [mr.to_abi(x).copy() for x in comp]
    assert cref.interaction(N, S, iface, c_comp, c_add) == 0
    for k, nm in enumerate(["R_mp", "R_pm", "T_pp", "T_mm", "J0p", "J0m"]):
        helpers.assert_op_close(got[False][k], c_comp[k], rtol=1e-11, what=f"iface {iface} {nm}")
        assert np.array_equal(got[True][k][::-1], got[False][k]), f"{nm}: reversed batch"
