"""MOM_OPT_SOURCES_ONLY (csrc/mom_strip2.hpp k_layer_s2<.., SRC>, csrc/mom_q4.hpp k_layer_q4<.., SRC>): a sweep launch of mom_rt_run
whose moments no caller can observe -- the (I,Q) sub-problem's, a full-problem launch from moment 1 on -- leaves the composite
R-+ and T++ out of its layers and forms the two riding rows the sources take from them with the same matrix instructions in the
same order.  So every output is `np.array_equal` with the option on and off, the same launches run, the same units leave the
two-buffer image, a second run on the handle repeats the first, and nothing else -- mom_download, the multisensor run, the Dual
run -- notices the option."""
import numpy as np
import pytest

import helpers
from test_gpu_strip_row_blocks import CASES, NAMES, THICK, _equal, _kw_blocks, _scene

pytestmark = pytest.mark.gpu


def _run(rtamd, m, sc, on, zero_skip=7, opts=()):
    """Two runs on a fresh handle; rt_run raises on a non-zero info, so a returned result is info == 0 on both."""
    L = rtamd._lib
    with rtamd.corert.make_handle(m) as h:
        h.set_option(L.MOM_OPT_SOURCES_ONLY, on)
        h.set_option(L.MOM_OPT_ZERO_SKIP, zero_skip)
        for k, v in opts:
            h.set_option(k, v)
        R, T = rtamd.corert.run_scene(h, sc)
        out = (R, T) + tuple(h.get_hdr())
        launches, resumed = h.timers()["layer_launches"], h.strip2_resumed()
        R2, T2 = rtamd.corert.run_scene(h, sc)
        again = (R2, T2) + tuple(h.get_hdr())
        for k, what in enumerate(NAMES):
            assert np.array_equal(out[k], again[k]), f"second run on the same handle, MOM_OPT_SOURCES_ONLY = {on}: {what}"
        assert h.strip2_resumed() == resumed and h.timers()["layer_launches"] == launches
    for k, what in enumerate(NAMES):
        assert np.all(np.isfinite(out[k])), what
    return out, launches, resumed


def _on_off(rtamd, m, sc, what, **kw):
    (a, la, ra), (b, lb, rb) = _run(rtamd, m, sc, 1, **kw), _run(rtamd, m, sc, 0, **kw)
    _equal(a, b, f"MOM_OPT_SOURCES_ONLY = 1 against 0, {what}")
    assert la == lb and ra == rb, (what, la, lb, ra, rb)
    return a, la, ra


@pytest.mark.parametrize("nS,lt,N,kw,skip,on,off", CASES)
def test_sources_only_headline_scenes(rtamd, nS, lt, N, kw, skip, on, off):
    """The nine scenes of the row-block file (N = 52, 56, 60; every KS - KW; KW = KS; the dead-block-only masks): the full problem's
    launch (m_first = 1, two-buffer image, k-step variant and row-block rule of the mask) and the sub-problem's (quad-block image)
    both take the sources-only form."""
    m, sc = _scene(rtamd, nS, lt, N, 4, 24, kw)
    KS, nbw = _kw_blocks(m)
    assert KS == N // 4 and KS - nbw == skip, (KS, nbw)
    for mask in sorted({on, off}):
        a, la, ra = _on_off(rtamd, m, sc, f"MOM_OPT_ZERO_SKIP = {mask}", zero_skip=mask)
        assert ra[0] > 0, ra                                          # the two-buffer launch ran


def test_sources_only_headline_against_oracle(rtamd, cref):
    m, sc = _scene(rtamd, 3, 33, 60, 4, 24, {})
    a, la, ra = _run(rtamd, m, sc, 1)
    Rr, Tr, Hr, upr, dwr, info = cref.rt_run_full(cref.pack_scene(helpers.oracle_scene(m)))
    assert info == 0
    tol = helpers.stokes_rtol(sc.ndoubl)
    helpers.assert_stokes_close(a[0], Rr, rtol=tol, what="R")
    helpers.assert_stokes_close(a[1], Tr, rtol=tol, what="T")
    helpers.assert_stokes_close(a[2], Hr, rtol=tol, what="hdr")


# The quad-block image's problems: (nS, l_trunc, N, MOM_OPT_SMALL_N, scene keywords).  The scenes of test_gpu_q4_zero_skip.py reach
# KS = 10 (NBW 9, 8, 6), 9 (NBW 5), 8 (NBW 6), 5 (NBW 4, 3); those of test_gpu_rt_run.py's small edges the sub-problems N0 = 24, 28
# (KS = 6, 7: NBW 4, 5) and the full problems of edge 20 .. 32 (m_first = 1 on the image: KS = 5 .. 8 with NBW 3, 4, 5, 6); the
# one-view N = 36 scene KS = 9 with NBW 7; the last eight the rest.  Each runs with MOM_OPT_ZERO_SKIP = 7 (the variant its zero-weight
# streams select) and 0 (NBW = NB, the kernel without the rule): every NBW = KS, KS - 1, KS - 2, KS - 4 of every KS = 5 .. 10.
ONE_VIEW = dict(vza=(30.0,), vaz=(0.0,))
FOUR_VIEWS = dict(vza=(0.0, 30.0, 60.0, 75.0), vaz=(0.0, 45.0, 120.0, 200.0))
Q4_SCENES = [
    pytest.param(3, 33, 60, 1, {}, id="N0-40-nbw9"),
    pytest.param(4, 23, 60, 1, {}, id="N0-32-nbw6"),
    pytest.param(4, 11, 40, 1, dict(sza=50.0), id="N40-nbw6-N0-20-nbw3"),
    pytest.param(4, 9, 36, 1, dict(vza=(0.0, 30.0, 70.0)), id="N36-nbw5-N0-20"),
    pytest.param(4, 13, 40, 1, dict(sza=60.0, vza=(0.0, 30.0, 70.0)), id="N40-nbw7-as-8"),
    pytest.param(4, 15, 40, 1, ONE_VIEW, id="N40-nbw8-N0-20-nbw4"),
    pytest.param(4, 13, 36, 1, ONE_VIEW, id="N36-nbw7"),
    pytest.param(3, 33, 60, 1, THICK, id="N0-40-thick"),
    pytest.param(4, 17, 48, 1, {}, id="N0-24"),
    pytest.param(4, 21, 56, 1, {}, id="N0-28"),
    pytest.param(4, 3, 20, 0, {}, id="N20-full"),
    pytest.param(4, 5, 24, 0, {}, id="N24-full"),
    pytest.param(4, 7, 28, 0, {}, id="N28-full"),
    pytest.param(4, 9, 32, 0, {}, id="N32-full"),
    # the variants the scenes above leave out: (KS, NBW) = (9, 8), (8, 7), (7, 6), (6, 5) as sub-problems of one-view scenes,
    # (8, 4), (7, 3), (6, 2) as full problems with four view angles, (5, 1) as the sub-problem of a two-node scene with seven
    pytest.param(3, 29, 51, 1, ONE_VIEW, id="N0-34-as-36-nbw8"),
    pytest.param(4, 25, 60, 1, ONE_VIEW, id="N0-30-as-32-nbw7"),
    pytest.param(4, 21, 52, 1, ONE_VIEW, id="N0-26-as-28-nbw6"),
    pytest.param(4, 19, 48, 1, ONE_VIEW, id="N0-24-nbw5"),
    pytest.param(4, 7, 32, 0, FOUR_VIEWS, id="N32-nbw4"),
    pytest.param(4, 5, 28, 0, FOUR_VIEWS, id="N28-nbw3"),
    pytest.param(4, 3, 24, 0, FOUR_VIEWS, id="N24-nbw2"),
    pytest.param(4, 3, 40, 1, dict(vza=(0.0, 10.0, 20.0, 30.0, 40.0, 50.0, 70.0), vaz=(0.0,) * 7), id="N40-nbw2-N0-20-nbw1"),
]


@pytest.mark.parametrize("nS,lt,N,small,kw", Q4_SCENES)
def test_sources_only_quad_block(rtamd, nS, lt, N, small, kw):
    m = rtamd.scenes.make_scene(nS, lt, 6, 24, seed=11 * nS + lt, **kw)
    sc = rtamd.prepare_scene(m)
    assert sc.N == N
    small_n = ((rtamd._lib.MOM_OPT_SMALL_N, small),)
    launches = {}
    for mask in (7, 0):
        a, launches[mask], ra = _on_off(rtamd, m, sc, f"quad-block, MOM_OPT_ZERO_SKIP = {mask}", zero_skip=mask, opts=small_n)
    with rtamd.corert.make_handle(m) as h:                            # the image ran: MOM_OPT_LEAN = 0 takes its launches away
        h.set_option(rtamd._lib.MOM_OPT_SMALL_N, small)
        h.set_option(rtamd._lib.MOM_OPT_LEAN, 0)
        rtamd.corert.run_scene(h, sc)
        without = h.timers()["layer_launches"]
    assert launches[7] == launches[0] and launches[7] > without, (launches, without)


@pytest.mark.parametrize("nS,lt,N", [(3, 33, 60), (4, 19, 52)])
def test_sources_only_thick_layers_resume(rtamd, nS, lt, N):
    """Thick layers: series beyond 12 terms, units leave both images in mid-sweep and the finishers carry them on over the
    meaningless R-+ / T++.  Equal outputs, and the same units leave."""
    m, sc = _scene(rtamd, nS, lt, N, 8, 32, THICK)
    a, la, ra = _on_off(rtamd, m, sc, "thick layers")
    assert 0 < ra[1] < ra[0], ra


def test_sources_only_brdf_surface(rtamd):
    """RPV surface: k_surface runs per moment on the state the sources-only launches left."""
    m, sc = _scene(rtamd, 4, 21, 56, 4, 24, {}, brdf="rpv")
    a, la, ra = _on_off(rtamd, m, sc, "RPV surface")
    assert ra[0] > 0


def test_sources_only_first_layer_without_doubling(rtamd):
    m, sc = _scene(rtamd, 3, 33, 60, 4, 24, {}, thin_first=True)
    assert sc.ndoubl[0] == 0 and np.max(sc.ndoubl[1:]) > 0 and np.all(np.asarray(sc.iface)[1:] == 3), (sc.ndoubl, sc.iface)
    a, la, ra = _on_off(rtamd, m, sc, "first layer ndoubl = 0")
    assert ra[0] > 0


def test_sources_only_download_contract(rtamd):
    """mom_download of the composite R-+ / T++: without the m = 0 reduction the one launch carries moment 0 and keeps all four
    operators -- equal with the option on and off; with the reduction MOM_ESTATE either way."""
    L = rtamd._lib
    m, sc = _scene(rtamd, 3, 33, 60, 4, 24, {})
    got = {}
    for on in (1, 0):
        with rtamd.corert.make_handle(m) as h:
            h.set_option(L.MOM_OPT_SOURCES_ONLY, on)
            h.set_option(L.MOM_OPT_M0_REDUCTION, 0)
            R, T = rtamd.corert.run_scene(h, sc)
            assert h.strip2_resumed()[0] > 0
            got[on] = (R, T, h.download(L.COMP["R_mp"]), h.download(L.COMP["T_pp"]))
        with rtamd.corert.make_handle(m) as h:
            h.set_option(L.MOM_OPT_SOURCES_ONLY, on)
            rtamd.corert.run_scene(h, sc)
            for which in ("R_mp", "T_pp"):
                with pytest.raises(rtamd.MomError) as e:
                    h.download(L.COMP[which])
                assert e.value.code == L.MOM_ESTATE and "sub-problem" in str(e.value)
    for k, what in enumerate(("R", "T", "download(R_mp)", "download(T_pp)")):
        assert np.array_equal(got[1][k], got[0][k]), what
    assert np.abs(got[1][2]).max() > 0 and np.abs(got[1][3]).max() > 0


def test_sources_only_leaves_multisensor_and_dual_alone(rtamd):
    """mom_rt_run_multisensor (k_combine, k_interlayer read all four operators) and mom_rt_run_dual never take the form."""
    L = rtamd._lib
    m, sc = _scene(rtamd, 3, 33, 60, 4, 6, {})
    levels = [3, 0, 2]
    ms = {}
    for on in (1, 0):
        with rtamd.corert.make_handle(m) as h:
            h.set_option(L.MOM_OPT_SOURCES_ONLY, on)
            rtamd.corert.scene_set(h, sc)
            uw, dw = h.rt_run_multisensor(levels)
            R, T = rtamd.corert.run_scene(h, sc)                      # the plain column on the same handle afterwards
            ms[on] = (np.asarray(uw), np.asarray(dw), R, T)
    for k, what in enumerate(("uwJ", "dwJ", "R after", "T after")):
        assert np.array_equal(ms[1][k], ms[0][k]), f"multisensor: {what}"
    md = rtamd.scenes.make_scene(3, 9, 4, 6, seed=8)
    scd = rtamd.prepare_scene(md)
    part = [rtamd.ScenePartial(dτ=0.1 * np.asarray(md.τ_rayl))]
    du = {}
    for on in (1, 0):
        with rtamd.corert.make_handle(md) as h:
            h.set_option(L.MOM_OPT_SOURCES_ONLY, on)
            rtamd.corert.scene_set(h, scd)
            rtamd.corert.scene_set_partials(h, scd, part)
            h.rt_run_dual()
            du[on] = tuple(h.get_RT()) + tuple(h.get_RT_partials())
    for k, what in enumerate(("R", "T", "dR", "dT")):
        assert np.array_equal(du[1][k], du[0][k]), f"dual: {what}"
    assert np.abs(du[1][2]).max() > 0
