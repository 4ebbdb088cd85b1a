"""MOM_OPT_ELEMENTAL (csrc/mom_elemental_tab.hpp; k_layer_s2<.., EL> of csrc/mom_strip2.hpp, k_layer_q4<.., EL> of csrc/mom_q4.hpp):
the two-buffer strip image and the quad-block image build the elemental layer from stream-pair tables computed once per scene, in
branch-free batches.  The form evaluates the expressions of elemental_build on the same operands in the same association, so with
the option on and off every output is `np.array_equal`, the same launches run, the same units leave the two-buffer image, and a
second run on the handle repeats the first.  Where the form does not apply (a scalar problem has no tables) or the path never
takes it (Float32, multisensor, Dual) the option changes nothing either."""
import numpy as np
import pytest

import helpers
from test_gpu_strip_row_blocks import NAMES, ONE_VIEW, THICK, _equal, _scene

pytestmark = pytest.mark.gpu


def _run(rtamd, m, sc, on, opts=()):
    """Two runs on a fresh handle; rt_run raises on a non-zero info, so a returned result is info == 0 on both."""
    L = rtamd._lib
    with rtamd.corert.make_handle(m) as h:
        h.set_option(L.MOM_OPT_ELEMENTAL, on)
        for k, v in opts:
            h.set_option(k, v)
        R, T = rtamd.corert.run_scene(h, sc)
        out = (R, T) + tuple(h.get_hdr())
        launches, resumed = h.timers()["layer_launches"], h.strip2_resumed()
        R2, T2 = rtamd.corert.run_scene(h, sc)
        again = (R2, T2) + tuple(h.get_hdr())
        for k, what in enumerate(NAMES):
            assert np.array_equal(out[k], again[k]), f"second run on the same handle, MOM_OPT_ELEMENTAL = {on}: {what}"
        assert h.strip2_resumed() == resumed and h.timers()["layer_launches"] == launches
    for k, what in enumerate(NAMES):
        assert np.all(np.isfinite(out[k])), what
    return out, launches, resumed


def _on_off(rtamd, m, sc, what, opts=()):
    (a, la, ra), (b, lb, rb) = _run(rtamd, m, sc, 1, opts), _run(rtamd, m, sc, 0, opts)
    _equal(a, b, f"MOM_OPT_ELEMENTAL = 1 against 0, {what}")
    assert la == lb and ra == rb, (what, la, lb, ra, rb)
    return a, la, ra


# nS, l_trunc, N, scene keywords.  Every scene has two phase-matrix bases (Rayleigh and one aerosol type) and regular streams
HEADLINE = [
    pytest.param(4, 19, 52, {}, id="N52-IQUV"),
    pytest.param(4, 21, 56, {}, id="N56-IQUV"),
    pytest.param(4, 23, 60, {}, id="N60-IQUV"),
    pytest.param(3, 33, 60, {}, id="N60-IQU"),                      # the headline's layout
    # sza = vza[1]: the Sun merges with the second view angle, stream 14 of 15 -- the source pass reads the tables at (iq, sq) off
    # the corner, and the sun-block columns are not the last ones
    pytest.param(4, 23, 60, dict(sza=30.0), id="N60-IQUV-sun-not-last"),
]


@pytest.mark.parametrize("nS,lt,N,kw", HEADLINE)
def test_elemental_form_headline_scenes(rtamd, nS, lt, N, kw):
    """Full problem on the two-buffer image (moments 1 ..), (I,Q) sub-problem on the quad-block image: both take the table form."""
    m, sc = _scene(rtamd, nS, lt, N, 4, 24, kw)
    assert sc.K == 2
    if kw:
        qp = m.quad_points
        assert qp.iμ0 < qp.Nquad, (qp.iμ0, qp.Nquad)
    a, la, ra = _on_off(rtamd, m, sc, "headline scene")
    assert ra[0] > 0, ra                                             # the two-buffer launch ran


def test_elemental_form_scalar_takes_the_other_form(rtamd):
    """N = 60 scalar: one component per stream, 3 x 60^2 table entries do not fit a buffer -- no tables, elemental_build as before."""
    m, sc = _scene(rtamd, 1, 115, 60, 4, 24, ONE_VIEW)
    a, la, ra = _on_off(rtamd, m, sc, "scalar N = 60")
    assert ra[0] > 0


def test_elemental_form_against_oracle(rtamd, cref):
    m, sc = _scene(rtamd, 3, 33, 60, 4, 24, {})
    a, la, ra = _run(rtamd, m, sc, 1)
    Rr, Tr, Hr, upr, dwr, info = cref.rt_run_full(cref.pack_scene(helpers.oracle_scene(m)))
    assert info == 0
    tol = helpers.stokes_rtol(sc.ndoubl)
    helpers.assert_stokes_close(a[0], Rr, rtol=tol, what="R")
    helpers.assert_stokes_close(a[1], Tr, rtol=tol, what="T")
    helpers.assert_stokes_close(a[2], Hr, rtol=tol, what="hdr")


def test_elemental_form_thick_layers_resume(rtamd):
    """Series beyond 12 terms: units leave both images in mid-sweep, the 8-wave image (elemental_build) redoes the layer they left
    at.  Equal outputs, and the same units leave."""
    m, sc = _scene(rtamd, 3, 33, 60, 8, 32, THICK)
    a, la, ra = _on_off(rtamd, m, sc, "thick layers")
    assert 0 < ra[1] < ra[0], ra


def test_elemental_form_brdf_surface(rtamd):
    m, sc = _scene(rtamd, 4, 21, 56, 4, 24, {}, brdf="rpv")
    a, la, ra = _on_off(rtamd, m, sc, "RPV surface")
    assert ra[0] > 0


def test_elemental_form_first_layer_without_doubling(rtamd):
    """ndoubl = 0: the multiplier of r-+ is 1.0 instead of sg_i, and the elemental layer goes to the composite state as it is."""
    m, sc = _scene(rtamd, 3, 33, 60, 4, 24, {}, thin_first=True)
    assert sc.ndoubl[0] == 0 and np.max(sc.ndoubl[1:]) > 0 and np.all(np.asarray(sc.iface)[1:] == 3), (sc.ndoubl, sc.iface)
    a, la, ra = _on_off(rtamd, m, sc, "first layer ndoubl = 0")
    assert ra[0] > 0


@pytest.mark.parametrize("option,value", [("MOM_OPT_M0_REDUCTION", 0), ("MOM_OPT_SOURCES_ONLY", 0)])
def test_elemental_form_with_other_options(rtamd, option, value):
    """MOM_OPT_M0_REDUCTION = 0: moment 0 (weights wt / 2) passes through the two-buffer image.  MOM_OPT_SOURCES_ONLY = 0: the
    instantiations of the two images with all four composite operators."""
    m, sc = _scene(rtamd, 3, 33, 60, 4, 24, {})
    a, la, ra = _on_off(rtamd, m, sc, f"{option} = {value}", opts=((getattr(rtamd._lib, option), value),))
    assert ra[0] > 0


# one (I,Q) sub-problem or full problem per edge of the quad-block image, KS = 5 .. 10: (nS, l_trunc, N, scene keywords)
Q4_SCENES = [
    pytest.param(4, 11, 40, dict(sza=50.0), id="KS10-N40-KS5-N0-20"),
    pytest.param(4, 17, 48, {}, id="KS6-N0-24"),
    pytest.param(4, 21, 56, {}, id="KS7-N0-28"),
    pytest.param(4, 23, 60, {}, id="KS8-N0-32"),
    pytest.param(3, 29, 51, ONE_VIEW, id="KS9-N0-34-as-36"),
    pytest.param(3, 33, 60, {}, id="KS10-N0-40"),
]


@pytest.mark.parametrize("nS,lt,N,kw", Q4_SCENES)
def test_elemental_form_quad_block(rtamd, nS, lt, N, kw):
    m = rtamd.scenes.make_scene(nS, lt, 6, 24, seed=11 * nS + lt, **kw)
    sc = rtamd.prepare_scene(m)
    assert sc.N == N and sc.K == 2
    a, launches, ra = _on_off(rtamd, m, sc, "quad-block image")
    with rtamd.corert.make_handle(m) as h:                            # the image ran: MOM_OPT_LEAN = 0 takes its launches away
        h.set_option(rtamd._lib.MOM_OPT_LEAN, 0)
        rtamd.corert.run_scene(h, sc)
        without = h.timers()["layer_launches"]
    assert launches > without, (launches, without)


def test_elemental_form_leaves_float32_multisensor_and_dual_alone(rtamd):
    L = rtamd._lib
    m, sc = _scene(rtamd, 3, 33, 60, 4, 6, {})
    f32 = {}
    for on in (1, 0):
        with rtamd.corert.make_handle(m, float_type="Float32") as h:
            h.set_option(L.MOM_OPT_ELEMENTAL, on)
            f32[on] = rtamd.corert.run_scene(h, sc)
    for k, what in enumerate(("R", "T")):
        assert np.array_equal(f32[1][k], f32[0][k]), f"Float32: {what}"
    levels = [3, 0, 2]
    ms = {}
    for on in (1, 0):
        with rtamd.corert.make_handle(m) as h:
            h.set_option(L.MOM_OPT_ELEMENTAL, on)
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
            h.set_option(L.MOM_OPT_ELEMENTAL, on)
            rtamd.corert.scene_set(h, scd)
            rtamd.corert.scene_set_partials(h, scd, part)
            h.rt_run_dual()
            du[on] = tuple(h.get_RT()) + tuple(h.get_RT_partials())
    for k, what in enumerate(("R", "T", "dR", "dT")):
        assert np.array_equal(du[1][k], du[0][k]), f"dual: {what}"
    assert np.abs(du[1][2]).max() > 0
