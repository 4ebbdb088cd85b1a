"""MOM_OPT_ZERO_SKIP bit 2 (csrc/mom_strip.hpp strip_mul<KS, KW, RB>): in the two-buffer strip image a 16-row tile of a strip product
whose blocks of four rows are only partly live -- rows of weighted entries and the riding source rows are, rows of zero-weight
streams and rows past the riding rows are not -- runs one v_mfma_f64_4x4x4_4b per live block instead of the v_mfma_f64_16x16x4.
The small instruction rounds like the large one (tools/mfma_f64_forms_check.hip) and the rows left out got exact zeros or are read
by nobody, so every output equals the run with the bit off (`==`: the sign of a zero may differ), the units that leave the image
through the resume table are the same, the 8-wave image gives the same numbers and the C oracle still agrees."""
import numpy as np
import pytest

import helpers

THICK = dict(aerosol_total=2.0, aerosol_p0=600.0, aerosol_σp=200.0, absorption=False)
ONE_VIEW = dict(vza=(30.0,), vaz=(0.0,))
NAMES = ("R", "T", "hdr", "bhr_uw", "bhr_dw")


def _run(rtamd, m, sc, mask, strip2=1):
    """Two runs on a fresh handle; rt_run raises on a non-zero info, so a returned result is info == 0 on both."""
    with rtamd.corert.make_handle(m) as h:
        h.set_option(rtamd._lib.MOM_OPT_ZERO_SKIP, mask)
        h.set_option(rtamd._lib.MOM_OPT_STRIP2, strip2)
        R, T = rtamd.corert.run_scene(h, sc)
        out = (R, T) + tuple(h.get_hdr())
        launches, resumed = h.timers()["layer_launches"], h.strip2_resumed()
        R2, T2 = rtamd.corert.run_scene(h, sc)
        again = (R2, T2) + tuple(h.get_hdr())
        for k, what in enumerate(NAMES):
            assert np.array_equal(out[k], again[k]), f"second run on the same handle, mask {mask}: {what}"
        assert h.strip2_resumed() == resumed
    return out, launches, resumed


def _scene(rtamd, nS, lt, N, Nz, S, kw, brdf=None, thin_first=False):
    m = rtamd.scenes.make_scene(nS, lt, Nz, S, seed=17 * nS + lt, **kw)
    if brdf:
        m.params.brdf = rtamd.corert.rpvSurfaceScalar(0.1, 0.8, 0.7, -0.1)
    if thin_first:
        m.τ_rayl[:, 0] *= 1e-4
        m.τ_abs[:, 0] *= 1e-4
    sc = rtamd.prepare_scene(m)
    assert sc.N == N
    return m, sc


def _kw_blocks(m):
    """(KS, blocks of four entries that hold a weighted one) of the full problem's stream set"""
    wt = np.asarray(m.quad_points.wt_μN)                             # one weight per entry of the operator edge
    return len(wt) // 4, -(-(int(np.nonzero(wt != 0.0)[0][-1]) + 1) // 4)


def _equal(a, b, what):
    for k, name in enumerate(NAMES):
        assert np.array_equal(a[k], b[k]), f"{what}: {name}"


# nS, l_trunc, N, scene keywords, KS - KW (k-steps the zero-weight streams leave out), mask with the rule / without it
CASES = [
    pytest.param(3, 33, 60, {}, 2, 7, 3, id="N60-IQU-3views"),        # the headline's: tile 3 = weighted | passenger | passenger | riding
    pytest.param(3, 35, 60, ONE_VIEW, 1, 7, 3, id="N60-IQU-1view"),   # tile 3 = weighted | weighted | passenger | riding
    pytest.param(4, 23, 60, {}, 3, 7, 3, id="N60-IQUV"),              # tile 3 = three passengers | riding: one small instruction
    pytest.param(4, 21, 56, {}, 3, 7, 3, id="N56-IQUV"),              # KW = 11: tile 2 has a passenger, tile 3 = 2 passengers | riding | dead
    pytest.param(4, 19, 52, {}, 3, 7, 3, id="N52-IQUV"),              # KW = 10: tile 2 = 2 weighted | 2 passengers, tile 3 = passenger | riding | 2 dead
    pytest.param(1, 107, 56, ONE_VIEW, 0, 7, 3, id="N56-scalar"),     # 54 + 2 streams: no zero-weight block, KW = KS, only the dead block drops
    pytest.param(1, 99, 52, ONE_VIEW, 0, 7, 3, id="N52-scalar"),      # 50 + 2 streams: KW = KS, two dead blocks
    pytest.param(4, 21, 56, {}, 3, 5, 1, id="N56-dead-only"),         # bit 1 off: KW = KS on a scene with zero-weight blocks
    pytest.param(4, 19, 52, {}, 3, 5, 1, id="N52-dead-only"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("nS,lt,N,kw,skip,on,off", CASES)
def test_row_blocks_equal_and_oracle(rtamd, cref, nS, lt, N, kw, skip, on, off):
    m, sc = _scene(rtamd, nS, lt, N, 4, 24, kw)
    KS, nbw = _kw_blocks(m)
    assert KS == N // 4 and KS - nbw == skip, (KS, nbw)
    (a, la, ra), (b, lb, rb) = _run(rtamd, m, sc, on), _run(rtamd, m, sc, off)
    _equal(a, b, f"MOM_OPT_ZERO_SKIP = {on} against {off}")
    assert ra == rb and ra[0] > 0, (ra, rb)                          # the two-buffer launch ran, the same units left it
    assert la == lb
    Rr, Tr, Hr, upr, dwr, info = cref.rt_run_full(cref.pack_scene(helpers.oracle_scene(m)))
    assert info == 0
    tol = helpers.stokes_rtol(sc.ndoubl)
    helpers.assert_stokes_close(a[0], Rr, rtol=tol, what="R")
    helpers.assert_stokes_close(a[1], Tr, rtol=tol, what="T")
    helpers.assert_stokes_close(a[2], Hr, rtol=tol, what="hdr")


@pytest.mark.gpu
def test_row_blocks_against_8wave_image(rtamd):
    """The headline's shape: the rule on, against the 8-wave image alone (no two-buffer launch)."""
    m, sc = _scene(rtamd, 3, 33, 60, 4, 24, {})
    (a, la, ra), (b, lb, rb) = _run(rtamd, m, sc, 7), _run(rtamd, m, sc, 7, strip2=0)
    _equal(a, b, "two-buffer image with the row-block rule against the 8-wave image")
    assert ra[0] > 0 and rb[0] == 0 and la == lb + 1                 # the two-buffer launch in front of the 8-wave one


@pytest.mark.gpu
@pytest.mark.parametrize("nS,lt,N", [(3, 33, 60), (4, 19, 52)])
def test_row_blocks_resume(rtamd, nS, lt, N):
    """Thick layers: series beyond 12 terms, units leave the image in mid-sweep and the 8-wave image finishes them -- the Frobenius
    sums that decide it are taken over rows < N only, so the same units leave with the rule on."""
    m, sc = _scene(rtamd, nS, lt, N, 8, 32, THICK)
    (a, la, ra), (b, lb, rb) = _run(rtamd, m, sc, 7), _run(rtamd, m, sc, 3)
    _equal(a, b, "MOM_OPT_ZERO_SKIP = 7 against 3, thick layers")
    assert ra == rb and 0 < ra[1] < ra[0], (ra, rb)
    assert la == lb


@pytest.mark.gpu
def test_row_blocks_brdf_surface(rtamd):
    m, sc = _scene(rtamd, 4, 21, 56, 4, 24, {}, brdf="rpv")
    (a, la, ra), (b, lb, rb) = _run(rtamd, m, sc, 7), _run(rtamd, m, sc, 3)
    _equal(a, b, "MOM_OPT_ZERO_SKIP = 7 against 3, RPV surface")
    assert ra == rb and ra[0] > 0 and la == lb


@pytest.mark.gpu
def test_row_blocks_first_layer_without_doubling(rtamd):
    """A first layer with ndoubl = 0: the elemental layer goes to the composite state as it is, no product before the second layer."""
    m, sc = _scene(rtamd, 3, 33, 60, 4, 24, {}, thin_first=True)
    assert sc.ndoubl[0] == 0 and np.max(sc.ndoubl[1:]) > 0 and np.all(np.asarray(sc.iface)[1:] == 3), (sc.ndoubl, sc.iface)
    (a, la, ra), (b, lb, rb) = _run(rtamd, m, sc, 7), _run(rtamd, m, sc, 3)
    _equal(a, b, "MOM_OPT_ZERO_SKIP = 7 against 3, first layer ndoubl = 0")
    assert ra == rb and ra[0] > 0 and la == lb
