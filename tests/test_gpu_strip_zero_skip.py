"""MOM_OPT_ZERO_SKIP bit 1 (csrc/mom_strip.hpp strip_mul<KS, KW>): the two-buffer strip image leaves out the k-steps of its strip
products that lie wholly in the zero-weight streams at the end of the stream set, and adds the one non-zero term of each such
column -- its diagonal entry -- by a plain fma.  The k-steps left out add exact zeros and the fma is the fused term the matrix
instruction would have added, so every output equals the run with the bit off (`==`: the sign of a zero may differ), and the image
still agrees with the C oracle."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import helpers

ROOT = Path(__file__).resolve().parent.parent
THICK = dict(aerosol_total=2.0, aerosol_p0=600.0, aerosol_σp=200.0, absorption=False)
ONE_VIEW = dict(vza=(30.0,), vaz=(0.0,))
NAMES = ("R", "T", "hdr", "bhr_uw", "bhr_dw")


def _run(rtamd, m, sc, mask):
    with rtamd.corert.make_handle(m) as h:
        h.set_option(rtamd._lib.MOM_OPT_ZERO_SKIP, mask)
        R, T = rtamd.corert.run_scene(h, sc)
        out = (R, T) + tuple(h.get_hdr())
        launches = h.timers()["layer_launches"]
        R2, T2 = rtamd.corert.run_scene(h, sc)                       # the resume table is reused: same answer again
        again = (R2, T2) + tuple(h.get_hdr())
        for k, what in enumerate(NAMES):
            assert np.array_equal(out[k], again[k]), f"second run on the same handle: {what}"
    return out, launches


# nS, l_trunc, N, scene keywords, BRDF; N_w weighted entries of the full problem -> KW = ceil(N_w / 4) of KS = N / 4 k-steps kept
@pytest.mark.gpu
@pytest.mark.parametrize("nS,lt,N,kw,brdf", [
    (3, 33, 60, {}, None),            # IQU, 20 streams: N_w = 51, KW = 13 of 15 -- the headline's; the boundary lies inside a k-step of strip 3
    (4, 23, 60, {}, None),            # IQUV, 15 streams: N_w = 48, KW = 12: 12 columns fixed up, all in strip 3
    (4, 21, 56, {}, None),            # IQUV, 14 streams: N_w = 44, KW = 11 of 14: fix-up in strips 2 and 3
    (4, 19, 52, {}, None),            # IQUV, 13 streams: N_w = 40, KW = 10 of 13: fix-up in strips 2 and 3, a layer with ndoubl = 0
    (3, 35, 60, ONE_VIEW, None),      # IQU, one view angle: N_w = 54, KW = 14: one k-step left out
    (1, 113, 60, {}, None),           # scalar, 60 streams: N_w = 57, KW = 15: nothing to leave out, the KW = KS kernel
    (3, 33, 60, THICK, None),         # thick layers: units leave through the resume table to the 8-wave image in mid-sweep
    (4, 19, 52, THICK, None),
    (4, 21, 56, {}, "rpv")])          # a non-Lambertian surface behind the sweep
def test_strip_zero_skip_equal_and_oracle(rtamd, cref, nS, lt, N, kw, brdf):
    m = rtamd.scenes.make_scene(nS, lt, 6, 24, seed=13 * nS + lt, **kw)
    if brdf:
        m.params.brdf = rtamd.corert.rpvSurfaceScalar(0.1, 0.8, 0.7, -0.1)
    sc = rtamd.prepare_scene(m)
    assert sc.N == N
    (on, n_on), (off, n_off) = _run(rtamd, m, sc, 3), _run(rtamd, m, sc, 1)
    for k, what in enumerate(NAMES):
        assert np.array_equal(on[k], off[k]), f"MOM_OPT_ZERO_SKIP = 3 against 1: {what}"
    assert n_on == n_off                                             # the two-buffer launch ran on both sides
    Rr, Tr, Hr, upr, dwr, info = cref.rt_run_full(cref.pack_scene(helpers.oracle_scene(m)))
    assert info == 0
    tol = helpers.stokes_rtol(sc.ndoubl)
    helpers.assert_stokes_close(on[0], Rr, rtol=tol, what="R")
    helpers.assert_stokes_close(on[1], Tr, rtol=tol, what="T")
    helpers.assert_stokes_close(on[2], Hr, rtol=tol, what="hdr")


def test_strip2_variant_host(tmp_path):
    """Host only: the instantiation a launch of the two-buffer image (KS = 13 .. 15, seven counts each) and of the quad-block image
    (KS = 5 .. 10: the counts 0, KS + 1 and KS .. KS - 5 down to 1) takes for its MomLaunchForm (mom_image_variants.hpp) -- the
    largest instantiated skip that is still exact, none for nbw = 0 or out of range (tools/image_variant_check.hip)."""
    exe = tmp_path / "image_variant_check"
    csrc = ROOT / "radiativetransfer.jl_amd" / "csrc"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "--offload-arch=gfx950", f"-I{ROOT / 'include'}", f"-I{csrc}",
                           str(ROOT / "tools" / "image_variant_check.hip"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    assert out.stdout.count(" ok") == 3 * 7 + (6 * 8 - 1) and "WRONG" not in out.stdout, out.stdout   # (KS = 5 has no count KS - 5)
