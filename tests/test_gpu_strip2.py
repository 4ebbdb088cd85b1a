"""The two-buffer 4-wave strip image (MOM_OPT_STRIP2, csrc/mom_strip2.hpp): operator edges 52, 56, 60 run on it first, two
workgroups per CU, and the 8-wave image's launch behind it finishes what it left.  Its chains perform the 8-wave image's strip
products on the same operands in the same order, so every output is BITWISE the option-off run's."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import helpers

ROOT = Path(__file__).resolve().parent.parent
THICK = dict(aerosol_total=2.0, aerosol_p0=600.0, aerosol_σp=200.0, absorption=False)


def _run(rtamd, m, sc, on):
    with rtamd.corert.make_handle(m) as h:
        h.set_option(rtamd._lib.MOM_OPT_STRIP2, on)
        R, T = rtamd.corert.run_scene(h, sc)
        out = (R, T) + tuple(h.get_hdr()) + (h.timers()["layer_launches"],)
        R2, T2 = rtamd.corert.run_scene(h, sc)                       # the resume table is reused: same answer again
        assert np.array_equal(R, R2) and np.array_equal(T, T2)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("nS,lt,N,kw,brdf", [
    (4, 19, 52, {}, None), (4, 21, 56, {}, None), (4, 23, 60, {}, None),        # IQUV, 13 / 14 / 15 streams (N = 52, 56: ndoubl = 0 layers)
    (4, 19, 52, THICK, None), (4, 23, 60, THICK, None),                         # thick layers: units leave the image and resume
    (3, 33, 60, {}, None), (3, 33, 60, THICK, None),                            # IQU, 20 streams (the headline's full problem)
    (1, 113, 60, {}, None),                                                     # scalar, 60 streams (no stream-pair tables)
    (4, 21, 56, {}, "rpv")])
def test_strip2_image_bitwise_and_oracle(rtamd, cref, nS, lt, N, kw, brdf):
    m = rtamd.scenes.make_scene(nS, lt, 6, 24, seed=7 * nS + lt, **kw)
    if brdf:
        m.params.brdf = rtamd.corert.rpvSurfaceScalar(0.1, 0.8, 0.7, -0.1)
    sc = rtamd.prepare_scene(m)
    assert sc.N == N
    on, off = _run(rtamd, m, sc, 1), _run(rtamd, m, sc, 0)
    for k, what in enumerate(("R", "T", "hdr", "bhr_uw", "bhr_dw")):
        assert np.array_equal(on[k], off[k]), f"two-buffer image vs 8-wave image: {what}"
    assert on[5] == off[5] + 1                                              # the two-buffer launch in front of the 8-wave one
    Rr, Tr, Hr, upr, dwr, info = cref.rt_run_full(cref.pack_scene(helpers.oracle_scene(m)))
    assert info == 0
    tol = helpers.stokes_rtol(sc.ndoubl)
    helpers.assert_stokes_close(on[0], Rr, rtol=tol, what="R")
    helpers.assert_stokes_close(on[1], Tr, rtol=tol, what="T")
    helpers.assert_stokes_close(on[2], Hr, rtol=tol, what="hdr")


def test_strip2_lds_budget_host(tmp_path):
    """Host only: for every edge and Stokes layout the dispatcher admits, two images plus the per-workgroup allowance fit the
    CU's 160 KiB, and the elemental tables end below the first t entry stored directly (tools/strip2_budget_check.hip)."""
    exe = tmp_path / "strip2_budget_check"
    csrc = ROOT / "radiativetransfer.jl_amd" / "csrc"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "--offload-arch=gfx950", f"-I{ROOT / 'include'}", f"-I{csrc}", "-DMOM_WAVES=4",
                           "-DMOM_TJ=4", "-DMOM_NO_STRAIGHT", "-DMOM_NS=mom2", str(ROOT / "tools" / "strip2_budget_check.hip"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    admitted = [ln for ln in out.stdout.splitlines() if "admitted" in ln]
    # 52: ns = 1, 2, 4; 56: 1, 4; 60: 1, 3, 4 (two components per stream at 56 / 60: the tables reach the direct entries)
    assert len(admitted) == 8 and "OVER" not in out.stdout, out.stdout
