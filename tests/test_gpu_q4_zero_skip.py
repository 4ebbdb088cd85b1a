"""MOM_OPT_ZERO_SKIP (csrc/mom_q4.hpp): the quad-block image leaves out the products whose operand is an exact zero because of the
zero-weight streams at the end of the stream set.  The terms left out are exact zeros, so every output equals the option-off
run's (`==`: the sign of a zero may differ), and the image still agrees with the C oracle."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import helpers

ROOT = Path(__file__).resolve().parent.parent
THICK = dict(aerosol_total=2.0, aerosol_p0=600.0, aerosol_σp=200.0, absorption=False)
NAMES = ("R", "T", "hdr", "bhr_uw", "bhr_dw")


def _run(rtamd, m, sc, on):
    with rtamd.corert.make_handle(m) as h:
        h.set_option(rtamd._lib.MOM_OPT_ZERO_SKIP, on)
        R, T = rtamd.corert.run_scene(h, sc)
        out = (R, T) + tuple(h.get_hdr())
        t = h.timers()
        R2, T2 = rtamd.corert.run_scene(h, sc)                       # the resume table is reused: same answer again
        again = (R2, T2) + tuple(h.get_hdr())
        for k, what in enumerate(NAMES):
            assert np.array_equal(out[k], again[k]), f"second run on the same handle: {what}"
    return out, t


# nS, l_trunc, N, scene keywords; the blocks of four entries with a weighted one (nbw) of the problems the image runs:
@pytest.mark.gpu
@pytest.mark.parametrize("nS,lt,N,kw", [
    (3, 33, 60, {}),                                # IQU, 20 streams: sub-problem N0 = 40, nbw = 9 of 10 (block 8 mixed) -- the headline's
    (4, 23, 60, {}),                                # IQUV, 15 streams: N0 = 30 + one dummy stream = 32, nbw = 6 of 8
    (4, 11, 40, dict(sza=50.0)),                    # IQUV, 10 streams: full problem N = 40, nbw = 6 of 10; N0 = 20, nbw = 3 of 5
    (4, 9, 36, dict(vza=(0.0, 30.0, 70.0))),        # IQUV, 9 streams: N = 36, nbw = 5 of 9; N0 = 18 + dummy = 20, nbw = 3 of 5
    (4, 13, 40, dict(sza=60.0, vza=(0.0, 30.0, 70.0))),  # the Sun merges with the Gauss node 0.5: 7 + 3 streams, nbw = 7 (runs as 8) of 10
    (4, 15, 40, dict(vza=(30.0,), vaz=(0.0,))),     # one view angle: 8 + 2 streams, nbw = 8 of 10; N0 = 20, nbw = 4 of 5
    (3, 33, 60, THICK)])                            # thick layers: units leave the image through the resume table
def test_q4_zero_skip_equal_and_oracle(rtamd, cref, nS, lt, N, kw):
    m = rtamd.scenes.make_scene(nS, lt, 6, 24, seed=11 * nS + lt, **kw)
    sc = rtamd.prepare_scene(m)
    assert sc.N == N
    (on, t_on), (off, t_off) = _run(rtamd, m, sc, 1), _run(rtamd, m, sc, 0)
    for k, what in enumerate(NAMES):
        assert np.array_equal(on[k], off[k]), f"MOM_OPT_ZERO_SKIP = 1 against 0: {what}"
    # the quad-block image ran: two first-stage launches in front of the finishers' two (N = 60: the two-buffer image for the
    # full problem, the quad-block image for the m = 0 sub-problem; N = 36 / 40: the quad-block image for both)
    for t in (t_on, t_off):
        assert t["reduced_launches"] == 1 and t["full_launches"] == 1
        assert t["layer_launches"] == t["reduced_launches"] + t["full_launches"] + 2
    Rr, Tr, Hr, upr, dwr, info = cref.rt_run_full(cref.pack_scene(helpers.oracle_scene(m)))
    assert info == 0
    tol = helpers.stokes_rtol(sc.ndoubl)
    helpers.assert_stokes_close(on[0], Rr, rtol=tol, what="R")
    helpers.assert_stokes_close(on[1], Tr, rtol=tol, what="T")
    helpers.assert_stokes_close(on[2], Hr, rtol=tol, what="hdr")


def test_q4_nbw_host(tmp_path):
    """Host only: the count of weighted block rows (mom_host.hpp mom_q4_nbw) on weight vectors with 0, 3 and 4 trailing zeros, a zero
    between weighted entries, dummy entries and no weighted entry at all (tools/q4_nbw_check.hip)."""
    exe = tmp_path / "q4_nbw_check"
    csrc = ROOT / "radiativetransfer.jl_amd" / "csrc"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "--offload-arch=gfx950", f"-I{ROOT / 'include'}", f"-I{csrc}",
                           str(ROOT / "tools" / "q4_nbw_check.hip"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    assert out.stdout.count(" ok") == 8 and "WRONG" not in out.stdout, out.stdout
