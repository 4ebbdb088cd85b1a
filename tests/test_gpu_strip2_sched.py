"""Scheduling of the two-buffer strip image (MOM_OPT_STRIP2_SCHED, csrc/mom_strip2.hpp): the shared unit queue and the asymmetric
chain priority change WHEN and WHERE a unit runs, never what it computes.  Units are independent (each owns its composite block),
so R and T must be bitwise equal with both halves on (3), with each half alone (1 = the default, 2), with the option off (0: fixed
stride, no priority) and with MOM_OPT_STRIP2 = 0 (the 8-wave image only)."""
import numpy as np
import pytest

THICK = dict(aerosol_total=2.0, aerosol_p0=600.0, aerosol_σp=200.0, absorption=False)


def _run(rtamd, m, sc, strip2, sched):
    with rtamd.corert.make_handle(m) as h:
        h.set_option(rtamd._lib.MOM_OPT_STRIP2, strip2)
        h.set_option(rtamd._lib.MOM_OPT_STRIP2_SCHED, sched)
        R, T = rtamd.corert.run_scene(h, sc)
        R2, T2 = rtamd.corert.run_scene(h, sc)          # the queue counter is reset on the stream before every launch
        assert np.array_equal(R, R2) and np.array_equal(T, T2)
        units, left = h.strip2_resumed()                # of the image's last launch: units given, units left to the 8-wave image
    return R, T, units, left


def _check(rtamd, m, N, resume):
    sc = rtamd.prepare_scene(m)
    assert sc.N == N
    R0, T0, units, _ = _run(rtamd, m, sc, 0, 3)
    assert units == 0                                   # MOM_OPT_STRIP2 = 0: the image did not run
    assert np.all(np.isfinite(R0)) and np.all(np.isfinite(T0))
    for sched in (3, 0, 1, 2):
        R, T, units, left = _run(rtamd, m, sc, 1, sched)
        assert units > 512 and units % 512 != 0, units  # more than one round of two workgroups per CU, the last one partial
        assert (0 < left < units) if resume else left == 0, f"{left} of {units} units left through resume[]"
        assert np.array_equal(R, R0), f"R: MOM_OPT_STRIP2_SCHED = {sched} against the 8-wave image"
        assert np.array_equal(T, T0), f"T: MOM_OPT_STRIP2_SCHED = {sched} against the 8-wave image"


# S = 333 spectral points: 333, 666 and 999 units are no multiples of the grid (two workgroups per CU), so the last round is partial
@pytest.mark.gpu
@pytest.mark.parametrize("nS,lt,N,Nz", [(4, 19, 52, 12), (4, 21, 56, 12), (3, 33, 60, 40)])   # N = 60: the headline's shape (IQU, 40 layers, 3 moments)
def test_strip2_sched_bitwise(rtamd, nS, lt, N, Nz):
    _check(rtamd, rtamd.scenes.make_scene(nS, lt, Nz, 333, seed=11 * nS + lt), N, resume=False)


@pytest.mark.gpu
@pytest.mark.parametrize("nS,lt,N", [(3, 33, 60), (4, 19, 52)])
def test_strip2_sched_resume(rtamd, nS, lt, N):
    """Thick layers: some series need more than 12 terms, those units leave the two-buffer image through resume[unit] and the
    8-wave launch behind it finishes them -- with the queue, a unit's index is no longer tied to the workgroup that ran it."""
    _check(rtamd, rtamd.scenes.make_scene(nS, lt, 8, 333, seed=5 * nS + lt, **THICK), N, resume=True)
