"""The Domke-PCW launches (csrc/mom_pcw.hip) at the shapes where their index arithmetic does real work, against the numpy oracle
(tests/pcw_oracle.py: MID_CASES) at the project's tight rule.  tests/test_gpu_pcw.py holds that rule at N_max = 31, 32 and 16 only,
where Np = N_max rounded up to 16 is 32 or 16 and no wavefront of k_pcw_gram takes a second chunk of radii.

  n33_r64, n48_r100   Np = 48: a 32-row macro tile of k_pcw_gram holds rows of two planes (prow = row % Np, the mask prow < keep, the
                      macro-tile swap of k_pcw_combine); 64 radii: no padding; 100 radii: the second trip of k_pcw_diag's loop
  n49_r7              one partial chunk of radii; n_i = 0
  n112_r650           Np = 7 x 16; G = 39 < 41 chunks: the stride c += G and the sum over part[G] of k_pcw_combine
  n300_r40            a lane of k_pcw_sums takes two orders n (tid + 1, tid + 257) and carries its sums across both columns
  (12, 950, 950)      mom_wigner_tables at its limit n_max + l_max = 1900: chains over n of 950 steps, walks of 1900 steps, integer
                      products within a factor of two of 2^63

Bound (pcw_oracle.rule_bound): relative to each array's largest magnitude, 8 x the distance of the Float64 oracle to its long-double
run on the same inputs, not below 2^-46; made here for the three small cases, stored in tests/golden/pcw_n112.npz and pcw_n300.npz
for the two whose long-double run takes 7 s and 97 s.  tests/test_oracle_pcw.py shows that each fault these cases are for would move
the result by more than 1e3 bounds.  Symbols: the absolute bounds of tests/test_oracle_pcw.py."""
import math

import numpy as np
import pytest

import pcw_oracle as po

pytestmark = pytest.mark.gpu

FIELDS = ("α", "β", "γ", "δ", "ϵ", "ζ")


def _optical(case):
    _, _, lam, n_r, n_i, _, _ = po.MID_CASES[case]
    return lam, n_r, n_i


@pytest.mark.parametrize("case", po.PAIR_MID_CASES)
def test_pair_averages_mid(rtamd, case):
    """launches (a) .. (d) alone: the four complex pair averages, each relative to its largest magnitude"""
    ref = po.mid_reference(case)
    r, wx, N = ref["r"], ref["wx"], ref["N"]
    got = rtamd._lib.pcw_pair_averages(r, wx, *_optical(case), N)
    worst = 0.0
    for name, g, a, dist in zip(("anam", "anbm", "bnam", "bnbm"), got, ref["pairs"], ref["d_pairs"]):
        big = float(np.abs(a).max())
        bound = max(8 * float(dist) / big, po.BOUND_FLOOR)
        d = float(np.abs(g - a).max()) / big
        worst = max(worst, d / bound)
        print(f"{case}: {name}: GPU - oracle = {d:.3e}, bound {bound:.3e} (largest {big:.3e})")
        assert g.shape == (N, N) and d <= bound, (case, name, d, bound)
        assert np.all(np.triu(g, 1) == 0)
    print(f"{case}: pairs: largest fraction of a bound used = {worst:.3f}")
    again = rtamd._lib.pcw_pair_averages(r, wx, *_optical(case), N)
    assert all(np.array_equal(x, y) for x, y in zip(got, again))


def _check_greek(case, greek, want, diff, what="GPU"):
    worst = 0.0
    for q, name in enumerate(FIELDS):
        big = float(np.abs(want[q]).max())
        bound = po.rule_bound(want[q], diff[q])
        d = float(np.abs(greek[q] - want[q]).max()) / big
        worst = max(worst, d / bound)
        print(f"{case}: {name}: {what} - oracle = {d:.3e}, bound {bound:.3e}")
        assert d <= bound, (case, name, d, bound)
    print(f"{case}: Greek rows: largest fraction of a bound used = {worst:.3f}")


@pytest.mark.parametrize("case", list(po.MID_CASES))
def test_sums_mid(rtamd, case):
    """all five launches: the six Greek rows and (C_sca, C_ext), not normalised"""
    ref = po.mid_reference(case)
    r, wx, N = ref["r"], ref["wx"], ref["N"]
    greek, C, ms = rtamd._lib.mie_pcw(r, wx, *_optical(case), N)
    assert greek.shape == (6, 2 * N - 1) and np.all(ms >= 0)
    _check_greek(case, greek, ref["greek"], ref["d_greek"])
    bound = po.rule_bound(ref["C"], ref["d_C"])
    d = float(np.abs(C - ref["C"]).max() / np.abs(ref["C"]).max())
    print(f"{case}: C: GPU - oracle = {d:.3e}, bound {bound:.3e}, fraction used {d / bound:.3f}")
    assert d <= bound
    greek2, C2, _ = rtamd._lib.mie_pcw(r, wx, *_optical(case), N)
    assert np.array_equal(greek, greek2) and np.array_equal(C, C2)


def test_public_call_mid(rtamd):
    """compute_aerosol_optical_properties(::MieModel{PCW}) at n48_r100: the rows divided by C_sca against the oracle's on the
    product's own host inputs, by the same rule; ω̃ and k bitwise from the direct call's C, which test_sums_mid holds to the rule"""
    sc = rtamd.scattering
    case = "n48_r100"
    r_max, nquad, lam, n_r, n_i, r_m, σ_g = po.MID_CASES[case]
    model = sc.make_mie_model(sc.PCW(), sc.Aerosol(sc.LogNormal(math.log(r_m), math.log(σ_g)), n_r, n_i), lam, None, None, r_max, nquad)
    r, wx, N = sc.pcw_inputs(model)
    assert N == po.MID_N_MAX[case] and len(r) == nquad
    o64 = po.pcw_sums(r, wx, lam, n_r, n_i, r_max)
    o80 = po.pcw_sums(r.astype(np.longdouble), wx.astype(np.longdouble), lam, n_r, n_i, r_max)
    n64, n80 = (1 / o64["C"][0]) * o64["greek"], (1 / o80["C"][0]) * o80["greek"]
    aero = sc.compute_aerosol_optical_properties(model)
    g = aero.greek_coefs
    rows = np.stack([g.α, g.β, g.γ, g.δ, g.ϵ, g.ζ])
    assert aero.fᵗ == 1.0 and rows.shape == (6, 2 * N - 1)
    _check_greek(case, rows, n64, (n64 - n80).astype(np.float64), what="public call")
    _, C, _ = rtamd._lib.mie_pcw(r, wx, lam, n_r, n_i, N)
    assert aero.ω̃ == C[0] / C[1] and aero.k == C[1]
    again = sc.compute_aerosol_optical_properties(model).greek_coefs
    assert np.array_equal(rows, np.stack([again.α, again.β, again.γ, again.δ, again.ϵ, again.ζ]))


def test_wigner_tables_at_the_limit(rtamd):
    """compute_wigner_values(12, 950, 950), 87 MB per table: n + l up to 1899, the largest mom_wigner_tables accepts; every column is
    walked from m = n + l - 1 down to m <= 12.  60 seeded entries with n + (l - 1) >= 1700 and every entry of the eight columns next
    to n = l = 950 against the exact symbols."""
    shape = po.LIMIT_TABLE
    A, B = rtamd.compute_wigner_values(*shape)
    assert A.shape == B.shape == shape
    samples, Ae, Be = po.limit_exact()
    assert len(samples) >= 60 + 8 and min(n + l - 1 for _, n, l in samples) >= 1700 and max(n + l - 1 for _, n, l in samples) == 1899
    idx = tuple(np.array(samples).T - 1)
    dA, dB = float(np.abs(A[idx] - Ae).max()), float(np.abs(B[idx] - Be).max())
    print(f"{shape}, {len(samples)} samples: max |A - exact| = {dA:.3e} (bound {po.A_BOUND:.0e}), max |B - exact| = {dB:.3e} "
          f"(bound {po.B_BOUND:.0e}); largest |exact| = {np.abs(Ae).max():.3e}, {np.abs(Be).max():.3e}")
    assert dA <= po.A_BOUND and dB <= po.B_BOUND
    outA, outB = po.out_of_range(*shape)
    assert np.all(A[outA] == 0) and np.all(B[outB] == 0)
    assert np.all(np.isfinite(A)) and np.all(np.isfinite(B))
    A2, B2 = rtamd.compute_wigner_values(*shape)
    assert np.array_equal(A, A2) and np.array_equal(B, B2)
