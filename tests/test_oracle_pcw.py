"""The PCW oracle (tests/pcw_oracle.py) against independent knowledge: its Wigner symbols against the exact Racah sums, its Greek
coefficients against the NAI-2 oracle (tests/mie_oracle.py: no Wigner symbol, a scattering-angle quadrature instead), and the stored
PCW result of the reference (tests/golden/pcw_aerosol_optics.npz).  No GPU: the device is checked in test_gpu_pcw.py.

Bounds on the symbols (absolute; the symbols are <= 0.58).  A column's value is reached through at most n_max chain steps over n and
2 n_max steps downward in m, each a handful of roundings in a recursion that runs in its stable direction: for the largest tables
here (n <= 121) that is 363 steps x 5 roundings x 2^-53 x 0.58 = 1.2e-13 if every error had the same sign -- A_BOUND = 2e-13.  The
(-1, -1, 2) symbol is fac ((m (m + 1) +- n (n + 1)) A + 2 sqrt(m (m + 1) n (n + 1)) W) with fac = ((l - 1) l (l + 1) (l + 2))^(-1/2)
<= 0.204: it multiplies the error of A by up to 0.204 x 2 x 241 x 242 = 2.4e4 (the error of A is relative to A, so most of that never
shows), and 2.4e4 x 2^-53 x 0.58 x a handful of roundings = 8e-12 -- B_BOUND = 1e-11."""
from pathlib import Path

import numpy as np
import pytest

import mie_oracle as mo
import pcw_oracle as po

A_BOUND, B_BOUND = po.A_BOUND, po.B_BOUND
GOLDEN = Path(__file__).resolve().parent / "golden" / "pcw_aerosol_optics.npz"


def test_exact_symbols_known_values():
    """(1 1 0; -1 1 0) = 1 / sqrt(3), (2 1 1; -1 1 0) = -sqrt(1 / 10) (eq. 28 at l = 1), (1 1 2; -1 -1 2) = 1 / sqrt(5); one ulp of 1
    is allowed because the right-hand sides are themselves rounded twice"""
    assert abs(po.wigner3j_exact(1, 1, 0, -1, 1, 0) - 1 / np.sqrt(3)) <= 2.0 ** -52
    assert abs(po.wigner3j_exact(2, 1, 1, -1, 1, 0) + np.sqrt(1 / 10)) <= 2.0 ** -52
    assert abs(po.wigner3j_exact(1, 1, 2, -1, -1, 2) - 1 / np.sqrt(5)) <= 2.0 ** -52
    assert po.wigner3j_exact(5, 1, 2, -1, 1, 0) == 0.0


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_symbols_every_entry_small_tables(dtype):
    A, B = po.compute_wigner_values(25, 13, 25, dtype)
    Ae, Be = po.exact_tables(25, 13, 25)
    dA, dB = float(np.abs(A - Ae).max()), float(np.abs(B - Be).max())
    print(f"{np.dtype(dtype).name}: (25, 13, 25): max |A - exact| = {dA:.3e}, max |B - exact| = {dB:.3e}")
    assert dA <= A_BOUND and dB <= B_BOUND
    outA, outB = po.out_of_range(25, 13, 25)
    assert outA.sum() > 1000 and np.all(A[outA] == 0) and np.all(B[outB] == 0) and np.all(Ae[outA] == 0) and np.all(Be[outB] == 0)
    assert np.count_nonzero(Ae) > 2000 and np.count_nonzero(Be) > 2000


def test_symbols_sampled_large_tables():
    """the shorthand compute_wigner_values(120): (241, 121, 241); most columns start beyond the table (n + l - 1 up to 361)"""
    A, B = po.compute_wigner_values(120)
    assert A.shape == (241, 121, 241)
    dA = dB = 0.0
    for m, n, l in po.in_range_samples(241, 121, 241):
        dA = max(dA, abs(A[m - 1, n - 1, l - 1] - po.wigner_A_exact(m, n, l)))
        dB = max(dB, abs(B[m - 1, n - 1, l - 1] - po.wigner_B_exact(m, n, l)))
    print(f"(241, 121, 241), 400 samples: max |A - exact| = {dA:.3e}, max |B - exact| = {dB:.3e}")
    assert dA <= A_BOUND and dB <= B_BOUND


@pytest.mark.parametrize("case", list(po.SMALL_CASES))
def test_pcw_against_nai2_oracle(case):
    """The two routes share a_n, b_n and nothing else.  Bound, absolute on coefficients of up to about 4.5: NAI-2 sums n_mu n_R N
    products (61 x 60 x 31 at the largest case) and PCW N^2 n_R x 16 products per coefficient, rounded to 2^-53: 1.1e5 x 1.1e-16 x
    4.5 = 5.6e-11 if all errors add; random signs give its square root scale.  Both are far above what is seen (about 2e-13)."""
    args = po.SMALL_CASES[case]
    g_pcw, om_pcw, k_pcw = po.aerosol_optics(*args)
    g_nai, om_nai, k_nai = mo.aerosol_optics(*args)
    L = min(g_pcw.shape[1], g_nai.shape[1])
    d = float(np.abs(g_pcw[:, :L] - g_nai[:, :L]).max())
    print(f"{case}: lengths {g_pcw.shape[1]} (PCW) and {g_nai.shape[1]} (NAI-2); max |PCW - NAI-2| = {d:.3e} of {np.abs(g_nai).max():.3f}; "
          f"omega {om_pcw - om_nai:.3e}, k {k_pcw / k_nai - 1:.3e}")
    assert d <= 5.6e-11
    assert abs(om_pcw - om_nai) <= 8 * np.finfo(np.float64).eps and abs(k_pcw / k_nai - 1) <= 8 * np.finfo(np.float64).eps
    assert np.abs(g_pcw[:, L:]).max(initial=0.0) <= 5.6e-11          # what one route has beyond the other's length is rounding
    assert abs(g_pcw[1, 0] - 1) <= 5.6e-11                            # beta_0 = 1


def test_long_double_run_is_close():
    """the arbiter run: the same text in long double, the distance the GPU tests take their bound from"""
    args = po.SMALL_CASES["n32"]
    g64, _, _ = po.aerosol_optics(*args)
    g80, _, _ = po.aerosol_optics(*args, dtype=np.longdouble)
    d = mo.rel_max(g64, g80.astype(np.float64))
    print(f"n32: Float64 - long double = {d:.3e} of the largest coefficient")
    assert 0 < d <= 1e-11


def test_fixture_round_trip():
    """tests/golden/pcw_aerosol_optics.npz: the six arrays, omega and k of the reference's test/test_pcw/PCW_AerosolOptics.jld"""
    z = np.load(GOLDEN)
    for name in ("alpha", "beta", "gamma", "delta", "epsilon", "zeta"):
        assert z[name].shape == (761,) and z[name].dtype == np.float64 and np.all(np.isfinite(z[name]))
    assert float(z["omega"]) == 0.7953832330041786 and float(z["k"]) == 70.77568760880085 and float(z["f_t"]) == 1.0
    assert z["beta"][0] == pytest.approx(1.0, abs=1e-12)
    assert np.all(z["alpha"][:2] == 0) and np.all(z["gamma"][:2] == 0) and np.all(z["zeta"][:2] == 0)


# ---- the middle cases of tests/test_gpu_pcw_shapes.py -----------------------------------------------------------------------------

def _launch_shape(N, nR):
    """Np, nChunks and G as mom_mie_pcw's host code forms them (csrc/mom_pcw.hip, pcw_run)"""
    Np, ld = -(-N // 16) * 16, -(-nR // 16) * 16
    rows = 4 * Np // 32
    return Np, ld // 16, min(max(4096 // (rows * (rows + 1) // 2), 1), ld // 16)


def test_mid_case_definitions():
    """every r_max gives the stated N_max, the per-radius n_max spans a range (the strict mask n < n_max,i is live), and each case
    has the launch shape it is there for"""
    shapes = {}
    for case, args in po.MID_CASES.items():
        r, wx, N = po.case_inputs(case)
        n_max_i = mo.n_max_of(2 * np.pi / args[2] * r)
        assert N == po.MID_N_MAX[case] and len(r) == args[1] and abs(wx.sum() - 1) < 1e-14
        assert n_max_i.min() <= N // 2 and N - 1 <= n_max_i.max() <= N and len(np.unique(n_max_i)) >= min(len(r), N // 4)
        shapes[case] = _launch_shape(N, len(r))
    assert shapes["n33_r64"] == (48, 4, 4) and shapes["n48_r100"] == (48, 7, 7)      # Np / 16 odd; 64 = 4 x 16; 100 > 64 lanes
    assert shapes["n49_r7"] == (64, 1, 1) and po.MID_CASES["n49_r7"][4] == 0.0
    assert shapes["n112_r650"] == (112, 41, 39)                                       # chunk groups 0 and 1 take chunks 39 and 40
    assert shapes["n300_r40"][0] == 304 and po.MID_N_MAX["n300_r40"] > 256


@pytest.mark.parametrize("case", list(po.MID_CASES))
def test_mid_bounds(case):
    """the bounds test_gpu_pcw_shapes.py takes: positive, never above 1e-11, never below the floor"""
    ref = po.mid_reference(case)
    bounds = [po.rule_bound(ref["greek"][q], ref["d_greek"][q]) for q in range(6)] + [po.rule_bound(ref["C"], ref["d_C"])]
    if ref["pairs"] is not None:
        bounds += [max(8 * float(d) / float(np.abs(a).max()), po.BOUND_FLOOR) for a, d in zip(ref["pairs"], ref["d_pairs"])]
    dist = [float(np.abs(ref["d_greek"][q]).max() / np.abs(ref["greek"][q]).max()) for q in range(6)]
    dist_C = float(np.abs(ref["d_C"]).max() / np.abs(ref["C"]).max())
    print(f"{case}: bounds {min(bounds):.3e} .. {max(bounds):.3e}; Float64 - long double: Greek rows "
          f"{', '.join(format(d, '.2e') for d in dist)}, C {dist_C:.2e}")
    assert all(po.BOUND_FLOOR <= b <= 1e-11 for b in bounds) and np.all(np.isfinite(ref["greek"]))
    assert np.abs(ref["d_greek"]).max() > 0


@pytest.mark.parametrize("case", ["n112_r650", "n300_r40"])
def test_stored_cases_round_trip(case):
    """tests/golden/pcw_n112.npz, pcw_n300.npz: the Float64 oracle run again (N_max = 300: about 23 s) is bitwise the stored one.
    The long-double half comes from tests/golden/make_golden.py only."""
    z = po.stored_case(case)
    args = po.MID_CASES[case]
    r, wx, N = po.case_inputs(case)
    assert np.array_equal(z["params"], np.array(args + (N,))) and np.array_equal(z["r"], r) and np.array_equal(z["wx"], wx)
    o = po.pcw_sums(r, wx, args[2], args[3], args[4], args[0])
    assert z["greek"].shape == (6, 2 * N - 1) and np.array_equal(z["greek"], o["greek"]) and np.array_equal(z["C"], o["C"])
    assert z["d_greek"].dtype == np.float64 and z["d_greek"].shape == (6, 2 * N - 1) and z["d_C"].shape == (2,)
    if case == "n112_r650":   # the pair averages mid_reference forms on its own are those of the whole run
        ref = po.mid_reference(case)
        assert all(np.array_equal(a, b) for a, b in zip(ref["pairs"], o["pairs"]))
        assert np.array_equal(z["big_pairs"], [np.abs(a).max() for a in o["pairs"]]) and np.all(z["d_pairs"] > 0)


# Sensitivity: each case can see the fault it is there for.  The Float64 oracle is run again with the part under test taken away;
# the rows beta and gamma (and C where the part feeds it) must move by at least 1e3 acceptance bounds, relative to the same
# largest magnitudes.  Conditions on the cases, not measurements: a case that fails one gets another size distribution.

def _moved(case, **change):
    """-> by how much of its bound each of beta, gamma and C moves when the oracle runs with `change`"""
    ref = po.mid_reference(case)
    r_max, _, lam, n_r, n_i, _, _ = po.MID_CASES[case]
    wx = change.pop("wx", ref["wx"])
    o = po.pcw_sums(ref["r"], wx, lam, n_r, n_i, r_max, **change)
    out = {}
    for name, got, want, diff in (("β", o["greek"][1], ref["greek"][1], ref["d_greek"][1]), ("γ", o["greek"][2], ref["greek"][2], ref["d_greek"][2]),
                                  ("C", o["C"], ref["C"], ref["d_C"])):
        out[name] = float(np.abs(got - want).max() / np.abs(want).max()) / po.rule_bound(want, diff)
    print(f"{case}: moved by {', '.join(f'{k} {v:.3e}' for k, v in out.items())} bounds")
    return out


def test_sensitivity_second_trip_of_the_radius_loop():
    """k_pcw_diag: a lane's second radius, index >= 64 (n48_r100)"""
    wx = po.mid_reference("n48_r100")["wx"].copy()
    wx[64:] = 0
    assert min(_moved("n48_r100", wx=wx).values()) >= 1e3


def test_sensitivity_second_chunk_of_a_group():
    """k_pcw_gram: the chunks c >= G = 39, the radii from index 16 x 39 on (n112_r650)"""
    wx = po.mid_reference("n112_r650")["wx"].copy()
    wx[16 * 39:] = 0
    assert min(_moved("n112_r650", wx=wx).values()) >= 1e3


def test_sensitivity_orders_above_256():
    """k_pcw_sums: a lane's second order, the Mie coefficients of n > 256 set to zero (n300_r40; formed by the generator)"""
    z, ref = po.stored_case("n300_r40"), po.mid_reference("n300_r40")
    moved = [float(z["sens_greek"][q]) / po.rule_bound(ref["greek"][q], ref["d_greek"][q]) for q in range(6)]
    moved_C = float(z["sens_C"]) / po.rule_bound(ref["C"], ref["d_C"])
    print(f"n300_r40: orders above 256 zeroed: moves {z['sens_greek']} (Greek rows), {float(z['sens_C']):.3e} (C) of the largest "
          f"magnitude; in bounds: {[float(f'{v:.3e}') for v in moved]}, C {moved_C:.3e}")
    assert min(moved) >= 1e3 and moved_C >= 1e3


def test_sensitivity_rows_of_two_planes_in_one_macro_tile():
    """k_pcw_gram at Np = 48: rows 32..47 of the plane Im a and rows 0..15 of the plane Re b share a macro tile; exchanged in what
    the pair averages read (n48_r100).  C does not read the pair averages."""
    def exchange(a, b):
        ai, br = a.imag.copy(), b.real.copy()
        ai[32:48], br[0:16] = b.real[0:16], a.imag[32:48]
        return a.real + 1j * ai, br + 1j * b.imag

    moved = _moved("n48_r100", pair_edit=exchange)
    assert moved["β"] >= 1e3 and moved["γ"] >= 1e3 and moved["C"] == 0


# ---- the symbols at the limit of mom_wigner_tables ----------------------------------------------------------------------------------

def test_scalar_walk_is_the_array_form():
    A, B = po.compute_wigner_values(25, 13, 25)
    for n in range(1, 14):
        for l in range(25):
            for m, (a, b) in po.wigner_column(n, l).items():
                if m <= 25:
                    assert A[m - 1, n - 1, l] == a and B[m - 1, n - 1, l] == b, (m, n, l)


def test_symbols_at_the_limit():
    """(12, 950, 950): n + l - 1 up to 1899, chains over n of 950 steps, walks of up to 1899 steps, the three-integer product of
    eq. 26 up to 0.76 x 2^63.  The array form would take minutes there (1900 steps on 950 x 950 arrays), so the sampled columns are
    walked by pcw_oracle.wigner_column, the same statements on scalars.  The bounds are those derived above for 363 steps: the count
    for 950 + 1900 steps, 2850 x 5 x 2^-53, is relative to the symbol, and the entries with m <= 12 of these columns are below 0.03
    (asserted), not 0.58: 5e-14 and, times the factor of about 2 that eq. 31 has here (fac n^2 is about 1), 1e-13."""
    samples, Ae, Be = po.limit_exact()
    assert len(samples) == len(set(samples)) >= 68 and all(abs(n - (l - 1)) <= m <= 12 and n + l - 1 >= 1700 for m, n, l in samples)
    n, l = 950, 949
    assert max((k * k - 1) * (k * k - (l - n) ** 2) * ((n + l + 1) ** 2 - k * k) for k in range(2, n + l + 2)) > 2 ** 62
    cols = {}
    dA = dB = 0.0
    for (m, n, l), a, b in zip(samples, Ae, Be):
        if (n, l) not in cols:
            cols[n, l] = po.wigner_column(n, l - 1)
        dA, dB = max(dA, abs(cols[n, l][m][0] - a)), max(dB, abs(cols[n, l][m][1] - b))
    print(f"(12, 950, 950), {len(samples)} samples in {len(cols)} columns: max |A - exact| = {dA:.3e}, max |B - exact| = {dB:.3e}; "
          f"largest |exact| = {np.abs(Ae).max():.3e}, {np.abs(Be).max():.3e}")
    assert dA <= A_BOUND and dB <= B_BOUND
    assert 1e-3 < np.abs(Ae).max() < 0.03 and 1e-3 < np.abs(Be).max() < 0.03
