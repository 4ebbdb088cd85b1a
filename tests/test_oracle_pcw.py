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
