"""The Mie kernels (csrc/mom_mie.hip) at the shapes the host layer never produces: n_mu, n_max and l_max independent of each other,
every weight-row form of k_mie_amp, the whole chunk walk, and k_mie_ab on unsorted size parameters up to x = 343.7.  The cases, the
conditions under which they reach their edges and the comparison rule are in tests/mie_shapes.py; test_oracle_mie_shapes.py shows
on the CPU that the conditions hold and that the rule rejects wrong results.

Every tolerance is computed from the oracle alone: 8 x the distance between its Float64 and its long-double run on the same inputs,
at least 2^-46, per array and per row on the row's own scale.  What has to be bitwise is compared with np.array_equal."""
import functools

import numpy as np
import pytest

import mie_dual_oracle as md
import mie_shapes as ms

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _device(shape, rows, dual, flags=0):
    """(bulk_f, C, greek) of one library call on the shape's inputs with the weight rows `rows` (a tuple of indices into the four)"""
    import rtamd
    inp = ms.device_inputs(shape)
    fn = rtamd._lib.mie_nai2_dual if dual else rtamd._lib.mie_nai2
    out = fn(inp["r"], inp["w"][list(rows)], ms.LAM, *shape.m, inp["w_mu"], inp["pi"], inp["tau"], *inp["legendre"], flags=flags)
    assert np.all(out[3] >= 0)
    for a in out[:3]:
        a.setflags(write=False)
    return dict(zip(ms.ARRAYS, out[:3]))


def _rows(nW):
    return tuple(range(nW))


def _report(name, form, factors):
    print(f"{name}: {form}: factor used of 8: " + ", ".join(f"{q} {v:.2f}" for q, v in factors.items()))


@pytest.mark.parametrize("name", list(ms.VALUE_CASES))
def test_value_form_against_oracle(rtamd, name):
    """bulk_f, C and greek of mom_mie_nai2 against the Float64 oracle, and the output shapes.

    chunk_walk is the case that showed what the device's own sin x, cos x cost: with them as the start of the upward psi
    recurrence bulk_f stood 3.5e-14 from the oracle against a bound of 1.6e-14 (factor 17.8 of 8), all of it from a_n, b_n
    (every radius there has x <= 0.57 with n_max >= 10, the recurrence runs far above x, and tau_n, pi_n ~ n^4 / 4 magnify the high
    orders at |mu| -> 1).  With the host's sin x, cos x (mom_mie.hip: mie_sin_cos) the factor is 0.78."""
    case = ms.VALUE_CASES[name]
    shape, nW = case.shape, case.nW
    got = _device(shape, _rows(nW), False)
    assert got["bulk_f"].shape == (nW, 4, shape.n_mu) and got["C"].shape == (nW, 2) and got["greek"].shape == (nW, 6, shape.l_max)
    bad, factors = ms.compare(got, *ms.oracle(shape))
    _report(name, "value", factors)
    assert bad == [], (name, bad)


@pytest.mark.parametrize("name", list(ms.DUAL_CASES))
def test_dual_form_against_oracle(rtamd, name):
    """rows 0 .. nW - 1 are bitwise the value call's; the two index rows against the forward-mode twin"""
    case = ms.DUAL_CASES[name]
    shape, nW = case.shape, case.nW
    got = _device(shape, _rows(nW), True)
    value = _device(shape, _rows(nW), False)
    assert got["bulk_f"].shape == (nW + 2, 4, shape.n_mu) and got["C"].shape == (nW + 2, 2)
    assert got["greek"].shape == (nW + 2, 6, shape.l_max)
    for q in ms.ARRAYS:
        assert np.array_equal(got[q][:nW], value[q]), (name, q)
    o64, o80 = ms.oracle_dual(shape)
    names = tuple("d_" + q for q in ms.ARRAYS)
    bad, factors = ms.compare({"d_" + q: got[q][nW:] for q in ms.ARRAYS}, o64, o80, names)
    _report(name, "Dual index rows", factors)
    assert bad == [], (name, bad)
    bad, _ = ms.compare({q: got[q][:nW] for q in ms.ARRAYS}, o64, o80)      # the twin's own value rows, too
    assert bad == [], (name, bad)


@pytest.mark.parametrize("nW", [2, 3, 4])
def test_value_rows_are_independent(rtamd, nW):
    """row k of a call with nW weight rows is bitwise the one-row call on weight row k (every row has accumulators of its own), and
    the rows fed in reversed order come back reversed"""
    shape = ms.Shape()
    together, reverse = _device(shape, _rows(nW), False), _device(shape, _rows(nW)[::-1], False)
    for k in range(nW):
        alone = _device(shape, (k,), False)
        for q in ms.ARRAYS:
            assert np.array_equal(together[q][k], alone[q][0]), (nW, k, q)
            assert np.array_equal(reverse[q][nW - 1 - k], together[q][k]), (nW, k, q)
    for k in range(1, nW):          # the rows do differ: the above is no comparison of a row with itself
        assert not np.array_equal(together["C"][k], together["C"][0])


@pytest.mark.parametrize("nW", [2, 3])
def test_dual_rows_are_independent(rtamd, nW):
    """as above in the Dual form; its two index rows are bitwise those of the one-row Dual call on weight row 0, and the reversed
    call (whose row 0 is another weight row) returns the reversed value rows"""
    shape = ms.Shape()
    together, reverse = _device(shape, _rows(nW), True), _device(shape, _rows(nW)[::-1], True)
    for k in range(nW):
        alone = _device(shape, (k,), True)
        for q in ms.ARRAYS:
            assert np.array_equal(together[q][k], alone[q][0]), (nW, k, q)
            assert np.array_equal(reverse[q][nW - 1 - k], together[q][k]), (nW, k, q)
    first, last = _device(shape, (0,), True), _device(shape, (nW - 1,), True)
    for q in ms.ARRAYS:
        assert np.array_equal(together[q][nW:], first[q][1:]), q
        assert np.array_equal(reverse[q][nW:], last[q][1:]), q
        assert not np.array_equal(together[q][nW:], reverse[q][nW:]), q


@pytest.mark.parametrize("dual", [False, True], ids=["value", "dual"])
@pytest.mark.parametrize("name", list(ms.REPEAT_CASES))
def test_repeatable_and_tile_k_rule(rtamd, name, dual):
    """a second call is bitwise the first (fixed-order reductions over the chunk walk), and so is a call whose radius tiles all run
    to the padded table's end (MOM_MIE_FULL_K): the tile rule leaves out products with exact zeros only"""
    shape = ms.REPEAT_CASES[name].shape
    first = _device(shape, (0,), dual)
    second = _device.__wrapped__(shape, (0,), dual)
    full = _device(shape, (0,), dual, rtamd._lib.MOM_MIE_FULL_K)
    for q in ms.ARRAYS:
        assert np.array_equal(first[q], second[q]), (name, q)
        assert np.array_equal(first[q], full[q]), (name, q)


@pytest.mark.parametrize("dual", [False, True], ids=["value", "dual"])
def test_spare_table_rows_change_nothing(rtamd, dual):
    """pi / tau tables with more rows than the largest n_max: the further rows multiply the planes' exact zeros, and a tile's k-loop
    ends at the tile's own bound whatever the table's size, so the result is bitwise that of the exact table"""
    exact = _device(ms.K_PADDING["spare_0"].shape, (0,), dual)
    for name, case in ms.K_PADDING.items():
        got = _device(case.shape, (0,), dual)
        for q in ms.ARRAYS:
            assert np.array_equal(got[q], exact[q]), (name, q)


# ------------------------------------------------------------------------------------------------------------------------------
# k_mie_ab alone
# ------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _coefficient_oracles(nX, m):
    x = ms.coefficient_x(nX)
    return tuple(md.mie_ab_dual(x, *m, dt, n_rows=ms.COEF_N_MAX) for dt in (np.float64, np.longdouble))


def _pair(t, part):
    """(a, b) [2, n_rows, nX] complex of mie_ab_dual's output: part None the value, 0 / 1 the partial d/dn_r / d/dn_i"""
    re_im = [(t[q].v if part is None else t[q].d[part]) for q in range(4)]
    return np.stack([re_im[0] + 1j * re_im[1], re_im[2] + 1j * re_im[3]])


@pytest.mark.parametrize("n_r,n_i", ms.COEF_MS)
@pytest.mark.parametrize("nX", ms.COEF_NX)
def test_coefficients(rtamd, nX, n_r, n_i):
    """a, b against mie_ab and da/dm, db/dm against the twin's d/dn_r and (times i) d/dn_i, per x on that x's own scale; exact zeros
    above each x's own n_max; the Dual call's a, b bitwise the value call's; the columns follow a permutation of x bitwise.
    (The value part of the twin is bitwise mie_ab: test_oracle_mie_dual.py.)"""
    x = ms.coefficient_x(nX)
    t64, t80 = _coefficient_oracles(nX, (n_r, n_i))
    n_max_x = t64[4]
    a0, b0 = rtamd._lib.mie_coefficients(x, n_r, n_i, ms.COEF_N_MAX)
    a, b, da, db = rtamd._lib.mie_coefficients_dual(x, n_r, n_i, ms.COEF_N_MAX)
    assert a0.shape == da.shape == (ms.COEF_N_MAX, nX)
    assert np.array_equal(a, a0) and np.array_equal(b, b0)
    worst = {}
    for what, got, part, rot in (("a, b", np.stack([a0, b0]), None, 1.0), ("d/dn_r", np.stack([da, db]), 0, 1.0),
                                 ("d/dn_i", np.stack([da, db]), 1, 1j)):
        ref, ext = _pair(t64, part), _pair(t80, part)
        for j in range(nX):
            big = np.abs(ref[:, :, j]).max()
            bound = max(8 * float(np.abs(ref[:, :, j] - ext[:, :, j]).max() / big), ms.FLOOR)
            d = float(np.abs(rot * got[:, :, j] - ref[:, :, j]).max() / big)
            worst[what] = max(worst.get(what, 0.0), 8 * d / bound)
            assert d <= bound, (what, j, x[j], d, bound)
    print(f"nX = {nX}, m = {n_r} + {n_i}i: factor used of 8: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    for j in range(nX):
        for arr in (a0, b0, da, db):
            assert np.all(arr[n_max_x[j]:, j] == 0) and np.any(arr[:n_max_x[j], j] != 0)
    perm = np.arange(nX)[::-1] if nX < 130 else np.argsort(x, kind="stable")      # reversed; sorted: other lanes, other blocks
    pa0, pb0 = rtamd._lib.mie_coefficients(x[perm], n_r, n_i, ms.COEF_N_MAX)
    pa, pb, pda, pdb = rtamd._lib.mie_coefficients_dual(x[perm], n_r, n_i, ms.COEF_N_MAX)
    for moved, still in ((pa0, a0), (pb0, b0), (pa, a), (pb, b), (pda, da), (pdb, db)):
        assert np.array_equal(moved, still[:, perm])
