"""The free-shape Mie oracle and the shape cases of tests/mie_shapes.py, on the CPU: the generalised oracle with its defaults is
bitwise the text it replaced, every case reaches the edge it is named after, the oracle's a_n, b_n agree with mpmath up to
x = 343.7, and the comparison rule the GPU tests use rejects three kinds of wrong result on every shape.  The device is
checked in test_gpu_mie_shapes.py."""
import numpy as np
import pytest

import mie_oracle as mo
import mie_dual_oracle as md
import mie_shapes as ms

CASE2 = (1.0, 37, 0.55, 1.3, 0.001, 0.3, 1.6)          # (r_max, nquad_radius, λ, n_r, n_i, r_m, σ_g) as in test_gpu_mie.py
ABSORBING = (0.5, 20, 0.76, 1.5, 0.1, 0.3, 1.6)


# ------------------------------------------------------------------------------------------------------------------------------
# the text of nai2_sums and nai2_sums_dual before they took free shapes, kept to pin the defaults bitwise
# ------------------------------------------------------------------------------------------------------------------------------

def _nai2_sums_fixed_shapes(r, wx_rows, lam, n_r, n_i):
    dt = r.dtype.type
    wx_rows = np.atleast_2d(wx_rows)
    k = 2 * mo.pi_of(dt) / dt(lam)
    x = k * r
    ar, ai, br, bi, nmax = mo.mie_ab(x, n_r, n_i, dt)
    n_top = int(mo.n_max_of(np.max(x).astype(np.float64)))
    assert n_top == ar.shape[0]
    mu, w_mu = mo.gausslegendre(2 * n_top - 1, dt)
    p, t = mo.mie_pi_tau(mu, n_top)
    l = np.arange(1, n_top + 1).astype(dt)
    c = ((2 * l + 1) / (l * (l + 1)))[:, None]
    a, b = c * (ar + 1j * ai), c * (br + 1j * bi)
    S1, S2 = t @ a + p @ b, p @ a + t @ b
    h = dt(0.5) / (x * x)
    f = np.stack([h * (np.abs(S1) ** 2 + np.abs(S2) ** 2), h * (S1 * np.conj(S2) + S2 * np.conj(S1)).real,
                  -h * (np.abs(S1) ** 2 - np.abs(S2) ** 2), -h * (S1 * np.conj(S2) - S2 * np.conj(S1)).imag])
    w2 = (2 * l + 1)[:, None]
    C_sca = 2 * mo.pi_of(dt) / k ** 2 * np.sum(w2 * (ar * ar + ai * ai + br * br + bi * bi), axis=0)
    C_ext = 2 * mo.pi_of(dt) / k ** 2 * np.sum(w2 * (ar + br), axis=0)
    C = np.stack([wx_rows @ C_sca, wx_rows @ C_ext], axis=1)
    wr = 4 * mo.pi_of(dt) * r * r * wx_rows
    bulk = np.einsum("fmi,ki->kfm", f, wr)
    l_max = mu.size
    P, P2, R2, T2 = mo.legendre_tables(mu, l_max)
    ll = np.arange(l_max).astype(dt)
    pre = (2 * ll + 1) / 2
    fac = np.zeros(l_max, dt)
    fac[2:] = pre[2:] * np.sqrt(1 / ((ll[2:] - 1) * ll[2:] * (ll[2:] + 1) * (ll[2:] + 2)))
    greek = np.zeros((wx_rows.shape[0], 6, l_max), dt)
    for kk in range(wx_rows.shape[0]):
        f11, f33, f12, f34 = (w_mu * bulk[kk, q] for q in range(4))
        greek[kk] = [fac * (f11 @ R2 + f33 @ T2), pre * (f11 @ P), fac * (f12 @ P2), pre * (f33 @ P), fac * (f34 @ P2),
                     fac * (f33 @ R2 + f11 @ T2)]
    return dict(bulk_f=bulk, C=C, greek=greek, mu=mu, w_mu=w_mu, x=x, n_max=nmax)


def _nai2_sums_dual_fixed_shapes(r, wx, lam, n_r, n_i):
    dt = r.dtype.type
    wx = np.asarray(wx, dtype=r.dtype).reshape(1, -1)
    k = 2 * mo.pi_of(dt) / dt(lam)
    x = k * r
    ar, ai, br, bi, nmax = md.mie_ab_dual(x, n_r, n_i, dt)
    n_top = int(mo.n_max_of(np.max(x).astype(np.float64)))
    assert n_top == ar.v.shape[0]
    mu, w_mu = mo.gausslegendre(2 * n_top - 1, dt)
    p, t = mo.mie_pi_tau(mu, n_top)
    l = np.arange(1, n_top + 1).astype(dt)
    c = ((2 * l + 1) / (l * (l + 1)))[:, None]
    a, b = c * (ar.v + 1j * ai.v), c * (br.v + 1j * bi.v)
    S1, S2 = t @ a + p @ b, p @ a + t @ b
    dS1r, dS1i = t @ (c * ar.d) + p @ (c * br.d), t @ (c * ai.d) + p @ (c * bi.d)
    dS2r, dS2i = p @ (c * ar.d) + t @ (c * br.d), p @ (c * ai.d) + t @ (c * bi.d)
    h = dt(0.5) / (x * x)
    f = np.stack([h * (np.abs(S1) ** 2 + np.abs(S2) ** 2), h * (S1 * np.conj(S2) + S2 * np.conj(S1)).real,
                  -h * (np.abs(S1) ** 2 - np.abs(S2) ** 2), -h * (S1 * np.conj(S2) - S2 * np.conj(S1)).imag])
    dn1 = 2 * (S1.real * dS1r + S1.imag * dS1i)
    dn2 = 2 * (S2.real * dS2r + S2.imag * dS2i)
    dre = 2 * (dS1r * S2.real + S1.real * dS2r + dS1i * S2.imag + S1.imag * dS2i)
    dim = 2 * (dS1i * S2.real + S1.imag * dS2r - dS1r * S2.imag - S1.real * dS2i)
    df = np.stack([h * (dn1 + dn2), h * dre, -h * (dn1 - dn2), -h * dim], axis=1)
    w2 = (2 * l + 1)[:, None]
    pre_c = 2 * mo.pi_of(dt) / k ** 2
    C_sca = pre_c * np.sum(w2 * (ar.v * ar.v + ai.v * ai.v + br.v * br.v + bi.v * bi.v), axis=0)
    C_ext = pre_c * np.sum(w2 * (ar.v + br.v), axis=0)
    dC_sca = pre_c * np.sum(w2 * (2 * (ar.v * ar.d + ai.v * ai.d + br.v * br.d + bi.v * bi.d)), axis=1)
    dC_ext = pre_c * np.sum(w2 * (ar.d + br.d), axis=1)
    C = np.stack([wx @ C_sca, wx @ C_ext], axis=1)
    d_C = np.stack([dC_sca @ wx[0], dC_ext @ wx[0]], axis=1)
    wr = 4 * mo.pi_of(dt) * r * r * wx
    bulk = np.einsum("fmi,ki->kfm", f, wr)
    d_bulk = np.einsum("cfmi,i->cfm", df, wr[0])
    l_max = mu.size
    P, P2, R2, T2 = mo.legendre_tables(mu, l_max)
    ll = np.arange(l_max).astype(dt)
    pre = (2 * ll + 1) / 2
    fac = np.zeros(l_max, dt)
    fac[2:] = pre[2:] * np.sqrt(1 / ((ll[2:] - 1) * ll[2:] * (ll[2:] + 1) * (ll[2:] + 2)))

    def project(bk):
        f11, f33, f12, f34 = (w_mu * bk[q] for q in range(4))
        return [fac * (f11 @ R2 + f33 @ T2), pre * (f11 @ P), fac * (f12 @ P2), pre * (f33 @ P), fac * (f34 @ P2),
                fac * (f33 @ R2 + f11 @ T2)]

    greek = np.zeros((1, 6, l_max), dt)
    greek[0] = project(bulk[0])
    d_greek = np.zeros((2, 6, l_max), dt)
    for cc in range(2):
        d_greek[cc] = project(d_bulk[cc])
    return dict(bulk_f=bulk, C=C, greek=greek, mu=mu, w_mu=w_mu, x=x, n_max=nmax, d_bulk_f=d_bulk, d_C=d_C, d_greek=d_greek)


def _model_inputs(case, dtype):
    r_max, nquad, _, _, _, r_m, σ_g = case
    r, wr = mo.gauleg_norm(nquad, 0, r_max, dtype)
    return r, mo.weights_wx(r, wr, r_m, σ_g)


@pytest.mark.parametrize("case", [CASE2, ABSORBING], ids=["case2", "absorbing"])
@pytest.mark.parametrize("dtype", [np.float64, np.longdouble], ids=["f64", "f80"])
def test_defaults_are_bitwise_the_fixed_shape_oracle(case, dtype):
    """nai2_sums and nai2_sums_dual without their keyword arguments return, bit for bit, what they returned before they had any;
    so does naming the defaults (the Gauss rule of 2 n_top - 1 nodes, n_rows = n_top, l_max = n_mu)."""
    _, _, lam, n_r, n_i, _, _ = case
    r, wx = _model_inputs(case, dtype)
    rows = np.stack([wx, wx * (r - r.mean()), wx * r])       # three rows: the value form's loop over them is part of the text
    old, new = _nai2_sums_fixed_shapes(r, rows, lam, n_r, n_i), mo.nai2_sums(r, rows, lam, n_r, n_i)
    n_top = int(mo.n_max_of(np.max(old["x"]).astype(np.float64)))
    mu, w_mu = mo.gausslegendre(2 * n_top - 1, dtype)
    named = mo.nai2_sums(r, rows, lam, n_r, n_i, mu=mu, w_mu=w_mu, n_rows=n_top, l_max=mu.size)
    assert set(old) == set(new) == set(named)
    for q in old:
        assert new[q].dtype == old[q].dtype and np.array_equal(new[q], old[q]), q
        assert np.array_equal(named[q], old[q]), q
    old_d, new_d = _nai2_sums_dual_fixed_shapes(r, wx, lam, n_r, n_i), md.nai2_sums_dual(r, wx, lam, n_r, n_i)
    assert set(old_d) == set(new_d)
    for q in old_d:
        assert new_d[q].dtype == old_d[q].dtype and np.array_equal(new_d[q], old_d[q]), q
    # the twin with three weight rows: its value part is the oracle's for those rows, its partials those of row 0 alone
    three = md.nai2_sums_dual(r, rows, lam, n_r, n_i)
    for q in ms.ARRAYS:
        assert np.array_equal(three[q], new[q]), q
        assert np.array_equal(three["d_" + q], new_d["d_" + q]), q


# ------------------------------------------------------------------------------------------------------------------------------
# every case reaches its edge
# ------------------------------------------------------------------------------------------------------------------------------

def test_kernel_constants():
    """the tiling constants the cases were laid out for; after a retune of the kernel the cases below have to be laid out again"""
    assert ms.kernel_constants() == (16, 32, 4, 128)


def test_case_table():
    assert len(ms.VALUE_CASES) == 29 and len(ms.DUAL_CASES) == 28 and all(c.nW == 1 for c in ms.ONE_ROW.values())
    assert set(c.shape for c in {**ms.VALUE_CASES, **ms.DUAL_CASES}.values()) == set(ms.SHAPES.values())
    for name, shape in ms.SHAPES.items():
        inp = ms.device_inputs(shape)
        assert inp["r"].shape == (shape.nR,) and np.all(np.diff(inp["r"]) > 0) and inp["r"][0] > 0, name
        assert inp["w"].shape == (4, shape.nR) and inp["w_mu"].shape == (shape.n_mu,), name
        assert inp["pi"].shape == inp["tau"].shape == (shape.n_mu, inp["n_rows"]), name
        assert all(t.shape == (shape.n_mu, shape.l_max) for t in inp["legendre"]), name
        assert inp["n_top"] == int(ms.oracle(shape)[0]["n_max"].max()), name


def test_weight_rows():
    """distinct, linearly independent, and exactly one of them changes sign"""
    for r_lo, nR, r_hi in ((ms.R_LO, 37, 1.0), (ms.TILE_K_R_LO, 128, 1.0), (ms.R_LO, 2057, 0.05)):
        w = ms.weight_rows(np.linspace(r_lo, r_hi, nR))
        assert w.shape == (4, nR) and np.linalg.matrix_rank(w / np.abs(w).max(axis=1, keepdims=True)) == 4
        signs = [bool(np.any(row > 0) and np.any(row < 0)) for row in w]
        assert signs == [False, True, False, False]
        assert abs(w[0].sum() - 1) <= 1e-14


def test_mu_block_cases_cross_the_block_edges():
    _, mu_block, _, _ = ms.kernel_constants()
    n = sorted(c.shape.n_mu for c in ms.MU_BLOCK.values())
    assert 1 in n
    for edge in (mu_block // 2, mu_block, 2 * mu_block):      # 16: the Dual form's block; 32, 64: the value form's
        assert {edge - 1, edge, edge + 1} <= set(n)
    assert all(c.shape.l_max != c.shape.n_mu and c.shape.n_mu != 2 * ms.device_inputs(c.shape)["n_top"] - 1
               for c in ms.MU_BLOCK.values())


def test_greek_cases():
    """l_max below, at and above n_mu and its padded size, and below 3, where gamma, epsilon, alpha and zeta have no entries"""
    _, mu_block, _, _ = ms.kernel_constants()
    l = sorted(c.shape.l_max for c in ms.GREEK.values())
    n_mu = ms.Shape().n_mu
    assert l == [1, 2, 3, 32, 38, 200] and all(c.shape.n_mu == n_mu for c in ms.GREEK.values())
    assert n_mu not in l and ms.round_up(n_mu, mu_block) not in l and min(l) == 1 and max(l) > ms.round_up(n_mu, mu_block)


def test_k_padding_cases():
    """the spare rows take the padded row count Kp past the next multiples of the k-step, with and without a remainder"""
    _, _, k_step, _ = ms.kernel_constants()
    n_top = ms.device_inputs(ms.Shape())["n_top"]
    Kp = [ms.round_up(n_top + c.shape.spare_rows, k_step) for c in ms.K_PADDING.values()]
    assert len(set(Kp)) >= 3 and min(Kp) == ms.round_up(n_top, k_step)
    assert {(n_top + c.shape.spare_rows) % k_step for c in ms.K_PADDING.values()} == set(range(k_step))


@pytest.mark.parametrize("name", ["tile_k", "absorbing_tile_k"])
def test_tile_k_conditions(name):
    tile_r, _, k_step, _ = ms.kernel_constants()
    shape = ms.SHAPES[name]
    o64, _ = ms.oracle(shape)
    n_max = o64["n_max"]
    assert np.all(np.diff(n_max) >= 0) and shape.nR == 8 * tile_r
    residues, short = ms.tile_k_conditions(n_max, ms.device_inputs(shape)["n_rows"], tile_r, k_step)
    print(f"{name}: last n_max of the tiles {ms.tile_last_n_max(n_max, tile_r)}, residues {residues}, tiles ending early {short}")
    assert residues == list(range(k_step))
    assert short >= 3


def test_chunk_walk_conditions():
    tile_r, mu_block, _, max_chunks = ms.kernel_constants()
    shape = ms.CHUNK_WALK
    n_tiles, G, rows, live = ms.chunk_walk_conditions(shape.n_mu, shape.nR, tile_r, mu_block, max_chunks)
    assert (n_tiles, G, rows, live) == (129, 62, 3, 5)        # one row forward, one fully reversed, one with 5 live chunks
    assert ms.round_up(shape.n_mu, mu_block) // mu_block == 33 and G < max_chunks
    assert int(ms.oracle(shape)[0]["n_max"].max()) <= 14


def test_coefficient_cases():
    """x is a permutation of the log grid, unsorted, and neighbouring lanes differ widely in their trip counts (downward plus
    upward recurrence)"""
    assert ms.COEF_N_MAX == int(mo.n_max_of(343.7)) + 3
    for nX in ms.COEF_NX:
        x = ms.coefficient_x(nX)
        assert x.shape == (nX,)
        if nX == 1:
            assert x[0] == ms.X_HI
            continue
        assert np.array_equal(np.sort(x), np.geomspace(ms.X_LO, ms.X_HI, nX)) and np.any(np.diff(x) < 0)
        n_max = mo.n_max_of(x)
        trips = mo.nmx_of(x, n_max, *ms.M_WEAK) - 1 + n_max
        print(f"nX = {nX}: trip counts {trips.min()} .. {trips.max()}, mean |difference of neighbours| {np.abs(np.diff(trips)).mean():.0f}")
        assert trips.min() <= 75 and trips.max() >= 800
        assert np.abs(np.diff(trips)).mean() >= 100
    assert max(ms.COEF_NX) > 2 * 64 and {63, 64, 65} <= set(ms.COEF_NX)


# ------------------------------------------------------------------------------------------------------------------------------
# the oracle against mpmath
# ------------------------------------------------------------------------------------------------------------------------------

MP_MS = [(1.3, 0.001), (1.5, 0.1), (1.33, 0.0), (1.75, 0.44), (0.8, 2.0)]
MP_XS = [0.001, 40.0, 100.0, 343.7]


@pytest.mark.parametrize("n_r,n_i", MP_MS)
def test_coefficients_against_mpmath(n_r, n_i):
    """mie_ab in Float64 against Bohren & Huffman 4.53 in mpmath at 60 digits, relative to the largest coefficient of that
    (m, x).  Bound: 8 x the distance between the Float64 and the long-double run of mie_ab at the same point -- the margin the
    GPU tests grant the device, so this shows that the long-double run is a valid arbiter up to x = 343.7.  Measured: the ratio
    distance-to-mpmath / distance-to-long-double is at most 1.18 (DESIGN section 4 lists the distances per point).
    x = 1000 is left out on purpose: see DESIGN section 4."""
    pytest.importorskip("mpmath")
    for x in MP_XS:
        o64, o80 = mo.mie_ab(x, n_r, n_i, np.float64), mo.mie_ab(x, n_r, n_i, np.longdouble)
        n_max = int(o64[4][0])
        a, b = mo.mie_ab_mp(x, complex(n_r, n_i), n_max)
        ref = np.stack([a, b])
        c64 = np.stack([o64[0][:, 0] + 1j * o64[1][:, 0], o64[2][:, 0] + 1j * o64[3][:, 0]])
        c80 = np.stack([o80[0][:, 0] + 1j * o80[1][:, 0], o80[2][:, 0] + 1j * o80[3][:, 0]])
        big = np.abs(ref).max()
        d_mp, d_80 = float(np.abs(c64 - ref).max() / big), float(np.abs(c64 - c80).max() / big)
        print(f"m = {n_r} + {n_i}i, x = {x}: n_max = {n_max}, Float64 - mpmath = {d_mp:.3e}, Float64 - long double = {d_80:.3e}, "
              f"ratio {d_mp / d_80:.2f}")
        assert d_mp <= 8 * d_80, (n_r, n_i, x, d_mp, d_80)


# ------------------------------------------------------------------------------------------------------------------------------
# the comparison rule is not vacuous
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(ms.SHAPES))
def test_checker_rejects_corrupted_results(name):
    """On every shape: the Float64 oracle's own output passes the rule of mie_shapes.compare, and three corruptions of it that an
    index or stride error in the kernel could produce do not."""
    o64, o80 = ms.oracle(ms.SHAPES[name])
    bad, factors = ms.compare({q: o64[q] for q in ms.ARRAYS}, o64, o80)
    assert bad == [] and all(v == 0 for v in factors.values())
    for what, wrong in ms.corruptions(o64).items():
        bad, _ = ms.compare(wrong, o64, o80)
        print(f"{name}: {what}: {len(bad)} violations, first: {bad[0] if bad else None}")
        assert bad, (name, what)
    # the rule looks only at the rows a call returned
    bad, _ = ms.compare({q: o64[q][:2] for q in ms.ARRAYS}, o64, o80)
    assert bad == []


# ------------------------------------------------------------------------------------------------------------------------------
# free shapes in the Dual twin
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mu_33", "lmax_38"])
def test_dual_twin_with_free_shapes(name):
    """The twin's value part is bitwise nai2_sums on the same free-shape inputs (rows 0 .. 2), and its two partials of the
    coefficients still obey d/dn_i = i d/dn_r within the bound of test_oracle_mie_dual.py::test_cauchy_riemann: per x, 8 x the
    twin's Float64 / long-double distance, at least 2^-46."""
    shape = ms.SHAPES[name]
    d64, _ = ms.oracle_dual(shape)
    i = ms.oracle_inputs(shape, np.float64)
    o64 = mo.nai2_sums(i["r"], i["wx"][:3], ms.LAM, *shape.m, mu=i["mu"], w_mu=i["w_mu"], n_rows=i["n_rows"], l_max=shape.l_max)
    for q in ms.ARRAYS:
        assert d64[q].shape[0] == 3 and np.array_equal(d64[q], o64[q]), q
        assert d64["d_" + q].shape == (2,) + o64[q].shape[1:]
    n_rows = ms.device_inputs(shape)["n_rows"]
    x = o64["x"]
    t64, t80 = (md.mie_ab_dual(x.astype(dt), *shape.m, dt, n_rows=n_rows) for dt in (np.float64, np.longdouble))

    def partial(t, c):
        return np.stack([t[0].d[c] + 1j * t[1].d[c], t[2].d[c] + 1j * t[3].d[c]])

    worst = 0.0
    for j in range(x.size):
        big = np.abs(partial(t64, 0)[:, :, j]).max()
        dist = max(float(np.abs(partial(t64, c)[:, :, j] - partial(t80, c)[:, :, j]).max() / big) for c in (0, 1))
        bound = max(8 * dist, ms.FLOOR)
        cr = float(np.abs(partial(t64, 1)[:, :, j] - 1j * partial(t64, 0)[:, :, j]).max() / big)
        worst = max(worst, cr / bound)
        assert cr <= bound, (name, j, cr, bound)
    print(f"{name}: largest |d/dn_i - i d/dn_r| / bound over the radii = {worst:.3f}")
