"""The InterpolationModel on the GPU (csrc/mom_lut.hip, mom_lut_*): prefilter, evaluation (value and Dual), the device build, the
profile calls into tau_abs / dtau_abs, state and errors -- against the numpy twin tests/lut_oracle.py, which tests/test_oracle_lut.py
checks against scipy's natural CubicSpline.

Tolerances: the project's Voigt parity figure, 1e-13 max|sigma| for coefficients and values and 1e-13 max|sigma| / step for the
partials (the twin itself stands 4e-16 from scipy); where a result is added to a table that holds another absorber, the rounding of
that sum, 2.3e-16 of the table's largest entry, comes on top.  All grids are dyadic, so node coordinates are exact."""
import re
from pathlib import Path

import numpy as np
import pytest

import lut_oracle as lo

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
TOL = 1e-13


def kernel_constant(name):
    """the literal `name = <integer>` of csrc/mom_lut.hip"""
    text = (ROOT / "radiativetransfer.jl_amd" / "csrc" / "mom_lut.hip").read_text()
    return int(re.search(rf"\b{name} = ([0-9]+)[,;]", text).group(1))


CHUNK, HALO, THREADS = (kernel_constant(k) for k in ("kNuChunk", "kNuHalo", "kNuThreads"))
SUPER = CHUNK * THREADS                      # unknowns per workgroup of the nu prefilter; an axis of n nodes has n - 2 unknowns
EVAL_BLOCK, EVAL_TILE = kernel_constant("kEvalBlock"), kernel_constant("kEvalTile")
NU, P, T = (lo.nodes(r) for r in (lo.NU_RANGE, lo.P_RANGE, lo.T_RANGE))


@pytest.fixture(scope="module")
def h(rtamd):
    with rtamd.Handle(4, 1, NU.size, 1) as hh:
        yield hh


@pytest.fixture(scope="module")
def model(rtamd, h):
    return rtamd.interpolation_model_from_table(h, lo.reference_table(), lo.NU_RANGE, lo.P_RANGE, lo.T_RANGE, 7, 1)


# ---- prefilter ----------------------------------------------------------------------------------------------------------
# nu lengths: the workload's 97; one unknown; shorter than a halo; one below, at and one above the edge of a thread's chunk and
# of a workgroup's stretch of chunks
NU_LENGTHS = [97, 3, HALO // 2, CHUNK + 1, CHUNK + 2, CHUNK + 3, SUPER + 1, SUPER + 2, SUPER + 3]


@pytest.mark.parametrize("k, n_nu", list(enumerate(NU_LENGTHS)))
def test_prefilter_matches_the_dense_solve(h, k, n_nu):
    n_p, n_t = (3, 5, 5, 3)[k % 4], (5, 3, 5, 3)[k % 4]
    tab = lo.synthetic_table(n_nu, n_p, n_t, seed=k)
    lut = h.lut_create((100.0, 0.25, n_nu), (0.0, 1.0, n_p), (0.0, 2.0, n_t))
    try:
        h.lut_set_table(lut, tab)
        c = h.lut_get_coefficients(lut)
        assert np.array_equal(h.lut_get_table(lut), tab)
    finally:
        h.lut_destroy(lut)
    ref = lo.coefficients(tab)
    assert c.shape == ref.shape == (n_nu + 2, n_p + 2, n_t + 2)
    err = np.abs(c - ref).max()
    print(f"prefilter nNu = {n_nu}: {err / tab.max():.2e} max sigma")
    assert err <= TOL * tab.max()


def test_prefilter_of_the_reference_table(h, model):
    err = np.abs(h.lut_get_coefficients(model.id) - lo.reference_twin().c).max()
    assert err <= TOL * lo.reference_table().max()


# ---- evaluation ---------------------------------------------------------------------------------------------------------
def _queries():
    rng = np.random.default_rng(5)
    off = np.sort(rng.uniform(NU[0], NU[-1], 3 * EVAL_BLOCK - 67))      # three workgroups, the last one partial
    mix = np.concatenate([NU[:1], off[:40], NU[30:33], NU[-1:]])
    return {
        "nodes": (NU, 431.7, 247.3),
        "off_node": (off, 431.7, 247.3),
        "first_nodes": (mix, P[0], T[0]),
        "last_nodes": (mix, P[-1], T[-1]),
        "interior_nodes": (mix, P[2], T[1]),
        "p_node_only": (off, P[3], 233.1),
        "descending": (off[::-1].copy(), 431.7, 247.3),
        "shuffled": (rng.permutation(off), 431.7, 247.3),
        "one_point": (np.array([12997.77]), 777.7, 205.0),
        "one_block_edge": (off[:EVAL_BLOCK], 210.0, 289.0),
        "one_past_block_edge": (off[:EVAL_BLOCK + 1], 210.0, 289.0),
    }


QUERIES = _queries()


@pytest.mark.parametrize("name", list(QUERIES))
def test_xsec_matches_the_twin(h, model, name):
    nu, p, t = QUERIES[name]
    sig = h.lut_xsec(model.id, nu, p, t)
    ref = lo.reference_twin().evaluate(nu, p, t)
    err = np.abs(sig - ref).max()
    print(f"xsec {name}: {err / lo.reference_table().max():.2e} max sigma")
    assert sig.shape == ref.shape and err <= TOL * lo.reference_table().max()


def test_the_two_forms_add_the_same_terms(h, model):
    """the staged form (monotone nu) and the 64-tap form (any order) give the same bits"""
    nu, p, t = QUERIES["shuffled"]
    order = np.argsort(nu)
    assert np.array_equal(h.lut_xsec(model.id, nu, p, t)[order], h.lut_xsec(model.id, nu[order], p, t))
    a, Ja = h.lut_xsec(model.id, nu, p, t, jacobian=True)
    b, Jb = h.lut_xsec(model.id, nu[order], p, t, jacobian=True)
    assert np.array_equal(a[order], b) and np.array_equal(Ja[order], Jb)


def test_queries_coarser_than_the_tile(h):
    """a workgroup whose outputs span more contracted-row entries than the tile holds takes the 64-tap form: same values"""
    n_nu = SUPER + 3
    assert n_nu > 2 * EVAL_TILE
    tab = lo.synthetic_table(n_nu, 3, 3, seed=21)
    rng3 = ((100.0, 0.25, n_nu), (0.0, 1.0, 3), (0.0, 2.0, 3))
    twin = lo.LutTwin(tab, *rng3)
    nu = np.sort(np.random.default_rng(2).uniform(100.0, 100.0 + 0.25 * (n_nu - 1), 300))
    lut = h.lut_create(*rng3)
    try:
        h.lut_set_table(lut, tab)
        sig, J = h.lut_xsec(lut, nu, 0.7, 3.1, jacobian=True)
    finally:
        h.lut_destroy(lut)
    ref, Jref = twin.evaluate(nu, 0.7, 3.1, jacobian=True)
    assert np.abs(sig - ref).max() <= TOL * tab.max()
    assert np.abs(J[:, 0] - Jref[:, 0]).max() <= TOL * tab.max() / 1.0 and np.abs(J[:, 1] - Jref[:, 1]).max() <= TOL * tab.max() / 2.0


def test_node_queries_return_the_line_by_line_sigma(h, model):
    tab = lo.reference_table()
    for i in (0, 2, P.size - 1):
        for j in (0, 1, T.size - 1):
            assert np.abs(h.lut_xsec(model.id, NU, P[i], T[j]) - tab[:, i, j]).max() <= TOL * tab.max()


# ---- Dual ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(QUERIES))
def test_jacobian_matches_the_twin(rtamd, h, model, name):
    nu, p, t = QUERIES[name]
    sig, J = rtamd.absorption.absorption_cross_section(model, nu, p, t, autodiff=True)
    assert np.array_equal(sig, rtamd.absorption.absorption_cross_section(model, nu, p, t))      # bitwise the value run
    ref, Jref = lo.reference_twin().evaluate(nu, p, t, jacobian=True)
    smax = lo.reference_table().max()
    err = [np.abs(J[:, k] - Jref[:, k]).max() / (smax / step) for k, step in enumerate((lo.P_RANGE[1], lo.T_RANGE[1]))]
    print(f"jacobian {name}: {err[0]:.2e} max sigma / p_step, {err[1]:.2e} max sigma / t_step")
    assert J.shape == (nu.size, 2) and max(err) <= TOL


# ---- device build -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("broadening", ["Voigt()", "Lorentz()"])
def test_device_build_is_the_profile_kernels_at_the_nodes(rtamd, h, broadening):
    ab, L = rtamd.absorption, rtamd._lib
    lines = lo.o2a_lines()
    pz, tz = np.tile(P, T.size), np.repeat(T, P.size)                   # node z = i + nP j
    # a table of the handle that the build must leave alone
    h.absorption_set_model(*ab.absorption_model(broadening))
    h.absorption_begin(pz.size, NU)
    ab.resident_line_table(h, lines, NU, lo.WING)
    h.voigt_tau_abs_profile(pz, tz, 0.0, lo.WING, np.ones(pz.size))
    tau = h.absorption_get()
    tables = []
    try:
        for batch in (0, 3):                                            # every node in one batch; seven batches, the last one short
            h.set_option(L.MOM_OPT_LUT_BATCH, batch)
            m = ab.make_interpolation_model(h, lines, broadening, lo.NU_RANGE, lo.P_RANGE, lo.T_RANGE, wing_cutoff=lo.WING)
            tables.append(h.lut_get_table(m.id))
            assert (m.mol, m.iso) == (7, 1) and len(m.build_ms) == 2
            c = h.lut_get_coefficients(m.id)
            m.close()
    finally:
        h.set_option(L.MOM_OPT_LUT_BATCH, 0)
    assert np.array_equal(tables[0], tables[1])
    assert np.array_equal(h.absorption_get(), tau)                      # tau_abs untouched ...
    h.voigt_tau_abs_profile(pz, tz, 0.0, lo.WING, np.ones(pz.size))     # ... and the grid and Nz: the same call adds the same again
    assert np.array_equal(h.absorption_get(), tau + tau)
    for j in range(T.size):
        for i in range(P.size):
            assert np.array_equal(tables[0][:, i, j], tau[:, i + P.size * j]), (i, j)
    assert np.abs(c - lo.coefficients(tables[0])).max() <= TOL * tables[0].max()
    if broadening == "Voigt()":
        ref = lo.reference_table()
        assert np.abs(tables[0] - ref).max() <= 1e-9 * ref.max()       # the bar of the device-prefactor test
    else:
        assert np.abs(tables[0] - lo.reference_table()).max() > 1e-3 * tables[0].max()     # another line shape
    h.absorption_set_model()


# ---- profile ------------------------------------------------------------------------------------------------------------
PROF_P = np.array([431.7, 437.0, 777.7])       # layers 1 and 2 in one (p, T) cell
PROF_T = np.array([247.3, 251.0, 205.0])
PROF_VCD, PROF_VMR = np.array([1.1e23, 2.4e24, 7.7e24]), 0.21


def test_profile_value_dual_and_accumulation(rtamd):
    ab = rtamd.absorption
    grid = np.sort(np.random.default_rng(9).uniform(NU[0], NU[-1], 2 * EVAL_BLOCK + 44))
    twin, smax = lo.reference_twin(), lo.reference_table().max()
    f = PROF_VCD * PROF_VMR
    ref = [twin.evaluate(grid, p, t, jacobian=True) for p, t in zip(PROF_P, PROF_T)]
    sig = np.stack([r[0] for r in ref], axis=1) * f                                         # [S, Nz]
    dsig = np.stack([np.stack([r[1][:, k] for r in ref], axis=1) * f for k in range(2)])     # [2, S, Nz]
    steps = (lo.P_RANGE[1], lo.T_RANGE[1])
    with rtamd.Handle(4, 1, grid.size, 1) as h:
        m = ab.interpolation_model_from_table(h, lo.reference_table(), lo.NU_RANGE, lo.P_RANGE, lo.T_RANGE)
        assert (m.mol, m.iso) == (-1, -1)
        # value call
        ab.compute_absorption_profile(h, m, grid, PROF_P, PROF_T, PROF_VCD, PROF_VMR)
        tau = h.absorption_get()
        assert np.abs(tau - sig).max() <= TOL * smax * f.max()
        with pytest.raises(rtamd.MomError):
            h.absorption_get_partials()                                 # no Dual call yet
        # Dual call on a fresh table
        ab.compute_absorption_profile(h, m, grid, PROF_P, PROF_T, PROF_VCD, PROF_VMR, dual=True)
        assert np.array_equal(h.absorption_get(), tau)
        dtau = h.absorption_get_partials()
        for k in range(2):
            assert np.abs(dtau[k] - dsig[k]).max() <= TOL * smax * f.max() / steps[k]
        # a value call after it: tau_abs doubles, dtau_abs stays
        ab.compute_absorption_profile(h, m, grid, PROF_P, PROF_T, PROF_VCD, PROF_VMR, begin=False)
        assert np.array_equal(h.absorption_get(), tau + tau) and np.array_equal(h.absorption_get_partials(), dtau)
        # on top of a line-by-line absorber
        lines = lo.o2a_lines()
        ab.compute_absorption_profile(h, lines, grid, PROF_P, PROF_T, PROF_VCD, PROF_VMR, wing_cutoff=lo.WING, device_prefactors=True,
                                      dual=True)
        a, da = h.absorption_get(), h.absorption_get_partials()
        ab.compute_absorption_profile(h, m, grid, PROF_P, PROF_T, PROF_VCD, PROF_VMR, begin=False, dual=True)
        b, db = h.absorption_get(), h.absorption_get_partials()
        assert np.abs((b - a) - sig).max() <= TOL * smax * f.max() + 2.3e-16 * b.max()
        for k in range(2):
            assert np.abs((db[k] - da[k]) - dsig[k]).max() <= TOL * smax * f.max() / steps[k] + 2.3e-16 * np.abs(db[k]).max()
        # the partials feed the Dual run unchanged
        part = ab.optics_partials(b + 0.05, np.full_like(b, 0.9), db[1])
        assert part.dτ.shape == b.shape and np.all(np.isfinite(part.dϖ)) and np.any(part.dϖ != 0)


# ---- state and errors ---------------------------------------------------------------------------------------------------
def _raises(rtamd, code, text=None):
    class Ctx:
        def __enter__(self):
            self.cm = pytest.raises(rtamd.MomError)
            self.e = self.cm.__enter__()
            return self

        def __exit__(self, *a):
            out = self.cm.__exit__(*a)
            assert self.e.value.code == code, self.e.value
            assert text is None or text in str(self.e.value), self.e.value
            return out
    return Ctx()


def test_create_refuses_short_axes_and_bad_steps(rtamd, h):
    L = rtamd._lib
    ok = [(100.0, 0.25, 5), (0.0, 1.0, 3), (0.0, 2.0, 3)]
    for axis, name in enumerate(("nu", "p", "T")):
        first, step, _ = ok[axis]
        for bad in ((first, step, 2), (first, 0.0, 3), (first, -1.0, 3)):
            rng = list(ok)
            rng[axis] = bad
            with _raises(rtamd, L.MOM_EINVAL, f"the {name} axis"):
                h.lut_create(*rng)


def test_ids_states_and_ranges(rtamd, h, model, tmp_path):
    L, ab = rtamd._lib, rtamd.absorption
    one = np.ones(1)
    # a wrong id and a destroyed one
    dead = h.lut_create(lo.NU_RANGE, lo.P_RANGE, lo.T_RANGE)
    h.lut_destroy(dead)
    for bad in (99, -1, dead):
        for call in (lambda: h.lut_xsec(bad, NU[:1], P[0], T[0]), lambda: h.lut_destroy(bad), lambda: h.lut_build(bad),
                     lambda: h.lut_get_coefficients(bad), lambda: h.lut_get_table(bad),
                     lambda: h.lut_tau_abs_profile(bad, one * P[0], one * T[0], one),
                     lambda: h.lut_tau_abs_profile(bad, one * P[0], one * T[0], one, dual=True)):
            with _raises(rtamd, L.MOM_EINVAL, "not a live table id"):
                call()
        assert h.lib.mom_lut_set_table(h._h, bad, L.dp(np.zeros(8))) == L.MOM_EINVAL
    # a table without coefficients
    empty = h.lut_create(lo.NU_RANGE, lo.P_RANGE, lo.T_RANGE)
    assert empty == dead                                             # the freed id is handed out again
    h.absorption_begin(1, NU)
    for call in (lambda: h.lut_xsec(empty, NU[:1], P[0], T[0]), lambda: h.lut_get_coefficients(empty), lambda: h.lut_get_table(empty),
                 lambda: h.lut_tau_abs_profile(empty, one * P[0], one * T[0], one)):
        with _raises(rtamd, L.MOM_ESTATE):
            call()
    # ... works once it has a table, and answers independently of the other live table
    other = 3.0 * lo.reference_table()
    h.lut_set_table(empty, other)
    nu, p, t = QUERIES["off_node"]
    a, b = h.lut_xsec(model.id, nu, p, t), h.lut_xsec(empty, nu, p, t)
    assert np.abs(b - 3.0 * a).max() <= TOL * other.max() and np.array_equal(a, h.lut_xsec(model.id, nu, p, t))
    ids = [h.lut_create(lo.NU_RANGE, lo.P_RANGE, lo.T_RANGE) for _ in range(8)]       # ten alive at once
    assert len(set(ids + [model.id, empty])) == 10
    for k in ids + [empty]:
        h.lut_destroy(k)
    # outside the axes: the library's text names the axis, Python raises ValueError; the end points are inside (tested above)
    for q, axis in (((np.array([NU[3], NU[0] - 1e-9]), P[1], T[1]), "nu"), ((np.array([NU[-1] + 1e-9]), P[1], T[1]), "nu"),
                    ((NU[:2], P[0] - 1e-9, T[1]), "p"), ((NU[:2], P[-1] + 1e-9, T[1]), "p"), ((NU[:2], P[1], T[0] - 1e-9), "T"),
                    ((NU[:2], P[1], T[-1] + 1e-9), "T"), ((NU[:2], float("nan"), T[1]), "p")):
        with _raises(rtamd, L.MOM_EINVAL, f"the table's {axis} axis"):
            h.lut_xsec(model.id, *q)
        with pytest.raises(ValueError, match=f"{axis} axis"):
            ab.absorption_cross_section(model, *q)
    with _raises(rtamd, L.MOM_EINVAL, "the table's p axis"):
        h.lut_tau_abs_profile(model.id, one * 1e4, one * T[1], one)
    with _raises(rtamd, L.MOM_EINVAL, "the table's T axis"):
        h.lut_tau_abs_profile(model.id, one * P[1], one * 10.0, one, dual=True)
    with pytest.raises(ValueError, match="T axis"):
        ab.compute_absorption_profile(h, model, NU, one * P[1], one * 10.0, one, 1.0)
    h.absorption_begin(1, NU + 0.5)                                   # a grid that leaves the nu range
    with _raises(rtamd, L.MOM_EINVAL, "the table's nu axis"):
        h.lut_tau_abs_profile(model.id, one * P[1], one * T[1], one)
    with _raises(rtamd, L.MOM_EINVAL, "bad argument"):
        h.lut_tau_abs_profile(model.id, P[:2], T[:2], np.ones(2))     # more layers than the table of mom_absorption_begin
    # save -> load -> evaluate
    path = tmp_path / "model.npz"
    ab.save_interpolation_model(model, path)
    back = ab.load_interpolation_model(h, path)
    assert (back.mol, back.iso, back.ν_grid, back.p_grid, back.t_grid) == (7, 1, model.ν_grid, model.p_grid, model.t_grid)
    s0, J0 = ab.absorption_cross_section(model, nu, p, t, autodiff=True)
    s1, J1 = ab.absorption_cross_section(back, nu, p, t, autodiff=True)
    assert back.id != model.id and np.array_equal(s0, s1) and np.array_equal(J0, J1)
    back.close()


def test_profile_and_build_need_their_inputs(rtamd):
    L, ab = rtamd._lib, rtamd.absorption
    with rtamd.Handle(4, 1, NU.size, 1) as h:
        m = ab.interpolation_model_from_table(h, lo.reference_table(), lo.NU_RANGE, lo.P_RANGE, lo.T_RANGE)
        with _raises(rtamd, L.MOM_ESTATE, "mom_absorption_begin"):
            h.lut_tau_abs_profile(m.id, P[:1], T[:1], np.ones(1))
        with _raises(rtamd, L.MOM_ESTATE, "mom_absorption_set_lines"):
            h.lut_build(m.id)
        # the T axis leaves the TIPS-2017 tables: the error of the line-by-line path
        with _raises(rtamd, L.MOM_EINVAL, "TIPS2017"):
            ab.make_interpolation_model(h, lo.o2a_lines(), "Voigt()", lo.NU_RANGE, lo.P_RANGE, (0.5, 30.0, 4), wing_cutoff=lo.WING)
        # the failed build left no table behind, and the first one still answers
        assert h.lut_create(lo.NU_RANGE, lo.P_RANGE, lo.T_RANGE) == m.id + 1
        assert np.abs(h.lut_xsec(m.id, NU, P[1], T[1]) - lo.reference_table()[:, 1, 1]).max() <= TOL * lo.reference_table().max()
