"""The numpy twin of the InterpolationModel (tests/lut_oracle.py) against an implementation that shares nothing with it:
scipy.interpolate.CubicSpline(bc_type="natural") applied axis by axis.  Along one axis the prefilter equations define the natural
cubic spline through the nodes, which is unique, and the axes commute.  No GPU.

Table: 40 synthetic O2-A lines on 97 x 5 x 4 dyadic nodes, filled by oracle/absref.py.  Tolerance: the project's Voigt parity figure,
1e-13 max|sigma| for values and 1e-13 max|sigma| / step for the partials; the measured distances stand next to each assertion."""
import numpy as np
import pytest
from scipy.interpolate import CubicSpline

import lut_oracle as lo

TOL = 1e-13


def scipy_eval(table, nu, p, T, d_p=0, d_t=0):
    """the natural spline along T, then p (each differentiated d_ times), then nu"""
    st = CubicSpline(lo.nodes(lo.T_RANGE), table, axis=2, bc_type="natural")
    a = (st.derivative(d_t) if d_t else st)(T)                                    # [nNu, nP]
    sp = CubicSpline(lo.nodes(lo.P_RANGE), a, axis=1, bc_type="natural")
    b = (sp.derivative(d_p) if d_p else sp)(p)                                    # [nNu]
    return CubicSpline(lo.nodes(lo.NU_RANGE), b, bc_type="natural")(nu)


def query_points():
    """(nu, p, T): off-node everywhere, the first node and the last node (delta = 1) of every axis, interior nodes"""
    nu_n, p_n, t_n = lo.nodes(lo.NU_RANGE), lo.nodes(lo.P_RANGE), lo.nodes(lo.T_RANGE)
    rng = np.random.default_rng(3)
    nu_off = np.sort(rng.uniform(nu_n[0], nu_n[-1], 61))
    nu_mix = np.concatenate([nu_n[:1], nu_n[-1:], nu_n[40:43], nu_off[:8]])
    return [(nu_off, 431.7, 247.3), (nu_mix, p_n[0], t_n[0]), (nu_mix, p_n[-1], t_n[-1]), (nu_mix, p_n[2], 233.1),
            (nu_mix, 777.7, t_n[1]), (nu_n, p_n[1], t_n[2]), (nu_off, p_n[0], t_n[-1])]


def test_dense_system_is_the_one_of_the_text():
    A = lo.padded_system(5)
    assert np.array_equal(A[0], [1, -2, 1, 0, 0, 0, 0]) and np.array_equal(A[6], [0, 0, 0, 0, 1, -2, 1])
    assert np.array_equal(A[3] * 6, [0, 0, 1, 4, 1, 0, 0])
    c = lo.prefilter_axis(np.array([1.0, 4.0, 9.0, 16.0, 25.0]), 0)
    # the first interior row minus the first boundary row: c_1 = f_1, and likewise at the other end
    assert abs(c[1] - 1.0) < 1e-14 and abs(c[5] - 25.0) < 1e-13
    assert abs(c[0] - 2 * c[1] + c[2]) < 1e-13 and abs(c[4] - 2 * c[5] + c[6]) < 1e-13


def test_twin_reproduces_the_nodes():
    tab, twin = lo.reference_table(), lo.reference_twin()
    worst = 0.0
    for i, p in enumerate(lo.nodes(lo.P_RANGE)):
        for j, T in enumerate(lo.nodes(lo.T_RANGE)):
            worst = max(worst, np.abs(twin.evaluate(lo.nodes(lo.NU_RANGE), p, T) - tab[:, i, j]).max())
    print(f"twin vs nodes: {worst / tab.max():.2e} max sigma")
    assert worst <= TOL * tab.max()          # measured 4.2e-16 max sigma


def test_twin_values_against_scipy():
    tab, twin = lo.reference_table(), lo.reference_twin()
    worst = 0.0
    for nu, p, T in query_points():
        worst = max(worst, np.abs(twin.evaluate(nu, p, T) - scipy_eval(tab, nu, p, T)).max())
    print(f"twin vs scipy, values: {worst / tab.max():.2e} max sigma")
    assert worst <= TOL * tab.max()          # measured 4.2e-16 max sigma


def test_twin_partials_against_scipy():
    tab, twin = lo.reference_table(), lo.reference_twin()
    worst = [0.0, 0.0]
    for nu, p, T in query_points():
        sig, J = twin.evaluate(nu, p, T, jacobian=True)
        assert np.array_equal(sig, twin.evaluate(nu, p, T))
        worst[0] = max(worst[0], np.abs(J[:, 0] - scipy_eval(tab, nu, p, T, d_p=1)).max())
        worst[1] = max(worst[1], np.abs(J[:, 1] - scipy_eval(tab, nu, p, T, d_t=1)).max())
    scale = [tab.max() / lo.P_RANGE[1], tab.max() / lo.T_RANGE[1]]
    print(f"twin vs scipy, d/dp: {worst[0] / scale[0]:.2e} max sigma / p_step, d/dT: {worst[1] / scale[1]:.2e} max sigma / t_step")
    assert worst[0] <= TOL * scale[0]        # measured 2.1e-16 max sigma / p_step
    assert worst[1] <= TOL * scale[1]        # measured 2.0e-16 max sigma / t_step


def test_partials_against_a_central_difference_of_the_twin():
    """the differentiated weights are the derivative of the weights: a sanity bar set by the difference (h^2 f''' / 6), not a parity"""
    twin, nu = lo.reference_twin(), lo.nodes(lo.NU_RANGE)[10:60] + 0.01
    p, T, hp, ht = 431.7, 247.3, 1e-3, 1e-4
    _, J = twin.evaluate(nu, p, T, jacobian=True)
    fd_p = (twin.evaluate(nu, p + hp, T) - twin.evaluate(nu, p - hp, T)) / (2 * hp)
    fd_t = (twin.evaluate(nu, p, T + ht) - twin.evaluate(nu, p, T - ht)) / (2 * ht)
    assert np.abs(J[:, 0] - fd_p).max() <= 1e-6 * np.abs(J[:, 0]).max()
    assert np.abs(J[:, 1] - fd_t).max() <= 1e-6 * np.abs(J[:, 1]).max()


@pytest.mark.parametrize("nu, p, T, axis", [(12994.9, 500.0, 250.0, "nu"), (13001.0625, 500.0, 250.0, "nu"), (12996.0, 199.9, 250.0, "p"),
                                            (12996.0, 800.1, 250.0, "p"), (12996.0, 500.0, 199.0, "T"), (12996.0, 500.0, 290.5, "T"),
                                            (float("nan"), 500.0, 250.0, "nu")])
def test_out_of_range_raises(nu, p, T, axis):
    with pytest.raises(ValueError, match=f"{axis} axis"):
        lo.reference_twin().evaluate(np.array([12996.0, nu]), p, T)


def test_end_points_are_inside():
    twin = lo.reference_twin()
    for rng in (lo.NU_RANGE,):
        first, step, n = rng
        twin.evaluate(np.array([first, first + step * (n - 1)]), lo.P_RANGE[0], lo.T_RANGE[0] + lo.T_RANGE[1] * (lo.T_RANGE[2] - 1))
