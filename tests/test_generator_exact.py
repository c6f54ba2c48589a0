"""
Host tests of the exact generator reference (tests/helpers/generator_exact.py, mpmath) and of the committed yardstick table
(tests/helpers/generator_fp_table.py): the reference is only worth something if it is right where it can be checked by other means.
"""
import math

import mpmath as mp
import numpy as np
import pytest
import torch

from helpers import generator_exact as E
from helpers import generator_fp_cases as C
from helpers import generator_fp_table as TABLE
from helpers import periodic_closed_forms as PC
from helpers import piecewise_kernels as PK

KINDS = C.KINDS + [(0, 1)]
LS, VAR, PERIOD = 0.7, 1.3, 1.7
CHECK_GAPS = (0.25, 0.5, 3.0)


def hyper(order):
    return (math.sqrt(order) / LS if order else 0.0), VAR, 2.0 * math.pi / PERIOD


def as_float(x):
    return np.array([[float(v) for v in row] for row in x])


@pytest.mark.parametrize("order,osc", KINDS)
def test_transition_is_the_matrix_exponential_of_the_feedback_matrix(order, osc):
    lam, var, omega = hyper(order)
    for gap in (2.0 ** -20, 0.25, 3.0):
        a = E.component(order, osc, lam, var, omega, gap, 0.0, False)["A"]
        with mp.workdps(E.DPS):
            want = mp.expm(E.feedback(order, osc, lam, omega) * mp.mpf(gap))
            worst = max(abs(want[i, j] - a[i][j]) for i in range(len(a)) for j in range(len(a)))
        assert worst < mp.mpf(10) ** -70


@pytest.mark.parametrize("order,osc", KINDS)
def test_stationary_covariance_is_stationary(order, osc):
    """F Pinf + Pinf F^T + (the diffusion) = 0 shows as Q(dt) -> Pinf for a long gap and Q(0) = 0: checked here through
    A Pinf A^T + Q = Pinf at a moderate gap, to 70 digits."""
    lam, var, omega = hyper(order)
    c = E.component(order, osc, lam, var, omega, 0.5, 0.0, False)
    if order == 0:
        assert all(x == 0 for row in c["Q"] for x in row)
        return
    with mp.workdps(E.DPS):
        a, p, q = mp.matrix(c["A"]), mp.matrix(c["Pinf"]), mp.matrix(c["Q"])
        rest = a * p * a.T + q - p
        assert max(abs(rest[i, j]) for i in range(a.rows) for j in range(a.rows)) < mp.mpf(10) ** -70
        assert min(mp.eigsy(q, eigvals_only=True)) > 0


def test_true_smallest_eigenvalue_at_a_short_gap():
    """The figure the module's docstring quotes: Matern-5/2, lengthscale 0.7, variance 1.3, dt = 2^-20."""
    lam, var, _ = hyper(5)
    q = E.component(5, 0, lam, var, 0.0, 2.0 ** -20, 0.0, False)["Q"]
    with mp.workdps(E.DPS):
        low = min(mp.eigsy(mp.matrix(q), eigvals_only=True))
    assert mp.mpf("1e-31") < low < mp.mpf("1e-29")


@pytest.mark.parametrize("order,osc", KINDS)
def test_agrees_with_the_float64_closed_forms_at_long_gaps(order, osc):
    lam, var, omega = hyper(order)
    comp = {"order": order, "osc": osc, "ls": LS, "var": VAR, "period": PERIOD}
    jitter = 1e-6
    for gap in CHECK_GAPS:
        a, q, p = PC.component_transitions(comp, np.array([gap]), jitter)
        c = E.component(order, osc, lam, var, omega, gap, jitter, False)
        np.testing.assert_allclose(a[0], as_float(c["A"]), rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(q[0], as_float(c["Q"]), rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(p, as_float(c["Pinf"]), rtol=1e-12, atol=1e-14)
        low = as_float(c["L"])
        np.testing.assert_allclose(low @ low.T, as_float(c["Q"]), rtol=1e-12, atol=1e-14)
        assert np.all(np.triu(low, 1) == 0)


@pytest.mark.parametrize("order,osc", KINDS)
def test_derivatives_agree_with_autograd_through_the_torch_closed_forms(order, osc):
    """ds/d(lam, var, omega) by mp.diff against float64 CPU autograd through ``_torch_transitions``, carried over from the kernels'
    leaves (lengthscale, the factors' variances, period) by the chain rule, at gaps where float64 does not cancel; the error is
    measured against the scale S."""
    lam, var, omega = hyper(order)
    comp = {"order": order, "osc": osc, "ls": LS, "var": VAR, "period": PERIOD}
    k = E.size(order, osc)
    rng = np.random.default_rng(C.DEFAULT_SEED)
    w_a, w_c = rng.normal(size=(k, k)), np.tril(rng.normal(size=(k, k)))
    jitter = 1e-6
    for gap in CHECK_GAPS:
        if order == 0 and not osc:          # A = [1], chol Q = sqrt(jitter): nothing depends on the variance, autograd has no graph
            _, ds, scale = E.weighted(E.component(order, osc, lam, var, omega, gap, jitter), w_a, w_c)
            assert all(ds[name] == 0 and scale[name] == 0 for name in E.PARAMS)
            continue
        leaves = []
        kern = PK.build([[comp]], [], jitter=jitter, leaves=leaves)
        a_s, chol, _ = kern._torch_transitions(torch.tensor([[gap]], dtype=torch.float64), True, False,
                                               torch.zeros((1, 1), dtype=torch.float64))
        (torch.sum(torch.tensor(w_a) * a_s[0, 0]) + torch.sum(torch.tensor(w_c) * chol[0, 0])).backward()
        grads = iter([0.0 if x.grad is None else float(x.grad) for x in leaves])
        got = {"lam": 0.0, "var": 0.0, "omega": 0.0}
        if order == 0:
            got["var"], g_p = next(grads), next(grads)
            got["omega"] = g_p / (-2.0 * math.pi / PERIOD ** 2)
        else:
            g_ls, g_var = next(grads), next(grads)
            if osc:
                _, g_p = next(grads), next(grads)
                g_var = g_var / PK.HO_VAR
                got["omega"] = g_p / (-2.0 * math.pi / PERIOD ** 2)
            got["lam"], got["var"] = g_ls / (-math.sqrt(order) / LS ** 2), g_var
        _, ds, scale = E.weighted(E.component(order, osc, lam, var, omega, gap, jitter), w_a, w_c)
        for name in E.PARAMS:
            if float(scale[name]) < 1e-60:
                assert got[name] == 0.0 or abs(got[name]) < 1e-12, (name, got[name])
                continue
            assert abs(got[name] - float(ds[name])) <= 1e-9 * float(scale[name]), (gap, name, got[name], float(ds[name]))


def test_prior_factor_and_its_derivatives():
    for order in C.PRIOR_ORDERS:
        lam, var, _ = hyper(order)
        pri = E.prior(order, lam, var, 1e-6)
        low = as_float(pri["L0"])
        p = PC.component_transitions({"order": order, "osc": 0, "ls": LS, "var": VAR, "period": None}, np.array([1.0]))[2]
        np.testing.assert_allclose(low @ low.T, p + 1e-6 * np.eye(len(p)), rtol=1e-12, atol=1e-14)
        h = 1e-6
        for name, (dl, dv) in {"lam": (h, 0.0), "var": (0.0, h)}.items():
            up, dn = E.prior(order, lam + dl, var + dv, 1e-6)["L0"], E.prior(order, lam - dl, var - dv, 1e-6)["L0"]
            np.testing.assert_allclose(as_float(pri["dL0"][name]), (as_float(up) - as_float(dn)) / (2 * h), rtol=1e-6, atol=1e-8)


def test_split_carries_the_reference_beyond_float64():
    with mp.workdps(E.DPS):
        x = mp.mpf(1) / 3
        hi, lo = E.split([[x]])
        assert abs(mp.mpf(float(hi[0, 0])) + mp.mpf(float(lo[0, 0])) - x) < mp.mpf(2) ** -100
    assert E.error(np.array([[1.0 / 3.0]]), [[x]])[0, 0] < 2.0 ** -54


# ---- the committed table -----------------------------------------------------------------------------------------------------------------
def test_table_has_every_key():
    assert set(TABLE.GENERATOR) == set(C.keys())
    for key, row in TABLE.GENERATOR.items():
        assert set(row) == set(C.FORWARD_NAMES + C.GRAD_NAMES), key
        assert all(v >= C.FLOOR[key[0]] * 0.99 for v in row.values())
    assert set(TABLE.PRIOR) == {(dt_name, order) for dt_name in C.DTYPES for order in C.PRIOR_ORDERS}
    assert set(TABLE.GPR) == set(C.GPR_SIGNATURES)


# one key per dtype and tensor, between them every kind of gap (zero, cancelling, moderate, long, 1e10) and of component
RECOMPUTED = [("f32", 3, 0, 2.0 ** -20, ("A", "Q0", "Q")), ("f32", 5, 1, 2.0 ** -7, ("LLt", "L", "g_lam", "g_var", "g_omega")),
              ("f32", 1, 2, 40.0, ("gA_lam", "gA_var", "gA_omega", "gC_lam", "gC_var")),
              ("f64", 5, 0, 2.0 ** -13, ("A", "Q0", "Q", "LLt", "L")), ("f64", 3, 2, 0.5, ("g_lam", "g_var", "g_omega", "gA_omega")),
              ("f64", 1, 0, 1e10, ("gA_lam", "gA_var", "gC_lam", "gC_var")), ("f64", 0, 0, 0.0, ("A", "Q"))]


@pytest.mark.parametrize("dt_name,order,osc,gap,names", RECOMPUTED)
def test_table_is_what_the_cases_compute(dt_name, order, osc, gap, names):
    yard = C.yardstick(dt_name, order, osc, gap, gaps=(gap,))
    row = TABLE.GENERATOR[(dt_name, order, osc, gap)]
    for name in names:
        assert f"{yard[name]:.2e}" == f"{row[name]:.2e}", (name, yard[name], row[name])


def test_table_prior_and_gpr_are_what_the_cases_compute():
    for key in [("f32", 5), ("f64", 3)]:
        yard = C.prior_yardstick(*key)
        assert {k: f"{v:.2e}" for k, v in yard.items()} == {k: f"{v:.2e}" for k, v in TABLE.PRIOR[key].items()}
    # (the oracle's factorisations go through LAPACK: builds may differ in the last place of a sum - a factor of three, not equality)
    sig = ("single", (3, 3))
    assert TABLE.GPR[sig] / 3.0 <= C.gpr_yardstick(sig) <= 3.0 * TABLE.GPR[sig]
