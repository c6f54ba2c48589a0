"""
CPU checks of the references the float32 block-tridiagonal tests rest on (tests/helpers/btd_fp32_closed_forms.py), in float64: every
form - sequential and partitioned, with every chunk length / radix the cases use - against the numpy restatement of the reference
(oracle.numpy_oracle) on the draws of the GPU tests, and against dense LAPACK on the assembled matrix where that is small; the
restated generators against the suite's; and that the committed yardstick table is what the cases and the script say.
"""
import numpy as np
import pytest

from oracle import numpy_oracle as O
from helpers import btd_fp32_closed_forms as F
from helpers import btd_fp32_cases as C
from helpers import btd_fp32_table as TABLE
from helpers.kl_closed_forms import tensor_error

OPERATORS = ("cholesky", "udl", "udl_eta", "solve", "inverse", "logdet_quad")
TOL = 1e-12


def every_plan(route, d, t, bsz):
    """None (sequential), the plans of every operator at this shape, and two that exercise ragged chunks on several levels."""
    found = {plan for op in OPERATORS for plan in C.plans(route, op, d, t, bsz)}
    return [None] + sorted(found, key=str) + ([(3, 2), (7, None)] if t > 3 else [])


def oracle_udl_extras(u_t, chol_d, eta):
    """m_post and chol(Delta^-1) the way oracle.numpy_oracle.kf_posterior_ssm forms them."""
    eye = np.broadcast_to(np.eye(chol_d.shape[-1]), chol_d.shape).copy()
    x = O.btd_solve(eye, u_t, eta, transpose_left=True)
    return O.btd_solve(chol_d, None, O.btd_solve(chol_d, None, x), transpose_left=True), np.linalg.cholesky(O._chol_solve(chol_d, eye))


@pytest.mark.parametrize("route,d,t,bsz", C.CASES)
def test_every_form_matches_the_oracle(route, d, t, bsz):
    diag, sub, x, eta = C.draw_spd(C.DEFAULT_SEED, d, t, bsz)
    ldiag, lsub, rhs = C.draw_factor(C.DEFAULT_SEED, d, t, bsz)
    want_l = O.btd_cholesky(diag, sub)
    want_quad = 0.5 * np.sum(O.btd_solve(*want_l, x) ** 2, axis=(-1, -2)) - O.btd_abs_log_det(want_l[0])
    want_inv = O.btd_block_diagonal_of_inverse(ldiag, lsub, return_sub=True)
    want_z = [O.btd_solve(ldiag, lsub, rhs, transpose_left=tr) for tr in (False, True)]
    if t > 1:
        want_u = O.btd_upper_diagonal_lower(diag, sub)
        want_u = want_u + oracle_udl_extras(*want_u, eta)
    for mode, (dg, sb) in enumerate(((ldiag, lsub), (ldiag, lsub), (diag, sub))):
        assert tensor_error(F.matvec(dg, sb, rhs, mode), O.btd_dense_mult(dg, sb, rhs, symmetric=mode == 2, transpose_left=mode == 1)) < TOL
    np.testing.assert_allclose(F.abs_log_det(ldiag), O.btd_abs_log_det(ldiag), rtol=TOL)
    for plan in every_plan(route, d, t, bsz):
        got = C.spd_forms(diag, sub, x, eta, np.float64, plan, plan, plan)
        assert tensor_error(got["chol.diag"], want_l[0]) < TOL, plan
        if t > 1:
            assert tensor_error(got["chol.sub"], want_l[1]) < TOL, plan
            for name, w in zip(("udl.u_t", "udl.chol_d"), want_u):
                assert tensor_error(got[name], w) < TOL, (plan, name)
            for name, w in zip(("eta.u_t", "eta.chol_d", "eta.m_post", "eta.chol_dinv"), want_u):
                assert tensor_error(got[name], w) < TOL, (plan, name)
        np.testing.assert_allclose(F.logdet_quad(diag, sub, x, plan), want_quad, rtol=TOL, atol=TOL * t * d)
        got = C.factor_forms(ldiag, lsub, rhs, np.float64, plan, plan)
        assert tensor_error(got["solve"], want_z[0]) < TOL and tensor_error(got["solve_t"], want_z[1]) < TOL, plan
        assert tensor_error(got["inv.diag"], want_inv[0]) < TOL, plan
        if t > 1:
            assert tensor_error(got["inv.sub"], want_inv[1]) < TOL, plan


@pytest.mark.parametrize("route,d,t,bsz", [c for c in C.CASES if c[2] <= 10])
def test_sequential_and_partitioned_forms_match_dense_lapack(route, d, t, bsz):
    diag, sub, x, eta = C.draw_spd(C.DEFAULT_SEED, d, t, bsz)
    ldiag, lsub, rhs = C.draw_factor(C.DEFAULT_SEED, d, t, bsz)
    dense, low = O.btd_to_dense(diag, sub, symmetric=True), O.btd_to_dense(ldiag, lsub, symmetric=False)
    flat = lambda v: v.reshape(bsz, t * d)                     # noqa: E731
    block = lambda m, i, j: m[:, i * d:(i + 1) * d, j * d:(j + 1) * d]          # noqa: E731
    inv = np.linalg.inv(low @ np.swapaxes(low, -1, -2))
    for plan in [None] + ([(2, 2), (3, None)] if t > 3 else []):
        got = C.spd_forms(diag, sub, x, eta, np.float64, plan, plan, plan)
        assert tensor_error(O.btd_to_dense(got["chol.diag"], got.get("chol.sub"), symmetric=False), np.linalg.cholesky(dense)) < TOL
        assert tensor_error(flat(got["sym.mult"]), (dense @ flat(x)[..., None])[..., 0]) < TOL
        if t > 1:
            # U D U^T = M with U^T unit lower block bidiagonal and D = chol_d chol_d^T; m_post = U^T M^-1 eta (the chain's offsets)
            u_low = O.btd_to_dense(np.broadcast_to(np.eye(d), diag.shape).copy(), got["eta.u_t"], symmetric=False)
            c_low = O.btd_to_dense(got["eta.chol_d"], None, symmetric=False)
            half = np.swapaxes(c_low, -1, -2) @ u_low
            assert tensor_error(np.swapaxes(half, -1, -2) @ half, dense) < TOL
            assert tensor_error(flat(got["eta.m_post"]), (u_low @ np.linalg.solve(dense, flat(eta)[..., None]))[..., 0]) < TOL
            q = got["eta.chol_dinv"] @ np.swapaxes(got["eta.chol_dinv"], -1, -2) @ got["eta.chol_d"] @ np.swapaxes(got["eta.chol_d"], -1, -2)
            assert tensor_error(q, np.broadcast_to(np.eye(d), q.shape).copy()) < TOL
        quad = 0.5 * np.sum(flat(x) * np.linalg.solve(dense, flat(x)[..., None])[..., 0], axis=-1) - 0.5 * np.linalg.slogdet(dense)[1]
        np.testing.assert_allclose(F.logdet_quad(diag, sub, x, plan), quad, rtol=TOL, atol=TOL * t * d)
        got = C.factor_forms(ldiag, lsub, rhs, np.float64, plan, plan)
        assert tensor_error(flat(got["solve"]), np.linalg.solve(low, flat(rhs)[..., None])[..., 0]) < TOL
        assert tensor_error(flat(got["solve_t"]), np.linalg.solve(np.swapaxes(low, -1, -2), flat(rhs)[..., None])[..., 0]) < TOL
        assert tensor_error(flat(got["mult"]), (low @ flat(rhs)[..., None])[..., 0]) < TOL
        assert tensor_error(flat(got["mult_t"]), (np.swapaxes(low, -1, -2) @ flat(rhs)[..., None])[..., 0]) < TOL
        np.testing.assert_allclose(got["logdet"], np.linalg.slogdet(low)[1], rtol=TOL, atol=TOL)
        for k in range(t):
            assert tensor_error(got["inv.diag"][:, k], block(inv, k, k)) < TOL
            if k + 1 < t:
                assert tensor_error(got["inv.sub"][:, k], block(inv, k + 1, k)) < TOL


def test_every_intermediate_keeps_float32():
    diag, sub, x, eta = (a.astype(np.float32) for a in C.draw_spd(C.DEFAULT_SEED, 3, 70, 2))
    ldiag, lsub, rhs = (a.astype(np.float32) for a in C.draw_factor(C.DEFAULT_SEED, 3, 70, 2))
    for plan in (None, (8, 5), (17, None)):
        outs = list(C.spd_forms(diag, sub, x, eta, np.float32, plan, plan, plan).values())
        outs += list(C.factor_forms(ldiag, lsub, rhs, np.float32, plan, plan).values()) + [F.logdet_quad(diag, sub, x, plan)]
        assert all(o.dtype == np.float32 for o in outs)


def test_the_restated_generators_are_the_suites():
    from test_gpu_block_tri_diag import random_spd_btd
    from test_gpu_btd_parallel import factor_and_matrix
    for d, t, bsz, has_sub in [(3, 4, 3, True), (6, 9, 2, False), (12, 5, 1, True), (1, 1, 2, False)]:
        want_d, want_s, _ = random_spd_btd(np.random.default_rng(5), (bsz,), t, d, has_sub, well=True)
        got_d, got_s = C.spd_btd(np.random.default_rng(5), bsz, t, d, has_sub)
        np.testing.assert_allclose(got_d, want_d, rtol=1e-14, atol=1e-15)
        assert (got_s is None) == (want_s is None)
        if has_sub:
            np.testing.assert_allclose(got_s, want_s, rtol=1e-14, atol=1e-15)
        want = factor_and_matrix(np.random.default_rng(6), (bsz,), t, d)
        got = C.factor_btd(np.random.default_rng(6), bsz, t, d)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert C.off_scale(15) == 0.3 and C.off_scale(12) == 0.3 and C.off_scale(48) == 0.15


def reduced_levels(t, len0=8, radix=C.PAR_RADIX):
    n, levels = -(-t // len0), 1
    while n > radix:
        n, levels = -(-n // radix), levels + 1
    return levels


def test_the_plans_cover_what_the_cases_claim():
    """The shapes cut the time axis where the routes' names say so: ragged tails, one to three reduced levels."""
    assert [C.plans(r, "cholesky", d, t, b) for r, d, t, b in C.CASES if r == "sweep"] == [[]] * 5
    for route in ("lane_par", "row_par"):
        assert all(C.plans(route, op, *shape) == [(8, C.PAR_RADIX)] for shape in C.ROUTES[route] for op in OPERATORS[:5])
    assert [C.plans("row", "cholesky", *s) for s in C.ROUTES["row"]] == [[], [], [(8, 5)], [(8, 5)]]
    assert C.plans("wave", "cholesky", 32, 130, 1)[0] == (17, None) and C.plans("wave", "solve", 32, 130, 1)[0] == (33, None)
    assert all(C.plans("panel", op, *shape) == [] for shape in C.ROUTES["panel"] for op in OPERATORS[:5])
    assert [reduced_levels(t) for t in (64, 70, 209, 777)] == [2, 2, 3, 3] and 70 % 8 and 209 % 8 and 777 % 8


def test_the_committed_table_covers_every_case_and_is_what_the_script_measures():
    assert set(TABLE.BTD) == set(C.CASES)
    for route, d, t, bsz in C.CASES:
        spd, factor = C.names_of(t)
        assert set(TABLE.BTD[(route, d, t, bsz)]) == set(spd) | set(factor)
    assert set(TABLE.NO_SUB) == set(C.NO_SUB_CASES) and all(set(v) == set(C.NO_SUB_NAMES) for v in TABLE.NO_SUB.values())
    assert set(TABLE.LOGDET_QUAD) == set(C.LOGDET_QUAD_CASES)
    every = [v for row in list(TABLE.BTD.values()) + list(TABLE.NO_SUB.values()) for v in row.values()] + list(TABLE.LOGDET_QUAD.values())
    # float32 has 24 bits: no yardstick below one rounding, none that would let half the digits go
    assert min(every) >= 0.99 * C.FP32_FLOOR and max(every) < 1e-5
    # cheap entries re-measured (BLAS / LAPACK builds may differ in the last place of a sum: a factor of three, not equality)
    for case in (("sweep", 3, 4, 3), ("lane_par", 3, 70, 2)):
        again = C.yardstick(*case)
        for name, v in TABLE.BTD[case].items():
            assert v / 3.0 <= again[name] <= 3.0 * v, (case, name)
    assert TABLE.LOGDET_QUAD[("sweep", 3, 4, 3)] / 3.0 <= C.logdet_quad_yardstick("sweep", 3, 4, 3) <= 3.0 * TABLE.LOGDET_QUAD[("sweep", 3, 4, 3)]
