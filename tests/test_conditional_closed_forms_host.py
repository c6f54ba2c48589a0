"""
CPU tests of tests/helpers/conditional_closed_forms.py - the reference tests/test_gpu_conditional_kernels.py and
tests/test_gpu_conditionals.py lean on - independently of the formulas it restates:

  (a) ``statistics`` against direct conditioning of the joint Gaussian of (x_-, x_t, x_+) on its two ends, in long double, by Gaussian
      elimination with partial pivoting (no Cholesky, no formula of the helper); the joint is built from a random marginal P_- of x_-,
      which the conditional must not depend on: two different P_-;
  (b) ``predict`` against the moments of [D E] applied to the dense pair marginal;
  (c) the float64 (and numpy float32) helper against the long-double helper: the worst ``|err| / (eps (magnitude + 1))`` stays below
      8, one eighth of the GPU tests' K = 64, so that the reference's own rounding cannot eat their tolerance.  Measured on the inputs
      of the GPU tests, d = 1..9: statistics 1.03 (float64) and 1.01 (float32, in units of float32's eps), predict 0.93 and 0.83; on
      the oracle's Matern transitions (signatures (1), (3), (5), (5,5), (1,3,5), (5,3,1), jitter 1e-10, gaps >= 0.3) 1.67;
  (d) ``posterior._predict_state_dense`` (the torch route of d > 9) on CPU tensors against ``predict``, end indices and N = 1 included.
"""
import numpy as np
import pytest
import torch

from markovflow_amd import posterior
from oracle import numpy_kernels as K
from helpers import conditional_closed_forms as CC

LD = np.longdouble
EPS64, EPS32 = 2.0 ** -52, 2.0 ** -23
REF_BOUND = 8.0                      # (c): one eighth of K_F64 = 64
DIMS = list(range(1, 10))


def _t(a):
    return np.swapaxes(a, -1, -2)


def solve_ld(a, b):
    """``a^-1 b`` in long double by Gaussian elimination with partial pivoting (numpy.linalg has no long double)."""
    a, b = np.array(a, dtype=LD), np.array(b, dtype=LD)
    n = a.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(a[k:, k])))
        a[[k, p]], b[[k, p]] = a[[p, k]], b[[p, k]]
        for r in range(k + 1, n):
            f = a[r, k] / a[k, k]
            a[r, k:] -= f * a[k, k:]
            b[r] -= f * b[k]
    x = np.zeros_like(b)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - a[k, k + 1:] @ x[k + 1:]) / a[k, k]
    return x


def worst_ratio(got, want, mag, eps):
    return float(np.max(np.abs(np.asarray(got, dtype=LD) - want) / (eps * (np.asarray(mag) + 1.0))))


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 5, 9])
def test_statistics_are_the_direct_conditional_of_the_joint_of_the_three_states(d):
    """x_t = A_mt x_- + q_1, x_+ = A_tp x_t + q_2 with x_- ~ N(0, P_-):
    Cov = [[P_-, ., .], [A_mt P_-, P_t, .], [A_tp A_mt P_-, A_tp P_t, A_tp P_t A_tp^T + Q_tp]], P_t = A_mt P_- A_mt^T + Q_mt.
    Both sides run in long double (eps 1.1e-19) on matrices whose condition numbers are below 1e3: 1e-15 is four digits of slack and
    still three digits below anything float64 could tell apart."""
    rng = np.random.default_rng(100 + d)
    n = 4
    a_mt, q_mt, a_tp, q_tp = (x.astype(LD) for x in CC.draw_statistics_inputs(rng, n, d))
    (d_m, e_m, t_m), _ = CC.statistics(a_mt, q_mt, a_tp, q_tp, dtype=LD)
    assert d_m.dtype == LD and t_m.dtype == LD
    for trial in range(2):                                               # the conditional does not depend on the marginal of x_-
        p_minus = CC._spd(rng, (n,), d).astype(LD) * (1.0 + 2.0 * trial)
        for i in range(n):
            p_t = a_mt[i] @ p_minus[i] @ a_mt[i].T + q_mt[i]
            k_tm, k_pm, k_pt = a_mt[i] @ p_minus[i], a_tp[i] @ a_mt[i] @ p_minus[i], a_tp[i] @ p_t
            k_pp = a_tp[i] @ p_t @ a_tp[i].T + q_tp[i]
            k_ends = np.block([[p_minus[i], k_pm.T], [k_pm, k_pp]])
            k_t_ends = np.hstack([k_tm, k_pt.T])                         # Cov(x_t, [x_-, x_+])
            want_p = solve_ld(k_ends, k_t_ends.T).T
            want_t = p_t - want_p @ k_t_ends.T
            assert float(np.max(np.abs(np.hstack([d_m[i], e_m[i]]) - want_p))) < 1e-15
            assert float(np.max(np.abs(t_m[i] - want_t))) < 1e-15
    assert np.array_equal(t_m, _t(t_m)), "T is returned symmetric"


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bsz,n,n_new,d", [(2, 4, 11, 3), (1, 1, 6, 2), (2, 3, 9, 9)])
def test_predict_is_the_projection_of_the_dense_pair_marginal(bsz, n, n_new, d):
    rng = np.random.default_rng(7 * d + n)
    case = CC.draw_predict_inputs(rng, bsz, n, n_new, d)
    assert all(set(case["idx"][b]) == set(range(n + 1)) for b in range(bsz)), "every insertion index, both ends included"
    for b in range(bsz):
        (mean, cov), (mag_mean, mag_cov) = CC.predict_series(case, b, dtype=LD)
        (d_m, e_m, t_m), _ = CC.statistics(*[case[k][b] for k in ("a_mt", "q_mt", "a_tp", "q_tp")], dtype=LD)
        for j, i in enumerate(case["idx"][b]):
            mu_m = case["means"][b, i - 1] if i > 0 else case["m0"][b]
            mu_p = case["means"][b, i] if i < n else case["m0"][b]
            p_m = case["covs"][b, i - 1] if i > 0 else case["p0"][b]
            p_p = case["covs"][b, i] if i < n else case["p0"][b]
            c = case["sub"][b, i - 1] if 0 < i < n else np.zeros((d, d))
            joint = np.block([[p_m, c.T], [c, p_p]]).astype(LD)
            if 0 < i < n:
                assert np.linalg.eigvalsh(joint.astype(np.float64)).min() > 0, "the drawn pair marginal is a covariance"
            proj = np.hstack([d_m[j], e_m[j]])
            want_mean = proj @ np.concatenate([mu_m, mu_p]).astype(LD)
            want_cov = t_m[j] + proj @ joint @ proj.T
            # two long-double evaluations of one polynomial in different orders: a few eps_ld of its magnitude
            assert np.all(np.abs(mean[j] - want_mean) <= 1e-17 * (mag_mean[j] + 1.0))
            assert np.all(np.abs(cov[j] - want_cov) <= 1e-17 * (mag_cov[j] + 1.0))
            assert np.all(mag_cov[j] >= np.abs(cov[j]).astype(np.float64) * (1 - 1e-12)), "a magnitude bounds its value"
        mean_only, mags_only = CC.predict_series(case, b, dtype=LD, with_cov=False)
        assert mean_only[1] is None and mags_only[1] is None and np.array_equal(mean_only[0], mean)


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------
def _rounded(arrays, ty):
    return [None if a is None else np.asarray(a).astype(ty).astype(np.float64) for a in arrays]


@pytest.mark.parametrize("ty,eps", [(np.float64, EPS64), (np.float32, EPS32)], ids=["f64", "f32"])
@pytest.mark.parametrize("d", DIMS)
def test_statistics_in_working_precision_against_long_double(d, ty, eps):
    ins = _rounded(CC.draw_statistics_inputs(np.random.default_rng(d), 193, d), ty)
    want, mags = CC.statistics(*ins, dtype=LD)
    got, mags_ty = CC.statistics(*ins, dtype=ty)
    assert all(g.dtype == ty for g in got) and all(m.dtype == np.float64 for m in mags_ty)
    for name, g, w, m in zip("DET", got, want, mags):
        ratio = worst_ratio(g, w, m, eps)
        print(f"RATIO helper {np.dtype(ty).name} statistics d={d} {name}: {ratio:.2f}")
        assert ratio <= REF_BOUND


@pytest.mark.parametrize("ty,eps", [(np.float64, EPS64), (np.float32, EPS32)], ids=["f64", "f32"])
@pytest.mark.parametrize("d", DIMS)
def test_predict_in_working_precision_against_long_double(d, ty, eps):
    case = CC.draw_predict_inputs(np.random.default_rng(50 + d), 3, 7, 43, d)
    case.update(zip(CC.PREDICT_KEYS, _rounded([case[k] for k in CC.PREDICT_KEYS], ty)))
    for b in range(3):
        want, mags = CC.predict_series(case, b, dtype=LD)
        got, _ = CC.predict_series(case, b, dtype=ty)
        for name, g, w, m in zip(("mean", "cov"), got, want, mags):
            ratio = worst_ratio(g, w, m, eps)
            print(f"RATIO helper {np.dtype(ty).name} predict d={d} series {b} {name}: {ratio:.2f}")
            assert ratio <= REF_BOUND


@pytest.mark.parametrize("sig", [(1,), (3,), (5,), (5, 5), (1, 3, 5), (5, 3, 1)])
def test_statistics_on_matern_transitions_with_gaps_of_at_least_0_3_against_long_double(sig):
    """The conditioning of Q_tp + A_tp Q_mt A_tp^T of a Matern-5/2 block grows as the gaps shrink; at gaps >= 0.3 the float64 helper
    still keeps its distance from the GPU tests' bound."""
    rng = np.random.default_rng(len(sig))
    ls, var = [0.6 + 0.5 * j for j in range(len(sig))], [1.0 + 0.3 * j for j in range(len(sig))]
    to_t, from_t = 0.3 + rng.exponential(0.3, size=40), 0.3 + rng.exponential(0.3, size=40)
    a_mt, q_mt, _ = K.concat_transitions(sig, ls, var, to_t, jitter=1e-10)
    a_tp, q_tp, _ = K.concat_transitions(sig, ls, var, from_t, jitter=1e-10)
    want, mags = CC.statistics(a_mt, q_mt, a_tp, q_tp, dtype=LD)
    got, _ = CC.statistics(a_mt, q_mt, a_tp, q_tp, dtype=np.float64)
    for name, g, w, m in zip("DET", got, want, mags):
        ratio = worst_ratio(g, w, m, EPS64)
        print(f"RATIO helper float64 matern {sig} {name}: {ratio:.2f}")
        assert ratio <= REF_BOUND


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bsz,n,n_new,d", [(2, 4, 11, 3), (2, 1, 5, 3), (2, 3, 9, 12), (1, 1, 4, 12)])
def test_torch_composition_of_the_fused_kernel_against_the_numpy_statement(bsz, n, n_new, d):
    """``_predict_state_dense`` in float64 on the CPU (LAPACK Cholesky and triangular solves, batched products): the same bound as a
    float64 kernel, 64 eps (magnitude + 1)."""
    case = CC.draw_predict_inputs(np.random.default_rng(3 * d + n), bsz, n, n_new, d)
    assert all({0, n} <= set(case["idx"][b]) for b in range(bsz))
    tt = lambda a: None if a is None else torch.tensor(a, dtype=torch.float64)                       # noqa: E731
    mean, cov = posterior._predict_state_dense(torch.tensor(case["idx"]), *[tt(case[k]) for k in CC.PREDICT_KEYS])
    assert tuple(mean.shape) == (bsz, n_new, d) and tuple(cov.shape) == (bsz, n_new, d, d)
    for b in range(bsz):
        want, mags = CC.predict_series(case, b)
        for name, g, w, m in zip(("mean", "cov"), (mean[b].numpy(), cov[b].numpy()), want, mags):
            ratio = worst_ratio(g, w, m, EPS64)
            print(f"RATIO torch route d={d} N={n} series {b} {name}: {ratio:.2f}")
            assert ratio <= 64.0
