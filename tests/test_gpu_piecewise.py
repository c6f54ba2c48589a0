"""
GPU tests of the piecewise-stationary kernel through the public interface (markovflow_amd/kernels.py: PiecewiseKernel;
GaussianProcessRegression and its posterior): the chain's marginals, the GPR log marginal likelihood, its backward and its
predictions against the dense references of tests/helpers/piecewise_closed_forms.py (the joint covariance of the chain by recursion;
none of it touches Kalman code).

The change points are themselves time points of every series and of the merged prediction grid, so that no transition crosses one
and the dense reference is the exact law of the process.  Tolerances are those of tests/test_gpu_kernels_periodic.py.
"""
import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from helpers import piecewise_closed_forms as PW
from helpers import piecewise_kernels as PK

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BSZ, T = 3, 40
NOISE = 0.1


def tt(x, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device=DEV)


def nn(x):
    return x.detach().cpu().numpy().astype(np.float64)


def qp(order, osc, ls, var, period):
    return {"order": order, "ls": ls, "var": var, "period": period, "osc": osc}


def m(order, ls, var):
    return {"order": order, "ls": ls, "var": var, "osc": 0}


# two or three segments with clearly different hyper-parameters
CASES = {
    "matern32_3seg": ([[m(3, 0.4, 1.5)], [m(3, 1.6, 0.3)], [m(3, 0.15, 2.5)]], [2.0, 4.0]),
    "m52xho_2seg": ([[qp(5, 2, 0.7, 1.3, 1.7)], [qp(5, 2, 0.25, 0.4, 0.6)]], [3.0]),
    "const_m12_3seg": ([[{"order": 0, "var": 0.5, "osc": 0}, m(1, 0.5, 1.0)], [{"order": 0, "var": 1.5, "osc": 0}, m(1, 2.0, 0.2)],
                        [{"order": 0, "var": 0.1, "osc": 0}, m(1, 0.2, 3.0)]], [2.0, 4.0]),
}


def times(rng, cps, bsz=BSZ, n=T, start=0.0, min_gap=0.049):
    """Increasing time points in [start, 6) of which the change points beyond ``start`` are members: every segment starts with its
    left end and holds its share of the points, one per cell of an even grid, away from the cell's ends (gaps of at least 0.05, as in
    tests/test_gpu_kernels_periodic.py: below that Q = Pinf - A Pinf A^T of a Matern-5/2 block loses its pivots to cancellation)."""
    edges = [start] + [c for c in cps if c > start] + [6.0]
    nseg = len(edges) - 1
    counts = [n // nseg + (1 if k < n % nseg else 0) for k in range(nseg)]
    parts = []
    for lo, hi, m_k in zip(edges[:-1], edges[1:], counts):
        cell = (hi - lo) / m_k
        inner = lo + (np.arange(1, m_k) + 0.35 + 0.3 * rng.random((bsz, m_k - 1))) * cell
        parts += [np.full((bsz, 1), lo), inner]
    t = np.concatenate(parts, axis=-1)
    assert np.all(np.diff(t, axis=-1) >= min_gap)
    return t


def count_calls(monkeypatch):
    seen = []
    real = _lib.call

    def spy(name, *args):
        seen.append(name)
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", spy)
    return seen


def gpr_of(segments, cps, t, y, jitter=0.0, leaves=None, noise=None):
    kern = PK.build(segments, cps, jitter=jitter, device=DEV, leaves=leaves)
    chol = tt(np.sqrt(NOISE) * np.eye(1)) if noise is None else noise.reshape(1, 1)
    return mfa.GaussianProcessRegression((tt(t), tt(y)), kern, chol_obs_covariance=chol)


# ---- 1. the chain ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_state_space_model_marginals_vs_recursion(rng, case):
    segments, cps = CASES[case]
    jitter = 1e-6
    t = times(rng, cps)
    kern = PK.build(segments, cps, jitter=jitter, device=DEV)
    ssm = kern.state_space_model(tt(t))
    assert ssm.state_dim == kern.state_dim and tuple(ssm.batch_shape) == (BSZ,)
    _, covs = ssm.marginals
    for s in range(BSZ):
        a_ref, q_ref, _, _ = PW.transitions(segments, cps, t[s, :-1], np.diff(t[s]), jitter=jitter)
        np.testing.assert_allclose(nn(ssm.state_transitions)[s], a_ref, rtol=1e-10, atol=1e-12)
        chol = nn(ssm.cholesky_process_covariances)[s]
        np.testing.assert_allclose(chol @ np.swapaxes(chol, -1, -2), q_ref, rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(nn(covs)[s], PW.state_marginals(segments, cps, t[s], jitter=jitter), rtol=1e-8, atol=1e-10)
    assert not nn(ssm.state_offsets).any() and not nn(ssm.initial_mean).any()


# ---- 2. the log marginal likelihood ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_gpr_log_likelihood_vs_dense_gp(rng, monkeypatch, case):
    """Fails if a fused route silently took segment 0's hyper-parameters: the materialised route (generator -> KalmanFilter) runs."""
    segments, cps = CASES[case]
    jitter = 1e-6 if case == "const_m12_3seg" else 0.0          # (an order-0 component needs a jitter: see Constant)
    t, y = times(rng, cps), rng.normal(size=(BSZ, T, 1))
    gpr = gpr_of(segments, cps, t, y, jitter=jitter)
    assert gpr._fused_log_likelihood_per_series() is None and gpr._fused_posterior_chain() is None
    ran = []
    real = mfa.models.KalmanFilter.log_likelihood
    monkeypatch.setattr(mfa.models.KalmanFilter, "log_likelihood", lambda self: ran.append(1) or real(self))
    seen = count_calls(monkeypatch)
    got = float(gpr.log_likelihood().cpu())
    assert ran == [1] and seen.count("mf_sde_piecewise_transitions") == 1
    assert "mf_sde_transitions" not in seen and "mf_sde_matern_transitions" not in seen
    want = sum(PW.dense_log_marginal(segments, cps, t[s], y[s, :, 0], NOISE, jitter=jitter) for s in range(BSZ))
    first_only = sum(PW.dense_log_marginal(segments[:1], [], t[s], y[s, :, 0], NOISE, jitter=jitter) for s in range(BSZ))
    print(f"{case}: state space {got!r}, dense {want!r}, rel {abs(got - want) / abs(want):.2e}; segment 0 everywhere: {first_only!r}")
    assert got == pytest.approx(want, rel=1e-8)
    assert abs(first_only - want) > 1e-3 * abs(want)              # (the two differ by far more than the tolerance)


def test_gpr_log_likelihood_per_series_hyperparameters(rng):
    cps = [2.0, 4.0]
    ls, var = 0.3 + rng.random((3, BSZ)), 0.5 + rng.random((3, BSZ))
    per = [[m(3, ls[k], var[k])] for k in range(3)]
    t, y = times(rng, cps), rng.normal(size=(BSZ, T, 1))
    got = float(gpr_of(per, cps, t, y).log_likelihood().cpu())
    want = sum(PW.dense_log_marginal([[m(3, ls[k, s], var[k, s])] for k in range(3)], cps, t[s], y[s, :, 0], NOISE) for s in range(BSZ))
    assert got == pytest.approx(want, rel=1e-8)


# ---- 3. its backward ---------------------------------------------------------------------------------------------------------------------
def dense_log_marginal_torch(kern, t, y, noise_chol):
    """The dense log marginal of one series in differentiable torch ops (CPU): K_ff from the torch-route transitions by recursion."""
    a_s, q_s = kern.transition_statistics_from_time_points(t)
    n, d = t.shape[0], kern.state_dim
    h = kern.generate_emission_model(t[:1]).emission_matrix.reshape(d)
    marg = [kern.initial_covariance(t[:1]).reshape(d, d)]
    for k in range(n - 1):
        marg.append(a_s[k] @ marg[-1] @ a_s[k].T + q_s[k])
    cols = []
    for i in range(n):
        u = marg[i] @ h
        col = [torch.zeros((), dtype=t.dtype)] * i + [h @ u]
        for j in range(i + 1, n):
            u = a_s[j - 1] @ u
            col.append(h @ u)
        cols.append(torch.stack(col))
    low = torch.tril(torch.stack(cols, dim=1))
    kff = low + torch.tril(low, -1).T
    kn = kff + noise_chol ** 2 * torch.eye(n, dtype=t.dtype)
    return -0.5 * (y @ torch.linalg.solve(kn, y) + torch.linalg.slogdet(kn)[1] + n * np.log(2 * np.pi))


@pytest.mark.parametrize("case", ["matern32_3seg", "m52xho_2seg"])
def test_gpr_backward_vs_cpu_autograd(rng, monkeypatch, case):
    """log_likelihood().backward() through the HIP generator's reverse mode against CPU autograd through the torch route and the
    dense marginal likelihood: every segment's leaves receive their gradient."""
    segments, cps = CASES[case]
    t, y = times(rng, cps), rng.normal(size=(BSZ, T))
    cpu_leaves, noise_c = [], torch.tensor(np.sqrt(NOISE), dtype=torch.float64, requires_grad=True)
    kern_c = PK.build(segments, cps, leaves=cpu_leaves)
    total = sum(dense_log_marginal_torch(kern_c, torch.tensor(t[s]), torch.tensor(y[s]), noise_c) for s in range(BSZ))
    total.backward()
    dev_leaves, noise_d = [], torch.tensor(np.sqrt(NOISE), dtype=torch.float64, device=DEV, requires_grad=True)
    gpr = gpr_of(segments, cps, t, y[..., None], leaves=dev_leaves, noise=noise_d)
    seen = count_calls(monkeypatch)
    ll = gpr.log_likelihood()
    ll.backward()
    assert seen.count("mf_sde_piecewise_transitions") == 1 and seen.count("mf_sde_piecewise_transitions_grad") == 1
    assert float(ll.detach()) == pytest.approx(float(total.detach()), rel=1e-8)
    assert len(dev_leaves) == len(cpu_leaves)
    for i, (g, c) in enumerate(zip(dev_leaves + [noise_d], cpu_leaves + [noise_c])):
        assert g.grad is not None and float(g.grad.abs()) > 0, f"leaf {i} received no gradient"
        np.testing.assert_allclose(nn(g.grad), c.grad.numpy(), rtol=1e-6, atol=1e-9, err_msg=f"leaf {i}")


# ---- 4. prediction -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["matern32_3seg", "m52xho_2seg"])
def test_posterior_predict_f_vs_dense_gp(rng, case):
    """New points inside every segment, between a change point and its neighbours among the training points and - for the
    Matern-only signature - before the first and beyond the last training point."""
    segments, cps = CASES[case]
    t, y = times(rng, cps), rng.normal(size=(BSZ, T, 1))
    rows = []
    for s in range(BSZ):
        new = []
        seg = PW.segment_index(t[s], cps)
        for k in range(len(cps) + 1):                   # inside every segment: the middle of two gaps between its training points
            inside = np.flatnonzero((seg[:-1] == k) & (seg[1:] == k))
            new += [0.5 * (t[s, i] + t[s, i + 1]) for i in rng.choice(inside, size=2, replace=False)]
        for c in cps:                                   # just before and just after a change point: inside the gaps next to it
            i = int(np.searchsorted(t[s], c))
            new += [0.5 * (t[s, i - 1] + c), 0.5 * (c + t[s, i + 1])]
        if case == "matern32_3seg":
            new += [t[s, 0] - 0.3, t[s, -1] + 0.2, t[s, -1] + 1.5]
        rows.append(np.sort(np.array(new)))
    t_new = np.stack(rows)
    gpr = gpr_of(segments, cps, t, y)
    f_mean, f_var = gpr.posterior.predict_f(tt(t_new))
    s_mean, s_cov = gpr.posterior.predict_state(tt(t_new))
    n_new, d = t_new.shape[-1], gpr.kernel.state_dim
    assert tuple(f_mean.shape) == (BSZ, n_new, 1) and tuple(f_var.shape) == (BSZ, n_new, 1)
    assert tuple(s_mean.shape) == (BSZ, n_new, d) and tuple(s_cov.shape) == (BSZ, n_new, d, d)
    for s in range(BSZ):
        mean, var = PW.dense_predict(segments, cps, t[s], y[s, :, 0], NOISE, t_new[s])
        np.testing.assert_allclose(nn(f_mean)[s, :, 0], mean, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(nn(f_var)[s, :, 0], var, rtol=1e-5, atol=1e-7)


# The rule for what lies before the first conditioning point - stationary under the kernel active AT that point - only shows when a
# new point lies before the first conditioning point in ANOTHER segment: series that start in segment 0, in the middle of segment 1
# and on the change point that opens segment 2, one prediction grid for all of them (the Matern-3/2 blocks stand the closer spacing
# of the late starters).
LATE_STARTS = (0.0, 2.9, 4.0)
COMMON_GRID = np.array([0.5, 1.7, 2.5, 3.3, 4.6, 5.2, 6.4])


def late_starters(rng):
    segments, cps = CASES["matern32_3seg"]
    t = np.concatenate([times(rng, cps, bsz=1, start=s0, min_gap=0.015) for s0 in LATE_STARTS])
    assert list(PW.segment_index(t[:, 0], cps)) == [0, 1, 2]
    return segments, cps, t, rng.normal(size=(BSZ, T, 1)), np.broadcast_to(COMMON_GRID, (BSZ, len(COMMON_GRID))).copy()


def test_predict_before_a_first_point_in_a_later_segment(rng):
    segments, cps, t, y, t_new = late_starters(rng)
    post = gpr_of(segments, cps, t, y).posterior
    f_mean, f_var = post.predict_f(tt(t_new))
    s_mean, s_cov = post.predict_state(tt(t_new))
    for s in range(BSZ):
        mean, var = PW.dense_predict(segments, cps, t[s], y[s, :, 0], NOISE, t_new[s])
        np.testing.assert_allclose(nn(f_mean)[s, :, 0], mean, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(nn(f_var)[s, :, 0], var, rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(nn(s_mean)[s, :, 0], mean, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(nn(s_cov)[s, :, 0, 0], var, rtol=1e-5, atol=1e-7)
    # far before the first point the prediction is the prior of the FIRST POINT's segment, not of the new point's (segment 0)
    pinf = [PW.steady_state(segments, cps, np.array([c]))[0, 0, 0] for c in (1.0, 3.0, 5.0)]
    assert nn(f_var)[2, 0, 0] == pytest.approx(pinf[2], rel=1e-3) and abs(pinf[2] - pinf[0]) > 0.3 * pinf[0]
    # ... and the rule is what the reference is built with: without it the dense value itself is another one
    grid = np.unique(np.concatenate([t[2], t_new[2]]))
    assert PW.dense_kff(segments, cps, grid)[0, 0] == pytest.approx(pinf[0])
    assert PW.dense_kff(segments, cps, grid, first=t[2, 0])[0, 0] == pytest.approx(pinf[2])


def test_sample_moments_agree_with_predict_state(rng):
    """sample_state / sample_f draw from the law predict_state reports, also before a first conditioning point that lies in a
    later segment: mean and variance of S = 4000 draws within 5 standard errors (sqrt(var / S) for the mean, var sqrt(2 / (S - 1))
    for the variance; the seed is fixed)."""
    segments, cps, t, y, t_new = late_starters(rng)
    post = gpr_of(segments, cps, t, y).posterior
    s_mean, s_cov = post.predict_state(tt(t_new))
    var = np.diagonal(nn(s_cov), axis1=-2, axis2=-1)
    num = 4000
    torch.manual_seed(1234)
    draws = nn(post.sample_state(tt(t_new), num))
    assert draws.shape == (num, BSZ, t_new.shape[-1], 2)
    assert np.all(np.abs(draws.mean(axis=0) - nn(s_mean)) <= 5.0 * np.sqrt(var / num))
    assert np.all(np.abs(draws.var(axis=0, ddof=1) - var) <= 5.0 * var * np.sqrt(2.0 / (num - 1)))
    torch.manual_seed(4321)
    f = nn(post.sample_f(tt(t_new), num))[..., 0]
    f_mean, f_var = (nn(x)[..., 0] for x in post.predict_f(tt(t_new)))
    assert np.all(np.abs(f.mean(axis=0) - f_mean) <= 5.0 * np.sqrt(f_var / num))
    assert np.all(np.abs(f.var(axis=0, ddof=1) - f_var) <= 5.0 * f_var * np.sqrt(2.0 / (num - 1)))


def test_posterior_samples(rng):
    segments, cps = CASES["matern32_3seg"]
    t, y = times(rng, cps), rng.normal(size=(BSZ, T, 1))
    t_new = np.sort(rng.random((BSZ, 5)) * 6.0, axis=-1)
    torch.manual_seed(0)
    f = gpr_of(segments, cps, t, y).posterior.sample_f(tt(t_new), 4)
    assert tuple(f.shape) == (4, BSZ, 5, 1) and bool(torch.isfinite(f).all())


# ---- 5. caches ---------------------------------------------------------------------------------------------------------------------------
def test_in_place_write_to_one_segments_lengthscale_is_seen(rng):
    segments, cps = CASES["matern32_3seg"]
    t, y = times(rng, cps), rng.normal(size=(BSZ, T, 1))
    gpr = gpr_of(segments, cps, t, y)
    before = float(gpr.log_likelihood().cpu())
    assert before == pytest.approx(float(gpr.log_likelihood().cpu()), rel=0, abs=0)
    with torch.no_grad():
        gpr.kernel.kernels[1].lengthscale.mul_(0.5)
    after = float(gpr.log_likelihood().cpu())
    changed = [[dict(c) for c in comps] for comps in segments]
    changed[1][0]["ls"] *= 0.5
    want = sum(PW.dense_log_marginal(changed, cps, t[s], y[s, :, 0], NOISE) for s in range(BSZ))
    assert after != before and after == pytest.approx(want, rel=1e-8)
    gpr.invalidate_hyperparameter_cache()
    assert float(gpr.log_likelihood().cpu()) == after


# ---- 6. unchanged behaviour --------------------------------------------------------------------------------------------------------------
def test_plain_matern_gpr_still_takes_the_fused_route(rng, monkeypatch):
    t, y = times(rng, [2.0]), rng.normal(size=(BSZ, T, 1))
    kern = mfa.Matern32(0.4, 1.5, device=DEV)
    gpr = mfa.GaussianProcessRegression((tt(t), tt(y)), kern, chol_obs_covariance=tt(np.sqrt(NOISE) * np.eye(1)))
    assert gpr._fused_log_likelihood_per_series() is not None
    seen = count_calls(monkeypatch)
    kern.state_space_model(tt(t))
    assert "mf_sde_matern_transitions" in seen and "mf_sde_piecewise_transitions" not in seen
