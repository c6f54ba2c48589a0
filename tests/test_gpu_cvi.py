"""
GPU tests of ``CVIGaussianProcess`` (markovflow_amd/models.py) against the dense CVI loop of
tests/helpers/likelihood_closed_forms.py: the same iteration on the kernel matrix, no state space form.

State space against dense: rtol 1e-6 / atol 1e-7, what tests/test_gpu_kernels_periodic.py uses for that comparison (prediction
variances: its rtol 1e-5).  The kernels carry jitter 0 and so does the dense loop.  Every series has at most 33 points.
(The comparisons of the model with the dense loop that need no particular device still need the filter, which is HIP only:
they are all here, the Bernoulli runs with seeds 0-5 at T = 7 and T = 33 included.)
"""
import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from markovflow_amd import likelihoods as ML
from helpers import likelihood_closed_forms as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = dict(rtol=1e-6, atol=1e-7)
M32 = [dict(order=3, ls=1.0, var=1.0, period=None, osc=0)]
M52_M32 = [dict(order=5, ls=1.3, var=0.8, period=None, osc=0), dict(order=3, ls=0.6, var=0.5, period=None, osc=0)]
RECORD = (1, 5, 25)


def tt(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64, device=DEV)


def nn(t):
    return t.detach().cpu().numpy()


def build_kernel(comps, lengthscales=None):
    cls = {1: mfa.Matern12, 3: mfa.Matern32, 5: mfa.Matern52}
    parts = [cls[c["order"]](c["ls"] if lengthscales is None else lengthscales[i], c["var"], device=DEV) for i, c in enumerate(comps)]
    return parts[0] if len(parts) == 1 else mfa.Sum(parts)


def build_likelihood(name):
    params = L.LIKELIHOODS[name][1]
    return {L.GAUSSIAN: lambda: mfa.Gaussian(params[0]), L.BERNOULLI: mfa.Bernoulli, L.POISSON: mfa.Poisson}[name]()


def build_model(name, comps, t, y, lr):
    return mfa.CVIGaussianProcess((tt(t), tt(y)[..., None]), build_kernel(comps), build_likelihood(name), learning_rate=lr)


_DENSE = {}


def dense_run(name, comps_key, num_points, seed, separated=False):
    """Data and the dense loop's record for one series: computed once, shared, not modified."""
    key = (name, comps_key, num_points, seed, separated)
    if key not in _DENSE:
        comps = {"m32": M32, "m52+m32": M52_M32}[comps_key]
        t, y = L.draw_series(L.LIKELIHOODS[name], comps, num_points, seed, separated=separated)
        rec, _ = L.dense_cvi(L.LIKELIHOODS[name], comps, t, y, lr=0.5, iterations=25, record=tuple(range(1, 26)))
        assert max(r["nat2"].max() for r in rec.values()) < 0.0, "every site precision of the reference run must be positive"
        _DENSE[key] = (comps, t, y, rec)
    return _DENSE[key]


def compare_with_dense(model, rec, where):
    np.testing.assert_allclose(nn(model.sites.nat1)[:, 0], rec["nat1"], err_msg=f"nat1 {where}", **TOL)
    np.testing.assert_allclose(nn(model.sites.nat2)[:, 0, 0], rec["nat2"], err_msg=f"nat2 {where}", **TOL)
    np.testing.assert_allclose(float(model.classic_elbo()), rec["classic_elbo"], err_msg=f"classic_elbo {where}", **TOL)
    np.testing.assert_allclose(float(model.elbo()), rec["elbo"], err_msg=f"elbo {where}", **TOL)
    # q through the natural parameters and q through the filter are one distribution
    q_mean, q_cov = model.dist_q.marginals
    f_mean, f_cov = model.posterior_kalman.posterior_state_space_model().marginals
    np.testing.assert_allclose(nn(q_mean), nn(f_mean), err_msg=f"marginal means {where}", **TOL)
    np.testing.assert_allclose(nn(q_cov), nn(f_cov), err_msg=f"marginal covariances {where}", **TOL)


def run_against_dense(name, comps_key, num_points, seed, separated=False):
    comps, t, y, rec = dense_run(name, comps_key, num_points, seed, separated)
    model = build_model(name, comps, t, y, lr=0.5)
    for it in range(1, 26):
        model.update_sites()
        if it in RECORD:
            compare_with_dense(model, rec[it], f"{name} T={num_points} seed={seed} iteration {it}")
    return model


def test_gaussian_likelihood_with_unit_learning_rate_is_gp_regression():
    """Well-separated time points: with uniform draws (two of the 33 points 9.5e-4 apart) and jitter 0 the cancellation in
    Q = P - A P A^T shows in BOTH routes - measured: dense -52.69496741, sites filter -52.69496750, fused GPR -52.69496787 -
    which says nothing about the model."""
    spec = L.LIKELIHOODS[L.GAUSSIAN]
    var = spec[1][0]
    for num_points in (7, 33):
        t, y = L.draw_series(spec, M32, num_points, seed=0, separated=True)
        model = build_model(L.GAUSSIAN, M32, t, y, lr=1.0)
        model.update_sites()
        # (1 - 1) nat + 1 g with the closed-form g: one division and one subtraction away from the data
        np.testing.assert_allclose(nn(model.sites.nat1)[:, 0], y / var, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(nn(model.sites.nat2)[:, 0, 0], np.full(num_points, -0.5 / var), rtol=1e-15, atol=0)
        gpr = mfa.GaussianProcessRegression((tt(t), tt(y)[:, None]), build_kernel(M32), chol_obs_covariance=tt([[np.sqrt(var)]]))
        assert float(model.elbo()) == pytest.approx(float(gpr.log_likelihood()), rel=1e-9)
        assert float(model.loss()) == pytest.approx(-float(gpr.log_likelihood()), rel=1e-9)
        np.testing.assert_allclose(float(model.elbo()), L.PC.dense_log_marginal(M32, t, y, var), **TOL)


@pytest.mark.parametrize("num_points", [7, 33])
@pytest.mark.parametrize("seed", range(6))
def test_bernoulli_runs_against_the_dense_loop(num_points, seed):
    run_against_dense(L.BERNOULLI, "m32", num_points, seed)


@pytest.mark.parametrize("num_points", [7, 33])
@pytest.mark.parametrize("seed", range(6))
def test_poisson_runs_against_the_dense_loop(num_points, seed):
    """Counts drawn with rate exp(f); nat2 < 0 throughout the dense run for each of these seeds (dense_run asserts it)."""
    run_against_dense(L.POISSON, "m32", num_points, seed)


def test_sum_of_two_materns_with_state_dimension_five():
    """Well-separated time points: a Matern-5/2 kernel matrix on uniform draws (gaps down to 1e-3) has a condition number beyond
    1e10, and the dense loop, which inverts it, is then no reference at 1e-6 (measured on such data: 3 of 33 sites 2.3e-7 off)."""
    model = run_against_dense(L.BERNOULLI, "m52+m32", 33, seed=1, separated=True)
    assert model.dist_q.state_dim == 5


def test_a_batch_of_three_series_equals_three_models():
    runs = [dense_run(L.BERNOULLI, "m32", 33, seed) for seed in range(3)]
    t, y = np.stack([r[1] for r in runs]), np.stack([r[2] for r in runs])
    batch = build_model(L.BERNOULLI, M32, t, y, lr=0.5)
    singles = [build_model(L.BERNOULLI, M32, r[1], r[2], lr=0.5) for r in runs]
    for _ in range(5):
        batch.update_sites()
        for m in singles:
            m.update_sites()
    assert tuple(batch.sites.nat1.shape) == (3, 33, 1) and tuple(batch.sites.nat2.shape) == (3, 33, 1, 1)
    for s, (m, r) in enumerate(zip(singles, runs)):
        # the same kernels on one series or on three: no more than the rounding of differently ordered sums
        np.testing.assert_allclose(nn(batch.sites.nat1)[s], nn(m.sites.nat1), rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(nn(batch.sites.nat2)[s], nn(m.sites.nat2), rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(nn(batch.sites.nat1)[s, :, 0], r[3][5]["nat1"], **TOL)
    assert float(batch.elbo()) == pytest.approx(sum(float(m.elbo()) for m in singles), rel=1e-10)
    assert float(batch.classic_elbo()) == pytest.approx(sum(float(m.classic_elbo()) for m in singles), rel=1e-10)
    assert float(batch.elbo()) == pytest.approx(sum(r[3][5]["elbo"] for r in runs), rel=1e-6)


def test_update_sites_is_one_launch_of_the_site_kernel_and_no_torch_route(monkeypatch):
    comps, t, y, _ = dense_run(L.BERNOULLI, "m32", 33, 0)
    model = build_model(L.BERNOULLI, comps, t, y, lr=0.5)
    seen = []
    real_rc = _lib.call_rc
    monkeypatch.setattr(_lib, "call_rc", lambda base, *a: (seen.append(base), real_rc(base, *a))[1])

    def no_torch(*a, **k):
        raise AssertionError("the torch route must not run on HIP tensors")

    monkeypatch.setattr(ML, "torch_variational_expectations", no_torch)
    monkeypatch.setattr(ML, "torch_predict_log_density", no_torch)
    versions = (model.sites.nat1._version, model.sites.nat2._version)
    model.update_sites()
    assert seen.count("mf_lik_cvi_site_update") == 1
    assert not any(s.startswith("mf_lik_") and s != "mf_lik_cvi_site_update" for s in seen)
    assert model.sites.nat1._version > versions[0] and model.sites.nat2._version > versions[1]
    model.classic_elbo()
    model.predict_log_density((tt(t[:4] + 0.01), tt(y[:4])[:, None]))
    assert seen.count("mf_lik_variational_expectations") == 1 and seen.count("mf_lik_predict_log_density") == 1


def test_elbo_sees_the_updated_sites():
    """No stale filter state: the value after an update is the value of a model built afresh around the new sites."""
    comps, t, y, rec = dense_run(L.POISSON, "m32", 33, 2)
    model = build_model(L.POISSON, comps, t, y, lr=0.5)
    model.update_sites()
    first = float(model.elbo())
    model.update_sites()
    second = float(model.elbo())
    assert first != second
    np.testing.assert_allclose(first, rec[1]["elbo"], **TOL)
    np.testing.assert_allclose(second, rec[2]["elbo"], **TOL)
    fresh = build_model(L.POISSON, comps, t, y, lr=0.5)
    fresh.sites = mfa.UnivariateGaussianSitesNat(model.sites.nat1.clone(), model.sites.nat2.clone())
    assert float(fresh.elbo()) == second


@pytest.mark.parametrize("name", [L.BERNOULLI, L.POISSON])
def test_prediction_at_new_time_points_against_the_dense_posterior(name):
    comps, t, y, rec = dense_run(name, "m32", 33, 3)
    model = build_model(name, comps, t, y, lr=0.5)
    for _ in range(25):
        model.update_sites()
    rng = np.random.default_rng(11)
    t_new = np.sort(np.concatenate([t[0] - 0.1 - rng.random(2), t[-1] + 0.1 + rng.random(2), rng.uniform(t[0], t[-1], 5)]))
    y_new = np.array([0.0, 1.0, 1.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0]) if name == L.BERNOULLI else np.arange(9.0) % 4
    mean, var = L.dense_predict(comps, t, rec[25]["nat1"], rec[25]["nat2"], t_new)
    f_mean, f_var = model.posterior.predict_f(tt(t_new))
    assert tuple(f_mean.shape) == (9, 1) and tuple(f_var.shape) == (9, 1)
    np.testing.assert_allclose(nn(f_mean)[:, 0], mean, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(nn(f_var)[:, 0], var, rtol=1e-5, atol=1e-7)
    density = model.predict_log_density((tt(t_new), tt(y_new)[:, None]))
    assert tuple(density.shape) == (9,)
    want = L.predict_log_density(L.LIKELIHOODS[name], mean, var, y_new)
    # d log density / d(mean, var) is O(1) on this data: the prediction's tolerances carry over
    np.testing.assert_allclose(nn(density), want, rtol=1e-5, atol=1e-6)


def test_elbo_backward_gives_the_lengthscale_gradient():
    """d elbo / d lengthscale (sites fixed) through the filter's backward against central differences of elbo(), and against
    autograd through the dense marginal likelihood of the sites model.  Well-separated time points (gaps of at least 0.07), where
    elbo() carries a relative rounding error of about 1e-12: with h = 1e-4 the differences' rounding error is
    1e-12 x 60 / 1e-4 = 6e-7 and their truncation h^2 / 6 x (a third derivative of order ten) = 2e-8, against a gradient of order
    0.1: rtol 1e-5.  (On uniform draws, gaps down to 1e-3, elbo() is good to 1e-7 only and the differences to 1e-3: measured.)"""
    comps, t, y, _ = dense_run(L.BERNOULLI, "m32", 33, 4, separated=True)
    model = build_model(L.BERNOULLI, comps, t, y, lr=0.5)
    for _ in range(5):
        model.update_sites()

    def elbo_at(ls, grad=False):
        ls_t = torch.tensor(ls, dtype=torch.float64, device=DEV, requires_grad=grad)
        m = mfa.CVIGaussianProcess((tt(t), tt(y)[:, None]), mfa.Matern32(ls_t, 1.0, device=DEV), mfa.Bernoulli(), learning_rate=0.5)
        m.sites = model.sites
        return m.elbo(), ls_t

    value, ls_t = elbo_at(1.0, grad=True)
    value.backward()
    h = 1e-4
    fd = (float(elbo_at(1.0 + h)[0]) - float(elbo_at(1.0 - h)[0])) / (2 * h)
    assert abs(float(ls_t.grad)) > 1e-2
    np.testing.assert_allclose(float(ls_t.grad), fd, rtol=1e-5, atol=1e-7)
    # dense: log N(m | 0, K(ls) + diag(1 / precision)) differentiated by torch on the CPU
    ls_c = torch.tensor(1.0, dtype=torch.float64, requires_grad=True)
    nat1, nat2 = model.sites.nat1.cpu()[:, 0], model.sites.nat2.cpu()[:, 0, 0]
    tc = torch.tensor(t, dtype=torch.float64)
    r = (tc[:, None] - tc[None, :]).abs() * (np.sqrt(3.0) / ls_c)
    kn = (1 + r) * torch.exp(-r) + torch.diag(1.0 / (-2.0 * nat2))
    m_sites = nat1 / (-2.0 * nat2)
    dense = -0.5 * (m_sites @ torch.linalg.solve(kn, m_sites) + torch.linalg.slogdet(kn)[1] + len(t) * np.log(2 * np.pi))
    dense.backward()
    assert float(value.detach()) == pytest.approx(float(dense.detach()), rel=1e-9)
    np.testing.assert_allclose(float(ls_t.grad), float(ls_c.grad), rtol=1e-6, atol=1e-9)
