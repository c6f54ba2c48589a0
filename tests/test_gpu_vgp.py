"""
GPU tests of ``VariationalGaussianProcess`` and ``dense_expected_log_likelihood`` (markovflow_amd/models.py): the reference's optimum
test, the fused data term against the torch composition on the same model, launch counts, the conjugate case against the GPR
posterior, the natural-gradient iteration against ``CVIGaussianProcess.update_sites`` (a natural-gradient step without momentum IS a
CVI step at ``lr = gamma``; Khan & Lin 2017), the hyper-parameter gradient and prediction.

``TOL`` = rtol 1e-6 / atol 1e-7, the ``TOL`` of tests/test_gpu_svgp.py, unless a test says otherwise.  The kernels carry jitter 0, every
series has at most 130 points, drawn one per cell of an even grid (``separated``: neighbouring points at least 0.4 span / N apart, so
that Q = P - A P A^T keeps its digits at jitter 0).  The series of the CVI comparison - Bernoulli and Poisson, Matern-3/2, 33 points,
seed 1 - were checked on the CPU with the dense CVI loop of tests/helpers/likelihood_closed_forms.py first: Poisson counts of at most
7, and dense posterior covariances of f with condition numbers below 700 (Poisson) and 1400 (Bernoulli) through the three steps,
under a prior kernel matrix of condition number 5.8e3 (tests/test_svgp_host.py explains which Poisson draw to avoid and why).  Float64 only: the float32 path is pinned at kernel level (tests/test_gpu_vgp_kernel.py).
"""
import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from markovflow_amd import likelihoods as ML
from markovflow_amd import models as MM
from helpers import likelihood_closed_forms as L
from helpers import vgp_closed_forms as VG

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = dict(rtol=1e-6, atol=1e-7)
M32 = [dict(order=3, ls=1.0, var=1.0, period=None, osc=0)]
M52_M32 = [dict(order=5, ls=1.3, var=0.8, period=None, osc=0), dict(order=3, ls=0.6, var=0.5, period=None, osc=0)]
D10 = [dict(order=5, ls=1.3, var=0.8, period=None, osc=0), dict(order=5, ls=0.9, var=0.4, period=None, osc=0),
       dict(order=3, ls=0.6, var=0.5, period=None, osc=0), dict(order=3, ls=1.1, var=0.3, period=None, osc=0)]
KERNELS = {"m32": M32, "m52+m32": M52_M32, "d10": D10}
FWD, ADJ = "mf_lik_dense_expectations", "mf_lik_dense_expectations_adjoint"


def tt(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def nn(t):
    return t.detach().cpu().numpy()


def build_kernel(comps, lengthscale=None):
    cls = {1: mfa.Matern12, 3: mfa.Matern32, 5: mfa.Matern52}
    parts = [cls[c["order"]](c["ls"] if lengthscale is None else lengthscale, c["var"], device=DEV, dtype=torch.float64) for c in comps]
    return parts[0] if len(parts) == 1 else mfa.Sum(parts)


def build_likelihood(name):
    params = L.LIKELIHOODS[name][1]
    return {L.GAUSSIAN: lambda: mfa.Gaussian(params[0]), L.BERNOULLI: mfa.Bernoulli, L.POISSON: mfa.Poisson,
            L.STUDENTT: lambda: mfa.StudentT(*params)}[name]()


_SERIES = {}


def series(name, comps_key, num_points, seeds):
    """``(x, y)`` stacked over ``seeds`` (one seed: no batch dimension), drawn once and shared, read-only."""
    key = (name, comps_key, num_points, seeds)
    if key not in _SERIES:
        drawn = [L.draw_series(L.LIKELIHOODS[name], KERNELS[comps_key], num_points, seed, separated=True) for seed in seeds]
        x, y = (np.stack([d[i] for d in drawn]) if len(seeds) > 1 else drawn[0][i] for i in (0, 1))
        x.setflags(write=False)
        y.setflags(write=False)
        _SERIES[key] = (x, y)
    return _SERIES[key]


def data(x, y):
    return tt(x), tt(y)[..., None]


def build_model(name, comps_key, num_points, seeds, **kwargs):
    x, y = series(name, comps_key, num_points, seeds)
    return mfa.VariationalGaussianProcess(data(x, y), build_kernel(KERNELS[comps_key]), build_likelihood(name), **kwargs)


def natgrad_steps(model, steps, **kwargs):
    opt = mfa.SSMNaturalGradient(**kwargs)
    for _ in range(steps):
        opt.minimize(model.loss, model.dist_q)
    return opt


def marginals(dist):
    with torch.no_grad():
        means, covs = dist.marginals
    return nn(means), nn(covs)


# ---- the optimum -------------------------------------------------------------------------------------------------------------------
def test_at_the_gpr_posterior_the_elbo_is_the_log_likelihood_and_its_gradient_vanishes():
    """The reference's test (tests/integration/models/test_variational.py:111-132): Matern-1/2, lengthscale 2, variance 2.25, unit
    Gaussian noise, 8 points, q = the GPR posterior; its rtol 1e-7 on the value and atol 1e-9 on every gradient."""
    rng = np.random.default_rng(8)
    x, y = np.sort(rng.uniform(0.0, 8.0, 8)), rng.normal(size=8)
    kernel = mfa.Matern12(2.0, 2.25, device=DEV)
    xy = data(x, y)
    gpr = mfa.GaussianProcessRegression(xy, kernel, chol_obs_covariance=tt(np.eye(1)))
    model = mfa.VariationalGaussianProcess(xy, kernel, mfa.Gaussian(1.0), initial_distribution=gpr.posterior_state_space_model())
    assert model._fused()
    elbo = model.elbo()
    np.testing.assert_allclose(float(elbo.detach()), float(gpr.log_likelihood()), rtol=1e-7)
    elbo.backward()
    for leaf in model.trainable_variables:
        assert leaf.grad is not None
        np.testing.assert_allclose(nn(leaf.grad), 0.0, atol=1e-9)
    np.testing.assert_allclose(float(model.loss().detach()), -float(elbo.detach()), rtol=1e-14)


# ---- fused against composed --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,comps_key,num_points,seeds", [
    (L.BERNOULLI, "m32", 33, (1,)), (L.POISSON, "m32", 130, (1, 2)), (L.GAUSSIAN, "m52+m32", 33, (1,)),
    (L.STUDENTT, "m32", 33, (1, 2)), (L.BERNOULLI, "d10", 33, (1,)), (L.BERNOULLI, "m52+m32", 130, (2,))])
def test_fused_elbo_and_its_gradients_against_the_torch_composition_on_the_same_model(name, comps_key, num_points, seeds, monkeypatch):
    model = build_model(name, comps_key, num_points, seeds)
    natgrad_steps(model, 2, gamma=0.5, momentum=False)                    # (a q that is not the prior)
    leaves = model.trainable_variables
    assert model._fused()
    fused = model.elbo()
    g_fused = torch.autograd.grad(fused, leaves)
    monkeypatch.setattr(model, "_fused", lambda: False)
    composed = model.elbo()
    g_composed = torch.autograd.grad(composed, leaves)
    np.testing.assert_allclose(float(fused.detach()), float(composed.detach()), **TOL)
    for a, b in zip(g_fused, g_composed):
        assert bool(torch.isfinite(a).all())
        np.testing.assert_allclose(nn(a), nn(b), **TOL)
    assert float(torch.triu(g_fused[1], 1).abs().max()) == 0.0 and float(torch.triu(g_fused[4], 1).abs().max()) == 0.0


def test_elbo_is_one_launch_of_the_expectations_kernel_and_backward_one_of_the_adjoint(monkeypatch):
    model = build_model(L.BERNOULLI, "m32", 33, (0,))
    model.elbo()
    seen = []
    real_rc = _lib.call_rc
    monkeypatch.setattr(_lib, "call_rc", lambda base, *a: (seen.append(base), real_rc(base, *a))[1])

    def no_torch(*a, **k):
        raise AssertionError("the torch route must not run on HIP tensors")

    monkeypatch.setattr(ML, "torch_variational_expectations", no_torch)
    monkeypatch.setattr(MM.variational, "dense_expected_log_likelihood_torch", no_torch)
    elbo = model.elbo()
    assert seen.count(FWD) == 1 and seen.count(ADJ) == 0
    assert "mf_lik_variational_expectations" not in seen
    assert not any(s.startswith("mf_lik_") and s != FWD for s in seen)
    del seen[:]
    elbo.backward()
    assert seen.count(ADJ) == 1, "the backward expands the forward's two derivatives per point: one launch"
    assert not any(s.startswith("mf_lik_") and s != ADJ for s in seen)
    assert all(leaf.grad is not None and bool(torch.isfinite(leaf.grad).all()) for leaf in model.trainable_variables)


def test_the_fused_function_is_differentiable_once_and_value_only_without_a_tape():
    model = build_model(L.BERNOULLI, "m32", 130, (1, 2))
    natgrad_steps(model, 1, gamma=0.5, momentum=False)
    lik = model.likelihood
    with torch.no_grad():
        means, covs = model.dist_q.marginals
    plain = MM.dense_expected_log_likelihood(lik, model._h, model._y, means, covs)
    assert tuple(plain.shape) == (2,) and not plain.requires_grad
    m, p = means.clone().requires_grad_(True), covs.clone().requires_grad_(True)
    taped = MM.dense_expected_log_likelihood(lik, model._h, model._y, m, p)
    assert torch.equal(taped.detach(), plain), "the value has the same bits with and without the adjoints"
    weight = tt([1.0, -2.5])
    g_means, g_covs = torch.autograd.grad(torch.sum(weight * taped), (m, p))
    assert torch.equal(g_covs, g_covs.transpose(-1, -2)), "g_var h h^T"
    for b in range(2):
        want = VG.dense_expectations(L.LIKELIHOODS[L.BERNOULLI], nn(model._h[b]), nn(means[b]), nn(covs[b]), nn(model._y[b]))
        adj = VG.dense_adjoint(nn(model._h[b]), want["g_mu"], want["g_var"], float(weight[b]))
        np.testing.assert_allclose(float(plain[b]), want["ve_sum"], rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(nn(g_means[b]), adj["g_means"], rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(nn(g_covs[b]), adj["g_covs"], rtol=1e-12, atol=1e-13)
    again = MM.dense_expected_log_likelihood(lik, model._h, model._y, m, p)
    with pytest.raises(RuntimeError, match="differentiable once"):
        torch.autograd.grad(again.sum(), (m, p), create_graph=True)
    with pytest.raises(NotImplementedError, match="no adjoint onto h"):
        MM.dense_expected_log_likelihood(lik, model._h.clone().requires_grad_(True), model._y, means, covs)


# ---- the conjugate case ------------------------------------------------------------------------------------------------------------
def test_one_step_at_unit_rate_with_a_gaussian_likelihood_lands_on_the_gpr_posterior():
    noise = L.LIKELIHOODS[L.GAUSSIAN][1][0]
    x, y = series(L.GAUSSIAN, "m32", 33, (0,))
    model = build_model(L.GAUSSIAN, "m32", 33, (0,))
    natgrad_steps(model, 1, gamma=1.0, momentum=False)
    gpr = mfa.GaussianProcessRegression(data(x, y), build_kernel(M32), chol_obs_covariance=tt([[np.sqrt(noise)]]))
    means, covs = marginals(model.dist_q)
    want_means, want_covs = marginals(gpr.posterior_state_space_model())
    np.testing.assert_allclose(means, want_means, **TOL)
    np.testing.assert_allclose(covs, want_covs, **TOL)
    with torch.no_grad():
        np.testing.assert_allclose(float(model.elbo()), float(gpr.log_likelihood()), **TOL)


# ---- the same iteration as CVI -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [L.BERNOULLI, L.POISSON])
def test_natural_gradient_without_momentum_reproduces_update_sites_step_for_step(name):
    x, y = series(name, "m32", 33, (1,))
    model = build_model(name, "m32", 33, (1,))
    cvi = mfa.CVIGaussianProcess(data(x, y), build_kernel(M32), build_likelihood(name), learning_rate=0.5)
    opt = mfa.SSMNaturalGradient(gamma=0.5, momentum=False)
    for it in range(1, 4):
        opt.minimize(model.loss, model.dist_q)
        cvi.update_sites()
        means, covs = marginals(model.dist_q)
        want_means, want_covs = marginals(cvi.dist_q)
        np.testing.assert_allclose(means, want_means, err_msg=f"step {it}", **TOL)
        np.testing.assert_allclose(covs, want_covs, err_msg=f"step {it}", **TOL)
        with torch.no_grad():
            np.testing.assert_allclose(float(model.elbo()), float(cvi.classic_elbo()), err_msg=f"step {it}", **TOL)


# ---- hyper-parameters --------------------------------------------------------------------------------------------------------------
def test_the_lengthscale_gradient_of_the_fused_elbo_is_that_of_the_kl_term(monkeypatch):
    trained = build_model(L.BERNOULLI, "m32", 33, (4,))
    natgrad_steps(trained, 3, gamma=0.5, momentum=False)
    x, y = series(L.BERNOULLI, "m32", 33, (4,))
    ls_t = torch.tensor(1.0, dtype=torch.float64, device=DEV, requires_grad=True)
    model = mfa.VariationalGaussianProcess(data(x, y), mfa.Matern32(ls_t, 1.0, device=DEV), mfa.Bernoulli(),
                                           initial_distribution=trained.dist_q)
    seen = []
    real_rc = _lib.call_rc
    monkeypatch.setattr(_lib, "call_rc", lambda base, *a: (seen.append(base), real_rc(base, *a))[1])
    value = model.elbo()
    assert seen.count(FWD) == 1, "a hyper-parameter under the tape keeps the fused data term: it enters through the KL only"
    grads = torch.autograd.grad(value, (ls_t,) + tuple(model.trainable_variables))
    kl = torch.sum(model.dist_q.kl_divergence(model.dist_p))
    (g_kl,) = torch.autograd.grad(kl, ls_t)
    assert abs(float(g_kl)) > 1e-2
    np.testing.assert_allclose(float(grads[0]), -float(g_kl), **TOL)
    np.testing.assert_allclose(float(value.detach()), float(trained.elbo().detach()), rtol=1e-12)
    g_plain = torch.autograd.grad(trained.elbo(), trained.trainable_variables)
    for a, b in zip(grads[1:], g_plain):
        np.testing.assert_allclose(nn(a), nn(b), **TOL)


# ---- prediction --------------------------------------------------------------------------------------------------------------------
def test_predict_f_at_the_data_points_is_the_projection_of_the_marginals_of_q():
    model = build_model(L.BERNOULLI, "m52+m32", 33, (1, 2))
    natgrad_steps(model, 2, gamma=0.5, momentum=False)
    f_mean, f_var = model.predict_f(model.time_points)
    assert tuple(f_mean.shape) == (2, 33, 1) and tuple(f_var.shape) == (2, 33, 1) and not f_mean.requires_grad
    means, covs = marginals(model.dist_q)
    h = nn(model._h)
    np.testing.assert_allclose(nn(f_mean)[..., 0], np.einsum("bki,bki->bk", h, means), **TOL)
    np.testing.assert_allclose(nn(f_var)[..., 0], np.einsum("bki,bkij,bkj->bk", h, covs, h), **TOL)
    x, _ = series(L.BERNOULLI, "m52+m32", 33, (1, 2))
    new_x = 0.5 * (x[:, 1:8] + x[:, :7])
    density = model.predict_log_density((tt(new_x), tt(np.ones((2, 7, 1)))))
    assert tuple(density.shape) == (2, 7) and bool(torch.isfinite(density).all()) and bool((density < 0).all())
    assert isinstance(model.dist_p, mfa.StateSpaceModel) and model.dist_p is not model.dist_p, "the prior is rebuilt on access"
