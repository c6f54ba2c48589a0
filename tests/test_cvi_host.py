"""
What of ``CVIGaussianProcess`` can be checked without a GPU.  The model's filter, smoother, ``naturals_to_ssm_params`` and
``kl_divergence`` are HIP kernels and CPU tensors fail loudly there (tests/test_host.py: there is no CPU fallback), so every
comparison of the MODEL with the dense loop lives in tests/test_gpu_cvi.py.  Here: construction and its errors, the site
initialisation, the two module-level functions, the loud failure on CPU tensors - and the dense loop itself, which is the
reference of the GPU tests: its Gaussian identities and the facts recorded for the Bernoulli runs.
"""
import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import models
from helpers import likelihood_closed_forms as L
from helpers import periodic_closed_forms as PC

M32 = [dict(order=3, ls=1.0, var=1.0, period=None, osc=0)]


def tt(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def test_construction_sites_and_properties():
    t, y = tt(np.linspace(0, 6, 7)), tt(np.arange(7.0) % 2)[:, None]
    kern, lik = mfa.Matern32(1.0, 1.0), mfa.Bernoulli()
    model = mfa.CVIGaussianProcess((t, y), kern, lik)
    assert model.learning_rate == 0.1 and model.kernel is kern and model.likelihood is lik
    assert model.time_points is t and model.observations is y and model.conditioning_points is t
    # variational_cvi.py:98-103
    assert isinstance(model.sites, mfa.UnivariateGaussianSitesNat)
    assert tuple(model.sites.nat1.shape) == (7, 1) and torch.all(model.sites.nat1 == 0)
    assert tuple(model.sites.nat2.shape) == (7, 1, 1) and torch.all(model.sites.nat2 == -1e-10)
    assert tuple(model.sites.log_norm.shape) == (7, 1) and torch.all(model.sites.log_norm == 0)
    batched = mfa.CVIGaussianProcess((t.expand(3, 7).contiguous(), y.expand(3, 7, 1).contiguous()), kern, lik, learning_rate=0.5)
    assert tuple(batched.sites.nat1.shape) == (3, 7, 1) and tuple(batched.sites.nat2.shape) == (3, 7, 1, 1)
    assert models.CVIGaussianProcess is mfa.CVIGaussianProcess
    with pytest.raises(ValueError, match=r"\[num_data, 1\]"):
        mfa.CVIGaussianProcess((t, y.expand(7, 2)), kern, lik)
    with pytest.raises(ValueError, match="time_points"):
        mfa.CVIGaussianProcess((t[:6], y), kern, lik)
    with pytest.raises(TypeError, match="Likelihood"):
        mfa.CVIGaussianProcess((t, y), kern, "bernoulli")
    with pytest.raises(ValueError, match="learning_rate"):
        mfa.CVIGaussianProcess((t, y), kern, lik, learning_rate=1.5)
    with pytest.raises(ValueError, match="time_points is torch.float32"):
        mfa.CVIGaussianProcess((t.float(), y), kern, lik)


def test_cpu_tensors_fail_loudly_in_the_model():
    t, y = tt(np.linspace(0, 6, 7)), tt(np.arange(7.0) % 2)[:, None]
    model = mfa.CVIGaussianProcess((t, y), mfa.Matern32(1.0, 1.0), mfa.Bernoulli())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.update_sites()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.elbo()


def test_local_objective_and_gradients_on_cpu():
    """The likelihood's CPU route serves the model's local objective: value, and gradients in [mu, var + mu^2]."""
    spec = L.LIKELIHOODS[L.BERNOULLI]
    mu, var, y = L.value_grid(L.BERNOULLI)
    model = mfa.CVIGaussianProcess((tt(np.arange(mu.size)), tt(y)[:, None]), mfa.Matern32(1.0, 1.0), mfa.Bernoulli())
    (ve, g_mu, g_var), _ = L.expectations(spec, mu, var, y)
    obj, (g1, g2) = model.local_objective_and_gradients(tt(mu)[:, None], tt(var)[:, None])
    assert float(obj) == pytest.approx(ve.sum(), rel=1e-12)
    np.testing.assert_allclose(g1.numpy()[:, 0], g_mu - 2 * g_var * mu, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(g2.numpy()[:, 0], g_var, rtol=1e-10, atol=1e-12)
    local = model.local_objective(tt(mu)[:, None], tt(var)[:, None], tt(y)[:, None])
    np.testing.assert_allclose(local.numpy(), ve, rtol=1e-12, atol=1e-13)


def test_back_project_nats_and_gradient_transformation(rng):
    n, d = 5, 3
    nat1, nat2, c = rng.normal(size=(2, n, 1)), -rng.random((2, n, 1)), rng.normal(size=(2, n, 1, d))
    b1, b2 = models.back_project_nats(tt(nat1), tt(nat2), tt(c))
    np.testing.assert_allclose(b1.numpy(), np.einsum("bnod,bno->bnd", c, nat1), rtol=1e-14, atol=0)
    np.testing.assert_allclose(b2.numpy(), np.einsum("bnod,bnoe,bno->bnde", c, c, nat2), rtol=1e-14, atol=0)
    u1, u2 = models.back_project_nats(tt(nat1[0]), tt(nat2[0]), tt(c[0]))                  # the reference's unbatched shapes
    assert torch.equal(u1, b1[0]) and torch.equal(u2, b2[0])
    with pytest.raises(ValueError, match="back_project_nats"):
        models.back_project_nats(tt(nat1), tt(nat2[..., 0]), tt(c))
    with pytest.raises(ValueError, match="back_project_nats"):
        models.back_project_nats(tt(nat1), tt(nat2), tt(c[:, :4]))
    mu, var, g_mu, g_var = (tt(rng.normal(size=(n, 1))) for _ in range(4))
    e1, e2 = models.gradient_transformation_mean_var_to_expectation((mu, var), (g_mu, g_var))
    assert torch.equal(e1, g_mu - 2.0 * g_var * mu) and e2 is g_var


# ---- the dense loop (the reference of tests/test_gpu_cvi.py) ----------------------------------------------------------------------
@pytest.mark.parametrize("num_points", [7, 33])
def test_dense_loop_gaussian_with_unit_learning_rate_is_exact_regression(num_points):
    """One step with rho = 1 puts the sites on the data, nat1 = y / variance and nat2 = -1 / (2 variance), and the marginal
    likelihood of the sites model is then the GP regression's."""
    lik = L.LIKELIHOODS[L.GAUSSIAN]
    var = lik[1][0]
    t, y = L.draw_series(lik, M32, num_points, seed=0)
    rec, (nat1, nat2) = L.dense_cvi(lik, M32, t, y, lr=1.0, iterations=1, record=(1,))
    np.testing.assert_allclose(nat1, y / var, rtol=1e-13, atol=0)
    np.testing.assert_allclose(nat2, np.full(num_points, -0.5 / var), rtol=1e-13, atol=0)
    assert rec[1]["elbo"] == pytest.approx(PC.dense_log_marginal(M32, t, y, var), rel=1e-11)
    # q is the exact posterior: the classic ELBO is the log marginal likelihood too
    assert rec[1]["classic_elbo"] == pytest.approx(PC.dense_log_marginal(M32, t, y, var), rel=1e-9)


@pytest.mark.parametrize("num_points", [7, 33])
@pytest.mark.parametrize("seed", range(6))
def test_dense_loop_bernoulli_runs_stay_in_the_domain_and_converge(num_points, seed):
    """The Bernoulli runs the GPU tests repeat (Matern-3/2, variance 1, lengthscale 1, times on [0, 6], rho = 0.5, 25 iterations):
    nat2 <= -0.10 throughout - every site precision is positive - and the largest site change in step 25 is at most 1.2e-6."""
    lik = L.LIKELIHOODS[L.BERNOULLI]
    t, y = L.draw_series(lik, M32, num_points, seed)
    assert set(np.unique(y)) <= {0.0, 1.0}
    rec, _ = L.dense_cvi(lik, M32, t, y, lr=0.5, iterations=25, record=tuple(range(1, 26)))
    assert max(r["nat2"].max() for r in rec.values()) <= -0.10
    assert max(np.abs(rec[25][k] - rec[24][k]).max() for k in ("nat1", "nat2")) <= 1.2e-6
    assert all(np.isfinite(r["elbo"]) and np.isfinite(r["classic_elbo"]) for r in rec.values())
    # the classic ELBO of a fixed point of the natural-gradient iteration is a maximum over the sites: it does not go down
    assert rec[25]["classic_elbo"] >= rec[5]["classic_elbo"] >= rec[1]["classic_elbo"]


def test_dense_predict_is_the_posterior_of_the_sites_model():
    lik = L.LIKELIHOODS[L.GAUSSIAN]
    t, y = L.draw_series(lik, M32, 9, seed=3)
    _, (nat1, nat2) = L.dense_cvi(lik, M32, t, y, lr=1.0, iterations=1)
    t_new = np.array([-0.5, 1.3, 2.9, 7.0])
    mean, var = L.dense_predict(M32, t, nat1, nat2, t_new)
    want_mean, want_var = PC.dense_predict(M32, t, y, lik[1][0], t_new)
    np.testing.assert_allclose(mean, want_mean, rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(var, want_var, rtol=1e-11, atol=1e-13)
