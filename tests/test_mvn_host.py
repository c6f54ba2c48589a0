"""
CPU tests (float64) of the ``MultivariateGaussian`` likelihood and its SVGP plumbing: the four methods against
``torch.distributions.MultivariateNormal``, the torch data term and the helper tests/helpers/mvn_closed_forms.py against a dense
per-point evaluation, and the refusals.  The model itself needs the HIP chain kernels: its ELBO is in tests/test_gpu_mvn.py.
"""
import math

import numpy as np
import pytest
import torch
from torch.distributions import MultivariateNormal

import markovflow_amd as mfa
from markovflow_amd import models as MM
from helpers import mvn_closed_forms as MC

TIGHT = dict(rtol=1e-11, atol=1e-11)
F64 = torch.float64


def chol_factor(p, seed=0):
    rng = np.random.default_rng(seed)
    return torch.tensor(np.tril(rng.uniform(-0.5, 0.5, size=(p, p)), -1) + np.diag(rng.uniform(0.6, 1.2, size=p)), dtype=F64)


def spd(rng, shape, dim):
    a = rng.normal(size=shape + (dim, dim))
    return torch.tensor(a @ np.swapaxes(a, -1, -2) / dim + 0.1 * np.eye(dim), dtype=F64)


@pytest.mark.parametrize("p", [1, 2, 4])
def test_the_four_methods_against_multivariate_normal(p):
    rng = np.random.default_rng(p)
    # the strict upper triangle is never read: garbage there changes nothing and gets no gradient
    leaf = (chol_factor(p) + torch.triu(torch.full((p, p), 7.0, dtype=F64), 1)).requires_grad_(True)
    lik = mfa.MultivariateGaussian(leaf)
    assert lik.obs_dim == lik.latent_dim == p and lik.trainable_variables == (leaf,)
    ref = leaf.detach().tril().requires_grad_(True)
    sigma = ref @ ref.T
    f, y, s = torch.tensor(rng.normal(size=(2, 5, p))), torch.tensor(rng.normal(size=(2, 5, p))), spd(rng, (2, 5), p)
    want = MultivariateNormal(f, sigma).log_prob(y) - 0.5 * torch.sum(torch.linalg.inv(sigma) * s, dim=(-1, -2))
    ve = lik.variational_expectations(f, s, y)
    np.testing.assert_allclose(ve.detach(), want.detach(), **TIGHT)
    np.testing.assert_allclose(lik.log_prob(f, y).detach(), MultivariateNormal(f, sigma).log_prob(y).detach(), **TIGHT)
    np.testing.assert_allclose(lik.predict_log_density(f, s, y).detach(), MultivariateNormal(f, sigma + s).log_prob(y).detach(), **TIGHT)
    mean, cov = lik.predict_mean_and_var(f, s)
    assert torch.equal(mean, f)
    np.testing.assert_allclose(cov.detach(), (sigma + s).detach(), **TIGHT)
    torch.sum(ve).backward()
    torch.sum(want).backward()
    assert float(torch.triu(leaf.grad, 1).abs().sum()) == 0.0, "the gradient that reaches the leaf is lower-triangular"
    np.testing.assert_allclose(leaf.grad, ref.grad.tril(), rtol=1e-10, atol=1e-10)
    for call in (lambda: lik.cvi_site_update(f, f, y, 0.5, f.clone(), f.clone()), lambda: lik.pep_site_update(f, f, y),
                 lambda: lik.log_expected_density(f, f, y)):
        with pytest.raises(NotImplementedError, match="full covariance"):
            call()
    with pytest.raises(ValueError, match="non-zero"):
        mfa.MultivariateGaussian(torch.zeros(2, 2, dtype=F64))


@pytest.mark.parametrize("p,two_d", [(2, 4), (3, 6), (5, 20)])
def test_the_torch_data_term_and_the_helper_against_a_dense_per_point_evaluation(p, two_d):
    rng = np.random.default_rng(10 * p + two_d)
    lengths = (3, 0, 70, 1)
    n, segs = sum(lengths), len(lengths)
    indices = torch.as_tensor(np.repeat(np.arange(segs), lengths))
    w, c = torch.tensor(rng.uniform(-0.7, 0.7, size=(n, p, two_d))), spd(rng, (n,), p)
    y, pm, pc = torch.tensor(rng.normal(size=(n, p))), torch.tensor(rng.normal(size=(segs, two_d))), spd(rng, (segs,), two_d)
    lik = mfa.MultivariateGaussian(chol_factor(p, 3))
    sigma = lik.chol_covariance @ lik.chol_covariance.T
    dense = np.zeros(segs)
    for k in range(n):                           # point by point, with torch.distributions
        mu, fk = w[k] @ pm[indices[k]], c[k] + w[k] @ pc[indices[k]] @ w[k].T
        dense[indices[k]] += float(MultivariateNormal(mu, sigma).log_prob(y[k]) - 0.5 * torch.sum(torch.linalg.inv(sigma) * fk))
    pm.requires_grad_(True), pc.requires_grad_(True)
    value = MM.sparse_mvn_expected_log_likelihood_torch(lik, w, c, y, indices, pm, pc)
    assert tuple(value.shape) == (segs,) and float(value.detach()[1]) == 0.0
    np.testing.assert_allclose(value.detach(), dense, **TIGHT)
    # the helper: its value, and its adjoints against autograd through the torch route
    got = MC.segment_expectations_mvn(w.numpy(), c.numpy(), y.numpy(), lik.precision(w).numpy(), np.concatenate([[0], np.cumsum(lengths)]),
                                      pm.detach().numpy(), pc.detach().numpy())
    const = p * math.log(2.0 * math.pi) + float(torch.logdet(sigma))
    np.testing.assert_allclose(-0.5 * (np.asarray(lengths) * const + got["quad_sum"]), dense, **TIGHT)
    g_mean, g_cov = torch.autograd.grad(torch.sum(value), (pm, pc))
    np.testing.assert_allclose(g_mean, got["g_mean"], **TIGHT)
    np.testing.assert_allclose(g_cov, got["g_cov"], **TIGHT)


def test_refusals_of_the_other_models_of_a_stack_kernel_and_of_a_wrong_output_dim():
    m32, m12 = mfa.Matern32(1.0, 1.0), mfa.Matern12(1.0, 1.0)
    kernel = mfa.IndependentMultiOutput([m32, m12])
    t, z = torch.linspace(0.0, 2.0, 6, dtype=F64), torch.linspace(0.0, 2.0, 3, dtype=F64)
    data = (t, torch.zeros((6, 1), dtype=F64))
    lik = mfa.MultivariateGaussian(chol_factor(2))
    zs, ks = torch.zeros((2, 1), dtype=F64), mfa.spatial_kernels.SquaredExponential(1.0, 1.0)
    chain = lambda d: mfa.StateSpaceModel(torch.zeros(d, dtype=F64), torch.eye(d, dtype=F64), torch.zeros(2, d, d, dtype=F64),  # noqa: E731
                                          torch.zeros(2, d, dtype=F64), torch.eye(d, dtype=F64).expand(2, d, d).contiguous())
    makers = [lambda: mfa.CVIGaussianProcess(data, kernel, lik), lambda: mfa.PowerExpectationPropagation(data, kernel, lik),
              lambda: mfa.SparseCVIGaussianProcess(kernel, z, lik), lambda: mfa.SparsePowerExpectationPropagation(kernel, z, lik),
              lambda: mfa.ImportanceWeightedVI(kernel, z, lik, 4), lambda: mfa.VariationalGaussianProcess(data, kernel, lik),
              lambda: mfa.SpatioTemporalSparseVariational(zs, z, ks, m32, lik), lambda: mfa.SpatioTemporalSparseCVI(zs, z, ks, m32, lik),
              lambda: mfa.CVIGaussianProcess(data, m32, mfa.MultivariateGaussian(chol_factor(1)))]
    for make in makers:
        with pytest.raises(NotImplementedError, match="only SparseVariationalGaussianProcess supports"):
            make()
    with pytest.raises(NotImplementedError, match="stack kernel"):
        mfa.SparseVariationalGaussianProcess(mfa.IndependentMultiOutputStack([m32, m12]), lik, z.expand(2, 3).contiguous(),
                                             initial_distribution=chain(2))
    for wrong in (m32, mfa.IndependentMultiOutput([m32] * 3)):
        with pytest.raises(ValueError, match="latent_dim = 2"):
            mfa.SparseVariationalGaussianProcess(wrong, lik, z, initial_distribution=chain(wrong.state_dim))
    model = mfa.SparseVariationalGaussianProcess(kernel, lik, z, initial_distribution=chain(3))
    with pytest.raises(ValueError, match=r"\[num_data, 2\]"):
        model.elbo(data)
    gpr = mfa.GaussianProcessRegression((t, torch.zeros((6, 2), dtype=F64)), kernel, chol_obs_covariance=chol_factor(2))
    assert isinstance(gpr.likelihood, mfa.MultivariateGaussian) and torch.equal(gpr.likelihood.chol_covariance, chol_factor(2))
