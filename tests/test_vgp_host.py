"""
CPU tests of the VGP model's host side (markovflow_amd/models.py: ``dense_expected_log_likelihood``,
``dense_expected_log_likelihood_torch``, ``VariationalGaussianProcess``), of the dense entry points' declarations and of the reference
the GPU tests lean on (tests/helpers/vgp_closed_forms.py): the helper's adjoints against autograd through its own torch value, the
torch composition against the helper within ``64 eps (magnitude + 1)``, the error paths, the symbols and the workspace formula.
"""
import os
import re

import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from markovflow_amd import models as MM
from conftest import ROOT
from helpers import likelihood_closed_forms as L
from helpers import vgp_closed_forms as VG

NAMES = [L.GAUSSIAN, L.BERNOULLI, L.POISSON, L.STUDENTT]
EPS = 2.0 ** -52


def tt(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def _case(seed, n, d, name, upper=0.0):
    rng = np.random.default_rng(seed)
    h = rng.uniform(-0.7, 0.7, size=(n, d))
    a = rng.normal(size=(n, d, d))
    covs = a @ a.transpose(0, 2, 1) / d + 0.1 * np.eye(d) + upper * np.triu(rng.uniform(-1.0, 1.0, size=(n, d, d)), k=1)
    means = rng.normal(size=(n, d))
    y = np.resize(np.asarray(L.OBSERVED[name]), n)
    return h, means, covs, y


def _likelihood(name):
    params = L.LIKELIHOODS[name][1]
    return {L.GAUSSIAN: lambda: mfa.Gaussian(params[0]), L.BERNOULLI: mfa.Bernoulli, L.POISSON: mfa.Poisson,
            L.STUDENTT: lambda: mfa.StudentT(*params)}[name]()


@pytest.mark.parametrize("name", NAMES)
def test_the_helpers_adjoints_are_the_gradients_of_its_own_value(name):
    h, means, covs, y = _case(7, 70, 5, name, upper=0.02)          # two tiles; a covariance that is not symmetric
    want = VG.dense_expectations(L.LIKELIHOODS[name], h, means, covs, y)
    m, p = tt(means).requires_grad_(True), tt(covs).requires_grad_(True)
    value = VG.dense_value_torch(L.LIKELIHOODS[name], h, m, p, y)
    assert abs(float(value.detach()) - want["ve_sum"]) <= 64 * EPS * (want["mag_ve_sum"] + 1)
    g_means, g_covs = torch.autograd.grad(value, (m, p))
    adj = VG.dense_adjoint(h, want["g_mu"], want["g_var"])
    h8 = np.abs(h)
    assert np.all(np.abs(g_means.numpy() - adj["g_means"]) <= 64 * EPS * (want["mag_g_mu"][:, None] * h8 + 1))
    assert np.all(np.abs(g_covs.numpy() - adj["g_covs"]) <= 64 * EPS * (want["mag_g_var"][:, None, None] * h8[:, :, None] * h8[:, None, :] + 1))
    assert float(np.abs(adj["g_covs"] - adj["g_covs"].transpose(0, 2, 1)).max()) <= 1e-15, "g_var h h^T: the unconstrained adjoint"
    scaled = VG.dense_adjoint(h, want["g_mu"], want["g_var"], weight=-1.5)
    np.testing.assert_allclose(scaled["g_covs"], -1.5 * adj["g_covs"], rtol=1e-15, atol=0)
    low = VG.dense_expectations(L.LIKELIHOODS[name], h, means, covs, y, dtype=np.float32)
    assert low["g_mu"].dtype == np.float32 and low["ve_sum"].dtype == np.float32 and low["mag_g_mu"].dtype == np.float64
    np.testing.assert_allclose(low["ve_sum"], want["ve_sum"], rtol=1e-4, atol=1e-4)
    empty = VG.dense_expectations(L.LIKELIHOODS[name], h[:0], means[:0], covs[:0], y[:0])
    assert float(empty["ve_sum"]) == 0.0 and empty["g_mu"].shape == (0,)


@pytest.mark.parametrize("n", [1, 9, 130])
@pytest.mark.parametrize("name", NAMES)
def test_torch_composition_of_the_expected_log_likelihood_against_the_numpy_statement(name, n):
    d = 4
    h, means, covs, y = _case(3, n, d, name, upper=0.02)
    want = VG.dense_expectations(L.LIKELIHOODS[name], h, means, covs, y)
    adj = VG.dense_adjoint(h, want["g_mu"], want["g_var"])
    m, p = tt(means).requires_grad_(True), tt(covs).requires_grad_(True)
    value = MM.dense_expected_log_likelihood_torch(_likelihood(name), tt(h), tt(y), m, p)
    assert tuple(value.shape) == ()
    assert abs(float(value.detach()) - want["ve_sum"]) <= 64 * EPS * (want["mag_ve_sum"] + 1)
    value.backward()
    h8 = np.abs(h)
    assert np.all(np.abs(m.grad.numpy() - adj["g_means"]) <= 64 * EPS * (want["mag_g_mu"][:, None] * h8 + 1))
    assert np.all(np.abs(p.grad.numpy() - adj["g_covs"]) <= 64 * EPS * (want["mag_g_var"][:, None, None] * h8[:, :, None] * h8[:, None, :] + 1))


def test_torch_composition_with_a_batch_equals_the_series_one_by_one():
    name, n, d = L.BERNOULLI, 7, 3
    cases = [_case(seed, n, d, name) for seed in (0, 1, 2)]
    st = lambda k: tt(np.stack([cs[k] for cs in cases]).reshape((1, 3) + cases[0][k].shape))      # noqa: E731  (batch shape (1, 3))
    value = MM.dense_expected_log_likelihood_torch(mfa.Bernoulli(), st(0), st(3), st(1), st(2))
    assert tuple(value.shape) == (1, 3)
    for b, cs in enumerate(cases):
        want = VG.dense_expectations(L.LIKELIHOODS[name], *cs)
        np.testing.assert_allclose(value.numpy()[0, b], want["ve_sum"], rtol=1e-12, atol=1e-13)


def test_the_functions_error_paths():
    h, means, covs, y = (tt(a) for a in _case(1, 6, 3, L.BERNOULLI))
    lik = mfa.Bernoulli()
    for fn in (MM.dense_expected_log_likelihood, MM.dense_expected_log_likelihood_torch):
        with pytest.raises(TypeError, match="likelihood"):
            fn(None, h, y, means, covs)
        with pytest.raises(ValueError, match="y has shape"):
            fn(lik, h, y[:-1], means, covs)
        with pytest.raises(ValueError, match="means has shape"):
            fn(lik, h, y, means[..., :2], covs)
        with pytest.raises(ValueError, match="covs has shape"):
            fn(lik, h, y, means, covs[..., :2])
        with pytest.raises(ValueError, match="h must have shape"):
            fn(lik, h[0, :], y, means, covs)
        with pytest.raises(ValueError, match="means is torch.float32"):
            fn(lik, h, y, means.float(), covs)
        with pytest.raises(TypeError, match="float32 and float64"):
            fn(lik, h.long(), y, means, covs)
    big = 13
    with pytest.raises(NotImplementedError, match="dense_expected_log_likelihood_torch"):
        MM.dense_expected_log_likelihood(lik, torch.zeros(4, big, dtype=torch.float64), torch.zeros(4, dtype=torch.float64),
                                         torch.zeros(4, big, dtype=torch.float64), torch.zeros(4, big, big, dtype=torch.float64))
    with pytest.raises(NotImplementedError, match="no adjoint onto h"):
        MM.dense_expected_log_likelihood(lik, h.clone().requires_grad_(True), y, means, covs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MM.dense_expected_log_likelihood(lik, h, y, means, covs)


def test_the_constructors_error_paths_and_members():
    t = tt(np.array([[0.1, 0.5, 1.2, 2.0], [0.0, 0.4, 0.9, 3.0]]))
    y = tt(np.array([[0.0, 1.0, 1.0, 0.0], [1.0, 1.0, 0.0, 0.0]]))[..., None]
    kernel, lik = mfa.Matern32(lengthscale=1.0, variance=1.0), mfa.Bernoulli()
    with pytest.raises(ValueError, match="observations must have shape"):
        mfa.VariationalGaussianProcess((t, y[..., 0]), kernel, lik)
    with pytest.raises(ValueError, match="time_points must have shape"):
        mfa.VariationalGaussianProcess((t[..., :3], y), kernel, lik)
    with pytest.raises(TypeError, match="likelihood"):
        mfa.VariationalGaussianProcess((t, y), kernel, "bernoulli")
    with pytest.raises(TypeError, match="kernel"):
        mfa.VariationalGaussianProcess((t, y), None, lik)
    with pytest.raises(ValueError, match="strictly increasing"):
        mfa.VariationalGaussianProcess((torch.flip(t, dims=[-1]), y), kernel, lik)
    tied = t.clone()
    tied[0, 1] = tied[0, 0]
    with pytest.raises(ValueError, match="strictly increasing"):
        mfa.VariationalGaussianProcess((tied, y), kernel, lik)
    with pytest.raises(ValueError, match="at least two"):
        mfa.VariationalGaussianProcess((t[..., :1], y[..., :1, :]), kernel, lik)
    with pytest.raises(ValueError, match="time_points is torch.float32"):
        mfa.VariationalGaussianProcess((t.float(), y), kernel, lik)
    with pytest.raises(TypeError, match="initial_distribution"):
        mfa.VariationalGaussianProcess((t, y), kernel, lik, initial_distribution="prior")
    d = kernel.state_dim

    def chain(batch, n, dim):
        eye = torch.eye(dim, dtype=torch.float64)
        return mfa.StateSpaceModel(torch.zeros(batch + (dim,), dtype=torch.float64), eye.expand(batch + (dim, dim)).clone(),
                                   0.5 * eye.expand(batch + (n - 1, dim, dim)).clone(), torch.zeros(batch + (n - 1, dim), dtype=torch.float64),
                                   eye.expand(batch + (n - 1, dim, dim)).clone())

    for bad in (chain((3,), 4, d), chain((2,), 5, d), chain((2,), 4, d + 1)):
        with pytest.raises(ValueError, match="initial_distribution must be a chain on the time points"):
            mfa.VariationalGaussianProcess((t, y), kernel, lik, initial_distribution=bad)
    model = mfa.VariationalGaussianProcess((t, y), kernel, lik, initial_distribution=chain((2,), 4, d))
    assert model.time_points is t and model.observations is y and model.kernel is kernel and model.likelihood is lik
    assert len(model.trainable_variables) == 5 and all(v.requires_grad and v.is_leaf for v in model.trainable_variables)
    assert model.trainable_variables == model.dist_q.trainable_variables
    assert isinstance(model.posterior, mfa.ConditionalProcess)
    assert model._h.is_contiguous() and tuple(model._h.shape) == (2, 4, d) and tuple(model._y.shape) == (2, 4)
    assert not model._fused(), "CPU tensors take the torch composition"
    assert "VariationalGaussianProcess" in mfa.__all__


def test_the_dense_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "markovflow_amd.h")).read()
    declared = set(re.findall(r"\b(mf_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in ("mf_lik_dense_expectations_f64", "mf_lik_dense_expectations_f32", "mf_lik_dense_expectations_adjoint_f64",
                 "mf_lik_dense_expectations_adjoint_f32", "mf_lik_dense_expectations_workspace_bytes"):
        assert name in declared and name in _lib.exported_symbols() and getattr(lib, name) is not None


def test_workspace_formula_and_argument_errors_need_no_gpu():
    lib = _lib.load()
    size = lib.mf_lik_dense_expectations_workspace_bytes
    for bsz, n, elem in ((1, 1, 8), (3, 64, 8), (3, 65, 4), (64, 10000, 8), (2, 195, 4)):
        assert int(size(bsz, n, elem)) == bsz * ((n + 63) // 64) * elem
    assert int(size(0, 5, 8)) == 0 and int(size(5, 0, 8)) == 0 and int(size(-1, 5, 8)) == 0 and int(size(5, 5, 0)) == 0
    fn, adj = lib.mf_lik_dense_expectations_f64, lib.mf_lik_dense_expectations_adjoint_f64
    x, w = np.polynomial.hermite.hermgauss(20)
    import ctypes
    nodes, weights = (ctypes.c_double * 20)(*x), (ctypes.c_double * 20)(*w)
    nulls = [None] * 4
    call = lambda bsz=2, n=5, d=3, lik=1, nq=20: fn(bsz, n, d, lik, None, nq, nodes, weights, *nulls, None, 0, None, None, None, None)   # noqa: E731
    assert call(bsz=-1) == -1 and call(n=-1) == -2 and call(d=0) == -100 and call(d=13) == -100
    assert call(lik=9) == -4 and call(lik=0) == -5 and call(nq=0) == -6 and call(nq=33) == -6
    assert call() == 0, "every output NULL: nothing asked for, nothing launched"
    assert adj(-1, 5, 3, *([None] * 7)) == -1 and adj(2, -5, 3, *([None] * 7)) == -2 and adj(2, 5, 13, *([None] * 7)) == -100
    assert adj(2, 5, 3, *([None] * 7)) == 0
