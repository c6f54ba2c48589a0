"""
CPU tests of the multi-stage likelihood and of the multi-latent SVGP plumbing (markovflow_amd/likelihoods.py:
``MultiStageLikelihood``, ``torch_multistage_variational_expectations``; markovflow_amd/models/segmented_ops.py:
``sparse_multi_expected_log_likelihood_torch``; the constructors of the models), against tests/helpers/multistage_closed_forms.py.

Values against the helper at rtol 1e-12 / atol 1e-13, the figure tests/test_gpu_svgp.py uses for float64 against closed forms.

The model itself does not run on CPU tensors - its chain operators (pair marginals, KL divergence) and the kernel's transitions are
HIP kernels and say so; the ELBO at ``q = prior`` and the natural-gradient trajectory against the dense helper (N = 40, M = 5 among
its cases) are therefore in tests/test_gpu_multistage.py.  Here the same two quantities are checked as far as the CPU reaches: the
data term of the ELBO at the prior's pair marginals and on the helper's projections, through the CPU route
``sparse_multi_expected_log_likelihood_torch``, and the helper's dense loop against itself.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from markovflow_amd import models as MM
from helpers import multistage_closed_forms as MS
from helpers import sparse_cvi_closed_forms as SC

TOL = dict(rtol=1e-6, atol=1e-7)
TIGHT = dict(rtol=1e-12, atol=1e-13)
M32X3 = [dict(order=3, ls=ls, var=var, period=None, osc=0) for ls, var in ((1.0, 1.0), (2.0, 0.7), (0.5, 1.3))]
NEW = ("mf_lik_sparse_multi_expectations", "mf_lik_multistage_variational_expectations")


def tt(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def grid(seed=0, reps=6):
    """``(mu [N, 3], var [N, 3], y [N])``: every observation of ``MS.OBSERVED`` at ``reps`` random marginals."""
    rng = np.random.default_rng(seed)
    y = np.repeat(np.asarray(MS.OBSERVED), reps)
    return rng.normal(size=(y.size, 3)), rng.uniform(0.05, 2.0, size=(y.size, 3)), y


def test_header_declares_the_new_entry_points_and_the_library_exports_them():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "markovflow_amd.h")).read()
    lib = _lib.load()
    for base in NEW:
        for suf in ("_f64", "_f32"):
            assert base + suf in _lib.exported_symbols() and re.search(r"\bint " + base + suf + r"\(", header)
            assert getattr(lib, base + suf) is not None
    size = NEW[0] + "_workspace_bytes"
    assert size in _lib.exported_symbols() and re.search(r"\bsize_t " + size + r"\(", header)
    assert int(getattr(lib, size)(7, 12, 8)) == 7 * (78 + 12 + 1) * 8 and int(getattr(lib, size)(0, 12, 8)) == 0
    assert mfa.MultiStageLikelihood is mfa.likelihoods.MultiStageLikelihood and "MultiStageLikelihood" in mfa.__all__
    assert mfa.MultiStageLikelihood().latent_dim == 3
    assert [c().latent_dim for c in (mfa.Gaussian, mfa.Bernoulli, mfa.Poisson, mfa.StudentT)] == [1, 1, 1, 1]


@pytest.mark.parametrize("nq", [1, 20, 32])
def test_expectations_and_log_prob_against_the_helper(nq):
    mu, var, y = grid(nq)
    lik = mfa.MultiStageLikelihood(nq)
    (ve, gm, gv), _ = MS.expectations(mu, var, y, nq)
    fmu, fvar = tt(mu).requires_grad_(True), tt(var).requires_grad_(True)
    got = lik.variational_expectations(fmu, fvar, tt(y)[:, None])
    assert tuple(got.shape) == (y.size,)
    np.testing.assert_allclose(got.detach().numpy(), ve, **TIGHT)
    torch.sum(got).backward()
    np.testing.assert_allclose(fmu.grad.numpy(), gm, **TIGHT)
    np.testing.assert_allclose(fvar.grad.numpy(), gv, **TIGHT)
    np.testing.assert_allclose(lik.log_prob(tt(mu), tt(y)[:, None]).numpy(), MS.log_prob(mu, y), **TIGHT)
    # a batch shape in front, and the torch statement called directly
    ve3, gm3, gv3 = mfa.likelihoods.torch_multistage_variational_expectations(lik, tt(mu).reshape(2, -1, 3), tt(var).reshape(2, -1, 3),
                                                                              tt(y).reshape(2, -1, 1))
    assert tuple(ve3.shape) == (2, y.size // 2) and tuple(gm3.shape) == (2, y.size // 2, 3)
    np.testing.assert_allclose(ve3.reshape(-1).numpy(), ve, **TIGHT)
    np.testing.assert_allclose(gv3.reshape(-1, 3).numpy(), gv, **TIGHT)


def test_an_observation_outside_the_three_branches_contributes_exactly_zero():
    lik = mfa.MultiStageLikelihood()
    y = tt([0.5, -1.0, float("nan"), 1.5, -0.0])[:, None]
    fmu, fvar = tt(np.full((5, 3), 0.3)).requires_grad_(True), tt(np.full((5, 3), 0.8)).requires_grad_(True)
    ve = lik.variational_expectations(fmu, fvar, y)
    torch.sum(ve).backward()
    assert ve[:4].tolist() == [0.0] * 4 and float(ve.detach()[4]) != 0.0, "-0.0 == 0 is the first branch"
    assert float(fmu.grad[:4].abs().max()) == 0.0 and float(fvar.grad[:4].abs().max()) == 0.0
    assert lik.log_prob(fmu.detach(), y)[:4].tolist() == [0.0] * 4
    (ve_h, gm_h, gv_h), _ = MS.expectations(fmu.detach().numpy(), fvar.detach().numpy(), y[:, 0].numpy())
    assert ve_h[:4].tolist() == [0.0] * 4 and not gm_h[:4].any() and not gv_h[:4].any()


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan")])
def test_a_variance_outside_the_domain_matters_only_on_a_latent_that_is_read(bad):
    lik = mfa.MultiStageLikelihood()
    y = tt([0.0, 1.0, 1.0, 3.0, 3.0, 0.5])[:, None]
    var = np.full((6, 3), 0.6)
    hit = [(0, 1), (0, 2), (1, 2), (5, 0), (5, 1), (5, 2)]          # unread latents: everything stays finite and equal to the helper
    for k, l in hit:
        var[k, l] = bad
    mu = np.linspace(-1.0, 1.0, 18).reshape(6, 3)
    ve, gm, gv = lik._expectations(tt(mu), tt(var), y)
    assert bool(torch.isfinite(ve).all() and torch.isfinite(gm).all() and torch.isfinite(gv).all())
    (ve_h, gm_h, gv_h), _ = MS.expectations(mu, var, y[:, 0].numpy())
    np.testing.assert_allclose(ve.numpy(), ve_h, **TIGHT)
    np.testing.assert_allclose(gm.numpy(), gm_h, **TIGHT)
    np.testing.assert_allclose(gv.numpy(), gv_h, **TIGHT)
    assert all(float(gm[k, l]) == 0.0 and float(gv[k, l]) == 0.0 for k, l in hit)
    var[2, 1] = var[3, 0] = var[4, 2] = bad                          # read latents: NaN in the value and in that latent's derivatives
    ve, gm, gv = lik._expectations(tt(mu), tt(var), y)
    assert torch.isnan(ve).tolist() == [False, False, True, True, True, False]
    want = np.zeros((6, 3), dtype=bool)
    want[2, 1] = want[3, 0] = want[4, 2] = True
    assert np.array_equal(torch.isnan(gm).numpy(), want) and np.array_equal(torch.isnan(gv).numpy(), want)
    (ve_h, gm_h, gv_h), _ = MS.expectations(mu, var, y[:, 0].numpy())
    assert np.array_equal(np.isnan(ve_h), torch.isnan(ve).numpy()) and np.array_equal(np.isnan(gm_h), want)
    np.testing.assert_allclose(gm.numpy()[~want], gm_h[~want], **TIGHT)


def test_backward_matches_autograd_through_the_helper_and_is_differentiable_once():
    mu, var, y = grid(5)
    lik = mfa.MultiStageLikelihood()
    weights = tt(np.random.default_rng(1).normal(size=y.size))
    fmu, fvar = tt(mu).requires_grad_(True), tt(var).requires_grad_(True)
    torch.sum(weights * lik.variational_expectations(fmu, fvar, tt(y)[:, None])).backward()
    hmu, hvar = tt(mu).requires_grad_(True), tt(var).requires_grad_(True)
    value = MS.expectations_torch(hmu, hvar, y)
    np.testing.assert_allclose(value.detach().numpy(), MS.expectations(mu, var, y)[0][0], **TIGHT)
    torch.sum(weights * value).backward()
    np.testing.assert_allclose(fmu.grad.numpy(), hmu.grad.numpy(), **TIGHT)
    np.testing.assert_allclose(fvar.grad.numpy(), hvar.grad.numpy(), **TIGHT)
    fmu, fvar = tt(mu).requires_grad_(True), tt(var).requires_grad_(True)
    with pytest.raises(RuntimeError, match="differentiable once"):
        torch.autograd.grad(torch.sum(lik.variational_expectations(fmu, fvar, tt(y)[:, None])), (fmu, fvar), create_graph=True)


def test_shape_and_dtype_checks_and_the_methods_the_reference_does_not_have():
    lik = mfa.MultiStageLikelihood()
    f, y = torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 1, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        lik.variational_expectations(f[:, :1], f[:, :1], y)
    with pytest.raises(ValueError, match="fvar has shape"):
        lik.variational_expectations(f, f[:3], y)
    with pytest.raises(ValueError, match="y has shape"):
        lik.log_prob(f, y[:, 0])
    with pytest.raises(ValueError, match="y has shape"):
        lik.variational_expectations(f, f, f)
    with pytest.raises(TypeError, match="float32 and float64"):
        lik.log_prob(f.long(), y.long())
    with pytest.raises(ValueError, match="float32"):
        lik.log_prob(f, y.float())
    with pytest.raises(ValueError, match=r"batch \+ \[3\]"):
        lik.sample_y(torch.zeros(4, 2, dtype=torch.float64))
    for call in (lambda: lik.predict_log_density(f, f + 1, y), lambda: lik.predict_mean_and_var(f, f + 1),
                 lambda: lik.cvi_site_update(f, f + 1, y, 0.5, f.clone(), f.clone())):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(ValueError, match="num_gauss_hermite_points"):
        mfa.MultiStageLikelihood(33)


def test_sample_y_follows_the_decision_tree():
    lik = mfa.MultiStageLikelihood()
    n = 20000
    f = torch.tensor([0.0, 0.0, math.log(3.0)], dtype=torch.float64).expand(n, 3)
    draw = lik.sample_y(f, generator=torch.Generator().manual_seed(11))
    assert tuple(draw.shape) == (n, 1) and draw.dtype == torch.float64
    assert bool((draw >= 0).all() and (draw == torch.round(draw)).all())
    assert torch.equal(draw, lik.sample_y(f, generator=torch.Generator().manual_seed(11))), "a seeded generator reproduces the draw"
    assert tuple(lik.sample_y(torch.zeros(2, 5, 3, dtype=torch.float32)).shape) == (2, 5, 1)
    y = draw[:, 0].numpy()
    p0 = 0.5                                                          # inv_probit(0) = 0.5 (1 - 2e-3) + 1e-3
    for value, p in ((0.0, p0), (1.0, (1.0 - p0) * p0)):
        assert abs(np.mean(y == value) - p) <= 5.0 * math.sqrt(p * (1.0 - p) / n)
    counts = y[y >= 2] - 2.0
    assert abs(counts.mean() - 3.0) <= 5.0 * math.sqrt(3.0 / counts.size), "Poisson(3): variance 3"


def _cpu_chain(m, d):
    eye = torch.eye(d, dtype=torch.float64)
    return mfa.StateSpaceModel(torch.zeros(d, dtype=torch.float64), eye, (0.5 * eye).expand(m - 1, d, d).contiguous(),
                               torch.zeros(m - 1, d, dtype=torch.float64), eye.expand(m - 1, d, d).contiguous())


def test_every_model_but_svgp_refuses_a_multi_latent_likelihood():
    kernel = mfa.IndependentMultiOutput([mfa.Matern32(1.0, 1.0) for _ in range(3)])
    t = torch.linspace(0.0, 2.0, 6, dtype=torch.float64)
    data = (t, torch.zeros((6, 1), dtype=torch.float64))
    z = torch.linspace(0.0, 2.0, 3, dtype=torch.float64)
    lik = mfa.MultiStageLikelihood()
    zs, ks = torch.zeros((2, 1), dtype=torch.float64), mfa.spatial_kernels.SquaredExponential(1.0, 1.0)
    makers = {
        "CVIGaussianProcess": lambda: mfa.CVIGaussianProcess(data, kernel, lik),
        "PowerExpectationPropagation": lambda: mfa.PowerExpectationPropagation(data, kernel, lik),
        "SparseCVIGaussianProcess": lambda: mfa.SparseCVIGaussianProcess(kernel, z, lik),
        "SparsePowerExpectationPropagation": lambda: mfa.SparsePowerExpectationPropagation(kernel, z, lik),
        "ImportanceWeightedVI": lambda: mfa.ImportanceWeightedVI(kernel, z, lik, 4),
        "VariationalGaussianProcess": lambda: mfa.VariationalGaussianProcess(data, kernel, lik),
        "SpatioTemporalSparseVariational": lambda: mfa.SpatioTemporalSparseVariational(zs, z, ks, mfa.Matern32(1.0, 1.0), lik),
        "SpatioTemporalSparseCVI": lambda: mfa.SpatioTemporalSparseCVI(zs, z, ks, mfa.Matern32(1.0, 1.0), lik),
    }
    public = {n for n, c in vars(mfa.models).items()
              if n in mfa.__all__ and isinstance(c, type) and (c.__module__ + ".").startswith(mfa.models.__name__ + ".")}
    assert set(makers) | {"GaussianProcessRegression", "SparseVariationalGaussianProcess"} == public
    for name, make in makers.items():
        with pytest.raises(NotImplementedError, match="SparseVariationalGaussianProcess"):
            make()
    with pytest.raises(NotImplementedError, match="SparseVariationalGaussianProcess"):
        MM.sparse_expected_log_likelihood(lik, *([torch.zeros(1)] * 6))          # the single-latent fused op refuses it too
    # the one model that takes it (a chain given: the prior chain of the default comes from the HIP transition kernels)
    model = mfa.SparseVariationalGaussianProcess(kernel, lik, z, initial_distribution=_cpu_chain(3, 6))
    assert model.likelihood is lik and model.dist_q.state_dim == 6
    for wrong in (mfa.Matern32(1.0, 1.0), mfa.IndependentMultiOutput([mfa.Matern32(1.0, 1.0), mfa.Matern12(1.0, 1.0)])):
        with pytest.raises(ValueError, match="latent_dim = 3"):
            mfa.SparseVariationalGaussianProcess(wrong, lik, z, initial_distribution=_cpu_chain(3, wrong.state_dim))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.elbo(data)                                   # CPU tensors fail loudly at the chain kernels, as for every likelihood


def test_the_fused_function_refuses_what_it_cannot_do():
    lik = mfa.MultiStageLikelihood()
    n, segs, two_d = 5, 2, 6
    w, c, y = torch.zeros(n, 3, two_d, dtype=torch.float64), torch.ones(n, 3, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    off, pm = torch.tensor([0, 3, 5]), torch.zeros(segs, two_d, dtype=torch.float64)
    pc = torch.eye(two_d, dtype=torch.float64).expand(segs, two_d, two_d).contiguous()
    with pytest.raises(TypeError, match="likelihood"):
        MM.sparse_multi_expected_log_likelihood("multistage", w, c, y, off, pm, pc)
    with pytest.raises(ValueError, match="latent rows"):
        MM.sparse_multi_expected_log_likelihood(mfa.Bernoulli(), w, c, y, off, pm, pc)
    with pytest.raises(ValueError, match="latent rows"):
        MM.sparse_multi_expected_log_likelihood(lik, w[:, :2], c[:, :2], y, off, pm, pc)
    with pytest.raises(ValueError, match="c has shape"):
        MM.sparse_multi_expected_log_likelihood(lik, w, c[:, 0], y, off, pm, pc)
    with pytest.raises(NotImplementedError, match="no adjoint onto w and c"):
        MM.sparse_multi_expected_log_likelihood(lik, w.clone().requires_grad_(True), c, y, off, pm, pc)
    for bad in (4, 20):
        with pytest.raises(NotImplementedError, match="sparse_multi_expected_log_likelihood_torch"):
            MM.sparse_multi_expected_log_likelihood(lik, torch.zeros(n, 3, bad, dtype=torch.float64), c, y, off,
                                                    torch.zeros(segs, bad, dtype=torch.float64),
                                                    torch.zeros(segs, bad, bad, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MM.sparse_multi_expected_log_likelihood(lik, w, c, y, off, pm, pc)


def _series(n=40, seed=3):
    """Times on [0, 6] and observations drawn with ``sample_y`` from three smooth latents."""
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(0.0, 6.0, size=n))
    f = np.stack([np.sin(x) - 0.3, np.cos(1.3 * x), 0.8 + 0.5 * np.sin(0.7 * x)], axis=-1)
    y = mfa.MultiStageLikelihood().sample_y(tt(f), generator=torch.Generator().manual_seed(seed))[:, 0].numpy()
    return x, y


def test_the_composed_data_term_on_cpu_against_the_helper():
    """The data term of the ELBO at ``q = prior`` through the CPU route, on the helper's per-latent projections (the product's own
    come from HIP kernels: tests/test_gpu_multistage.py compares the two).  With the prior's pair marginals every point has
    ``(mu, s2) = (0, k_l(0))``, so the sum is ``sum_i VE(0, [k_l(0)]_l, y_i)`` (and the KL term of that ELBO is 0)."""
    x, y = _series()
    z = np.array([0.6, 1.9, 3.1, 4.2, 5.5])
    idx, w_h, c_h = MS.conditional_projections_multi(M32X3, x, z)
    w, c, indices = tt(w_h), tt(c_h), torch.as_tensor(idx)
    kuu = SC.dense_state_prior(M32X3, z)
    pinf = SC._transition(M32X3, 1.0)[2]
    pm, pc = SC.pair_marginals(np.zeros(kuu.shape[0]), kuu, pinf, 6)
    lik = mfa.MultiStageLikelihood()
    pair_mean, pair_cov = tt(pm).requires_grad_(True), tt(pc).requires_grad_(True)
    value = MM.sparse_multi_expected_log_likelihood_torch(lik, w, c, tt(y), indices, pair_mean, pair_cov)
    assert tuple(value.shape) == (6,)
    k0 = np.tile(np.array([comp["var"] for comp in M32X3]), (40, 1))
    want = MS.expectations(np.zeros((40, 3)), k0, y)[0][0]
    np.testing.assert_allclose(float(torch.sum(value.detach())), want.sum(), **TOL)
    seg = MS.segment_expectations_multi(w_h, c_h, y, SC.offsets_of(idx, 6), pm, pc)
    np.testing.assert_allclose(value.detach().numpy(), seg["ve_sum"], **TOL)
    torch.sum(value).backward()
    np.testing.assert_allclose(pair_mean.grad.numpy(), seg["g_mean"], **TOL)
    np.testing.assert_allclose(pair_cov.grad.numpy(), seg["g_cov"], **TOL)
    # a batch shape in front: the series one by one
    both = MM.sparse_multi_expected_log_likelihood_torch(lik, w.expand(2, 40, 3, 12), c.expand(2, 40, 3), tt(y).expand(2, 40),
                                                         indices.expand(2, 40), tt(pm).expand(2, 6, 12), tt(pc).expand(2, 6, 12, 12))
    assert tuple(both.shape) == (2, 6) and torch.equal(both[0], value.detach()) and torch.equal(both[1], value.detach())


def test_the_helpers_adjoints_are_the_gradients_of_its_own_value_and_its_dense_loop_climbs():
    rng = np.random.default_rng(2)
    lengths, two_d = (3, 0, 70, 1), 6
    n, segs = sum(lengths), len(lengths)
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    w, c = rng.uniform(-0.7, 0.7, size=(n, 3, two_d)), rng.uniform(0.05, 0.5, size=(n, 3))
    a = rng.normal(size=(segs, two_d, two_d))
    cov, mean = a @ a.transpose(0, 2, 1) / two_d + 0.1 * np.eye(two_d), rng.normal(size=(segs, two_d))
    y = np.resize(np.asarray(MS.OBSERVED), n)
    want = MS.segment_expectations_multi(w, c, y, offsets, mean, cov)
    pm, pc = tt(mean).requires_grad_(True), tt(cov).requires_grad_(True)
    value = MS.segment_value_torch_multi(w, c, y, offsets, pm, pc)
    eps = 2.0 ** -52
    assert np.all(np.abs(value.detach().numpy() - want["ve_sum"]) <= 64 * eps * (want["mag_ve_sum"] + 1))
    g_mean, g_cov = torch.autograd.grad(torch.sum(value), (pm, pc))
    assert np.all(np.abs(g_mean.numpy() - want["g_mean"]) <= 64 * eps * (want["mag_g_mean"] + 1))
    assert np.all(np.abs(g_cov.numpy() - want["g_cov"]) <= 64 * eps * (want["mag_g_cov"] + 1))
    assert want["ve_sum"][1] == 0.0 and not want["g_cov"][1].any(), "an empty segment"
    low = MS.segment_expectations_multi(w, c, y, offsets, mean, cov, dtype=np.float32)
    assert low["g_cov"].dtype == np.float32 and low["mag_g_cov"].dtype == np.float64
    np.testing.assert_allclose(low["ve_sum"], want["ve_sum"], rtol=1e-4, atol=1e-4)
    x, obs = _series()
    run = MS.DenseNatGradMulti(M32X3, x, obs, np.array([0.6, 1.9, 3.1, 4.2, 5.5]), gamma=0.05)
    k0 = np.tile(np.array([comp["var"] for comp in M32X3]), (40, 1))
    np.testing.assert_allclose(run.elbo(), MS.expectations(np.zeros((40, 3)), k0, obs)[0][0].sum(), **TOL)      # q = prior: KL = 0
    elbos = [run.elbo()]
    for _ in range(5):
        run.step()
        elbos.append(run.elbo())
    assert all(b > a for a, b in zip(elbos, elbos[1:])), "five natural-gradient steps at gamma = 0.05 climb"
    fmu, fvar = run.predict_f(np.array([0.1, 3.0, 5.9]))
    assert fmu.shape == (3, 3) and fvar.shape == (3, 3) and np.all(fvar > 0)
