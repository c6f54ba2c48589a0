"""
CPU tests of the stack kernels' plumbing (markovflow_amd/emission_model.py: ``StackEmissionModel``; markovflow_amd/kernels.py:
``StackKernel``, ``IndependentMultiOutputStack``; markovflow_amd/likelihoods.py: ``HeteroscedasticGaussian``;
markovflow_amd/models/segmented_ops.py: ``sparse_stack_expected_log_likelihood_torch``; the constructors of the models), against
einsum, autograd, Gauss-Hermite product rules and tests/helpers/stack_closed_forms.py.

Values against closed forms at rtol 1e-12 / atol 1e-13, the figure tests/test_multistage_host.py uses.  The heteroscedastic
expectation is checked against a 64-point Gauss-Hermite product rule at rtol 1e-10: on ``|m| <= 2``, ``v`` in [0.05, 1] the integrand
``exp(-F1)`` is entire and the rule's own error is far below that, which the test asserts first by comparing the 64-point rule with
a 96-point one.

The model itself does not run on CPU tensors (its chain operators are HIP kernels): tests/test_gpu_stack.py.
"""
import os
import re

import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from markovflow_amd import likelihoods as ML
from markovflow_amd import models as MM
from helpers import stack_closed_forms as ST

TIGHT = dict(rtol=1e-12, atol=1e-13)
NEW_SYMBOLS = ("mf_lik_stack_expectations_f64", "mf_lik_stack_expectations_f32", "mf_lik_stack_expectations_workspace_bytes")


def tt(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def test_new_symbols_in_header_and_table():
    header = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "markovflow_amd.h")
    text = open(header).read()
    names = set(_lib.exported_symbols())
    lib = _lib.load()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b" + sym + r"\(", text), sym
        assert sym in names, sym
        assert getattr(lib, sym) is not None
    size = lib.mf_lik_stack_expectations_workspace_bytes
    assert int(size(7, 18, 3, 8)) == 7 * (3 * (171 + 18) + 1) * 8 and int(size(7, 4, 2, 4)) == 7 * (2 * (10 + 4) + 1) * 4
    assert int(size(0, 4, 2, 4)) == 0 and int(size(7, 3, 2, 4)) == 0 and int(size(7, 20, 2, 4)) == 0
    for name in ("StackKernel", "IndependentMultiOutputStack", "StackEmissionModel", "HeteroscedasticGaussian"):
        assert name in mfa.__all__ and getattr(mfa, name) is not None


# ---- the emission model -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [(), (2,)])
def test_stack_emission_model_shapes_and_values_against_einsum(lead):
    rng = np.random.default_rng(0)
    k, n, d = 3, 5, 2
    h = rng.normal(size=lead + (k, n, 1, d))
    state, a = rng.normal(size=lead + (k, n, d)), rng.normal(size=lead + (k, n, d, d))
    cov = a @ np.swapaxes(a, -1, -2)
    em = mfa.StackEmissionModel(tt(h))
    assert em.output_dim == k and em.num_data == n and em.state_dim == d and tuple(em.batch_shape) == lead + (k,)
    f = em.project_state_to_f(tt(state))
    assert tuple(f.shape) == lead + (n, k)
    np.testing.assert_allclose(f.numpy(), np.einsum("...knd,...knd->...nk", h[..., 0, :], state), **TIGHT)
    want = np.einsum("...kni,...knij,...knj->...nk", h[..., 0, :], cov, h[..., 0, :])
    var = em.project_state_covariance_to_f(tt(cov))
    assert tuple(var.shape) == lead + (n, k)
    np.testing.assert_allclose(var.numpy(), want, **TIGHT)
    full = em.project_state_covariance_to_f(tt(cov), full_output_cov=True)
    assert tuple(full.shape) == lead + (n, k, k)
    np.testing.assert_allclose(full.numpy(), want[..., None] * np.eye(k), **TIGHT)
    both = em.project_state_marginals_to_f(tt(state), tt(cov), full_output_cov=True)
    assert torch.equal(both[0], f) and torch.equal(both[1], full)


def test_stack_emission_model_refusals():
    with pytest.raises(ValueError, match="at least 4D"):
        mfa.StackEmissionModel(torch.zeros(5, 1, 2))
    with pytest.raises(ValueError, match="ONE output"):
        mfa.StackEmissionModel(torch.zeros(3, 5, 2, 2))
    em = mfa.StackEmissionModel(torch.zeros(3, 5, 1, 2))
    with pytest.raises(ValueError):
        em.project_state_to_f(torch.zeros(5, 2))
    with pytest.raises(ValueError):
        em.project_state_covariance_to_f(torch.zeros(3, 5, 2, 3))


# ---- the kernels --------------------------------------------------------------------------------------------------------------------
def _children():
    return [mfa.Matern12(1.5, 0.9), mfa.Matern32(1.2, 1.1), mfa.Matern52(1.6, 0.8)]


def test_stack_kernel_properties_padding_and_the_batch_shape_check():
    jitter = 1e-3
    kern = mfa.IndependentMultiOutputStack(_children(), jitter=jitter)
    assert isinstance(kern, mfa.StackKernel) and isinstance(kern, mfa.StationaryKernel)
    assert kern.state_dim == 3 and kern.num_kernels == 3 and kern.output_dim == 3 and len(kern.kernels) == 3
    assert mfa.StackKernel(_children()).output_dim == 1
    f, p = kern.feedback_matrix, kern.steady_state_covariance
    assert tuple(f.shape) == (3, 3, 3) and tuple(p.shape) == (3, 1, 3, 3)
    for i, child in enumerate(kern.kernels):
        dk = child.state_dim
        assert torch.equal(f[i, :dk, :dk], child.feedback_matrix) and torch.equal(p[i, 0, :dk, :dk], child.steady_state_covariance)
        assert float(f[i, dk:].abs().sum()) == 0.0 and float(f[i, :, dk:].abs().sum()) == 0.0
        assert torch.equal(p[i, 0, dk:, dk:], torch.eye(3 - dk, dtype=torch.float64)) and float(p[i, 0, :dk, dk:].abs().sum()) == 0.0
    leaves = [x for c in kern._components() for x in c._leaves()]
    assert len(leaves) == 6 and all(any(x is y for y in leaves) for child in kern.kernels for x in child._leaves())
    t = torch.linspace(0.0, 1.0, 4, dtype=torch.float64).expand(2, 3, 4)
    assert tuple(kern.initial_mean((2, 3)).shape) == (2, 3, 3)
    p0 = kern.initial_covariance(t[..., :1])
    assert tuple(p0.shape) == (2, 3, 3, 3)
    np.testing.assert_allclose(p0[1, 0].numpy(), np.diag([0.9, 1.0 + jitter, 1.0 + jitter]), **TIGHT)
    em = kern.generate_emission_model(t)
    assert isinstance(em, mfa.StackEmissionModel) and tuple(em.emission_matrix.shape) == (2, 3, 4, 1, 3) and em.output_dim == 3
    assert torch.equal(em.emission_matrix[0, 1, 2, 0], torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64))
    for call in (lambda: kern.initial_mean((2,)), lambda: kern.initial_mean(()), lambda: kern.initial_covariance(t[:, :2, :1]),
                 lambda: kern.generate_emission_model(t[0, 0]), lambda: kern.state_transitions(t[:, :2, :-1], t[:, :2, 1:])):
        with pytest.raises(ValueError, match=r"\(\.\.\., 3\), got \("):
            call()


def test_stack_kernel_constructor_refusals_and_arithmetic():
    weights = lambda t: torch.ones(tuple(t.shape) + (2, 2), dtype=t.dtype)          # noqa: E731
    factor = mfa.FactorAnalysisKernel(weights, [mfa.Matern12(1.0, 1.0), mfa.Matern32(1.0, 1.0)], 2)
    piecewise = mfa.PiecewiseKernel([mfa.Matern12(1.0, 1.0), mfa.Matern12(2.0, 1.0)], torch.tensor([0.5], dtype=torch.float64))
    two = mfa.IndependentMultiOutput([mfa.Matern12(1.0, 1.0), mfa.Matern12(1.0, 1.0)])
    for cls in (mfa.StackKernel, mfa.IndependentMultiOutputStack):
        with pytest.raises(ValueError, match="at least one"):
            cls([])
        with pytest.raises(TypeError):
            cls([mfa.Matern12(1.0, 1.0), piecewise])
        with pytest.raises(TypeError):
            cls([factor])
        with pytest.raises(TypeError):
            cls([mfa.Matern12(1.0, 1.0), "matern"])
        with pytest.raises(ValueError, match="output_dim == 1"):
            cls([mfa.Matern12(1.0, 1.0), two])
    a = mfa.IndependentMultiOutputStack([mfa.Matern12(1.0, 1.0), mfa.Matern32(1.0, 1.0)], jitter=1e-6)
    b = mfa.IndependentMultiOutputStack([mfa.Matern32(2.0, 0.5), mfa.Matern12(2.0, 0.5)])
    total = a + b
    assert isinstance(total, mfa.IndependentMultiOutputStack) and total.num_kernels == 2 and total.state_dim == 3
    assert all(isinstance(k, mfa.Sum) for k in total.kernels) and total.kernels[0].kernels[0] is a.kernels[0]
    with pytest.raises(ValueError):
        a + mfa.IndependentMultiOutputStack(_children())
    with pytest.raises(NotImplementedError, match="StackKernel"):
        mfa.Sum([mfa.StackKernel([mfa.Matern12(1.0, 1.0)]), mfa.Matern12(1.0, 1.0)])


def test_every_model_but_the_svgp_refuses_a_stack_kernel():
    kern = mfa.IndependentMultiOutputStack([mfa.Matern12(1.0, 1.0), mfa.Matern32(1.0, 1.0)])
    t = torch.linspace(0.0, 1.0, 6, dtype=torch.float64)
    xy, z, lik = (t, torch.zeros(6, 1, dtype=torch.float64)), t[::2].clone(), mfa.Gaussian(0.5)
    space = torch.zeros(2, 1, dtype=torch.float64)
    from markovflow_amd import spatial_kernels
    builders = [lambda: mfa.GaussianProcessRegression(xy, kern), lambda: mfa.VariationalGaussianProcess(xy, kern, lik),
                lambda: mfa.CVIGaussianProcess(xy, kern, lik), lambda: mfa.PowerExpectationPropagation(xy, kern, lik),
                lambda: mfa.SparseCVIGaussianProcess(kern, z, lik), lambda: mfa.SparsePowerExpectationPropagation(kern, z, lik),
                lambda: mfa.ImportanceWeightedVI(kern, z, lik, 4),
                lambda: mfa.SpatioTemporalSparseVariational(space, z, spatial_kernels.Matern32(1.0, 1.0), kern, lik),
                lambda: mfa.SpatioTemporalSparseCVI(space, z, spatial_kernels.Matern32(1.0, 1.0), kern, lik)]
    for build in builders:
        with pytest.raises(NotImplementedError, match="SparseVariationalGaussianProcess"):
            build()
    with pytest.raises(NotImplementedError, match="IndependentMultiOutputStack"):
        mfa.SparseVariationalGaussianProcess(mfa.StackKernel([mfa.Matern12(1.0, 1.0), mfa.Matern32(1.0, 1.0)]), lik, z.expand(2, 3))
    with pytest.raises(ValueError, match=r"\(\.\.\., 2\)"):
        mfa.SparseVariationalGaussianProcess(kern, lik, z)                            # inducing points without the chain dimension
    with pytest.raises(ValueError, match="latent_dim"):
        mfa.SparseVariationalGaussianProcess(kern, mfa.MultiStageLikelihood(), z.expand(2, 3))


# ---- the heteroscedastic Gaussian ---------------------------------------------------------------------------------------------------
def _marginals(n=40, seed=1):
    rng = np.random.default_rng(seed)
    return rng.uniform(-2.0, 2.0, size=(n, 2)), rng.uniform(0.05, 1.0, size=(n, 2)), rng.normal(scale=1.5, size=n)


def test_heteroscedastic_expectation_against_the_gauss_hermite_product_rule_and_the_helper():
    mu, var, y = _marginals()
    q64, q96 = ST.gauss_hermite_product(mu, var, y, 64), ST.gauss_hermite_product(mu, var, y, 96)
    np.testing.assert_allclose(q64, q96, rtol=1e-12, atol=0.0, err_msg="the 64-point rule has converged on these inputs")
    lik = mfa.HeteroscedasticGaussian()
    assert lik.latent_dim == 2 and lik._id == 5
    ve = lik.variational_expectations(tt(mu), tt(var), tt(y)[:, None])
    assert tuple(ve.shape) == (40,)
    np.testing.assert_allclose(ve.numpy(), q64, rtol=1e-10, atol=0.0)
    (ve_h, gm_h, gv_h), _ = ST.hetero_expectations(mu, var, y)
    got = lik._expectations(tt(mu), tt(var), tt(y)[:, None])
    for g, want in zip(got, (ve_h, gm_h, gv_h)):
        np.testing.assert_allclose(g.numpy(), want, **TIGHT)
    f = np.random.default_rng(2).normal(size=(40, 2))
    np.testing.assert_allclose(lik.log_prob(tt(f), tt(y)[:, None]).numpy(), ST.hetero_log_prob(f, y), **TIGHT)


def test_heteroscedastic_derivatives_against_autograd_of_the_torch_statement_and_differentiable_once():
    mu, var, y = _marginals(seed=3)
    lik = mfa.HeteroscedasticGaussian()
    fmu, fvar = tt(mu).requires_grad_(True), tt(var).requires_grad_(True)
    want = torch.autograd.grad(torch.sum(ML.torch_heteroscedastic_variational_expectations(fmu, fvar, tt(y)[:, None])), (fmu, fvar))
    ve = lik.variational_expectations(fmu, fvar, tt(y)[:, None])
    got = torch.autograd.grad(torch.sum(ve), (fmu, fvar))
    for g, w in zip(got, want):
        np.testing.assert_allclose(g.numpy(), w.numpy(), **TIGHT)
    m0, m1, v0, v1 = mu[:, 0], mu[:, 1], var[:, 0], var[:, 1]
    e = np.exp(-m1 + 0.5 * v1)
    big = e * ((m0 - y) ** 2 + v0)
    np.testing.assert_allclose(got[0].numpy(), np.stack([-e * (m0 - y), -0.5 * (1.0 - big)], axis=-1), **TIGHT)
    np.testing.assert_allclose(got[1].numpy(), np.stack([-0.5 * e, -0.25 * big], axis=-1), **TIGHT)
    again = lik.variational_expectations(fmu, fvar, tt(y)[:, None])
    with pytest.raises(RuntimeError, match="differentiable once"):
        torch.autograd.grad(torch.sum(again), (fmu, fvar), create_graph=True)


def test_heteroscedastic_predictions_the_nan_rule_and_what_is_not_available():
    mu, var, y = _marginals(n=8, seed=4)
    lik = mfa.HeteroscedasticGaussian()
    mean, variance = lik.predict_mean_and_var(tt(mu), tt(var))
    assert tuple(mean.shape) == (8, 1) and tuple(variance.shape) == (8, 1)
    np.testing.assert_allclose(mean.numpy()[:, 0], mu[:, 0], **TIGHT)
    np.testing.assert_allclose(variance.numpy()[:, 0], var[:, 0] + np.exp(mu[:, 1] + 0.5 * var[:, 1]), **TIGHT)
    bad = var.copy()
    bad[1, 0], bad[2, 1], bad[3, 0], bad[4, 1] = 0.0, -1.0, float("nan"), float("nan")
    ve, g_mu, g_var = lik._expectations(tt(mu), tt(bad), tt(y)[:, None])
    rows = np.array([False, True, True, True, True, False, False, False])
    assert np.array_equal(np.isnan(ve.numpy()), rows)
    assert np.array_equal(np.isnan(g_mu.numpy()), np.repeat(rows[:, None], 2, axis=1))
    assert np.array_equal(np.isnan(g_var.numpy()), np.repeat(rows[:, None], 2, axis=1))
    (ve_h, gm_h, gv_h), _ = ST.hetero_expectations(mu, bad, y)
    assert np.array_equal(np.isnan(ve_h), rows) and np.array_equal(np.isnan(gm_h), np.isnan(g_mu.numpy()))
    with pytest.raises(NotImplementedError):
        lik.predict_log_density(tt(mu), tt(var), tt(y)[:, None])
    for name in ("cvi_site_update", "log_expected_density", "grad_log_expected_density", "pep_site_update"):
        with pytest.raises(NotImplementedError, match="two latent functions"):
            getattr(lik, name)(tt(mu), tt(var), tt(y)[:, None])
    with pytest.raises(ValueError):
        lik.variational_expectations(tt(mu[:, :1]), tt(var[:, :1]), tt(y)[:, None])
    sample = lik.sample_y(tt(mu), generator=torch.Generator().manual_seed(0))
    assert tuple(sample.shape) == (8, 1) and bool(torch.isfinite(sample).all())
    with pytest.raises(NotImplementedError, match="latent_dim > 1"):
        mfa.CVIGaussianProcess((torch.zeros(4, dtype=torch.float64), torch.zeros(4, 1, dtype=torch.float64)), mfa.Matern12(1.0, 1.0), lik)


# ---- the torch composition ----------------------------------------------------------------------------------------------------------
def _segments(rng, lat, n, segs, two_d):
    cuts = np.sort(rng.integers(0, n + 1, size=segs - 1))
    offsets = np.concatenate([[0], cuts, [n]]).astype(np.int64)
    a = rng.normal(size=(lat, segs, two_d, two_d))
    return dict(offsets=offsets, indices=np.repeat(np.arange(segs), np.diff(offsets)), w=rng.uniform(-0.7, 0.7, size=(lat, n, two_d)),
                c=rng.uniform(0.05, 0.5, size=(lat, n)), pair_mean=rng.normal(size=(lat, segs, two_d)),
                pair_cov=a @ a.transpose(0, 1, 3, 2) / two_d + 0.1 * np.eye(two_d))


@pytest.mark.parametrize("lik_id", [ST.MULTISTAGE, ST.HETERO])
def test_torch_composition_against_the_helper_with_a_shared_segmentation(lik_id):
    rng = np.random.default_rng(lik_id)
    lat, n, segs, two_d = ST.LATENTS[lik_id], 150, 5, 4
    lik = mfa.MultiStageLikelihood() if lik_id == ST.MULTISTAGE else mfa.HeteroscedasticGaussian()
    series = [_segments(rng, lat, n, segs, two_d) for _ in range(2)]
    y = [np.resize(np.array([0.0, 1.0, 2.0, 5.0, 0.5]), n) if lik_id == ST.MULTISTAGE else rng.normal(size=n) for _ in range(2)]
    stack = lambda key: tt(np.stack([s[key] for s in series]))          # noqa: E731
    pm, pc = stack("pair_mean").requires_grad_(True), stack("pair_cov").requires_grad_(True)
    out = MM.sparse_stack_expected_log_likelihood_torch(lik, stack("w"), stack("c"), tt(np.stack(y)),
                                                        torch.as_tensor(np.stack([s["indices"] for s in series])), pm, pc)
    assert tuple(out.shape) == (2, segs)
    g_mean, g_cov = torch.autograd.grad(torch.sum(out), (pm, pc))
    for b, s in enumerate(series):
        want = ST.segment_expectations_stack(s["w"], s["c"], y[b], s["offsets"], s["pair_mean"], s["pair_cov"], lik_id)
        np.testing.assert_allclose(out[b].detach().numpy(), want["ve_sum"], **TIGHT)
        np.testing.assert_allclose(g_mean[b].numpy(), want["g_mean"], **TIGHT)
        np.testing.assert_allclose(g_cov[b].numpy(), want["g_cov"], **TIGHT)


def test_torch_composition_with_per_chain_segmentations_and_per_chain_orders():
    """Chains with segmentations of their own: the total over the segments is the sum over the points of the likelihood's expectation
    at the per-chain marginals, whatever pair a point is booked on; and rows permuted per chain with ``orders`` give the same total."""
    rng = np.random.default_rng(7)
    lat, n, segs, two_d = 2, 90, 4, 6
    lik = mfa.HeteroscedasticGaussian()
    chains = [_segments(rng, lat, n, segs, two_d) for _ in range(lat)]           # chain k uses its own offsets; w, c, pairs of draw 0
    base, y = chains[0], rng.normal(size=n)
    indices = np.stack([chains[k]["indices"] for k in range(lat)])
    fmu = np.stack([np.einsum("ni,ni->n", base["w"][k], base["pair_mean"][k][indices[k]]) for k in range(lat)], axis=-1)
    fvar = np.stack([base["c"][k] + np.einsum("ni,nij,nj->n", base["w"][k], base["pair_cov"][k][indices[k]], base["w"][k])
                     for k in range(lat)], axis=-1)
    want = ST.hetero_expectations(fmu, fvar, y)[0][0]
    args = (tt(base["w"]), tt(base["c"]), tt(y), torch.as_tensor(indices), tt(base["pair_mean"]), tt(base["pair_cov"]))
    out = MM.sparse_stack_expected_log_likelihood_torch(lik, *args)
    assert tuple(out.shape) == (segs,)
    np.testing.assert_allclose(out.numpy(), np.bincount(indices[0], weights=want, minlength=segs), **TIGHT)
    orders = np.stack([rng.permutation(n) for _ in range(lat)])
    take = lambda a: np.stack([a[k][orders[k]] for k in range(lat)])          # noqa: E731  (chain k's rows in the order orders[k])
    permuted = MM.sparse_stack_expected_log_likelihood_torch(lik, tt(take(base["w"])), tt(take(base["c"])), tt(y),
                                                             torch.as_tensor(take(indices)), tt(base["pair_mean"]), tt(base["pair_cov"]),
                                                             orders=torch.as_tensor(orders))
    np.testing.assert_allclose(permuted.numpy(), out.numpy(), **TIGHT)
    with pytest.raises(ValueError, match="chains"):
        MM.sparse_stack_expected_log_likelihood_torch(mfa.MultiStageLikelihood(), *args)
    with pytest.raises(NotImplementedError):
        MM.sparse_stack_expected_log_likelihood(mfa.HeteroscedasticGaussian(), tt(np.zeros((2, 5, 20))), tt(np.ones((2, 5))),
                                                tt(np.zeros(5)), torch.tensor([0, 5]), tt(np.zeros((2, 1, 20))),
                                                tt(np.zeros((2, 1, 20, 20))))
