"""
CPU tests of the factor-analysis kernel and of the multi-output SVGP plumbing (markovflow_amd/emission_model.py:
``ComposedPairEmissionModel``; markovflow_amd/kernels.py: ``FactorAnalysisKernel``; markovflow_amd/models/segmented_ops.py:
``sparse_factor_expected_log_likelihood_torch``, ``sparse_multi_output_expected_log_likelihood_torch``; the constructors of the
models), against explicit numpy products and tests/helpers/factor_closed_forms.py.

Values against numpy at rtol 1e-12 / atol 1e-13, the figure tests/test_multistage_host.py uses for float64 against closed forms; the
two torch compositions against each other (value and autograd gradients) to 1e-10 relative.

The models themselves do not run on CPU tensors (their chain operators are HIP kernels): ``elbo``, ``predict_f`` and the fused data
term are in tests/test_gpu_factor_analysis.py and tests/test_gpu_factor_kernel.py.
"""
import os
import re

import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from markovflow_amd import models as MM
from helpers import factor_closed_forms as FC
from helpers import likelihood_closed_forms as L

TIGHT = dict(rtol=1e-12, atol=1e-13)
FN = "mf_lik_sparse_factor_expectations"


def tt(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def children():
    return [mfa.Matern52(lengthscale=1.3, variance=0.8), mfa.Matern32(lengthscale=0.6, variance=1.4)]


A0 = np.array([[1.0, 0.3], [-0.5, 0.8], [0.2, -1.1], [0.9, 0.4], [-0.7, -0.2]])


def time_weights(t):
    """``A(t) = t (x) A0``, the factor-analysis notebook's weight function."""
    return t[..., None, None] * torch.as_tensor(A0, dtype=t.dtype, device=t.device)


def factor_kernel(**kwargs):
    return mfa.FactorAnalysisKernel(time_weights, children(), output_dim=5, **kwargs)


def test_header_declares_the_new_entry_points_and_the_library_exports_them():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "markovflow_amd.h")).read()
    lib = _lib.load()
    assert FN in _lib._SIGS and len(_lib._SIGS[FN][1]) == 28
    for suf in ("_f64", "_f32"):
        assert FN + suf in _lib.exported_symbols() and re.search(r"\bint " + FN + suf + r"\(", header)
        assert getattr(lib, FN + suf) is not None
    size = FN + "_workspace_bytes"
    assert size in _lib.exported_symbols() and re.search(r"\bsize_t " + size + r"\(", header)
    for tiles, two_d, elem in ((7, 12, 8), (3, 18, 4), (0, 10, 8)):
        assert int(getattr(lib, size)(tiles, two_d, elem)) == int(lib.mf_lik_sparse_expectations_workspace_bytes(tiles, two_d, elem))
    assert int(getattr(lib, size)(7, 12, 8)) == 7 * (78 + 12 + 1) * 8
    for name in ("FactorAnalysisKernel", "ComposedPairEmissionModel"):
        assert name in mfa.__all__ and getattr(mfa, name) is not None
    assert mfa.FactorAnalysisKernel is mfa.kernels.FactorAnalysisKernel


def test_entry_point_argument_checks_return_before_a_launch():
    """Every check below returns its code before anything touches a device: -(position), and -101 for what is not instantiated."""
    import ctypes
    nq = 20
    x, w = np.polynomial.hermite.hermgauss(nq)
    nodes, weights = (ctypes.c_double * nq)(*x), (ctypes.c_double * nq)(*w)
    var = (ctypes.c_double * 1)(0.7)
    tail = [*([None] * 7), 0, None, None, None, 0, None, None, None, None, None]
    call = lambda *a: _lib.call_rc(FN, torch.float64, *a)                # noqa: E731
    ok = (1, 0, 1, 10, 2, 5, 0, var, nq, nodes, weights)
    assert call(*ok, *tail) == 0, "N = 0 and no output: nothing to do"
    for pos, value, want in ((0, -1, -1), (1, -1, -2), (2, 0, -3), (5, 0, -6), (6, 4, -7), (6, -1, -7), (7, None, -8), (8, 0, -9),
                             (8, 33, -9), (9, None, -10), (10, None, -11), (4, 5, -101), (4, 1, -101), (3, 9, -101), (3, 2, -101),
                             (3, 20, -101), (5, 1025, -101)):
        args = list(ok)
        args[pos] = value
        assert call(*args, *tail) == want, (pos, value)
    assert call(1, 0, 1, 6, 4, 5, 0, var, nq, nodes, weights, *tail) == -101, "2d < 2 L"
    assert call(1, 0, 1, 8, 4, 5, 0, var, nq, nodes, weights, *tail) == 0
    bad_tiles = list(tail)
    bad_tiles[7] = 3
    assert call(*ok, *bad_tiles) == -19, "tiles without points"
    with pytest.raises(NotImplementedError, match="not instantiated"):
        _lib.call(FN, torch.float64, 1, 0, 1, 10, 5, 5, 0, var, nq, nodes, weights, *tail)


@pytest.mark.parametrize("batch", [(), (2,)])
def test_composed_pair_emission_model_against_numpy(batch):
    rng = np.random.default_rng(3)
    n, p, l, d = 7, 5, 2, 5
    outer, inner = rng.normal(size=batch + (n, p, l)), rng.normal(size=batch + (n, l, d))       # the outer matrix varies in time
    mean, root = rng.normal(size=batch + (n, d)), rng.normal(size=batch + (n, d, d))
    cov = root @ np.swapaxes(root, -1, -2)
    em = mfa.ComposedPairEmissionModel(mfa.EmissionModel(tt(outer)), mfa.EmissionModel(tt(inner)))
    h = outer @ inner
    assert (em.output_dim, em.inner_dim, em.state_dim, em.num_data) == (p, l, d, n) and isinstance(em, mfa.EmissionModel)
    np.testing.assert_allclose(em.emission_matrix.numpy(), h, **TIGHT)
    np.testing.assert_allclose(em.inner_emission_matrix.numpy(), inner, **TIGHT)
    np.testing.assert_allclose(em.project_state_to_f(tt(mean)).numpy(), np.einsum("...pd,...d->...p", h, mean), **TIGHT)
    np.testing.assert_allclose(em.project_state_to_g(tt(mean)).numpy(), np.einsum("...ld,...d->...l", inner, mean), **TIGHT)
    full_f, full_g = h @ cov @ np.swapaxes(h, -1, -2), inner @ cov @ np.swapaxes(inner, -1, -2)
    np.testing.assert_allclose(em.project_state_covariance_to_f(tt(cov), full_output_cov=True).numpy(), full_f, **TIGHT)
    np.testing.assert_allclose(em.project_state_covariance_to_f(tt(cov)).numpy(), np.diagonal(full_f, axis1=-2, axis2=-1), **TIGHT)
    np.testing.assert_allclose(em.project_state_covariance_to_g(tt(cov)).numpy(), full_g, **TIGHT)       # full by default
    np.testing.assert_allclose(em.project_state_covariance_to_g(tt(cov), full_output_cov=False).numpy(),
                               np.diagonal(full_g, axis1=-2, axis2=-1), **TIGHT)
    g_mean, g_cov = em.project_state_marginals_to_g(tt(mean), tt(cov))
    np.testing.assert_allclose(g_mean.numpy(), np.einsum("...ld,...d->...l", inner, mean), **TIGHT)
    np.testing.assert_allclose(g_cov.numpy(), full_g, **TIGHT)
    assert tuple(em.project_state_marginals_to_g(tt(mean), tt(cov), full_output_cov=False)[1].shape) == batch + (n, l)
    f_mean, f_var = em.project_state_marginals_to_f(tt(mean), tt(cov))
    assert tuple(f_mean.shape) == batch + (n, p) and tuple(f_var.shape) == batch + (n, p)
    # under autograd: the gradient of sum(H_outer H_inner x) with respect to the outer matrix is x^T H_inner^T per row
    outer_t = tt(outer).requires_grad_(True)
    em2 = mfa.ComposedPairEmissionModel(mfa.EmissionModel(outer_t), mfa.EmissionModel(tt(inner)))
    torch.sum(em2.project_state_to_f(tt(mean))).backward()
    want = np.broadcast_to(np.einsum("...ld,...d->...l", inner, mean)[..., None, :], outer.shape)
    np.testing.assert_allclose(outer_t.grad.numpy(), want, **TIGHT)
    with pytest.raises(ValueError, match="does not compose"):
        mfa.ComposedPairEmissionModel(mfa.EmissionModel(tt(outer)), mfa.EmissionModel(tt(rng.normal(size=batch + (n, l + 1, d)))))


def test_factor_analysis_kernel_is_independent_multi_output_with_a_mixed_emission():
    kernel, imo = factor_kernel(), mfa.IndependentMultiOutput(children())
    assert (kernel.state_dim, kernel.output_dim, kernel.latent_dim) == (5, 5, 2)
    assert isinstance(kernel, mfa.kernels.ConcatKernel) and len(kernel._components()) == 2
    for got, want in ((kernel.feedback_matrix, imo.feedback_matrix), (kernel.steady_state_covariance, imo.steady_state_covariance),
                      (kernel.initial_mean(()), imo.initial_mean(()))):
        assert torch.equal(got, want)
    dt = tt([0.1, 0.7, 2.0])
    for got, want in zip(kernel._torch_transitions(dt, True, True), imo._torch_transitions(dt, True, True)):
        assert (got is None and want is None) or torch.equal(got, want), "A, chol Q and Q are the children's"
    b = kernel.loading_matrix
    assert b.is_leaf and b.requires_grad and b.dtype == torch.float64 and torch.equal(b.detach(), torch.eye(2, dtype=torch.float64))
    assert kernel.trainable_variables == (b,)
    fixed = factor_kernel(trainable=False)
    assert not fixed.loading_matrix.requires_grad and fixed.trainable_variables == ()
    assert all(x is not b for comp in kernel._components() for x in comp._leaves()), "not a hyper-parameter of the chain"
    assert not kernel._needs_grad(), "the loading matrix under the tape is not a chain hyper-parameter under the tape"
    single = mfa.FactorAnalysisKernel(time_weights, [mfa.Matern32(1.0, 1.0, dtype=torch.float32)] * 2, output_dim=5)
    assert single.loading_matrix.dtype == torch.float32
    # the emission: A(t) B H_inner, with B != I
    with torch.no_grad():
        b.copy_(tt([[1.2, -0.4], [0.3, 0.7]]))
    t = tt([[0.2, 0.9, 1.7], [0.0, 0.5, 3.0]])
    em = kernel.generate_emission_model(t)
    assert isinstance(em, mfa.ComposedPairEmissionModel) and em.inner_dim == 2
    h_inner = imo.generate_emission_model(t).emission_matrix.numpy()
    want = (t.numpy()[..., None, None] * A0) @ b.detach().numpy() @ h_inner
    np.testing.assert_allclose(em.emission_matrix.detach().numpy(), want, **TIGHT)
    np.testing.assert_allclose(kernel.mixing_weights(t).detach().numpy(), (t.numpy()[..., None, None] * A0) @ b.detach().numpy(), **TIGHT)
    assert torch.equal(kernel.latent_emission_model(t).emission_matrix, imo.generate_emission_model(t).emission_matrix)
    assert torch.equal(em.inner_emission_matrix, kernel.latent_emission_model(t).emission_matrix)
    torch.sum(em.emission_matrix).backward()
    assert b.grad is not None and float(b.grad.abs().max()) > 0.0


def test_factor_analysis_kernel_refuses_what_it_cannot_mix():
    t = tt([0.1, 0.4, 2.0])
    for bad, shape in ((lambda x: x[..., None, None] * tt(A0[:4]), r"\(3, 4, 2\)"), (lambda x: tt(A0), r"\(5, 2\)"),
                       (lambda x: x[..., None, None] * tt(A0.T), r"\(3, 2, 5\)")):
        with pytest.raises(ValueError, match=shape):
            mfa.FactorAnalysisKernel(bad, children(), output_dim=5).mixing_weights(t)
    with pytest.raises(ValueError, match=r"\(3, 5, 2\).*float32"):
        mfa.FactorAnalysisKernel(lambda x: (x[..., None, None] * tt(A0)).float(), children(), output_dim=5).generate_emission_model(t)
    with pytest.raises(ValueError, match="output_dim == 1"):
        mfa.FactorAnalysisKernel(time_weights, [mfa.Matern32(1.0, 1.0, output_dim=2), mfa.Matern12(1.0, 1.0, output_dim=2)], output_dim=5)
    change = mfa.PiecewiseKernel([mfa.Matern32(1.0, 1.0), mfa.Matern32(2.0, 1.0)], tt([1.0]))
    with pytest.raises(NotImplementedError, match="non-stationary"):
        mfa.FactorAnalysisKernel(time_weights, [mfa.Matern32(1.0, 1.0), change], output_dim=5)
    leg = mfa.LatentExponentiallyGenerated(tt(np.eye(2)), tt(np.zeros((2, 2))), output_dim=1)
    with pytest.raises(NotImplementedError, match="LatentExponentiallyGenerated"):
        mfa.FactorAnalysisKernel(time_weights, [mfa.Matern32(1.0, 1.0), leg], output_dim=5)


def test_models_written_for_one_observed_series_refuse_the_kernel_at_construction():
    kernel, lik = factor_kernel(trainable=False), mfa.Gaussian(0.7)
    t, z = tt(np.linspace(0.0, 3.0, 6)), tt([0.5, 1.5, 2.5])
    data = (t, torch.zeros(6, 1, dtype=torch.float64))
    space = mfa.spatial_kernels
    kernel_space = next(getattr(space, n) for n in dir(space) if isinstance(getattr(space, n), type)
                        and issubclass(getattr(space, n), space.SpatialKernel) and getattr(space, n) is not space.SpatialKernel)
    for build in (lambda: mfa.CVIGaussianProcess(data, kernel, lik), lambda: mfa.PowerExpectationPropagation(data, kernel, lik),
                  lambda: mfa.SparseCVIGaussianProcess(kernel, z, lik), lambda: mfa.SparsePowerExpectationPropagation(kernel, z, lik),
                  lambda: mfa.VariationalGaussianProcess(data, kernel, lik), lambda: mfa.ImportanceWeightedVI(kernel, z, lik, 4),
                  lambda: mfa.SpatioTemporalSparseVariational(torch.zeros(2, 1, dtype=torch.float64), z, kernel_space(1.0, 1.0), kernel, lik),
                  lambda: mfa.SpatioTemporalSparseCVI(torch.zeros(2, 1, dtype=torch.float64), z, kernel_space(1.0, 1.0), kernel, lik)):
        with pytest.raises(NotImplementedError, match="FactorAnalysisKernel"):
            build()


def test_prior_covariance_of_f_is_the_weighted_sum_of_the_matern_covariances():
    """With ``B != I``: ``Cov[f(t), f(t')] = H(t) expm(F (t - t')) P_inf H(t')^T`` for ``t >= t'``, built from the kernel's emission and
    state-space matrices, against ``sum_l W_.l(t) k_l(t - t') W_.l(t')^T`` from the Matern formulas."""
    kernel = factor_kernel()
    with torch.no_grad():
        kernel.loading_matrix.copy_(tt([[1.2, -0.4], [0.3, 0.7]]))
    times = np.array([0.3, 0.35, 1.0, 2.2, 4.0])
    t = tt(times)
    with torch.no_grad():
        h = kernel.generate_emission_model(t).emission_matrix
        f, pinf = kernel.feedback_matrix, kernel.steady_state_covariance
        got = np.zeros((5, 5, 5, 5))
        for i in range(5):
            for j in range(5):
                lo, hi = (j, i) if times[i] >= times[j] else (i, j)
                block = h[hi] @ torch.linalg.matrix_exp(f * float(times[hi] - times[lo])) @ pinf @ h[lo].T          # [P(hi), P(lo)]
                got[i, :, j, :] = (block if hi == i else block.T).numpy()
        weights = kernel.mixing_weights(t).numpy()
    want = FC.factor_prior_covariance([(5, 1.3, 0.8, times), (3, 0.6, 1.4, times)], weights)
    np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-12)


def factor_inputs(seed, poisson, n=23, lat=2, two_d=6, outs=5, segs=4, batch=()):
    """Random inputs inside the domain: S_pair SPD + 0.1 I, Cg = c c^T / L + 0.05 I, wg in +-0.7, W in +-1 (+-0.5: Poisson)."""
    rng = np.random.default_rng(seed)
    a, c = rng.normal(size=batch + (segs, two_d, two_d)), rng.normal(size=batch + (n, lat, lat))
    d = dict(wg=rng.uniform(-0.7, 0.7, size=batch + (n, lat, two_d)), cg=c @ np.swapaxes(c, -1, -2) / lat + 0.05 * np.eye(lat),
             mix=rng.uniform(-0.5, 0.5, size=batch + (n, outs, lat)) * (1.0 if poisson else 2.0),
             y=rng.integers(0, 10, size=batch + (n, outs)).astype(np.float64) if poisson else rng.normal(size=batch + (n, outs)),
             pair_cov=a @ np.swapaxes(a, -1, -2) / two_d + 0.1 * np.eye(two_d), pair_mean=rng.normal(size=batch + (segs, two_d)))
    cuts = np.sort(rng.integers(0, n + 1, size=batch + (segs - 1,)), axis=-1)
    d["offsets"] = np.concatenate([np.zeros(batch + (1,), dtype=np.int64), cuts, np.full(batch + (1,), n)], axis=-1)
    d["indices"] = (np.arange(n) >= d["offsets"][..., 1:-1, None]).sum(axis=-2)
    return d


@pytest.mark.parametrize("name", [L.GAUSSIAN, L.POISSON])
def test_torch_composition_against_the_numpy_helper(name):
    lik = mfa.Gaussian(0.7) if name == L.GAUSSIAN else mfa.Poisson()
    d = factor_inputs(1, name == L.POISSON, batch=(2,))
    args = [tt(d[k]) for k in ("wg", "cg", "mix", "y")] + [torch.tensor(d["indices"])] + [tt(d["pair_mean"]), tt(d["pair_cov"])]
    for i in (2, 5, 6):
        args[i].requires_grad_(True)
    got = MM.sparse_factor_expected_log_likelihood_torch(lik, *args)
    assert tuple(got.shape) == (2, 4)
    torch.sum(got).backward()
    for b in range(2):
        want = FC.segment_expectations_factor(L.LIKELIHOODS[name], d["wg"][b], d["cg"][b], d["mix"][b], d["y"][b], d["offsets"][b],
                                              d["pair_mean"][b], d["pair_cov"][b])
        np.testing.assert_allclose(got[b].detach().numpy(), want["ve_sum"], **TIGHT)
        np.testing.assert_allclose(args[5].grad[b].numpy(), want["g_mean"], **TIGHT)
        np.testing.assert_allclose(args[6].grad[b].numpy(), want["g_cov"], **TIGHT)
        np.testing.assert_allclose(args[2].grad[b].numpy(), want["g_w"], **TIGHT)


@pytest.mark.parametrize("name", [L.GAUSSIAN, L.POISSON, L.BERNOULLI])
def test_factor_composition_against_the_plain_multi_output_composition_on_the_composed_rows(name):
    lik = {L.GAUSSIAN: mfa.Gaussian(0.7), L.POISSON: mfa.Poisson(), L.BERNOULLI: mfa.Bernoulli()}[name]
    d = factor_inputs(2, name == L.POISSON, lat=3, two_d=8)
    if name == L.BERNOULLI:
        d["y"] = (d["y"] > 0).astype(np.float64)
    idx = torch.tensor(d["indices"])
    wg, cg, y = tt(d["wg"]), tt(d["cg"]), tt(d["y"])
    leaves_a = [tt(d[k]).requires_grad_(True) for k in ("pair_mean", "pair_cov", "mix")]
    leaves_b = [tt(d[k]).requires_grad_(True) for k in ("pair_mean", "pair_cov", "mix")]
    factor = MM.sparse_factor_expected_log_likelihood_torch(lik, wg, cg, leaves_a[2], y, idx, leaves_a[0], leaves_a[1])
    mix = leaves_b[2]
    w, c = mix @ wg, torch.einsum("kpl,klq,kpq->kp", mix, cg, mix)                          # w_p = sum_l W_pl wg_l, c_p = W_p Cg W_p^T
    np.testing.assert_allclose(w.detach().numpy(), FC.composed_rows(d["wg"], d["cg"], d["mix"])[0], **TIGHT)
    plain = MM.sparse_multi_output_expected_log_likelihood_torch(lik, w, c, y, idx, leaves_b[0], leaves_b[1])
    scale = float(plain.detach().abs().max())
    assert float((factor - plain).detach().abs().max()) <= 1e-10 * scale
    weights = tt(np.random.default_rng(0).normal(size=4))
    torch.sum(weights * factor).backward()
    torch.sum(weights * plain).backward()
    for a, b in zip(leaves_a, leaves_b):
        assert float((a.grad - b.grad).abs().max()) <= 1e-10 * float(b.grad.abs().max())


def test_fused_function_checks_its_arguments_before_any_launch():
    d = factor_inputs(4, False)
    lik = mfa.Gaussian(0.7)
    wg, cg, mix, y, pm, pc = (tt(d[k]) for k in ("wg", "cg", "mix", "y", "pair_mean", "pair_cov"))
    off = torch.tensor(d["offsets"])
    with pytest.raises(NotImplementedError, match="sparse_factor_expected_log_likelihood_torch"):
        MM.sparse_factor_expected_log_likelihood(lik, wg.clone().requires_grad_(True), cg, mix, y, off, pm, pc)
    five = factor_inputs(4, False, lat=5, two_d=10)
    with pytest.raises(NotImplementedError, match="L = 5"):
        MM.sparse_factor_expected_log_likelihood(lik, *(tt(five[k]) for k in ("wg", "cg", "mix", "y")), torch.tensor(five["offsets"]),
                                                 tt(five["pair_mean"]), tt(five["pair_cov"]))
    with pytest.raises(ValueError, match="cg has shape"):
        MM.sparse_factor_expected_log_likelihood(lik, wg, cg[..., 0], mix, y, off, pm, pc)
    with pytest.raises(ValueError, match="y has shape"):
        MM.sparse_factor_expected_log_likelihood_torch(lik, wg, cg, mix, y[..., :3], torch.tensor(d["indices"]), pm, pc)
