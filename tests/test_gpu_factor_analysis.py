"""
GPU tests of ``SparseVariationalGaussianProcess`` with multi-output observations: a ``FactorAnalysisKernel`` (the fused data term
``mf_lik_sparse_factor_expectations_*`` and its torch composition) and any other kernel with several outputs
(``sparse_multi_output_expected_log_likelihood_torch``); ``GaussianProcessRegression`` with the kernel through its generic route.

B = 2 series, N = 150 points, M = 12 inducing points, [Matern52, Matern32] (2d = 10, L = 2), P = 5 observed series and the
factor-analysis notebook's weight function A(t) = t (x) A0, float64.

Tolerances.  The fused route against the torch composition on the same model: 1e-9 relative (value, the gradients onto the leaves of
``dist_q`` and onto the loading matrix); the loading matrix's gradient against a central difference of the fused ELBO: 1e-6 relative
(h = 1e-5: the rounding term 1e-16 |elbo| / h is 1e-7 for |elbo| < 1e4 and the truncation h^2 f''' / 6 smaller still, against 1e-6 of
a gradient whose largest entry exceeds 1 - both asserted); the selecting kernel against ``IndependentMultiOutput``: 1e-10 relative; ``GaussianProcessRegression`` against the dense Gaussian
log density: 1e-9 relative.  float32: the fused ELBO against the composed one to 2e-4 relative, and - the construction of
tests/test_gpu_multistage.py - against the float64 ELBO within S x 4 x e32 x (largest segment magnitude + 1) summed over the series,
e32 the normalised error of the helper evaluated in numpy float32.
"""
import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from helpers import factor_closed_forms as FC
from helpers import likelihood_closed_forms as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SPAN = 4.0
B, N, M, P = 2, 150, 12, 5
A0 = 0.35 * np.array([[1.0, 0.3], [-0.5, 0.8], [0.2, -1.1], [0.9, 0.4], [-0.7, -0.2]])
NOISE = 0.3
FUSED = "mf_lik_sparse_factor_expectations"


def tt(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def nn(t):
    return t.detach().cpu().numpy()


def children(dtype=torch.float64, first_ls=1.3):
    return [mfa.Matern52(first_ls, 0.8, device=DEV, dtype=dtype), mfa.Matern32(0.6, 1.4, device=DEV, dtype=dtype)]


def time_weights(t):
    return t[..., None, None] * torch.as_tensor(A0, dtype=t.dtype, device=t.device)


def factor_kernel(dtype=torch.float64, trainable=True, first_ls=1.3):
    return mfa.FactorAnalysisKernel(time_weights, children(dtype, first_ls), output_dim=P, trainable=trainable)


_SERIES = {}


def series(name=L.GAUSSIAN, n=N):
    """``(x [B, n], y [B, n, P], z [B, M])``, read-only: one time per cell of an even grid on [0, SPAN], the inducing points likewise;
    ``y`` from two smooth latents mixed by A(t): Gaussian noise, or Poisson counts of exp(f)."""
    if (name, n) not in _SERIES:
        rng = np.random.default_rng(11)
        x = (np.arange(n) + 0.5 + rng.uniform(-0.3, 0.3, size=(B, n))) * SPAN / n
        z = (np.arange(M) + 0.5 + rng.uniform(-0.2, 0.2, size=(B, M))) * SPAN / M
        g = np.stack([np.sin(1.7 * x + 0.3), 0.8 * np.cos(2.3 * x)], axis=-1)                   # [B, n, 2]
        f = np.einsum("bn,pl,bnl->bnp", x, A0, g)
        y = f + np.sqrt(NOISE) * rng.normal(size=f.shape) if name == L.GAUSSIAN else rng.poisson(np.exp(f)).astype(np.float64)
        for a in (x, y, z):
            a.setflags(write=False)
        _SERIES[(name, n)] = (x, y, z)
    return _SERIES[(name, n)]


def likelihood(name=L.GAUSSIAN):
    return mfa.Gaussian(NOISE) if name == L.GAUSSIAN else mfa.Poisson()


def build_model(kernel, z, name=L.GAUSSIAN, dtype=torch.float64, **kwargs):
    return mfa.SparseVariationalGaussianProcess(kernel, likelihood(name), tt(z, dtype), **kwargs)


def moved_model(kernel, xy, z, steps=2):
    """A model whose ``q`` is not the prior: a few natural-gradient steps with the loading matrix held."""
    model = build_model(kernel, z)
    opt = mfa.SSMNaturalGradient(gamma=0.1, momentum=False)
    for _ in range(steps):
        opt.minimize(lambda: model.loss(xy), model.dist_q)
    return model


def spy(monkeypatch):
    seen = []
    real_rc = _lib.call_rc
    monkeypatch.setattr(_lib, "call_rc", lambda base, *a: (seen.append(base), real_rc(base, *a))[1])
    return seen


def close(a, b, rel, what):
    a, b = nn(a), nn(b)
    err, scale = float(np.abs(a - b).max()), float(np.abs(b).max())
    print(f"REL {what}: {err / scale if scale else err:.3e}")
    assert err <= rel * scale, f"{what}: {err:.3e} against {rel} x {scale:.3e}"


def test_fused_elbo_and_its_gradients_against_the_torch_route_with_a_fixed_loading_matrix(monkeypatch):
    x, y, z = series()
    xy = (tt(x), tt(y))
    kernel = factor_kernel(trainable=False)
    model = moved_model(kernel, xy, z)
    leaves = model.trainable_variables
    seen = spy(monkeypatch)
    fused = model.elbo(xy)
    assert seen.count(FUSED) == 1 and not any(s.startswith("mf_lik_") and s != FUSED for s in seen)
    del seen[:]
    g_fused = torch.autograd.grad(fused, leaves)
    assert not any(s.startswith("mf_lik_") for s in seen), "the backward reuses the forward's adjoints: no second launch"
    cached = model._projection_cache
    model.elbo(xy)
    assert model._projection_cache is cached, "wg, cg, the sort order and the tile table are cached"
    monkeypatch.setattr(model, "_fused", lambda time_points: False)
    del seen[:]
    composed = model.elbo(xy)
    assert FUSED not in seen and "mf_lik_variational_expectations" in seen
    g_composed = torch.autograd.grad(composed, leaves)
    close(fused, composed, 1e-9, "elbo fused against composed")
    for i, (a, b) in enumerate(zip(g_fused, g_composed)):
        close(a, b, 1e-9, f"gradient onto leaf {i} of dist_q")


def test_loading_matrix_gradient_from_the_fused_route_against_the_torch_route_and_central_differences(monkeypatch):
    x, y, z = series()
    xy = (tt(x), tt(y))
    kernel = factor_kernel()
    with torch.no_grad():
        kernel.loading_matrix.copy_(tt([[1.1, -0.3], [0.2, 0.8]]))
    model = moved_model(kernel, xy, z)
    b = kernel.loading_matrix
    assert b.requires_grad and model._fused(xy[0]) and not kernel._needs_grad()
    seen = spy(monkeypatch)
    cached = model._projection_cache
    fused = model.elbo(xy)
    assert seen.count(FUSED) == 1 and model._projection_cache is cached, "a trainable loading matrix stays on the fused path"
    (g_fused,) = torch.autograd.grad(fused, b)
    monkeypatch.setattr(model, "_fused", lambda time_points: False)
    (g_composed,) = torch.autograd.grad(model.elbo(xy), b)
    monkeypatch.undo()
    close(g_fused, g_composed, 1e-9, "loading matrix gradient fused against composed")
    h, fd = 1e-5, torch.zeros_like(b)
    with torch.no_grad():
        for i in range(2):
            for j in range(2):
                vals = []
                for sign in (1.0, -1.0):
                    b[i, j] += sign * h
                    vals.append(float(model.elbo(xy)))
                    b[i, j] -= sign * h
                fd[i, j] = (vals[0] - vals[1]) / (2.0 * h)
        assert model._projection_cache is cached, "a step on the loading matrix keeps the cached projections"
    assert float(g_fused.abs().max()) > 1.0 and abs(float(fused.detach())) < 1e4
    close(g_fused, fd, 1e-6, "loading matrix gradient against central differences")


def test_a_lengthscale_under_the_tape_takes_the_torch_route_and_gets_its_gradient(monkeypatch):
    x, y, z = series()
    xy = (tt(x), tt(y))
    trained = moved_model(factor_kernel(trainable=False), xy, z)
    ls = torch.tensor(1.3, dtype=torch.float64, device=DEV, requires_grad=True)
    kernel = factor_kernel(first_ls=ls)
    model = build_model(kernel, z, initial_distribution=trained.dist_q)
    seen = spy(monkeypatch)
    value = model.elbo(xy)
    assert FUSED not in seen and kernel._needs_grad()
    g_ls, g_b = torch.autograd.grad(value, [ls, kernel.loading_matrix])
    assert np.isfinite(float(g_ls)) and float(g_ls) != 0.0 and float(g_b.abs().max()) > 0.0
    with torch.no_grad():
        close(value, trained.elbo(xy), 1e-9, "elbo through the graph against the fused elbo")
    assert FUSED in seen


def test_a_selecting_weight_function_gives_the_multi_output_elbo_of_independent_multi_output(monkeypatch):
    """P = L = 2, A = I, B = I: f = g, so the factor route must agree with the plain multi-output term on
    ``IndependentMultiOutput`` - another kernel class, other projections (dense rows w [N, P, 2d]) and another function."""
    x, y, z = series()
    xy = (tt(x), tt(y[..., :2]))
    eye = lambda t: torch.eye(2, dtype=t.dtype, device=t.device).expand(tuple(t.shape) + (2, 2)).contiguous()      # noqa: E731
    select = mfa.FactorAnalysisKernel(eye, children(), output_dim=2, trainable=False)
    factor = moved_model(select, xy, z)
    plain = build_model(mfa.IndependentMultiOutput(children()), z, initial_distribution=factor.dist_q)
    seen = spy(monkeypatch)
    with torch.no_grad():
        a = factor.elbo(xy)
        assert seen.count(FUSED) == 1
        del seen[:]
        b = plain.elbo(xy)
        assert not any(s.startswith("mf_lik_sparse") for s in seen) and "mf_lik_variational_expectations" in seen
    close(a, b, 1e-10, "selecting factor kernel against IndependentMultiOutput")
    g_a = torch.autograd.grad(factor.elbo(xy), factor.trainable_variables)
    g_b = torch.autograd.grad(plain.elbo(xy), plain.trainable_variables)
    for i, (u, v) in enumerate(zip(g_a, g_b)):
        close(u, v, 1e-9, f"gradient onto leaf {i}: factor against multi-output")
    # observations [N, 1] keep the single-output path on either kernel
    del seen[:]
    with torch.no_grad():
        one = plain.elbo((xy[0], xy[1][..., :1]))
    assert "mf_lik_sparse_expectations" in seen and np.isfinite(float(one))


def test_the_elbo_of_shuffled_data_has_the_bits_of_the_sorted_data(monkeypatch):
    x, y, z = series()
    perm = np.stack([np.random.default_rng(5 + b).permutation(N) for b in range(B)])
    xs, ys = np.take_along_axis(x, perm, 1), np.take_along_axis(y, perm[..., None], 1)
    model = moved_model(factor_kernel(), (tt(x), tt(y)), z)
    with torch.no_grad():
        assert torch.equal(model.elbo((tt(x), tt(y))), model.elbo((tt(xs), tt(ys))))
        monkeypatch.setattr(model, "_fused", lambda time_points: False)
        close(model.elbo((tt(xs), tt(ys))), model.elbo((tt(x), tt(y))), 1e-12, "composed route, shuffled against sorted")


@pytest.mark.parametrize("name", [L.GAUSSIAN, L.POISSON])
def test_natural_gradient_steps_alternated_with_adam_on_the_loading_matrix_do_not_decrease_the_elbo(name, monkeypatch):
    x, y, z = series(name)
    xy = (tt(x), tt(y))
    kernel = factor_kernel()
    model = build_model(kernel, z, name)
    with torch.no_grad():
        start = float(model.elbo(xy))
    seen = spy(monkeypatch)
    natgrad = mfa.SSMNaturalGradient(0.5)
    adam = torch.optim.Adam([kernel.loading_matrix], lr=0.01)
    for _ in range(10):
        natgrad.minimize(lambda: model.loss(xy), model.dist_q)
        adam.zero_grad()
        model.loss(xy).backward()
        adam.step()
    with torch.no_grad():
        end = float(model.elbo(xy))
    print(f"ELBO {name}: {start:.4f} -> {end:.4f}")
    assert np.isfinite(end) and end >= start
    assert seen.count(FUSED) >= 20 and "mf_lik_variational_expectations" not in seen, "every step stayed on the fused path"
    assert not torch.equal(kernel.loading_matrix.detach(), torch.eye(2, dtype=torch.float64, device=DEV))


def test_predictions_have_one_column_per_output_and_the_latents_one_per_latent():
    x, y, z = series()
    kernel = factor_kernel()
    model = moved_model(kernel, (tt(x), tt(y)), z)
    t_new = tt(np.sort(np.random.default_rng(2).uniform(-0.5, SPAN + 0.5, size=(B, 9)), axis=-1))
    mean, var = model.predict_f(t_new)
    assert tuple(mean.shape) == (B, 9, P) and tuple(var.shape) == (B, 9, P) and bool((var > 0).all())
    assert tuple(model.predict_f(t_new, full_output_cov=True)[1].shape) == (B, 9, P, P)
    with torch.no_grad():
        s_mean, s_cov = model.posterior.predict_state(t_new)
        g_mean, g_cov = kernel.generate_emission_model(t_new).project_state_marginals_to_g(s_mean, s_cov)
        l_mean, l_var = kernel.latent_emission_model(t_new).project_state_marginals_to_f(s_mean, s_cov)
        w = kernel.mixing_weights(t_new)
    assert tuple(g_mean.shape) == (B, 9, 2) and tuple(g_cov.shape) == (B, 9, 2, 2) and tuple(l_var.shape) == (B, 9, 2)
    assert torch.equal(g_mean, l_mean) and bool((l_var > 0).all())
    close((w @ g_mean[..., None])[..., 0], mean, 1e-12, "f = W g")
    close(torch.sum((w @ g_cov) * w, dim=-1), var, 1e-12, "var f = diag(W Sig_g W^T)")


def test_refusals():
    x, y, z = series()
    model = build_model(factor_kernel(), z)
    with pytest.raises(ValueError, match=r"\[num_data, 1\]"):
        model.elbo((tt(x), tt(y[..., :3])))
    with pytest.raises(NotImplementedError, match="several outputs"):
        model.predict_log_density((tt(x[:, :9]), tt(y[:, :9])))
    five = mfa.IndependentMultiOutput([mfa.Matern12(1.0, 1.0, device=DEV) for _ in range(P)])
    iw = mfa.ImportanceWeightedVI(five, tt(z), mfa.Gaussian(NOISE), 4)
    with pytest.raises(ValueError, match=r"\[num_data, 1\]"):
        iw.elbo((tt(x), tt(y)))
    with pytest.raises(NotImplementedError, match="FactorAnalysisKernel"):
        mfa.ImportanceWeightedVI(factor_kernel(), tt(z), mfa.Gaussian(NOISE), 4)
    multi = mfa.SparseVariationalGaussianProcess(mfa.IndependentMultiOutput(children() + children()[:1]), mfa.MultiStageLikelihood(), tt(z))
    with pytest.raises(ValueError, match=r"\[num_data, 1\]"):
        multi.elbo((tt(x), tt(y[..., :3])))


def test_a_float32_model_agrees_with_the_composed_route_and_with_the_float64_elbo(monkeypatch):
    x, y, z = series()
    model64 = moved_model(factor_kernel(trainable=False), (tt(x), tt(y)), z)
    with torch.no_grad():
        exact = float(model64.elbo((tt(x), tt(y))))
        pair_mean, pair_cov = model64._pair_marginals()
        mix = model64.kernel.mixing_weights(tt(x))
    _, wg, cg, _, offsets, _ = model64._projections(tt(x))
    r32 = lambda t: nn(t).astype(np.float32).astype(np.float64)          # noqa: E731
    bound = 0.0
    for b in range(B):
        args = (L.GAUSSIAN, (NOISE,)), r32(wg[b]), r32(cg[b]), r32(mix[b]), r32(tt(y)[b]), nn(offsets[b]), r32(pair_mean[b]), r32(pair_cov[b])
        want, low = FC.segment_expectations_factor(*args), FC.segment_expectations_factor(*args, dtype=np.float32)
        e32 = float((np.abs(low["ve_sum"].astype(np.float64) - want["ve_sum"]) / (want["mag_ve_sum"] + 1.0)).max())
        bound += (M + 1) * 4.0 * e32 * (float(want["mag_ve_sum"].max()) + 1.0)
    q64 = model64.dist_q
    q32 = mfa.StateSpaceModel(*(t.detach().to(torch.float32) for t in (q64.initial_mean, q64.cholesky_initial_covariance,
                                                                        q64.state_transitions, q64.state_offsets,
                                                                        q64.cholesky_process_covariances)))
    model32 = build_model(factor_kernel(torch.float32, trainable=False), z, dtype=torch.float32, initial_distribution=q32)
    xy32 = (tt(x, torch.float32), tt(y, torch.float32))
    seen = spy(monkeypatch)
    elbo32 = model32.elbo(xy32)
    assert elbo32.dtype == torch.float32 and seen.count(FUSED) == 1
    torch.autograd.grad(elbo32, model32.trainable_variables)
    monkeypatch.setattr(model32, "_fused", lambda time_points: False)
    with torch.no_grad():
        composed = model32.elbo(xy32)
    got = float(elbo32.detach())
    print(f"ERR f32 elbo: |elbo32 - elbo64| {abs(got - exact):.3e}  bound {bound:.3e}  (|elbo| {abs(exact):.3f})")
    close(elbo32, composed, 2e-4, "float32 elbo fused against composed")
    assert abs(got - exact) <= bound


def test_gaussian_process_regression_takes_the_kernel_through_its_generic_route():
    n = 40
    x, y, _ = series(n=n)
    kernel = factor_kernel(trainable=False)
    chol = tt(np.sqrt(NOISE) * np.eye(P))
    gpr = mfa.GaussianProcessRegression((tt(x), tt(y)), kernel, chol_obs_covariance=chol)
    with torch.no_grad():
        got = float(gpr.log_likelihood())
    want = 0.0
    for b in range(B):
        weights = x[b][:, None, None] * A0
        cov = FC.factor_prior_covariance([(5, 1.3, 0.8, x[b]), (3, 0.6, 1.4, x[b])], weights)
        want += FC.dense_gaussian_log_density(cov, y[b], NOISE)
    print(f"REL gpr log_likelihood: {abs(got - want) / abs(want):.3e}")
    assert abs(got - want) <= 1e-9 * abs(want)
