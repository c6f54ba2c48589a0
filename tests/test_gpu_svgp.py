"""
GPU tests of ``SparseVariationalGaussianProcess`` (markovflow_amd/models.py) and ``SSMNaturalGradient`` (markovflow_amd/ssm_natgrad.py)
against dense references: the dense sparse CVI loop of tests/helpers/sparse_cvi_closed_forms.py (a natural-gradient step without
momentum IS a CVI step at ``lr = gamma``), the dense natural-gradient loop of tests/helpers/svgp_closed_forms.py (momentum), the
GPR model and Titsias' collapsed bound (the conjugate case).

State space against dense: rtol 1e-6 / atol 1e-7, the ``TOL`` of tests/test_gpu_sparse_cvi.py, unless a test says otherwise.  The
kernels carry jitter 0 and so do the dense loops.  Every series has at most 33 points and at most 8 inducing points.
"""
import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib, conditionals
from markovflow_amd import likelihoods as ML
from markovflow_amd import models as MM
from helpers import likelihood_closed_forms as L
from helpers import sparse_cvi_closed_forms as SC
from helpers import svgp_closed_forms as SV

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = dict(rtol=1e-6, atol=1e-7)
M12 = [dict(order=1, ls=1.0, var=1.0, period=None, osc=0)]
M32 = [dict(order=3, ls=1.0, var=1.0, period=None, osc=0)]
M52_M32 = [dict(order=5, ls=1.3, var=0.8, period=None, osc=0), dict(order=3, ls=0.6, var=0.5, period=None, osc=0)]
D10 = [dict(order=5, ls=1.3, var=0.8, period=None, osc=0), dict(order=5, ls=0.9, var=0.4, period=None, osc=0),
       dict(order=3, ls=0.6, var=0.5, period=None, osc=0), dict(order=3, ls=1.1, var=0.3, period=None, osc=0)]
KERNELS = {"m12": M12, "m32": M32, "m52+m32": M52_M32, "d10": D10}
Z5 = np.array([0.6, 1.9, 3.1, 4.2, 5.5])          # five inducing points inside the data's span [0, 6]


def tt(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def nn(t):
    return t.detach().cpu().numpy()


def build_kernel(comps, dtype=torch.float64):
    cls = {1: mfa.Matern12, 3: mfa.Matern32, 5: mfa.Matern52}
    parts = [cls[c["order"]](c["ls"], c["var"], device=DEV, dtype=dtype) for c in comps]
    return parts[0] if len(parts) == 1 else mfa.Sum(parts)


def build_likelihood(name):
    params = L.LIKELIHOODS[name][1]
    return {L.GAUSSIAN: lambda: mfa.Gaussian(params[0]), L.BERNOULLI: mfa.Bernoulli, L.POISSON: mfa.Poisson}[name]()


def build_model(name, comps, z, dtype=torch.float64, **kwargs):
    return mfa.SparseVariationalGaussianProcess(build_kernel(comps, dtype), build_likelihood(name), tt(z, dtype), **kwargs)


def data(x, y, dtype=torch.float64):
    return tt(x, dtype), tt(y, dtype)[..., None]


def natgrad_steps(model, xy, steps, **kwargs):
    opt = mfa.SSMNaturalGradient(**kwargs)
    for _ in range(steps):
        opt.minimize(lambda: model.loss(xy), model.dist_q)
    return opt


def q_marginals(model):
    with torch.no_grad():
        means, covs = model.dist_q.marginals
    return nn(means), nn(covs)


def compare_q_with_dense(model, mu, sigma, where, tol=TOL):
    """``dist_q``'s marginal means and covariances against a dense Gaussian over the stacked states."""
    means, covs = q_marginals(model)
    m, d = means.shape[-2:]
    np.testing.assert_allclose(means, mu.reshape(m, d), err_msg=f"marginal means {where}", **tol)
    blocks = np.stack([sigma[i * d:(i + 1) * d, i * d:(i + 1) * d] for i in range(m)])
    np.testing.assert_allclose(covs, blocks, err_msg=f"marginal covariances {where}", **tol)


_SERIES = {}


def series(name, comps_key, num_points, seed, separated=False):
    key = (name, comps_key, num_points, seed, separated)
    if key not in _SERIES:
        x, y = L.draw_series(L.LIKELIHOODS[name], KERNELS[comps_key], num_points, seed, separated=separated)
        x.setflags(write=False)
        y.setflags(write=False)
        _SERIES[key] = (x, y)
    return _SERIES[key]


# ---- the optimum -------------------------------------------------------------------------------------------------------------------
def test_at_the_gpr_posterior_the_elbo_is_the_log_likelihood_and_its_gradient_vanishes():
    """The reference's set-up (tests/integration/models/test_sparse_variational.py:32-147): Matern-1/2, lengthscale 2, variance
    2.25, unit noise, 8 points, Z = X, q = the GPR posterior; its atol 1e-9 on the gradient."""
    rng = np.random.default_rng(8)
    x, y = np.sort(rng.uniform(0.0, 8.0, 8)), rng.normal(size=8)
    kernel = mfa.Matern12(2.0, 2.25, device=DEV)
    xy = data(x, y)
    gpr = mfa.GaussianProcessRegression(xy, kernel, chol_obs_covariance=tt(np.eye(1)))
    model = mfa.SparseVariationalGaussianProcess(kernel, mfa.Gaussian(1.0), tt(x), initial_distribution=gpr.posterior_state_space_model())
    elbo = model.elbo(xy)
    np.testing.assert_allclose(float(elbo.detach()), float(gpr.log_likelihood()), rtol=1e-7)
    elbo.backward()
    for leaf in model.trainable_variables:
        assert leaf.grad is not None
        np.testing.assert_allclose(nn(leaf.grad), 0.0, atol=1e-9)


# ---- fused against composed --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,comps_key", [(L.BERNOULLI, "m32"), (L.POISSON, "m32"), (L.GAUSSIAN, "m12"), (L.BERNOULLI, "m52+m32")])
def test_fused_elbo_and_its_gradients_against_the_torch_composition_on_the_same_model(name, comps_key, monkeypatch):
    x, y = series(name, comps_key, 33, 1, separated=True)
    xy = data(x, y)
    model = build_model(name, KERNELS[comps_key], Z5)
    natgrad_steps(model, xy, 2, gamma=0.5, momentum=False)                # (a q that is not the prior)
    leaves = model.trainable_variables
    fused = model.elbo(xy)
    g_fused = torch.autograd.grad(fused, leaves)
    monkeypatch.setattr(model, "_fused", lambda time_points: False)
    composed = model.elbo(xy)
    g_composed = torch.autograd.grad(composed, leaves)
    np.testing.assert_allclose(float(fused.detach()), float(composed.detach()), **TOL)
    for a, b in zip(g_fused, g_composed):
        np.testing.assert_allclose(nn(a), nn(b), **TOL)
    assert float(torch.triu(g_fused[1], 1).abs().max()) == 0.0 and float(torch.triu(g_fused[4], 1).abs().max()) == 0.0


def test_elbo_is_one_launch_of_the_expectations_kernel_and_no_torch_route(monkeypatch):
    x, y = series(L.BERNOULLI, "m32", 33, 0)
    xy = data(x, y)
    model = build_model(L.BERNOULLI, M32, Z5)
    projections = []
    real_stats = conditionals._conditional_statistics
    monkeypatch.setattr(conditionals, "_conditional_statistics", lambda *a: (projections.append(1), real_stats(*a))[1])
    model.elbo(xy)
    seen = []
    real_rc = _lib.call_rc
    monkeypatch.setattr(_lib, "call_rc", lambda base, *a: (seen.append(base), real_rc(base, *a))[1])

    def no_torch(*a, **k):
        raise AssertionError("the torch route must not run on HIP tensors")

    monkeypatch.setattr(ML, "torch_variational_expectations", no_torch)
    monkeypatch.setattr(MM.sparse, "sparse_expected_log_likelihood_torch", no_torch)
    elbo = model.elbo(xy)
    assert len(projections) == 1, "w, c, the offsets and the tile table are cached with the data"
    assert seen.count("mf_lik_sparse_expectations") == 1
    assert not any(s.startswith("mf_lik_") and s != "mf_lik_sparse_expectations" for s in seen)
    del seen[:]
    elbo.backward()
    assert not any(s.startswith("mf_lik_") for s in seen), "the backward reuses the forward's adjoints: no second launch"
    assert all(leaf.grad is not None and bool(torch.isfinite(leaf.grad).all()) for leaf in model.trainable_variables)
    model.elbo(data(x[:20], y[:20]))
    assert len(projections) == 2, "other data: not the cached projections"


def test_the_fused_function_is_differentiable_once_and_value_only_without_a_tape():
    x, y = series(L.BERNOULLI, "m32", 33, 0)
    model = build_model(L.BERNOULLI, M32, Z5)
    _, w, c, _, offsets, tiles = model._projections(tt(x))
    with torch.no_grad():
        pair_mean, pair_cov = model._pair_marginals()
    lik = mfa.Bernoulli()
    plain = MM.sparse_expected_log_likelihood(lik, w, c, tt(y), offsets, pair_mean, pair_cov, tiles=tiles)
    assert tuple(plain.shape) == (6,) and not plain.requires_grad
    pm, pc = pair_mean.clone().requires_grad_(True), pair_cov.clone().requires_grad_(True)
    taped = MM.sparse_expected_log_likelihood(lik, w, c, tt(y), offsets, pm, pc)
    assert torch.equal(taped.detach(), plain), "the value has the same bits with and without the adjoints"
    g_mean, g_cov = torch.autograd.grad(taped.sum(), (pm, pc))
    assert torch.equal(g_cov, g_cov.transpose(-1, -2))
    want = SV.segment_expectations(L.LIKELIHOODS[L.BERNOULLI], nn(w), nn(c), y, nn(offsets), nn(pair_mean), nn(pair_cov))
    np.testing.assert_allclose(nn(plain), want["ve_sum"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(nn(g_mean), want["g_mean"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(nn(g_cov), want["g_cov"], rtol=1e-12, atol=1e-13)
    again = MM.sparse_expected_log_likelihood(lik, w, c, tt(y), offsets, pm, pc)
    with pytest.raises(RuntimeError, match="differentiable once"):
        torch.autograd.grad(again.sum(), (pm, pc), create_graph=True)


# ---- natural gradient without momentum ---------------------------------------------------------------------------------------------
def test_natural_gradient_without_momentum_reproduces_update_sites_step_for_step():
    x, y = series(L.BERNOULLI, "m32", 33, 1)
    xy = data(x, y)
    model = build_model(L.BERNOULLI, M32, Z5)
    cvi = mfa.SparseCVIGaussianProcess(build_kernel(M32), tt(Z5), mfa.Bernoulli(), learning_rate=0.5)
    opt = mfa.SSMNaturalGradient(gamma=0.5, momentum=False)
    for it in range(1, 6):
        opt.minimize(lambda: model.loss(xy), model.dist_q)
        cvi.update_sites(xy)
        means, covs = q_marginals(model)
        want_means, want_covs = cvi.dist_q.marginals
        np.testing.assert_allclose(means, nn(want_means), err_msg=f"step {it}", **TOL)
        np.testing.assert_allclose(covs, nn(want_covs), err_msg=f"step {it}", **TOL)
        with torch.no_grad():
            np.testing.assert_allclose(float(model.elbo(xy)), float(cvi.classic_elbo(xy)), err_msg=f"step {it}", **TOL)
    assert opt.effective_lr == 0.5


@pytest.mark.parametrize("name,comps_key,separated", [(L.BERNOULLI, "m32", False), (L.POISSON, "m32", False),
                                                      (L.BERNOULLI, "m52+m32", True)])
def test_natural_gradient_without_momentum_against_the_dense_sparse_cvi_loop(name, comps_key, separated):
    comps = KERNELS[comps_key]
    x, y = series(name, comps_key, 33, 1, separated)
    xy = data(x, y)
    model = build_model(name, comps, Z5)
    dense = SC.DenseSparseCVI(L.LIKELIHOODS[name], comps, x, y, Z5, 0.5)
    opt = mfa.SSMNaturalGradient(gamma=0.5, momentum=False)
    for it in range(1, 6):
        opt.minimize(lambda: model.loss(xy), model.dist_q)
        dense.step()
        compare_q_with_dense(model, *dense.posterior(), f"{name} {comps_key} step {it}")
        with torch.no_grad():
            np.testing.assert_allclose(float(model.elbo(xy)), dense.classic_elbo(), err_msg=f"step {it}", **TOL)


# ---- the conjugate case ------------------------------------------------------------------------------------------------------------
def test_one_step_at_unit_rate_with_a_gaussian_likelihood_lands_on_the_collapsed_bound():
    noise = L.LIKELIHOODS[L.GAUSSIAN][1][0]
    x, y = series(L.GAUSSIAN, "m12", 33, 0, separated=True)
    xy = data(x, y)
    model = build_model(L.GAUSSIAN, M12, Z5)
    natgrad_steps(model, xy, 1, gamma=1.0, momentum=False)
    with torch.no_grad():
        np.testing.assert_allclose(float(model.elbo(xy)), SC.collapsed_bound(M12, x, y, Z5, noise), **TOL)
    # Z = X: the bound is tight (the reference's tolerance, tests/integration/test_ssm_natgrad.py:46-66)
    full = build_model(L.GAUSSIAN, M12, x)
    natgrad_steps(full, xy, 1, gamma=1.0, momentum=False)
    gpr = mfa.GaussianProcessRegression(xy, build_kernel(M12), chol_obs_covariance=tt([[np.sqrt(noise)]]))
    with torch.no_grad():
        np.testing.assert_allclose(float(full.elbo(xy)), float(gpr.log_likelihood()), atol=1e-5, rtol=1e-6)


# ---- momentum ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [L.BERNOULLI, L.POISSON])
def test_momentum_steps_against_the_dense_natural_gradient_loop(name):
    x, y = series(name, "m32", 33, 1)
    xy = data(x, y)
    model = build_model(name, M32, Z5)
    dense = SV.DenseNatGrad(L.LIKELIHOODS[name], M32, x, y, Z5, gamma=0.1, momentum=True)
    opt = mfa.SSMNaturalGradient(gamma=0.1, momentum=True)
    for it in range(1, 6):
        opt.minimize(lambda: model.loss(xy), model.dist_q)
        dense.step()
        compare_q_with_dense(model, *dense.posterior(), f"{name} momentum step {it}")
        assert tuple(opt.effective_lr.shape) == ()
        np.testing.assert_allclose(float(opt.effective_lr), dense.effective_lr, err_msg=f"effective_lr, step {it}", **TOL)
        with torch.no_grad():
            np.testing.assert_allclose(float(model.elbo(xy)), dense.elbo(), err_msg=f"step {it}", **TOL)


def test_momentum_on_a_batch_of_two_by_three_evolves_every_series_as_it_does_alone():
    z = np.stack([Z5 + 0.05 * s for s in range(6)]).reshape(2, 3, 5)
    draws = [series(L.BERNOULLI, "m32", 33, seed) for seed in range(6)]
    x, y = (np.stack([d[k] for d in draws]).reshape(2, 3, 33) for k in (0, 1))
    batch = build_model(L.BERNOULLI, M32, z)
    opt = natgrad_steps(batch, data(x, y), 5, gamma=0.1, momentum=True)
    assert tuple(opt.effective_lr.shape) == (2, 3)
    means, covs = q_marginals(batch)
    assert means.shape == (2, 3, 5, 2)
    rates = nn(opt.effective_lr)
    for s in range(6):
        i, j = divmod(s, 3)
        single = build_model(L.BERNOULLI, M32, z[i, j])
        one = natgrad_steps(single, data(x[i, j], y[i, j]), 5, gamma=0.1, momentum=True)
        m1, c1 = q_marginals(single)
        np.testing.assert_allclose(means[i, j], m1, err_msg=f"series {s}", **TOL)
        np.testing.assert_allclose(covs[i, j], c1, err_msg=f"series {s}", **TOL)
        np.testing.assert_allclose(rates[i, j], float(one.effective_lr), err_msg=f"series {s}", **TOL)
    assert np.ptp(rates) > 1e-6, "the series differ: one shared norm would not reproduce them"


# ---- Adam --------------------------------------------------------------------------------------------------------------------------
def test_adam_on_the_trainable_variables_increases_the_elbo_and_keeps_the_choleskys_lower_triangular():
    x, y = series(L.BERNOULLI, "m32", 33, 2)
    xy = data(x, y)
    model = build_model(L.BERNOULLI, M32, Z5)
    with torch.no_grad():
        start = float(model.elbo(xy))
    adam = torch.optim.Adam(model.trainable_variables, lr=0.02)
    for _ in range(20):
        adam.zero_grad()
        model.loss(xy).backward()
        adam.step()
    with torch.no_grad():
        assert float(model.elbo(xy)) > start
    _, chol_p0, _, _, chol_q = model.trainable_variables
    assert float(torch.triu(chol_p0, 1).abs().max()) == 0.0 and float(torch.triu(chol_q, 1).abs().max()) == 0.0


# ---- minibatches -------------------------------------------------------------------------------------------------------------------
def test_num_data_scaling_and_shuffled_minibatches():
    x, y = series(L.POISSON, "m32", 33, 1)
    xy = data(x, y)
    plain = build_model(L.POISSON, M32, Z5)
    natgrad_steps(plain, xy, 2, gamma=0.5, momentum=False)
    scaled = build_model(L.POISSON, M32, Z5, num_data=33, initial_distribution=plain.dist_q)          # (the same q, bit for bit)
    with torch.no_grad():
        full = float(plain.elbo(xy))
        assert float(scaled.elbo(xy)) == full, "num_data = N on the full batch: scale 1"
        pick = np.array([4, 17, 29])
        sub = data(x[pick], y[pick])
        kl = float(torch.sum(plain.dist_q.kl_divergence(plain.dist_p)))
        np.testing.assert_allclose(float(scaled.elbo(sub)), 11.0 * (float(plain.elbo(sub)) + kl) - kl, rtol=1e-12)
        assert abs(float(scaled.elbo(sub)) - full) > 1e-3 and abs(float(plain.elbo(sub)) - full) > 1e-3
        perm = np.random.default_rng(5).permutation(33)
        assert float(plain.elbo(data(x[perm], y[perm]))) == full, "shuffled data: the bits of the sorted data"
    shuffled = data(x[perm], y[perm])
    g_sorted = torch.autograd.grad(plain.elbo(xy), plain.trainable_variables)
    g_shuffled = torch.autograd.grad(plain.elbo(shuffled), plain.trainable_variables)
    assert all(torch.equal(a, b) for a, b in zip(g_sorted, g_shuffled))


# ---- prediction --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [L.BERNOULLI, L.POISSON])
def test_predict_f_and_log_density_against_the_dense_posterior(name):
    x, y = series(name, "m32", 33, 1)
    xy = data(x, y)
    model = build_model(name, M32, Z5)
    dense = SV.DenseNatGrad(L.LIKELIHOODS[name], M32, x, y, Z5, gamma=0.5)
    natgrad_steps(model, xy, 5, gamma=0.5, momentum=False)
    for _ in range(5):
        dense.step()
    rng = np.random.default_rng(11)
    t_new = np.sort(np.concatenate([x[0] - 0.1 - rng.random(2), x[-1] + 0.1 + rng.random(2), rng.uniform(x[0], x[-1], 5)]))
    y_new = np.array([0.0, 1.0, 1.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0]) if name == L.BERNOULLI else np.arange(9.0) % 4
    mean, var = dense.predict_f(t_new)
    f_mean, f_var = model.predict_f(tt(t_new))
    assert tuple(f_mean.shape) == (9, 1) and tuple(f_var.shape) == (9, 1)
    np.testing.assert_allclose(nn(f_mean)[:, 0], mean, **TOL)
    np.testing.assert_allclose(nn(f_var)[:, 0], var, **TOL)
    density = model.predict_log_density((tt(t_new), tt(y_new)[:, None]))
    assert tuple(density.shape) == (9,)
    want = L.predict_log_density(L.LIKELIHOODS[name], mean, var, y_new)
    np.testing.assert_allclose(nn(density), want, **TOL)


# ---- the torch route ---------------------------------------------------------------------------------------------------------------
def test_pairs_of_dimension_twenty_take_the_torch_route_and_agree_with_the_dense_loop(monkeypatch):
    """Well-separated data AND inducing points, for the reason tests/test_gpu_sparse_cvi.py gives for its Matern-5/2 sum."""
    x, y = series(L.BERNOULLI, "d10", 33, 1, separated=True)
    xy = data(x, y)
    model = build_model(L.BERNOULLI, D10, Z5)
    assert model.dist_q.state_dim == 10
    seen = []
    real_rc = _lib.call_rc
    monkeypatch.setattr(_lib, "call_rc", lambda base, *a: (seen.append(base), real_rc(base, *a))[1])
    dense = SC.DenseSparseCVI(L.LIKELIHOODS[L.BERNOULLI], D10, x, y, Z5, 0.5)
    opt = mfa.SSMNaturalGradient(gamma=0.5, momentum=False)
    for it in range(1, 4):
        opt.minimize(lambda: model.loss(xy), model.dist_q)
        dense.step()
        compare_q_with_dense(model, *dense.posterior(), f"d = 10 step {it}")
        with torch.no_grad():
            np.testing.assert_allclose(float(model.elbo(xy)), dense.classic_elbo(), err_msg=f"step {it}", **TOL)
    assert "mf_lik_sparse_expectations" not in seen and "mf_lik_variational_expectations" in seen


def test_elbo_backward_gives_the_lengthscale_gradient_through_the_composed_route(monkeypatch):
    """d elbo / d lengthscale with q held fixed, against central differences; the data are shuffled, so the branch sorts them.  The
    error budget is that of ``test_classic_elbo_backward_gives_the_lengthscale_gradient`` (tests/test_gpu_sparse_cvi.py): well-separated
    points, a value good to about 1e-12 relative, |value| below 60, h = 1e-4: rounding 1e-12 x 60 / 1e-4 = 6e-7 and truncation
    h^2 / 6 x (a third derivative of order ten) = 2e-8, against a gradient of order 0.1 or more: rtol 1e-5."""
    x, y = series(L.BERNOULLI, "m32", 33, 4, separated=True)
    perm = np.random.default_rng(9).permutation(33)
    xy, shuffled = data(x, y), data(x[perm], y[perm])
    trained = build_model(L.BERNOULLI, M32, Z5)
    natgrad_steps(trained, xy, 3, gamma=0.5, momentum=False)
    seen = []
    real_rc = _lib.call_rc
    monkeypatch.setattr(_lib, "call_rc", lambda base, *a: (seen.append(base), real_rc(base, *a))[1])

    def elbo_at(ls, grad=False):
        ls_t = torch.tensor(ls, dtype=torch.float64, device=DEV, requires_grad=grad)
        m = mfa.SparseVariationalGaussianProcess(mfa.Matern32(ls_t, 1.0, device=DEV), mfa.Bernoulli(), tt(Z5),
                                                 initial_distribution=trained.dist_q)
        return m.elbo(shuffled), ls_t, m

    value, ls_t, model = elbo_at(1.0, grad=True)
    assert value.requires_grad and "mf_lik_sparse_expectations" not in seen, "w and c are under the tape: the composed route"
    with torch.no_grad():
        np.testing.assert_allclose(float(model.elbo(xy)), float(value.detach()), rtol=1e-10)      # both routes, one value
        np.testing.assert_allclose(float(trained.elbo(xy)), float(value.detach()), rtol=1e-10)
    assert "mf_lik_sparse_expectations" in seen
    (g_ls,) = torch.autograd.grad(value, ls_t)
    h = 1e-4
    with torch.no_grad():
        fd = (float(elbo_at(1.0 + h)[0]) - float(elbo_at(1.0 - h)[0])) / (2 * h)
    assert abs(float(g_ls)) > 1e-2
    np.testing.assert_allclose(float(g_ls), fd, rtol=1e-5, atol=1e-7)
    # the leaves of q get their gradients through the same graph: those of the fused route on the sorted data
    g_q = torch.autograd.grad(model.elbo(shuffled), model.trainable_variables)
    g_fused = torch.autograd.grad(trained.elbo(xy), trained.trainable_variables)
    for a, b in zip(g_q, g_fused):
        np.testing.assert_allclose(nn(a), nn(b), **TOL)


# ---- float32 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [L.BERNOULLI, L.POISSON])
def test_float32_fused_elbo_is_as_accurate_as_the_float32_composition(name, monkeypatch):
    """The bound of tests/test_gpu_conditionals.py: the fused route's error against the float64 model is at most 4 x the composed
    route's float32 error plus 8 eps32 |elbo|."""
    x, y = series(name, "m32", 33, 1)
    model64 = build_model(name, M32, Z5)
    natgrad_steps(model64, data(x, y), 3, gamma=0.5, momentum=False)
    with torch.no_grad():
        exact = float(model64.elbo(data(x, y)))
    q64 = model64.dist_q
    q32 = mfa.StateSpaceModel(*(t.detach().to(torch.float32) for t in (q64.initial_mean, q64.cholesky_initial_covariance,
                                                                        q64.state_transitions, q64.state_offsets,
                                                                        q64.cholesky_process_covariances)))
    model32 = build_model(name, M32, Z5, dtype=torch.float32, initial_distribution=q32)
    xy32 = data(x, y, torch.float32)
    with torch.no_grad():
        fused = float(model32.elbo(xy32))
        monkeypatch.setattr(model32, "_fused", lambda time_points: False)
        composed = float(model32.elbo(xy32))
    eps32 = 2.0 ** -23
    print(f"ERR f32 elbo {name}: fused {abs(fused - exact):.3e}  composed {abs(composed - exact):.3e}  |elbo| {abs(exact):.3f}")
    assert abs(fused - exact) <= 4.0 * abs(composed - exact) + 8.0 * eps32 * abs(exact)
