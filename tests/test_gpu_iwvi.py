"""
GPU tests of ``ImportanceWeightedVI`` and ``ImportanceWeightedPosteriorProcess``: the fused route (``mf_lik_iw_log_weights_*``) against
the torch composition under one seed, the routing, the density terms against dense numpy, the statistics of the bound on a Gaussian
problem whose marginal likelihood is known, and the posterior process.

float64 and the project's state-space-against-dense tolerance, ``TOL`` = rtol 1e-6 / atol 1e-7 (tests/test_gpu_svgp.py), unless a test
says otherwise.  The statistical test makes ONE seeded call with 4096 samples and compares at five standard errors computed from the
samples themselves (a chance of about 6e-7 per condition for a normal mean).  Measured on an MI355X with the seeds of the test:
``log p(y)`` = -37.84, the SVGP bound -43.87, mean L_1 -43.86 (0.23 SE from the bound), mean L_8 -39.70: 55 SE above L_1 and 24 SE below
``log p(y)`` - the conditions hold with wide room and still tell the three quantities apart.
"""
import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from helpers import iwvi_closed_forms as IW
from helpers import likelihood_closed_forms as L
from helpers import periodic_closed_forms as PC
from helpers import sparse_cvi_closed_forms as SC
from helpers import svgp_closed_forms as SV

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = dict(rtol=1e-6, atol=1e-7)
M12 = [dict(order=1, ls=1.0, var=1.0, period=None, osc=0)]
M32 = [dict(order=3, ls=1.0, var=1.0, period=None, osc=0)]
M52_M12 = [dict(order=5, ls=1.3, var=0.8, period=None, osc=0), dict(order=1, ls=0.6, var=0.5, period=None, osc=0)]
KERNELS = {"m32": M32, "m52+m12": M52_M12}
Z5 = np.array([0.6, 1.9, 3.1, 4.2, 5.5])
FN = "mf_lik_iw_log_weights"


def tt(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def nn(t):
    return t.detach().cpu().numpy()


def build_kernel(comps):
    cls = {1: mfa.Matern12, 3: mfa.Matern32, 5: mfa.Matern52}
    parts = [cls[c["order"]](c["ls"], c["var"], device=DEV) for c in comps]
    return parts[0] if len(parts) == 1 else mfa.Sum(parts)


def build_likelihood(name):
    params = L.LIKELIHOODS[name][1]
    return {L.GAUSSIAN: lambda: mfa.Gaussian(params[0]), L.BERNOULLI: mfa.Bernoulli, L.POISSON: mfa.Poisson}[name]()


def trained_q(name, comps, z, xy, steps=2):
    """A ``q`` that is not the prior: a few natural-gradient steps of the SVGP model."""
    svgp = mfa.SparseVariationalGaussianProcess(build_kernel(comps), build_likelihood(name), z)
    opt = mfa.SSMNaturalGradient(gamma=0.5, momentum=False)
    for _ in range(steps):
        opt.minimize(lambda: svgp.loss(xy), svgp.dist_q)
    return svgp


def two_series(name, comps, num_points=150):
    """B = 2 series of unsorted points with their observations, and the inducing points.  The prior is drawn on the MERGED time
    points at jitter 0, where Q = P - A P A^T of a Matern-5/2 component loses its digits for gaps below 1e-3: the data sit one per cell
    of an even grid (``separated``: at least 0.4 cells apart) and the inducing points on cell boundaries (at least 0.2 cells from
    either neighbour; a cell is 6 / num_points >= 0.04)."""
    xs, ys = zip(*(L.draw_series(L.LIKELIHOODS[name], comps, num_points, seed, separated=True) for seed in (11, 12)))
    perm = np.random.default_rng(13).permutation(num_points)
    x, y = np.stack(xs)[:, perm], np.stack(ys)[:, perm]
    cell = 6.0 / num_points
    on_grid = np.round(Z5 / cell)
    return (tt(x), tt(y)[..., None]), tt(np.stack([on_grid * cell, (on_grid + 1.0) * cell]))


@pytest.mark.parametrize("comps_key", ["m32", "m52+m12"])
@pytest.mark.parametrize("name", [L.BERNOULLI, L.POISSON])
def test_fused_and_torch_routes_agree_under_one_seed(name, comps_key, monkeypatch):
    comps = KERNELS[comps_key]
    xy, z = two_series(name, comps)
    start = trained_q(name, comps, z, xy).dist_q
    model = mfa.ImportanceWeightedVI(build_kernel(comps), z, build_likelihood(name), 4, initial_distribution=start)
    seen = []
    real_rc = _lib.call_rc
    monkeypatch.setattr(_lib, "call_rc", lambda base, *a: (seen.append(base), real_rc(base, *a))[1])

    def evaluate(objective):
        torch.manual_seed(5)
        value = objective(xy)
        return value, torch.autograd.grad(value, model.trainable_variables)

    for objective in (model.elbo, model.dregs_objective):
        seen.clear()
        fused, g_fused = evaluate(objective)
        assert seen.count(FN) == 1, "the fused route: one call of the kernel pair"
        with monkeypatch.context() as patch:
            patch.setattr(model, "_fused", lambda time_points: False)
            seen.clear()
            composed, g_composed = evaluate(objective)
            assert FN not in seen
        assert np.isfinite(float(fused.detach()))
        np.testing.assert_allclose(float(fused.detach()), float(composed.detach()), **TOL)
        assert len(g_fused) == 5
        for a, b in zip(g_fused, g_composed):
            assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0.0
            np.testing.assert_allclose(nn(a), nn(b), **TOL)
    # the seed decides the draw: another seed, another value; the same seed, the same bits
    torch.manual_seed(5)
    again = float(model.elbo(xy).detach())
    torch.manual_seed(6)
    other = float(model.elbo(xy).detach())
    torch.manual_seed(5)
    assert float(model.elbo(xy).detach()) == again and other != again


def test_a_kernel_hyper_parameter_under_the_tape_takes_the_torch_route_and_gets_its_gradient(monkeypatch):
    xy, z = two_series(L.BERNOULLI, M32, 40)
    start = trained_q(L.BERNOULLI, M32, z, xy).dist_q
    ls = torch.tensor(1.0, dtype=torch.float64, device=DEV, requires_grad=True)
    model = mfa.ImportanceWeightedVI(mfa.Matern32(ls, 1.0, device=DEV), z, mfa.Bernoulli(), 4, initial_distribution=start)
    seen = []
    real_rc = _lib.call_rc
    monkeypatch.setattr(_lib, "call_rc", lambda base, *a: (seen.append(base), real_rc(base, *a))[1])
    torch.manual_seed(7)
    value = model.elbo(xy)
    assert FN not in seen and value.requires_grad
    grads = torch.autograd.grad(value, (ls,) + tuple(model.trainable_variables))
    assert all(bool(torch.isfinite(g).all()) for g in grads) and abs(float(grads[0])) > 1e-6
    # with the hyper-parameter fixed: the fused route, and under the same seed the same value
    fixed = mfa.ImportanceWeightedVI(mfa.Matern32(1.0, 1.0, device=DEV), z, mfa.Bernoulli(), 4, initial_distribution=start)
    torch.manual_seed(7)
    same = fixed.elbo(xy)
    assert FN in seen
    assert np.isfinite(float(same.detach()))
    np.testing.assert_allclose(float(value.detach()), float(same.detach()), **TOL)


def dense_q(dist_q, b):
    """Mean and covariance of the stacked states of series ``b`` of a chain, from the plain recursion."""
    mu0, cp0, a_s, b_s, cq = (torch.as_tensor(nn(t)[b]) for t in (dist_q.initial_mean, dist_q.cholesky_initial_covariance,
                                                                 dist_q.state_transitions, dist_q.state_offsets,
                                                                 dist_q.cholesky_process_covariances))
    mean, cov = SV.dense_moments(mu0, cp0, a_s, b_s, cq)
    return mean.numpy(), cov.numpy()


@pytest.mark.parametrize("name", [L.BERNOULLI, L.POISSON])
def test_log_importance_weights_against_dense_numpy(name):
    comps = M52_M12
    xy, z = two_series(name, comps, 60)
    order = torch.argsort(xy[0], dim=-1)
    xy = (torch.gather(xy[0], -1, order), torch.gather(xy[1][..., 0], -1, order)[..., None])
    start = trained_q(name, comps, z, xy).dist_q
    model = mfa.ImportanceWeightedVI(build_kernel(comps), z, build_likelihood(name), 3, initial_distribution=start)
    post = model.posterior
    torch.manual_seed(8)
    with torch.no_grad():
        samples_s, samples_u = post.proposal_process.sample_state_trajectories(xy[0], (3,))
        got = post.log_importance_weights(samples_s, samples_u, xy)
    assert tuple(got.shape) == (3,)
    h = PC.emission(comps, ())[0]
    want = np.zeros(3)
    for b in range(2):
        lik = IW.iw_log_weights(L.LIKELIHOODS[name], h, None, nn(xy[1])[b, :, 0], np.array([0, 60]), nn(samples_s)[:, b], None)
        kuu = SC.dense_state_prior(comps, nn(z)[b])
        q_mean, q_cov = dense_q(model.dist_q, b)
        for k in range(3):
            u = nn(samples_u)[k, b].reshape(-1)
            want[k] += lik["log_lik"][k, 0] + IW.dense_gaussian_logpdf(u, np.zeros_like(u), kuu) - IW.dense_gaussian_logpdf(u, q_mean, q_cov)
    np.testing.assert_allclose(nn(got), want, **TOL)
    # under the tape the torch composition: the same numbers
    taped = post.log_importance_weights(samples_s.clone().requires_grad_(True), samples_u, xy)
    np.testing.assert_allclose(nn(taped), want, **TOL)
    # stop_gradient: no gradient reaches q through log q(u) alone (fixed samples), and the value is the same
    for stop, reaches in ((False, True), (True, False)):
        value = post.log_importance_weights(samples_s, samples_u, xy, stop_gradient=stop)
        np.testing.assert_allclose(nn(value), want, **TOL)
        assert value.requires_grad == reaches
    grads = torch.autograd.grad(post.log_importance_weights(samples_s, samples_u, xy).sum(), model.trainable_variables)
    assert all(float(g.abs().max()) > 0.0 for g in grads)


def test_the_bound_tightens_with_the_number_of_samples_and_stays_below_the_marginal_likelihood():
    name, noise = L.GAUSSIAN, L.LIKELIHOODS[L.GAUSSIAN][1][0]
    x, y = L.draw_series(L.LIKELIHOODS[name], M12, 30, seed=21)
    z = np.linspace(0.5, 5.5, 6)
    xy = (tt(x), tt(y)[..., None])
    svgp = mfa.SparseVariationalGaussianProcess(build_kernel(M12), build_likelihood(name), tt(z))
    mfa.SSMNaturalGradient(gamma=1.0, momentum=False).minimize(lambda: svgp.loss(xy), svgp.dist_q)      # the optimal q in one step
    with torch.no_grad():
        bound = float(svgp.elbo(xy))
    log_py = PC.dense_log_marginal(M12, x, y, noise)
    np.testing.assert_allclose(bound, SC.collapsed_bound(M12, x, y, z, noise), **TOL)
    assert bound < log_py - 1.0, "the three quantities are apart"
    model = mfa.ImportanceWeightedVI(build_kernel(M12), tt(z), build_likelihood(name), 4096, initial_distribution=svgp.dist_q)
    torch.manual_seed(22)
    with torch.no_grad():
        log_w = nn(model.log_weights(xy))
    assert log_w.shape == (4096,)
    from scipy import special
    l8 = special.logsumexp(log_w.reshape(512, 8), axis=1) - np.log(8.0)
    se1, se8 = log_w.std(ddof=1) / np.sqrt(4096.0), l8.std(ddof=1) / np.sqrt(512.0)
    print(f"log p(y) {log_py:.3f}  bound {bound:.3f}  mean L1 {log_w.mean():.3f} (SE {se1:.3f})  mean L8 {l8.mean():.3f} (SE {se8:.3f})")
    assert abs(log_w.mean() - bound) <= 5.0 * se1
    assert l8.mean() >= log_w.mean() - 5.0 * se8
    assert l8.mean() <= log_py + 5.0 * se8
    assert l8.mean() > log_w.mean() + 5.0 * se8, "and the simulation's margin is there: L_8 is visibly tighter"


def test_posterior_process_expected_value_samples_and_errors():
    xy, z = two_series(L.BERNOULLI, M32, 40)
    start = trained_q(L.BERNOULLI, M32, z, xy).dist_q
    model = mfa.ImportanceWeightedVI(build_kernel(M32), z, mfa.Bernoulli(), 6, initial_distribution=start)
    post = model.posterior
    new = tt(np.stack([np.linspace(0.2, 5.8, 7)] * 2))
    with torch.no_grad():
        torch.manual_seed(9)
        mean = post.expected_value(new, xy)
        torch.manual_seed(9)
        samples, log_w, _ = post._iwvi_samples_and_weights(new, xy, (6,))
        assert tuple(mean.shape) == (2, 7, 1) and tuple(samples.shape) == (6, 2, 7, 2) and tuple(log_w.shape) == (6,)
        weights = torch.softmax(log_w, dim=0)
        np.testing.assert_allclose(nn(mean), nn(torch.sum(weights[:, None, None, None] * samples[..., :1], dim=0)), rtol=1e-12, atol=1e-13)
        squares = post.expected_value(new, xy, func=torch.square)
        assert tuple(squares.shape) == (2, 7, 1) and float(squares.min()) >= 0.0
        # resampling: every returned trajectory is one of the K candidates of its draw
        torch.manual_seed(10)
        states, cond = post.sample_state_trajectories(new, (3,), input_data=xy)
        torch.manual_seed(10)
        cand, _, cand_u = post._iwvi_samples_and_weights(new, xy, (3, 6))
        assert tuple(states.shape) == (3, 2, 7, 2) and tuple(cond.shape) == (3, 6, 2, 5, 2) and torch.equal(cond, cand_u)
        for i in range(3):
            assert any(torch.equal(states[i], cand[i, k]) for k in range(6))
        f = post.sample_f(new, 4, input_data=xy)
        assert tuple(f.shape) == (4, 2, 7, 1) and tuple(post.sample_state(new, 4, input_data=xy).shape) == (4, 2, 7, 2)
    for method in (post.sample_f, post.sample_state, post.sample_state_trajectories):
        with pytest.raises(ValueError, match="input_data"):
            method(new, 2)
    with pytest.raises(ValueError, match="input_data"):
        post.expected_value(new, None)
    with pytest.raises(NotImplementedError):
        post.predict_f(new)
    with pytest.raises(NotImplementedError):
        post.predict_state(new)
    with pytest.raises(NotImplementedError):
        model.predict_f(new)


def test_constructor_and_elbo_errors():
    xy, z = two_series(L.BERNOULLI, M32, 40)
    kernel = build_kernel(M32)
    for bad in (0, -3, 1.5):
        with pytest.raises(ValueError, match="num_importance_samples"):
            mfa.ImportanceWeightedVI(kernel, z, mfa.Bernoulli(), bad)
    model = mfa.ImportanceWeightedVI(kernel, z, mfa.Bernoulli(), 2)
    for method in (model.elbo, model.dregs_objective):
        with pytest.raises(ValueError, match="batch shape"):
            method((xy[0][0], xy[1][0]))
        with pytest.raises(ValueError, match="float32"):
            method((xy[0].float(), xy[1].float()))
        with pytest.raises(ValueError, match=r"\[num_data, 1\]"):
            method((xy[0], xy[1][..., 0]))
    assert bool(torch.isfinite(model.elbo(xy)))
