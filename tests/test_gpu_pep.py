"""
GPU tests of ``PowerExpectationPropagation`` (markovflow_amd/models.py) against the dense PEP loop of
tests/helpers/pep_closed_forms.py: the same iteration on the kernel matrix with the scalar cavity, no state space form.

State space against dense: rtol 1e-6 / atol 1e-7, as tests/test_gpu_cvi.py (prediction variances: its rtol 1e-5).  The kernels carry
jitter 0 and so does the dense loop.  Series come from ``draw_series(..., separated=True)`` on a Matern-3/2 kernel and have at most
33 points.  Only the Gaussian and Bernoulli likelihoods run in model loops: with these draws the discretised g2 of Poisson and
Student-t makes 1 + v_c g2 <= 0 at some points, whose sites are then skipped - that is the kernel-level skip test's subject
(tests/test_gpu_pep_kernel.py), not a tolerance comparison's.
"""
import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from markovflow_amd import likelihoods as ML
from helpers import likelihood_closed_forms as L
from helpers import pep_closed_forms as P

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = dict(rtol=1e-6, atol=1e-7)
M32 = [dict(order=3, ls=1.0, var=1.0, period=None, osc=0)]
M52_M32 = [dict(order=5, ls=1.3, var=0.8, period=None, osc=0), dict(order=3, ls=0.6, var=0.5, period=None, osc=0)]
RECORD = (1, 5, 25)


def tt(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64, device=DEV)


def nn(t):
    return t.detach().cpu().numpy()


def build_kernel(comps):
    cls = {1: mfa.Matern12, 3: mfa.Matern32, 5: mfa.Matern52}
    parts = [cls[c["order"]](c["ls"], c["var"], device=DEV) for c in comps]
    return parts[0] if len(parts) == 1 else mfa.Sum(parts)


def build_likelihood(name):
    params = L.LIKELIHOODS[name][1]
    return {L.GAUSSIAN: lambda: mfa.Gaussian(params[0]), L.BERNOULLI: mfa.Bernoulli}[name]()


def build_model(name, comps, t, y, lr, alpha):
    return mfa.PowerExpectationPropagation((tt(t), tt(y)[..., None]), build_kernel(comps), build_likelihood(name), learning_rate=lr,
                                           alpha=alpha)


_DENSE = {}


def dense_run(name, num_points, seed, alpha, lr=0.5, iterations=25):
    """Data and the dense loop's record for one series: computed once, shared, not modified.  (``dense_pep`` asserts that it skipped
    no site and kept every site precision positive.)"""
    key = (name, num_points, seed, alpha, lr, iterations)
    if key not in _DENSE:
        t, y = L.draw_series(L.LIKELIHOODS[name], M32, num_points, seed, separated=True)
        rec = P.dense_pep(L.LIKELIHOODS[name], M32, t, y, alpha, lr, iterations, record=tuple(range(1, iterations + 1)))
        _DENSE[key] = (t, y, rec)
    return _DENSE[key]


def compare_with_dense(model, rec, where):
    np.testing.assert_allclose(nn(model.sites.nat1)[:, 0], rec["nat1"], err_msg=f"nat1 {where}", **TOL)
    np.testing.assert_allclose(nn(model.sites.nat2)[:, 0, 0], rec["nat2"], err_msg=f"nat2 {where}", **TOL)
    np.testing.assert_allclose(nn(model.sites.log_norm)[:, 0], rec["log_norm"], err_msg=f"log_norm {where}", **TOL)
    np.testing.assert_allclose(float(model.energy()), rec["energy"], err_msg=f"energy {where}", **TOL)
    cav_mu, cav_var = model.compute_cavity()
    assert tuple(cav_mu.shape) == tuple(cav_var.shape) == tuple(model.observations.shape)
    np.testing.assert_allclose(nn(cav_mu)[:, 0], rec["cav_mu"], err_msg=f"cavity mean {where}", **TOL)
    np.testing.assert_allclose(nn(cav_var)[:, 0], rec["cav_var"], err_msg=f"cavity variance {where}", **TOL)
    # q through the natural parameters and q through the filter are one distribution
    q_mean, q_cov = model.dist_q.marginals
    f_mean, f_cov = model.posterior_kalman.posterior_state_space_model().marginals
    np.testing.assert_allclose(nn(q_mean), nn(f_mean), err_msg=f"marginal means {where}", **TOL)
    np.testing.assert_allclose(nn(q_cov), nn(f_cov), err_msg=f"marginal covariances {where}", **TOL)


def cavity_dxd_torch(model):
    """The reference's route (pep.py:120-148) with torch on the device, from ``dist_q.marginals``."""
    means, covs = model.dist_q.marginals
    eye = torch.eye(covs.shape[-1], dtype=covs.dtype, device=covs.device).expand_as(covs)
    prec = _lib.chol_solve(torch.linalg.cholesky(covs), eye)          # (two triangular solves: see _lib.chol_solve)
    h = model.kernel.generate_emission_model(model.time_points).emission_matrix          # [.., N, 1, d]
    bp1, bp2 = mfa.models.back_project_nats(model.sites.nat1, model.sites.nat2[..., 0], h)
    th2 = -0.5 * prec - model.alpha * bp2
    th1 = (prec @ means[..., None])[..., 0] - model.alpha * bp1
    cav_cov = 0.5 * _lib.chol_solve(torch.linalg.cholesky(-th2), eye)
    cav_mean = (cav_cov @ th1[..., None])[..., 0]
    return (h @ cav_mean[..., None])[..., 0], (h @ cav_cov @ h.transpose(-1, -2))[..., 0]


@pytest.mark.parametrize("num_points", [7, 33])
def test_gaussian_likelihood_with_unit_power_and_rate_is_gp_regression(num_points):
    spec = L.LIKELIHOODS[L.GAUSSIAN]
    var = spec[1][0]
    t, y = L.draw_series(spec, M32, num_points, seed=0, separated=True)
    model = build_model(L.GAUSSIAN, M32, t, y, lr=1.0, alpha=1.0)
    model.update_sites()
    # the tolerances tests/test_gpu_cvi.py uses for this statement.  nat2 = g2 / (2 den) with g2 = -1 / (variance + v_c) and the
    # Gaussian den in closed form, variance / (variance + v_c): four roundings, inside 1e-15 = 4.5 eps
    np.testing.assert_allclose(nn(model.sites.nat1)[:, 0], y / var, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(nn(model.sites.nat2)[:, 0, 0], np.full(num_points, -0.5 / var), rtol=1e-15, atol=0)
    gpr = mfa.GaussianProcessRegression((tt(t), tt(y)[:, None]), build_kernel(M32), chol_obs_covariance=tt([[np.sqrt(var)]]))
    exact = float(gpr.log_likelihood())
    assert float(model.elbo()) == pytest.approx(exact, rel=1e-9)
    assert float(model.loss()) == pytest.approx(-exact, rel=1e-9)
    assert float(model.energy()) == pytest.approx(exact, rel=1e-9)
    dense = L.PC.dense_log_marginal(M32, t, y, var)
    np.testing.assert_allclose(float(model.elbo()), dense, **TOL)
    np.testing.assert_allclose(float(model.energy()), dense, **TOL)


def test_gaussian_likelihood_with_half_power_converges_geometrically():
    """alpha = 0.5, lr = 1: each update halves the distance to the exact sites, nat1 = (1 - 0.5^k) y / variance after k updates, and
    the energy reaches the exact log marginal likelihood (the dense loop: to 1e-14 on the CPU)."""
    spec = L.LIKELIHOODS[L.GAUSSIAN]
    var = spec[1][0]
    t, y = L.draw_series(spec, M32, 33, seed=0, separated=True)
    model = build_model(L.GAUSSIAN, M32, t, y, lr=1.0, alpha=0.5)
    for it in range(1, 61):
        model.update_sites()
        if it == 3:
            np.testing.assert_allclose(nn(model.sites.nat1)[:, 0], (1 - 0.5 ** 3) * y / var, **TOL)
    np.testing.assert_allclose(float(model.energy()), L.PC.dense_log_marginal(M32, t, y, var), **TOL)


@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("num_points", [7, 33])
@pytest.mark.parametrize("seed", range(6))
def test_bernoulli_runs_against_the_dense_loop(num_points, seed, alpha):
    t, y, rec = dense_run(L.BERNOULLI, num_points, seed, alpha)
    model = build_model(L.BERNOULLI, M32, t, y, lr=0.5, alpha=alpha)
    for it in range(1, 26):
        model.update_sites()
        if it in RECORD:
            compare_with_dense(model, rec[it], f"T={num_points} seed={seed} alpha={alpha} iteration {it}")


@pytest.mark.parametrize("comps", [M32, M52_M32], ids=["d2", "d5"])
def test_scalar_cavity_is_the_d_by_d_route_on_the_device(comps):
    """``compute_cavity()`` against pep.py:120-148 written with torch on ``dist_q.marginals``.  The d x d route inverts the marginal
    covariances (condition numbers up to ~1e6 at d = 5): the state-space-against-dense tolerance."""
    t, y = L.draw_series(L.LIKELIHOODS[L.BERNOULLI], comps, 33, seed=1, separated=True)
    model = build_model(L.BERNOULLI, comps, t, y, lr=0.5, alpha=0.5)
    for _ in range(5):
        model.update_sites()
    assert model.dist_q.state_dim == sum((c["order"] + 1) // 2 for c in comps)
    cav_mu, cav_var = model.compute_cavity()
    want_mu, want_var = cavity_dxd_torch(model)
    np.testing.assert_allclose(nn(cav_mu), nn(want_mu), **TOL)
    np.testing.assert_allclose(nn(cav_var), nn(want_var), **TOL)
    again = model.compute_cavity_from_marginals(model.dist_q.marginals)
    assert torch.equal(again[0], cav_mu) and torch.equal(again[1], cav_var)


def test_a_batch_of_three_series_equals_three_models():
    runs = [dense_run(L.BERNOULLI, 33, seed, 0.5) for seed in range(3)]
    t, y = np.stack([r[0] for r in runs]), np.stack([r[1] for r in runs])
    batch = build_model(L.BERNOULLI, M32, t, y, lr=0.5, alpha=0.5)
    singles = [build_model(L.BERNOULLI, M32, r[0], r[1], lr=0.5, alpha=0.5) for r in runs]
    for _ in range(5):
        batch.update_sites()
        for m in singles:
            m.update_sites()
    assert tuple(batch.sites.nat1.shape) == (3, 33, 1) and tuple(batch.sites.nat2.shape) == (3, 33, 1, 1)
    assert tuple(batch.sites.log_norm.shape) == (3, 33, 1)
    energy = batch.energy()
    assert tuple(energy.shape) == (3,) and tuple(batch.compute_log_norm().shape) == (3, 33)
    for s, (m, r) in enumerate(zip(singles, runs)):
        # the same kernels on one series or on three: no more than the rounding of differently ordered sums
        np.testing.assert_allclose(nn(batch.sites.nat1)[s], nn(m.sites.nat1), rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(nn(batch.sites.nat2)[s], nn(m.sites.nat2), rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(nn(batch.sites.log_norm)[s], nn(m.sites.log_norm), rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(nn(batch.sites.nat1)[s, :, 0], r[2][5]["nat1"], **TOL)
        assert float(energy[s]) == pytest.approx(float(m.energy()), rel=1e-9)
        np.testing.assert_allclose(float(energy[s]), r[2][5]["energy"], **TOL)
    assert float(batch.elbo()) == pytest.approx(sum(float(m.elbo()) for m in singles), rel=1e-10)


def test_site_indices_update_only_those_sites():
    t, y, _ = dense_run(L.BERNOULLI, 33, 0, 0.5)
    both = np.stack([t, t]), np.stack([y, 1.0 - y])
    model = build_model(L.BERNOULLI, M32, *both, lr=0.5, alpha=0.5)
    full = build_model(L.BERNOULLI, M32, *both, lr=0.5, alpha=0.5)
    model.update_sites()
    full.update_sites()
    before = [t_.clone() for t_ in (model.sites.nat1, model.sites.nat2, model.sites.log_norm)]
    model.update_sites(site_indices=torch.tensor([0, 3], device=DEV))
    full.update_sites()
    rest = [i for i in range(33) if i not in (0, 3)]
    for now, was, everything in zip((model.sites.nat1, model.sites.nat2, model.sites.log_norm), before,
                                    (full.sites.nat1, full.sites.nat2, full.sites.log_norm)):
        assert torch.equal(now[:, rest], was[:, rest]), "the other sites keep their bits, in every series"
        assert torch.equal(now[:, [0, 3]], everything[:, [0, 3]]), "the chosen sites are the full update's"
        assert not bool(torch.any(now[:, [0, 3]] == was[:, [0, 3]]))
    model.update_sites(site_indices=torch.tensor([], dtype=torch.long))
    assert torch.equal(model.sites.nat1[:, rest], before[0][:, rest])


def test_update_sites_is_one_launch_of_the_site_kernel_and_no_torch_route(monkeypatch):
    t, y, _ = dense_run(L.BERNOULLI, 33, 0, 0.5)
    model = build_model(L.BERNOULLI, M32, t, y, lr=0.5, alpha=0.5)
    seen = []
    real_rc = _lib.call_rc
    monkeypatch.setattr(_lib, "call_rc", lambda base, *a: (seen.append(base), real_rc(base, *a))[1])

    def no_torch(*a, **k):
        raise AssertionError("the torch route must not run on HIP tensors")

    for route in ("torch_variational_expectations", "torch_predict_log_density", "torch_log_expected_density", "torch_pep_site_update"):
        monkeypatch.setattr(ML, route, no_torch)
    versions = [s._version for s in (model.sites.nat1, model.sites.nat2, model.sites.log_norm)]
    model.update_sites()
    assert seen.count("mf_lik_pep_site_update") == 1
    assert not any(s.startswith("mf_lik_") and s != "mf_lik_pep_site_update" for s in seen)
    assert all(s._version > v for s, v in zip((model.sites.nat1, model.sites.nat2, model.sites.log_norm), versions))
    del seen[:]
    model.update_sites(site_indices=torch.tensor([1, 2], device=DEV))
    assert [s for s in seen if s.startswith("mf_lik_")] == ["mf_lik_pep_site_update"]
    del seen[:]
    model.energy()
    assert [s for s in seen if s.startswith("mf_lik_")] == ["mf_lik_log_expected_density"]
    obj, (l1, l2) = model.local_objective_gradients(*model.compute_cavity())
    assert tuple(obj.shape) == (33,) and tuple(l1.shape) == tuple(l2.shape) == (33, 1)
    assert tuple(model.local_objective(*model.compute_cavity(), model.observations).shape) == (33,)


def test_elbo_sees_the_updated_sites():
    """No stale filter state: the value after an update is the value of a model built afresh around the new sites."""
    t, y, _ = dense_run(L.BERNOULLI, 33, 2, 1.0)
    model = build_model(L.BERNOULLI, M32, t, y, lr=0.5, alpha=1.0)
    model.update_sites()
    first = (float(model.elbo()), float(model.energy()))
    model.update_sites()
    second = (float(model.elbo()), float(model.energy()))
    assert first[0] != second[0] and first[1] != second[1]
    fresh = build_model(L.BERNOULLI, M32, t, y, lr=0.5, alpha=1.0)
    fresh.sites = mfa.UnivariateGaussianSitesNat(model.sites.nat1.clone(), model.sites.nat2.clone(), model.sites.log_norm.clone())
    assert (float(fresh.elbo()), float(fresh.energy())) == second


def test_prediction_at_new_time_points_against_the_dense_posterior():
    t, y, rec = dense_run(L.BERNOULLI, 33, 3, 0.5)
    model = build_model(L.BERNOULLI, M32, t, y, lr=0.5, alpha=0.5)
    for _ in range(25):
        model.update_sites()
    rng = np.random.default_rng(11)
    t_new = np.sort(np.concatenate([t[0] - 0.1 - rng.random(2), t[-1] + 0.1 + rng.random(2), rng.uniform(t[0], t[-1], 5)]))
    y_new = np.array([0.0, 1.0, 1.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0])
    mean, var = L.dense_predict(M32, t, rec[25]["nat1"], rec[25]["nat2"], t_new)
    f_mean, f_var = model.posterior.predict_f(tt(t_new))
    assert tuple(f_mean.shape) == (9, 1) and tuple(f_var.shape) == (9, 1)
    np.testing.assert_allclose(nn(f_mean)[:, 0], mean, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(nn(f_var)[:, 0], var, rtol=1e-5, atol=1e-7)
    density = model.predict_log_density((tt(t_new), tt(y_new)[:, None]))
    assert tuple(density.shape) == (9,)
    want = L.predict_log_density(L.LIKELIHOODS[L.BERNOULLI], mean, var, y_new)
    # d log density / d(mean, var) is O(1) on this data: the prediction's tolerances carry over
    np.testing.assert_allclose(nn(density), want, rtol=1e-5, atol=1e-6)


def test_elbo_backward_gives_the_lengthscale_gradient():
    """d elbo / d lengthscale (sites fixed) through the filter's backward against central differences of elbo(): shape and tolerance
    of the CVI test of the same name (well-separated points, elbo() good to about 1e-12 relative; h = 1e-4: rounding
    1e-12 x 60 / 1e-4 = 6e-7, truncation 2e-8, against a gradient of order 0.1: rtol 1e-5)."""
    t, y, _ = dense_run(L.BERNOULLI, 33, 4, 0.5)
    model = build_model(L.BERNOULLI, M32, t, y, lr=0.5, alpha=0.5)
    for _ in range(5):
        model.update_sites()

    def elbo_at(ls, grad=False):
        ls_t = torch.tensor(ls, dtype=torch.float64, device=DEV, requires_grad=grad)
        m = mfa.PowerExpectationPropagation((tt(t), tt(y)[:, None]), mfa.Matern32(ls_t, 1.0, device=DEV), mfa.Bernoulli(),
                                            learning_rate=0.5, alpha=0.5)
        m.sites = model.sites
        return m.elbo(), ls_t

    value, ls_t = elbo_at(1.0, grad=True)
    value.backward()
    h = 1e-4
    fd = (float(elbo_at(1.0 + h)[0]) - float(elbo_at(1.0 - h)[0])) / (2 * h)
    assert abs(float(ls_t.grad)) > 1e-2
    np.testing.assert_allclose(float(ls_t.grad), fd, rtol=1e-5, atol=1e-7)
    assert not model.energy().requires_grad
