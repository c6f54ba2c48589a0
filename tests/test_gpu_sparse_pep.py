"""
GPU tests of ``SparsePowerExpectationPropagation`` (markovflow_amd/models.py) against the dense sparse-PEP loop of
tests/helpers/sparse_pep_closed_forms.py - one Gaussian over the stacked inducing states, the site normaliser from M + 1 leave-one-out
posteriors - and, with the inducing points on the data, against ``PowerExpectationPropagation`` and ``GaussianProcessRegression``.

Tolerances are those of tests/test_gpu_pep.py and tests/test_gpu_sparse_cvi.py for the same kind of comparison: state space against
dense, and the sparse model against the full one on Z = X, rtol 1e-6 / atol 1e-7 (prediction variances: rtol 1e-5); a batch against
its series one by one rtol 1e-10 / atol 1e-12.  Series come from ``draw_series`` on a Matern-3/2 kernel and have at most 33 points.
The dense loop runs the Bernoulli likelihood (it asserts that it skipped no segment: with these draws the discretised g2 of Poisson
makes 1 + fvar g2 <= 0 at some points, as tests/test_gpu_pep.py notes); Poisson runs against ``PowerExpectationPropagation``, which
skips what this model skips.
"""
import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from markovflow_amd import likelihoods as ML
from markovflow_amd import models as MM
from helpers import likelihood_closed_forms as L
from helpers import sparse_pep_closed_forms as SP

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = dict(rtol=1e-6, atol=1e-7)
M32 = [dict(order=3, ls=1.0, var=1.0, period=None, osc=0)]
Z5 = np.array([0.6, 1.9, 3.1, 4.2, 5.5])          # five inducing points inside the data's span [0, 6]
FN = "mf_lik_sparse_pep_site_update"


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
    return {L.GAUSSIAN: lambda: mfa.Gaussian(params[0]), L.BERNOULLI: mfa.Bernoulli, L.POISSON: mfa.Poisson}[name]()


def build_model(name, comps, z, lr=0.5, alpha=0.5):
    return mfa.SparsePowerExpectationPropagation(build_kernel(comps), tt(z), build_likelihood(name), learning_rate=lr, alpha=alpha)


def data(x, y):
    return tt(x), tt(y)[..., None]


_DENSE = {}


def dense_run(name, num_points, seed, z, alpha, separated=False, iterations=10):
    """Data and the dense loop's record for one series: computed once, shared, not modified.  (The loop asserts that it skipped no
    segment and that every cavity exists.)"""
    key = (name, num_points, seed, tuple(z), alpha, separated, iterations)
    if key not in _DENSE:
        x, y = L.draw_series(L.LIKELIHOODS[name], M32, num_points, seed, separated=separated)
        rec, run = SP.dense_sparse_pep(L.LIKELIHOODS[name], M32, x, y, np.asarray(z), alpha, 0.5, iterations,
                                       record=tuple(range(1, iterations + 1)))
        _DENSE[key] = (x, y, rec, run)
    return _DENSE[key]


def compare_with_dense(model, xy, rec, where):
    np.testing.assert_allclose(nn(model.nat1), rec["nat1"], err_msg=f"nat1 {where}", **TOL)
    np.testing.assert_allclose(nn(model.nat2), rec["nat2"], err_msg=f"nat2 {where}", **TOL)
    np.testing.assert_allclose(nn(model.log_norm), rec["log_norm"], err_msg=f"log_norm {where}", **TOL)
    np.testing.assert_allclose(float(model.energy(xy)), rec["energy"], err_msg=f"energy {where}", **TOL)


def run_against_dense(name, num_points, seed, z, alpha, separated=False, iterations=10, record=(1, 5, 10)):
    x, y, rec, run = dense_run(name, num_points, seed, z, alpha, separated, iterations)
    model = build_model(name, M32, z, alpha=alpha)
    xy = data(x, y)
    for it in range(1, iterations + 1):
        model.update_sites(xy)
        if it in record:
            compare_with_dense(model, xy, rec[it], f"{name} N={num_points} seed={seed} alpha={alpha} iteration {it}")
    return model, xy, run


@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("seed", [0, 1])
def test_thirty_three_points_on_five_inducing_points_against_the_dense_loop(seed, alpha):
    model, xy, run = run_against_dense(L.BERNOULLI, 33, seed, Z5, alpha)
    assert tuple(model.nat1.shape) == (6, 4) and tuple(model.nat2.shape) == (6, 4, 4) and tuple(model.log_norm.shape) == (6,)
    # the cavity, the counts and the normalisers of the final q
    counts = model.compute_num_data_per_interval(xy[0])
    assert nn(counts).tolist() == run.counts.tolist() and int(counts.sum()) == 33
    np.testing.assert_allclose(nn(model.fraction_sites(xy[0])), np.where(run.counts > 0, 1.0 / np.maximum(run.counts, 1.0), 0.0), rtol=1e-15)
    cm, cc, _ = run.cavity()
    got_m, got_c = model.compute_cavity_state_pairs(xy[0])
    np.testing.assert_allclose(nn(got_m), cm, **TOL)
    np.testing.assert_allclose(nn(got_c), cc, **TOL)
    fmu, fvar = model.compute_cavity(xy[0])
    assert tuple(fmu.shape) == tuple(fvar.shape) == (33, 1)
    want_mu, want_var = run.cavity_f()
    np.testing.assert_allclose(nn(fmu)[:, 0], want_mu, **TOL)
    np.testing.assert_allclose(nn(fvar)[:, 0], want_var, **TOL)
    log_norm = model.compute_log_norm(xy)
    assert tuple(log_norm.shape) == (6,)
    np.testing.assert_allclose(nn(log_norm), run.log_norms(), **TOL)
    obj, (l1, l2) = model.local_objective_gradients(fmu, fvar, xy[1])
    assert tuple(obj.shape) == (33,) and tuple(l1.shape) == tuple(l2.shape) == (33, 1)
    assert torch.equal(model.local_objective(fmu, fvar, xy[1]), obj)
    # prediction
    t_new = np.array([-0.5, 0.3, 1.9, 2.7, 4.9, 6.4])
    mean, var = run.predict_f(t_new)
    f_mean, f_var = model.posterior.predict_f(tt(t_new))
    np.testing.assert_allclose(nn(f_mean)[:, 0], mean, **TOL)
    np.testing.assert_allclose(nn(f_var)[:, 0], var, rtol=1e-5, atol=1e-7)
    y_new = np.array([0.0, 1.0, 1.0, 0.0, 1.0, 0.0])
    density = model.predict_log_density((tt(t_new), tt(y_new)[:, None]))
    np.testing.assert_allclose(nn(density), L.predict_log_density(L.LIKELIHOODS[L.BERNOULLI], mean, var, y_new), rtol=1e-5, atol=1e-6)
    assert float(model.loss(xy)) == -float(model.classic_elbo(xy)) and np.isfinite(float(model.classic_elbo(xy)))


@pytest.mark.parametrize("z", [(3.0,), (-2.5, -1.7, -0.4), (0.5, 0.6, 0.7, 3.0, 3.1, 5.0, 7.5, 8.0)],
                         ids=["one-inducing-point", "all-left-of-the-data", "gaps-without-data"])
def test_inducing_layouts_with_empty_segments(z):
    """M = 1 (a chain without transitions), every inducing point left of the data (all 33 points share the last site: beta = alpha /
    33), and - 8 points of data on [0, 6] in well-separated cells - gaps between inducing points that hold no data: an empty segment
    decays and carries no normaliser."""
    num_points = 33 if len(z) < 8 else 8
    model, xy, run = run_against_dense(L.BERNOULLI, num_points, 2, z, 0.5, separated=True, iterations=5, record=(1, 5))
    assert tuple(model.nat1.shape) == (len(z) + 1, 4)
    if len(z) == 3:
        assert run.counts.tolist() == [0, 0, 0, 33]
    if len(z) == 8:
        empty = np.flatnonzero(run.counts == 0)
        assert len(empty) >= 3
        assert float(model.nat1[empty].abs().max()) == 0.0 and float(model.log_norm[empty].abs().max()) == 0.0


@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("name", [L.BERNOULLI, L.POISSON])
def test_inducing_points_on_the_data_reproduce_the_dense_site_model_step_for_step(name, alpha):
    """Z = X: every segment but the last holds one point, w selects u_m and c = 0, beta = alpha: the pair cavity projects to the scalar
    cavity and Gamma to G(mu_c, v_c) - G(m, s).  (The dense-site model starts nat2 at -1e-10, this one at 0: far below the tolerance.)"""
    x, y = L.draw_series(L.LIKELIHOODS[name], M32, 8, seed=3, separated=True)
    sparse = build_model(name, M32, x, alpha=alpha)
    full = mfa.PowerExpectationPropagation(data(x, y), build_kernel(M32), build_likelihood(name), learning_rate=0.5, alpha=alpha)
    xy = data(x, y)
    t_new = tt(np.sort(np.concatenate([[x[0] - 0.4, x[-1] + 0.7], 0.5 * (x[1:] + x[:-1])[::2]])))
    for it in range(1, 6):
        sparse.update_sites(xy)
        full.update_sites()
        np.testing.assert_allclose(float(sparse.energy(xy)), float(full.energy()), err_msg=f"energy, iteration {it}", **TOL)
        (m_s, v_s), (m_f, v_f) = sparse.posterior.predict_f(t_new), full.posterior.predict_f(t_new)
        np.testing.assert_allclose(nn(m_s), nn(m_f), err_msg=f"iteration {it}", **TOL)
        np.testing.assert_allclose(nn(v_s), nn(v_f), rtol=1e-5, atol=1e-7, err_msg=f"iteration {it}")
        # the pairs embed the univariate sites: [0, h]-projected blocks
        np.testing.assert_allclose(nn(sparse.nat1)[:-1, 2], nn(full.sites.nat1)[:, 0], **TOL)
        np.testing.assert_allclose(nn(sparse.nat2)[:-1, 2, 2], nn(full.sites.nat2)[:, 0, 0], **TOL)
        np.testing.assert_allclose(nn(sparse.log_norm)[:-1], nn(full.sites.log_norm)[:, 0], **TOL)
    assert float(sparse.nat1.abs().max()) > 0.0


def test_gaussian_likelihood_on_the_data_with_unit_power_and_rate_is_gp_regression():
    """One step at alpha = lr = 1 lands on the exact sites and the energy is the log marginal likelihood: against
    ``GaussianProcessRegression`` and against the dense kernel matrix (a sparse-against-full comparison, as
    tests/test_gpu_sparse_cvi.py's of the same name)."""
    var = L.LIKELIHOODS[L.GAUSSIAN][1][0]
    x, y = L.draw_series(L.LIKELIHOODS[L.GAUSSIAN], M32, 8, seed=0, separated=True)
    model = build_model(L.GAUSSIAN, M32, x, lr=1.0, alpha=1.0)
    xy = data(x, y)
    model.update_sites(xy)
    np.testing.assert_allclose(nn(model.nat1)[:-1, 2], y / var, **TOL)
    np.testing.assert_allclose(nn(model.nat2)[:-1, 2, 2], np.full(8, -0.5 / var), **TOL)
    gpr = mfa.GaussianProcessRegression((tt(x), tt(y)[:, None]), build_kernel(M32), chol_obs_covariance=tt([[np.sqrt(var)]]))
    np.testing.assert_allclose(float(model.energy(xy)), float(gpr.log_likelihood()), **TOL)
    np.testing.assert_allclose(float(model.energy(xy)), L.PC.dense_log_marginal(M32, x, y, var), **TOL)


def test_a_batch_of_two_by_three_series_equals_six_models():
    z = np.stack([Z5 + 0.05 * s for s in range(6)]).reshape(2, 3, 5)
    runs = [dense_run(L.BERNOULLI, 33, seed, z.reshape(6, 5)[seed], 0.5) for seed in range(6)]
    x = np.stack([r[0] for r in runs]).reshape(2, 3, 33)
    y = np.stack([r[1] for r in runs]).reshape(2, 3, 33)
    batch = build_model(L.BERNOULLI, M32, z)
    singles = [build_model(L.BERNOULLI, M32, z.reshape(6, 5)[s]) for s in range(6)]
    for _ in range(5):
        batch.update_sites(data(x, y))
        for s, m in enumerate(singles):
            m.update_sites(data(x.reshape(6, 33)[s], y.reshape(6, 33)[s]))
    assert tuple(batch.nat1.shape) == (2, 3, 6, 4) and tuple(batch.nat2.shape) == (2, 3, 6, 4, 4) and tuple(batch.log_norm.shape) == (2, 3, 6)
    energy = batch.energy(data(x, y))
    assert tuple(energy.shape) == (2, 3) and tuple(batch.compute_log_norm(data(x, y)).shape) == (2, 3, 6)
    for s, (m, r) in enumerate(zip(singles, runs)):
        i, j = divmod(s, 3)
        for got, one in ((batch.nat1, m.nat1), (batch.nat2, m.nat2), (batch.log_norm, m.log_norm)):
            np.testing.assert_allclose(nn(got)[i, j], nn(one), rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(nn(batch.nat1)[i, j], r[2][5]["nat1"], **TOL)
        np.testing.assert_allclose(nn(batch.log_norm)[i, j], r[2][5]["log_norm"], **TOL)
        assert float(energy[i, j]) == pytest.approx(float(m.energy(data(x.reshape(6, 33)[s], y.reshape(6, 33)[s]))), rel=1e-9)
        np.testing.assert_allclose(float(energy[i, j]), r[2][5]["energy"], **TOL)


def test_update_sites_is_one_call_of_the_kernel_pair_and_no_torch_route(monkeypatch):
    x, y, _, _ = dense_run(L.BERNOULLI, 33, 0, Z5, 0.5)
    model = build_model(L.BERNOULLI, M32, Z5)
    xy = data(x, y)                     # (the projection cache is keyed on the data TENSOR)
    seen = []
    real_rc = _lib.call_rc
    monkeypatch.setattr(_lib, "call_rc", lambda base, *a: (seen.append(base), real_rc(base, *a))[1])

    def no_torch(*a, **k):
        raise AssertionError("the torch route must not run on HIP tensors")

    for route in ("torch_variational_expectations", "torch_predict_log_density", "torch_log_expected_density", "torch_pep_site_update"):
        monkeypatch.setattr(ML, route, no_torch)
    monkeypatch.setattr(MM.segmented_ops, "torch_log_expected_density", no_torch)
    monkeypatch.setattr(MM.sparse, "sparse_pep_site_update_torch", no_torch)
    sites = (model.nat1, model.nat2, model.log_norm)
    versions = [s._version for s in sites]
    model.update_sites(xy)
    assert seen.count(FN) == 1
    assert not any(s.startswith("mf_lik_") and s != FN for s in seen)
    assert all(s._version > v for s, v in zip(sites, versions))
    assert all(float(s.abs().max()) > 0.0 for s in sites)
    del seen[:]
    model.energy(xy)
    assert [s for s in seen if s.startswith("mf_lik_")] == [FN], "evaluation-only mode, one call"
    del seen[:]
    model.update_sites(xy)
    assert seen.count(FN) == 1 and "mf_sde_conditional_statistics" not in seen, "the projections are cached with the data"


def test_pairs_of_dimension_twenty_take_the_torch_route(monkeypatch):
    comps = [dict(order=5, ls=1.0 + 0.3 * i, var=0.5, period=None, osc=0) for i in range(3)] + [dict(order=1, ls=1.0, var=0.3, period=None,
                                                                                                  osc=0)]
    x, y = L.draw_series(L.LIKELIHOODS[L.BERNOULLI], M32, 33, seed=0, separated=True)
    model = mfa.SparsePowerExpectationPropagation(build_kernel(comps), tt(Z5), mfa.Bernoulli(), learning_rate=0.5, alpha=0.5)
    assert model.nat1.shape[-1] == 20
    seen, calls = [], []
    real_rc, real_torch = _lib.call_rc, MM.sparse_pep_site_update_torch
    monkeypatch.setattr(_lib, "call_rc", lambda base, *a: (seen.append(base), real_rc(base, *a))[1])
    monkeypatch.setattr(MM.sparse, "sparse_pep_site_update_torch", lambda *a, **k: (calls.append(1), real_torch(*a, **k))[1])
    model.update_sites(data(x, y))
    assert len(calls) == 1 and FN not in seen
    assert all(bool(torch.isfinite(s).all()) and float(s.abs().max()) > 0.0 for s in (model.nat1, model.nat2, model.log_norm))
    assert np.isfinite(float(model.energy(data(x, y)))) and len(calls) == 2


def test_unsorted_data_and_mismatched_batches_raise():
    x, y, _, _ = dense_run(L.BERNOULLI, 33, 0, Z5, 0.5)
    model = build_model(L.BERNOULLI, M32, Z5)
    before = model.nat1.clone()
    with pytest.raises(ValueError, match="time_points must be sorted"):
        model.update_sites(data(x[::-1].copy(), y))
    with pytest.raises(ValueError, match="time_points must be sorted"):
        model.energy(data(x[::-1].copy(), y))
    with pytest.raises(ValueError, match="batch shape"):
        model.update_sites(data(np.stack([x, x]), np.stack([y, y])))
    assert torch.equal(model.nat1, before)
