"""
GPU tests of ``SparseCVIGaussianProcess`` (markovflow_amd/models.py) against the dense sparse CVI loop of
tests/helpers/sparse_cvi_closed_forms.py: the same iteration on ONE dense Gaussian over the stacked inducing states, no
block-tridiagonal algebra.

State space against dense: rtol 1e-6 / atol 1e-7, the ``TOL`` of tests/test_gpu_cvi.py (prediction variances: its rtol 1e-5).  The
kernels carry jitter 0 and so does the dense loop.  Every series has at most 33 points and at most 8 inducing points; every dense
run asserts that its ``dist_q`` stays positive definite (``dense_posterior``), so the reference is a reference.
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

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = dict(rtol=1e-6, atol=1e-7)
M12 = [dict(order=1, ls=1.0, var=1.0, period=None, osc=0)]
M32 = [dict(order=3, ls=1.0, var=1.0, period=None, osc=0)]
M52_M32 = [dict(order=5, ls=1.3, var=0.8, period=None, osc=0), dict(order=3, ls=0.6, var=0.5, period=None, osc=0)]
KERNELS = {"m12": M12, "m32": M32, "m52+m32": M52_M32}
RECORD = (1, 5, 25)
Z5 = np.array([0.6, 1.9, 3.1, 4.2, 5.5])          # five inducing points inside the data's span [0, 6]


def tt(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64, device=DEV)


def nn(t):
    return t.detach().cpu().numpy()


def build_kernel(comps, lengthscales=None):
    cls = {1: mfa.Matern12, 3: mfa.Matern32, 5: mfa.Matern52}
    parts = [cls[c["order"]](c["ls"] if lengthscales is None else lengthscales[i], c["var"], device=DEV) for i, c in enumerate(comps)]
    return parts[0] if len(parts) == 1 else mfa.Sum(parts)


def build_likelihood(name):
    params = L.LIKELIHOODS[name][1]
    return {L.GAUSSIAN: lambda: mfa.Gaussian(params[0]), L.BERNOULLI: mfa.Bernoulli, L.POISSON: mfa.Poisson}[name]()


def build_model(name, comps, z, lr=0.5):
    return mfa.SparseCVIGaussianProcess(build_kernel(comps), tt(z), build_likelihood(name), learning_rate=lr)


def data(x, y):
    return tt(x), tt(y)[..., None]


_DENSE = {}


def dense_run(name, comps_key, num_points, seed, z, separated=False, iterations=25):
    """Data and the dense loop's record for one series: computed once, shared, not modified."""
    key = (name, comps_key, num_points, seed, tuple(z), separated, iterations)
    if key not in _DENSE:
        comps = KERNELS[comps_key]
        x, y = L.draw_series(L.LIKELIHOODS[name], comps, num_points, seed, separated=separated)
        rec, run = SC.dense_sparse_cvi(L.LIKELIHOODS[name], comps, x, y, np.asarray(z), lr=0.5, iterations=iterations,
                                       record=tuple(range(1, iterations + 1)))
        _DENSE[key] = (comps, x, y, rec, run)
    return _DENSE[key]


def compare_with_dense(model, xy, rec, where):
    np.testing.assert_allclose(nn(model.nat1), rec["nat1"], err_msg=f"nat1 {where}", **TOL)
    np.testing.assert_allclose(nn(model.nat2), rec["nat2"], err_msg=f"nat2 {where}", **TOL)
    np.testing.assert_allclose(float(model.classic_elbo(xy)), rec["classic_elbo"], err_msg=f"classic_elbo {where}", **TOL)


def run_against_dense(name, comps_key, num_points, seed, z, separated=False, iterations=25, record=RECORD):
    comps, x, y, rec, _ = dense_run(name, comps_key, num_points, seed, z, separated, iterations)
    model = build_model(name, comps, z)
    xy = data(x, y)
    for it in range(1, iterations + 1):
        model.update_sites(xy)
        if it in record:
            compare_with_dense(model, xy, rec[it], f"{name} {comps_key} N={num_points} seed={seed} iteration {it}")
    return model


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("name", [L.BERNOULLI, L.POISSON])
def test_runs_against_the_dense_sparse_loop(name, seed):
    model = run_against_dense(name, "m32", 33, seed, Z5)
    assert tuple(model.nat1.shape) == (6, 4) and tuple(model.nat2.shape) == (6, 4, 4)


def test_sum_of_two_materns_with_pairs_of_dimension_ten():
    """Well-separated data AND inducing points, for the reason ``dense_run`` of tests/test_gpu_cvi.py gives: a Matern-5/2 kernel
    matrix on close points is no reference at 1e-6 once it is inverted."""
    model = run_against_dense(L.BERNOULLI, "m52+m32", 33, 1, Z5, separated=True)
    assert model.dist_q.state_dim == 5 and tuple(model.nat2.shape) == (6, 10, 10)


def test_inducing_points_on_the_data_reproduce_the_cvi_model_step_for_step():
    comps = M32
    x, y = L.draw_series(L.LIKELIHOODS[L.BERNOULLI], comps, 8, seed=3, separated=True)
    sparse = build_model(L.BERNOULLI, comps, x)
    full = mfa.CVIGaussianProcess(data(x, y), build_kernel(comps), mfa.Bernoulli(), learning_rate=0.5)
    xy = data(x, y)
    t_new = tt(np.sort(np.concatenate([[x[0] - 0.4, x[-1] + 0.7], 0.5 * (x[1:] + x[:-1])[::2]])))
    for it in range(1, 6):
        sparse.update_sites(xy)
        full.update_sites()
        if it in (1, 5):
            np.testing.assert_allclose(float(sparse.classic_elbo(xy)), float(full.classic_elbo()), err_msg=f"iteration {it}", **TOL)
            (m_s, v_s), (m_f, v_f) = sparse.posterior.predict_f(t_new), full.posterior.predict_f(t_new)
            np.testing.assert_allclose(nn(m_s), nn(m_f), err_msg=f"iteration {it}", **TOL)
            np.testing.assert_allclose(nn(v_s), nn(v_f), rtol=1e-5, atol=1e-7, err_msg=f"iteration {it}")
            # the pairs embed the univariate sites: [0, h]-projected blocks
            np.testing.assert_allclose(nn(sparse.nat1)[:-1, 2], nn(full.sites.nat1)[:, 0], **TOL)
            np.testing.assert_allclose(nn(sparse.nat2)[:-1, 2, 2], nn(full.sites.nat2)[:, 0, 0], **TOL)


def test_gaussian_likelihood_with_unit_learning_rate_is_the_collapsed_sparse_bound():
    """Matern-1/2: the state is f, so the inducing states are inducing function values, and one step at lr = 1 lands on the optimal
    q(u) of Titsias' bound; classic_elbo is then the collapsed bound and predict_f the sparse GP predictive, both computed densely."""
    noise = L.LIKELIHOODS[L.GAUSSIAN][1][0]
    x, y = L.draw_series(L.LIKELIHOODS[L.GAUSSIAN], M12, 33, seed=0, separated=True)
    model = build_model(L.GAUSSIAN, M12, Z5, lr=1.0)
    xy = data(x, y)
    model.update_sites(xy)
    np.testing.assert_allclose(float(model.classic_elbo(xy)), SC.collapsed_bound(M12, x, y, Z5, noise), **TOL)
    t_new = np.array([-0.5, 0.3, 1.9, 2.7, 4.9, 6.4])
    mean, var = SC.sparse_gp_predict(M12, x, y, Z5, noise, t_new)
    f_mean, f_var = model.posterior.predict_f(tt(t_new))
    np.testing.assert_allclose(nn(f_mean)[:, 0], mean, **TOL)
    np.testing.assert_allclose(nn(f_var)[:, 0], var, rtol=1e-5, atol=1e-7)
    assert float(model.loss(xy)) == -float(model.classic_elbo(xy))


@pytest.mark.parametrize("z", [(3.0,), (-2.5, -1.7, -0.4), (0.5, 0.6, 0.7, 3.0, 3.1, 5.0, 7.5, 8.0)],
                         ids=["one-inducing-point", "all-left-of-the-data", "gaps-without-data"])
def test_inducing_layouts(z):
    """M = 1 (a chain without transitions), every inducing point left of the data (all the points in the last pair), and - with 8 points
    of data on [0, 6] in well-separated cells - gaps between inducing points that hold no data, inducing points beyond the data."""
    num_points = 33 if len(z) < 8 else 8
    model = run_against_dense(L.POISSON, "m32", num_points, 2, z, separated=True, iterations=5, record=(1, 5))
    assert tuple(model.nat1.shape) == (len(z) + 1, 4)
    _, _, _, _, run = dense_run(L.POISSON, "m32", num_points, 2, z, True, 5)
    counts = np.diff(run.offsets)
    if len(z) == 3:
        assert list(counts) == [0, 0, 0, 33]
    if len(z) == 8:
        assert (counts == 0).sum() >= 3
        empty = np.flatnonzero(counts == 0)
        assert float(model.nat1[empty].abs().max()) == 0.0, "a pair without data keeps its zero sites"


def test_a_batch_of_three_series_equals_three_models():
    z = np.stack([Z5, Z5 + 0.1, Z5 - 0.2])
    runs = [dense_run(L.BERNOULLI, "m32", 33, seed, z[seed]) for seed in range(3)]
    x, y = np.stack([r[1] for r in runs]), np.stack([r[2] for r in runs])
    batch = build_model(L.BERNOULLI, M32, z)
    singles = [build_model(L.BERNOULLI, M32, z[s]) for s in range(3)]
    for _ in range(5):
        batch.update_sites(data(x, y))
        for s, m in enumerate(singles):
            m.update_sites(data(x[s], y[s]))
    assert tuple(batch.nat1.shape) == (3, 6, 4) and tuple(batch.nat2.shape) == (3, 6, 4, 4)
    for s, (m, r) in enumerate(zip(singles, runs)):
        np.testing.assert_allclose(nn(batch.nat1)[s], nn(m.nat1), rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(nn(batch.nat2)[s], nn(m.nat2), rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(nn(batch.nat1)[s], r[3][5]["nat1"], **TOL)
        np.testing.assert_allclose(nn(batch.nat2)[s], r[3][5]["nat2"], **TOL)
    total = float(batch.classic_elbo(data(x, y)))
    assert total == pytest.approx(sum(float(m.classic_elbo(data(x[s], y[s]))) for s, m in enumerate(singles)), rel=1e-10)
    assert total == pytest.approx(sum(r[3][5]["classic_elbo"] for r in runs), rel=1e-6)


def test_update_sites_is_one_launch_of_the_sparse_site_kernel_and_no_torch_route(monkeypatch):
    comps, x, y, _, _ = dense_run(L.BERNOULLI, "m32", 33, 0, Z5)
    model = build_model(L.BERNOULLI, comps, Z5)
    seen = []
    real_rc = _lib.call_rc
    monkeypatch.setattr(_lib, "call_rc", lambda base, *a: (seen.append(base), real_rc(base, *a))[1])

    def no_torch(*a, **k):
        raise AssertionError("the torch route must not run on HIP tensors")

    monkeypatch.setattr(ML, "torch_variational_expectations", no_torch)
    monkeypatch.setattr(ML, "torch_predict_log_density", no_torch)
    monkeypatch.setattr(MM.sparse, "sparse_cvi_site_update_torch", no_torch)
    versions = (model.nat1._version, model.nat2._version)
    model.update_sites(data(x, y))
    assert seen.count("mf_lik_sparse_cvi_site_update") == 1
    assert not any(s.startswith("mf_lik_") and s != "mf_lik_sparse_cvi_site_update" for s in seen)
    assert model.nat1._version > versions[0] and model.nat2._version > versions[1]
    assert float(model.nat1.abs().max()) > 0.0
    del seen[:]
    model.classic_elbo(data(x, y))
    assert [s for s in seen if s.startswith("mf_lik_")] == ["mf_lik_sparse_cvi_site_update"], "projection-only mode, one launch"


def test_second_update_reuses_the_projections_and_a_length_scale_written_in_place_is_seen(monkeypatch):
    comps, x, y, rec, _ = dense_run(L.POISSON, "m32", 33, 1, Z5)
    xy = data(x, y)
    ls = torch.tensor(1.0, dtype=torch.float64, device=DEV)
    model = mfa.SparseCVIGaussianProcess(mfa.Matern32(ls, 1.0, device=DEV), tt(Z5), mfa.Poisson(), learning_rate=0.5)
    calls = []
    real = conditionals._conditional_statistics
    monkeypatch.setattr(conditionals, "_conditional_statistics", lambda *a: (calls.append(1), real(*a))[1])
    model.update_sites(xy)
    model.update_sites(xy)
    model.classic_elbo(xy)
    assert len(calls) == 1, "w, c and the offsets depend on the hyper-parameters, x and z only: built once"
    np.testing.assert_allclose(nn(model.nat1), rec[2]["nat1"], **TOL)
    fresh = mfa.SparseCVIGaussianProcess(mfa.Matern32(1.25, 1.0, device=DEV), tt(Z5), mfa.Poisson(), learning_rate=0.5)
    fresh.nat1.copy_(model.nat1)
    fresh.nat2.copy_(model.nat2)
    ls.mul_(1.25)                                        # (1.0 x 1.25 is exact: the two models now hold the same numbers)
    model.update_sites(xy)
    assert len(calls) == 2, "an in-place change of a length scale must be seen by the next step"
    stale = nn(model.nat1).copy()
    fresh.update_sites(xy)
    assert len(calls) == 3
    np.testing.assert_allclose(nn(model.nat1), nn(fresh.nat1), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(nn(model.nat2), nn(fresh.nat2), rtol=1e-12, atol=1e-14)
    assert np.abs(stale - rec[3]["nat1"]).max() > 1e-4, "and the step with the new length scale is not the old one's"
    # other data through the same model: not the cached projections of the first
    model.update_sites(data(x[:20], y[:20]))
    assert len(calls) == 4


def test_classic_elbo_backward_gives_the_lengthscale_gradient():
    """d classic_elbo / d lengthscale with the sites held fixed, against central differences.  The error budget is that of
    ``test_elbo_backward_gives_the_lengthscale_gradient`` (tests/test_gpu_cvi.py): well-separated points, a value good to about
    1e-12 relative, |value| below 60, h = 1e-4: rounding 1e-12 x 60 / 1e-4 = 6e-7 and truncation h^2 / 6 x (a third derivative of
    order ten) = 2e-8, against a gradient of order 0.1 or more: rtol 1e-5."""
    comps, x, y, rec, _ = dense_run(L.BERNOULLI, "m32", 33, 4, Z5, separated=True)
    xy = data(x, y)

    def elbo_at(ls, grad=False):
        ls_t = torch.tensor(ls, dtype=torch.float64, device=DEV, requires_grad=grad)
        m = mfa.SparseCVIGaussianProcess(mfa.Matern32(ls_t, 1.0, device=DEV), tt(Z5), mfa.Bernoulli(), learning_rate=0.5)
        m.nat1.copy_(tt(rec[5]["nat1"]))
        m.nat2.copy_(tt(rec[5]["nat2"]))
        return m.classic_elbo(xy), ls_t, m

    value, ls_t, model = elbo_at(1.0, grad=True)
    assert value.requires_grad
    np.testing.assert_allclose(float(value.detach()), rec[5]["classic_elbo"], **TOL)
    with torch.no_grad():
        np.testing.assert_allclose(float(model.classic_elbo(xy)), float(value.detach()), rtol=1e-10)     # both routes, one value
    value.backward()
    h = 1e-4
    fd = (float(elbo_at(1.0 + h)[0]) - float(elbo_at(1.0 - h)[0])) / (2 * h)
    assert abs(float(ls_t.grad)) > 1e-2
    np.testing.assert_allclose(float(ls_t.grad), fd, rtol=1e-5, atol=1e-7)
    loss, ls_2, _ = elbo_at(1.0, grad=True)
    (-loss).backward()
    assert float(ls_2.grad) == pytest.approx(-float(ls_t.grad), rel=1e-12)


@pytest.mark.parametrize("name", [L.BERNOULLI, L.POISSON])
def test_prediction_and_log_density_at_new_time_points_against_the_dense_posterior(name):
    comps, x, y, rec, run = dense_run(name, "m32", 33, 1, Z5)
    model = build_model(name, comps, Z5)
    model.nat1.copy_(tt(rec[25]["nat1"]))
    model.nat2.copy_(tt(rec[25]["nat2"]))
    rng = np.random.default_rng(11)
    t_new = np.sort(np.concatenate([x[0] - 0.1 - rng.random(2), x[-1] + 0.1 + rng.random(2), rng.uniform(x[0], x[-1], 5)]))
    y_new = np.array([0.0, 1.0, 1.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0]) if name == L.BERNOULLI else np.arange(9.0) % 4
    mean, var = run.predict_f(t_new)
    f_mean, f_var = model.posterior.predict_f(tt(t_new))
    assert tuple(f_mean.shape) == (9, 1) and tuple(f_var.shape) == (9, 1)
    np.testing.assert_allclose(nn(f_mean)[:, 0], mean, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(nn(f_var)[:, 0], var, rtol=1e-5, atol=1e-7)
    density = model.predict_log_density((tt(t_new), tt(y_new)[:, None]))
    assert tuple(density.shape) == (9,)
    want = L.predict_log_density(L.LIKELIHOODS[name], mean, var, y_new)
    # d log density / d(mean, var) is O(1) on this data: the prediction's tolerances carry over
    np.testing.assert_allclose(nn(density), want, rtol=1e-5, atol=1e-6)
