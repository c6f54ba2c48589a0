"""
CPU tests of markovflow_amd/likelihoods.py (the torch route CPU tensors take), of the argument checks of the ``mf_lik_*`` entry
points (which return before any launch) and of ``UnivariateGaussianSitesNat`` with leading batch dimensions, against the
numpy / scipy reference of tests/helpers/likelihood_closed_forms.py.

Tolerances (float64, eps = 2^-52): ``|err| <= K eps (magnitude + 1)`` with the magnitudes of the helper - the sum of the absolute
terms of each expression - and K = 64: both
sides are IEEE double evaluations of the same short expressions by different libm's.
"""
import ctypes

import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from markovflow_amd import likelihoods as ML
from helpers import likelihood_closed_forms as L

EPS = 2.0 ** -52
K_HOST = 64.0
NAMES = [L.GAUSSIAN, L.BERNOULLI, L.POISSON, L.STUDENTT]


def make(name, nq=20):
    params = L.LIKELIHOODS[name][1]
    if name == L.GAUSSIAN:
        return mfa.Gaussian(variance=params[0], num_gauss_hermite_points=nq)
    if name == L.BERNOULLI:
        return mfa.Bernoulli(num_gauss_hermite_points=nq)
    if name == L.POISSON:
        return mfa.Poisson(num_gauss_hermite_points=nq)
    return mfa.StudentT(scale=params[0], df=params[1], num_gauss_hermite_points=nq)


def col(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype).reshape(-1, 1)


def within(got, want, mag, k=K_HOST, eps=EPS):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    ratio = np.abs(got - want) / (eps * (np.asarray(mag) + 1.0))
    assert np.all(np.isfinite(got)), "non-finite result"
    assert ratio.max() <= k, f"largest error {ratio.max():.1f} eps (magnitude + 1) at point {int(ratio.argmax())}"


@pytest.mark.parametrize("name", NAMES)
def test_log_prob_matches_scipy(name):
    mu, _, y = L.value_grid(name)
    got = make(name).log_prob(col(mu), col(y))
    assert tuple(got.shape) == (mu.size,)
    want = L.log_prob(L.LIKELIHOODS[name], mu, y)
    within(got.numpy(), want, np.abs(want))


@pytest.mark.parametrize("name", NAMES)
def test_torch_expectations_match_the_helper(name):
    mu, var, y = L.value_grid(name)
    lik = make(name)
    (ve, g_mu, g_var), mags = L.expectations(L.LIKELIHOODS[name], mu, var, y)
    got = lik._expectations(col(mu), col(var), col(y))
    for g, want, mag in zip(got, (ve, g_mu, g_var), mags):
        within(g.numpy()[:, 0], want, mag)
    out = lik.variational_expectations(col(mu), col(var), col(y))
    assert tuple(out.shape) == (mu.size,)
    within(out.numpy(), ve, mags[0])
    # leading batch dimensions: batch + [N, 1] -> batch + [N]
    shaped = lik.variational_expectations(*(col(a).reshape(4, -1, 1) for a in (mu, var, y)))
    assert tuple(shaped.shape) == (4, mu.size // 4) and torch.equal(shaped.reshape(-1), out)


@pytest.mark.parametrize("name", [L.GAUSSIAN, L.POISSON])
def test_gaussian_and_poisson_take_their_closed_forms(name):
    mu, var, y = L.value_grid(name)
    want = L.closed_form(L.LIKELIHOODS[name], mu, var, y)
    _, mags = L.expectations(L.LIKELIHOODS[name], mu, var, y)
    for nq in (1, 20):                       # the rule plays no part
        got = make(name, nq)._expectations(col(mu), col(var), col(y))
        for g, w, mag in zip(got, want, mags):
            within(g.numpy()[:, 0], w, mag)


def test_gaussian_quadrature_with_20_points_is_exact():
    """log N(y | f, v) is a quadratic in f: the 20-point rule integrates it exactly, derivatives included."""
    lik = L.LIKELIHOODS[L.GAUSSIAN]
    mu, var, y = L.value_grid(L.GAUSSIAN)
    vals, mags = L.quadrature(lik, mu, var, y, nq=20)
    for v, want, mag in zip(vals, L.closed_form(lik, mu, var, y), mags):
        within(v, want, mag)


@pytest.mark.parametrize("name", NAMES)
def test_backward_matches_central_differences_of_the_helper(name):
    """d VE / d(mu, var) through backward() against central differences of the helper's value.  Steps: 1e-4 in mu and
    1e-3 min(var, 1) in var.  The bound is the differences' own error: rounding, 8 eps (magnitude + 1) / h, and truncation,
    h^2 |third derivative| / 6, taken as 1e-5 of the derivative's magnitude (the sum of its absolute terms: the net derivative can
    be far smaller by cancellation, the third derivative is not).  The largest truncation among these functions is that of
    exp(mu + var / 2): (h / 2)^2 / 6 = 4e-8 relative."""
    spec = L.LIKELIHOODS[name]
    mu, var, y = L.value_grid(name)
    fmu, fvar = col(mu).requires_grad_(True), col(var).requires_grad_(True)
    make(name).variational_expectations(fmu, fvar, col(y)).sum().backward()
    (_, g_mu, g_var), mags = L.expectations(spec, mu, var, y)
    value = lambda m, v: L.expectations(spec, m, v, y)[0][0]        # noqa: E731
    h_mu, h_var = 1e-4, 1e-3 * np.minimum(var, 1.0)
    fd_mu = (value(mu + h_mu, var) - value(mu - h_mu, var)) / (2 * h_mu)
    fd_var = (value(mu, var + h_var) - value(mu, var - h_var)) / (2 * h_var)
    for got, fd, h, mag in ((fmu.grad, fd_mu, h_mu, mags[1]), (fvar.grad, fd_var, h_var, mags[2])):
        got = got.numpy()[:, 0]
        bound = 1e-5 * mag + 8 * EPS * (mags[0] + 1.0) / h
        assert np.all(np.abs(got - fd) <= bound), float(np.max(np.abs(got - fd) / bound))
    # and the analytic derivatives of the helper
    within(fmu.grad.numpy()[:, 0], g_mu, mags[1])
    within(fvar.grad.numpy()[:, 0], g_var, mags[2])


def test_backward_refuses_a_second_order_graph():
    fmu = torch.zeros(3, 1, dtype=torch.float64, requires_grad=True)
    fvar = torch.ones(3, 1, dtype=torch.float64, requires_grad=True)
    out = mfa.Bernoulli().variational_expectations(fmu, fvar, torch.ones(3, 1, dtype=torch.float64)).sum()
    with pytest.raises(RuntimeError, match="differentiable once"):
        torch.autograd.grad(out, fmu, create_graph=True)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("nq", [7, 20])
def test_predict_log_density_matches_the_helper(name, nq):
    mu, var, y = L.value_grid(name)
    got = make(name, nq).predict_log_density(col(mu), col(var), col(y))
    assert tuple(got.shape) == (mu.size,)
    want = L.predict_log_density(L.LIKELIHOODS[name], mu, var, y, nq)
    within(got.numpy(), want, L.predict_log_density_magnitude(L.LIKELIHOODS[name], mu, var, y, nq))


@pytest.mark.parametrize("name", NAMES)
def test_predict_mean_and_var_against_a_100_point_quadrature(name):
    """Variances up to 1: the closed forms are exact integrals, the 100-point rule converges to them only while the integrand
    (the probit of a line, exp(2 f)) stays smooth on the scale of the nodes; at var = 100 it does not (the peak of
    exp(2 f) N(f) lies beyond the outermost node).  rtol 1e-8 is the rule's error there, not the closed forms'."""
    mu, var, _ = L.value_grid(name, variances=(1e-6, 1e-2, 1.0))
    mean, variance = make(name).predict_mean_and_var(col(mu), col(var))
    assert tuple(mean.shape) == (mu.size, 1) and tuple(variance.shape) == (mu.size, 1)
    want_mean, want_var = L.predict_mean_and_var(L.LIKELIHOODS[name], mu, var, nq=100)
    np.testing.assert_allclose(mean.numpy()[:, 0], want_mean, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(variance.numpy()[:, 0], want_var, rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("lr", [0.1, 1.0])
def test_cvi_site_update_on_cpu_tensors(name, lr, rng):
    mu, var, y = L.value_grid(name)
    (_, g_mu, g_var), mags = L.expectations(L.LIKELIHOODS[name], mu, var, y)
    nat1_0, nat2_0 = rng.normal(size=mu.size), -0.5 - rng.random(mu.size)
    nat1, nat2 = col(nat1_0), col(nat2_0).reshape(-1, 1, 1)
    make(name).cvi_site_update(col(mu), col(var), col(y), lr, nat1, nat2)
    within(nat1.numpy()[:, 0], (1 - lr) * nat1_0 + lr * (g_mu - 2 * g_var * mu), np.abs(nat1_0) + mags[1] + 2 * mags[2] * np.abs(mu))
    within(nat2.numpy()[:, 0, 0], (1 - lr) * nat2_0 + lr * g_var, np.abs(nat2_0) + mags[2])


@pytest.mark.parametrize("name", NAMES)
def test_a_bad_variance_gives_nan_in_its_own_point_only(name):
    mu, var, y = (a[:12].copy() for a in L.value_grid(name))
    lik = make(name)
    clean = lik._expectations(col(mu), col(var), col(y)) + (lik.predict_log_density(col(mu), col(var), col(y))[:, None],)
    var[3], var[7], var[8] = 0.0, np.nan, -1.0
    dirty = lik._expectations(col(mu), col(var), col(y)) + (lik.predict_log_density(col(mu), col(var), col(y))[:, None],)
    bad = np.array([3, 7, 8])
    good = np.setdiff1d(np.arange(12), bad)
    for c, d in zip(clean, dirty):
        assert torch.isnan(d[bad]).all() and torch.equal(c[good], d[good])


def test_constructor_and_argument_errors():
    for bad in (0, 33, 2.5):
        with pytest.raises(ValueError, match="num_gauss_hermite_points"):
            mfa.Bernoulli(num_gauss_hermite_points=bad)
    with pytest.raises(ValueError, match="variance"):
        mfa.Gaussian(variance=0.0)
    with pytest.raises(ValueError, match="scale and df"):
        mfa.StudentT(scale=-1.0)
    with pytest.raises(ValueError, match="scale and df"):
        mfa.StudentT(df=0.0)
    with pytest.raises(ValueError, match="df > 2"):
        mfa.StudentT(df=2.0).predict_mean_and_var(torch.zeros(2, 1), torch.ones(2, 1))
    lik = mfa.Poisson()
    z = torch.zeros(4, 1, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"batch \+ \[N, 1\]"):
        lik.variational_expectations(torch.zeros(4, dtype=torch.float64), z, z)
    one = torch.zeros(1, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"batch \+ \[N, 1\]"):
        lik.log_prob(one, one)                                # [1] is not batch + [N, 1]
    with pytest.raises(ValueError, match="fvar has shape"):
        lik.variational_expectations(z, torch.zeros(3, 1, dtype=torch.float64), z)
    with pytest.raises(ValueError, match="y is torch.float32"):
        lik.predict_log_density(z, z + 1, z.float())
    with pytest.raises(TypeError, match="float32 and float64"):
        lik.log_prob(z.long(), z.long())
    with pytest.raises(ValueError, match="learning_rate"):
        lik.cvi_site_update(z, z + 1, z, 1.5, z.clone(), z.clone())
    with pytest.raises(ValueError, match="one element per data point"):
        lik.cvi_site_update(z, z + 1, z, 0.5, torch.zeros(3, 1, dtype=torch.float64), z.clone())
    assert isinstance(lik, mfa.Likelihood) and mfa.likelihoods.Poisson is mfa.Poisson
    assert mfa.StudentT().num_gauss_hermite_points == 20 and mfa.Gaussian().variance == 1.0


def test_entry_points_return_codes_without_touching_the_gpu():
    """Every argument check of the three entry points returns before a launch: the negative position of the argument."""
    lib = _lib.load()
    arr = lambda *v: (ctypes.c_double * len(v))(*v)       # noqa: E731
    x, w = np.polynomial.hermite.hermgauss(20)
    nodes, weights, var = arr(*x), arr(*w), arr(0.5)
    for suf in ("_f64", "_f32"):
        ve = getattr(lib, "mf_lik_variational_expectations" + suf)
        site = getattr(lib, "mf_lik_cvi_site_update" + suf)
        pld = getattr(lib, "mf_lik_predict_log_density" + suf)
        tail_ve, tail_site, tail_pld = (None,) * 7, (None, None, None, 0.5, None, None, None, None), (None,) * 5
        for fn, tail in ((ve, tail_ve), (site, tail_site), (pld, tail_pld)):
            assert fn(-1, 0, var, 20, nodes, weights, *tail) == -1
            assert fn(4, -1, var, 20, nodes, weights, *tail) == -2
            assert fn(4, 4, var, 20, nodes, weights, *tail) == -2
            assert fn(4, 0, None, 20, nodes, weights, *tail) == -3               # Gaussian without its variance
            assert fn(4, 0, arr(-1.0), 20, nodes, weights, *tail) == -3
            assert fn(4, 3, arr(1.0, 0.0, 0.0), 20, nodes, weights, *tail) == -3   # Student-t, df = 0
            assert fn(4, 1, None, 0, nodes, weights, *tail) == -4
            assert fn(4, 1, None, 33, nodes, weights, *tail) == -4
            assert fn(4, 1, None, 20, None, weights, *tail) == -5
            assert fn(4, 1, None, 20, nodes, None, *tail) == -6
            assert fn(4, 1, None, 20, nodes, arr(*([0.0] * 20)), *tail) == -6   # weights are positive
            assert fn(0, 1, None, 20, nodes, weights, *tail) == 0               # nothing to do: no launch
            assert fn(4, 1, None, 20, nodes, weights, *tail) == -7              # fmu
        assert site(4, 1, None, 20, nodes, weights, None, None, None, 1.5, None, None, None, None) == -10
        assert site(4, 1, None, 20, nodes, weights, None, None, None, float("nan"), None, None, None, None) == -10


def test_sites_accept_leading_batch_dimensions_and_keep_their_error_cases():
    z = torch.zeros
    sites = mfa.UnivariateGaussianSitesNat(torch.ones(3, 5, 1), -0.25 * torch.ones(3, 5, 1, 1), z(3, 5, 1))
    assert (sites.num_data, sites.output_dim) == (5, 1)
    assert tuple(sites.means.shape) == (3, 5, 1) and torch.allclose(sites.means, torch.full((3, 5, 1), 2.0))
    assert tuple(sites.precisions.shape) == (3, 5, 1, 1) and torch.allclose(sites.precisions, torch.full((3, 5, 1, 1), 0.5))
    assert tuple(sites.log_det_precisions.shape) == (3, 5, 1, 1)
    deep = mfa.UnivariateGaussianSitesNat(z(2, 3, 5, 1), -torch.ones(2, 3, 5, 1, 1))
    assert (deep.num_data, deep.output_dim) == (5, 1) and deep.log_norm is None
    flat = mfa.UnivariateGaussianSitesNat(z(6, 1), -torch.ones(6, 1, 1), z(6, 1))            # as before
    assert (flat.num_data, flat.output_dim) == (6, 1)
    for args in ((z(6, 2), z(6, 1, 1)), (z(6), z(6, 1, 1)), (z(6, 1), z(6, 1)), (z(6, 1), z(5, 1, 1)), (z(6, 1), z(6, 1, 2)),
                 (z(6, 1), z(6, 1, 1), z(6)), (z(6, 1), z(6, 1, 1), z(5, 1)), (z(3, 5, 1), z(5, 1, 1)), (z(3, 5, 1), z(3, 5, 1)),
                 (z(3, 5, 1), z(3, 5, 1, 1), z(5, 1))):
        with pytest.raises(ValueError, match="must have shape"):
            mfa.UnivariateGaussianSitesNat(*args)
    em = mfa.EmissionModel(z(3, 5, 2, 4))
    with pytest.raises(ValueError, match="not compatible"):
        mfa.KalmanFilterWithSites(None, em, sites)
