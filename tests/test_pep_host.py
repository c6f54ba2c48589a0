"""
CPU tests of power expectation propagation: the numpy reference of tests/helpers/pep_closed_forms.py against itself (second
derivatives against central differences, g1 and g2 against differences of I, the Gaussian closed form against the quadrature, the
scalar cavity against the reference's d x d route, the dense loop's fixed points), the torch routes of markovflow_amd/likelihoods.py
against it, and the argument checks of the model, the likelihood methods and the two ``mf_lik_*`` entry points (which return before
any launch).

Tolerances (float64, eps = 2^-52): the torch routes against the helper ``|err| <= K eps (magnitude + 1)`` with the helper's
magnitudes and K = 64, as tests/test_likelihoods_host.py.  Finite differences: stated at each test.
"""
import ctypes

import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from markovflow_amd import likelihoods as ML
from helpers import likelihood_closed_forms as L
from helpers import pep_closed_forms as P

EPS = 2.0 ** -52
K_HOST = 64.0
NAMES = [L.GAUSSIAN, L.BERNOULLI, L.POISSON, L.STUDENTT]
ALPHAS = [1.0, 0.5]
M32 = [dict(order=3, ls=1.0, var=1.0, period=None, osc=0)]


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


def within(what, got, want, mag, k=K_HOST):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.all(np.isfinite(got)), f"{what}: non-finite result"
    ratio = np.abs(got - want) / (EPS * (np.asarray(mag) + 1.0))
    assert ratio.max() <= k, f"{what}: largest error {ratio.max():.1f} eps (magnitude + 1) at point {int(ratio.argmax())}"


def site_inputs(name, alpha, seed=0):
    """The grid as posterior marginals with sites whose cavity exists and whose den is at least 0.1 (found with the helper)."""
    spec = L.LIKELIHOODS[name]
    m, s, y = L.value_grid(name)
    rng = np.random.default_rng(seed)
    nat1 = 0.3 * rng.normal(size=m.size) / np.sqrt(s)
    log_norm = rng.normal(size=m.size)
    nat2 = np.full(m.size, np.nan)
    for c in (-0.3, 0.5, 3.0, 30.0, 300.0, 3000.0):       # 1 / v_c = (1 + c) / s: a tighter cavity brings den towards 1
        trial = np.where(np.isnan(nat2), c / (2 * alpha * s), nat2)
        r = P.pep_site_update(spec, m, s, y, alpha, 1.0, nat1, trial, log_norm)
        nat2 = np.where(np.isnan(nat2) & (r["den"] >= 0.1) & ~r["skipped"], trial, nat2)
    assert not np.isnan(nat2).any(), "no site with den >= 0.1 found for some grid point"
    return m, s, y, nat1, nat2, log_norm


@pytest.mark.parametrize("name", NAMES)
def test_second_derivative_against_central_differences_of_the_first(name):
    """h = 1e-5 on f in [-3, 3]: truncation h^2 / 6 |l''''| ~ 1e-10 x (a fourth derivative, at most e^3 y-scale ~ 50), rounding
    eps |l'| / h ~ 1e-9 for |l'| up to 40: 1e-7 relative to (|l''| + 1)."""
    spec = L.LIKELIHOODS[name]
    f, _, y = L.value_grid(name)
    h = 1e-5
    fd = (L.dlog_prob(spec, f + h, y) - L.dlog_prob(spec, f - h, y)) / (2 * h)
    got = P.d2log_prob(spec, f, y)
    assert np.all(np.abs(got - fd) <= 1e-7 * (np.abs(got) + 1.0))
    assert np.all(P.d2log_prob_terms(spec, f, y) >= np.abs(got) * (1 - 1e-12))


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name", NAMES)
def test_helper_derivatives_against_finite_differences_of_the_helper_value(name, alpha):
    """g1 and g2 are the derivatives of the DISCRETISED I in mu, so differences of I check them whatever the rule's accuracy.
    Variances 1e-2 ... 1e2 (at 1e-6 the third derivative of the Student-t sum is too large for one h).  h = 1e-4: truncation
    h^2 x (third / fourth derivative, bounded by a few hundred on this grid), rounding 4 eps (|I| + mag) / h^2 ~ 1e-5 for the second
    difference at |I| ~ 1000 (Poisson, y = 40) and 1e-7 at |I| < 50: relative 1e-3 of (|g2| + 1) at |I| < 50, and points beyond that are left to the
    first derivative."""
    spec = L.LIKELIHOODS[name]
    mu, var, y = L.value_grid(name, variances=(1e-2, 1.0, 1e2))
    h = 1e-4
    (i0, g1, g2), _ = P.log_expected_density(spec, mu, var, y, alpha)
    ip = P.log_expected_density(spec, mu + h, var, y, alpha)[0][0]
    im = P.log_expected_density(spec, mu - h, var, y, alpha)[0][0]
    np.testing.assert_array_less(np.abs((ip - im) / (2 * h) - g1), 1e-5 * (np.abs(g1) + np.abs(i0) + 1.0))
    small = np.abs(i0) < 50.0
    assert small.sum() > mu.size // 2
    np.testing.assert_array_less(np.abs((ip - 2 * i0 + im) / (h * h) - g2)[small], 1e-3 * (np.abs(g2) + 1.0)[small])


@pytest.mark.parametrize("alpha", ALPHAS)
def test_gaussian_closed_form_against_the_quadrature_at_32_nodes(alpha):
    """p^alpha N is a Gaussian integrand: the 32-point rule integrates it to rounding where the integrand's width is within the
    rule's reach of the likelihood's, sqrt(2 var) x_32 ~ 10 sqrt(var) against sqrt(0.7 / alpha): variances up to 1."""
    spec = L.LIKELIHOODS[L.GAUSSIAN]
    mu, var, y = L.value_grid(L.GAUSSIAN, variances=(1e-6, 1e-2, 1.0))
    closed, _ = P.log_expected_density(spec, mu, var, y, alpha)
    x, w = np.polynomial.hermite.hermgauss(32)
    f = mu[:, None] + np.sqrt(2 * var)[:, None] * x
    vals = alpha * L.log_prob(spec, f, y[:, None]) + np.log(w / np.sqrt(np.pi))
    from scipy import special
    led = special.logsumexp(vals, axis=-1)
    p = np.exp(vals - led[:, None])
    a = alpha * L.dlog_prob(spec, f, y[:, None])
    g1 = np.sum(p * a, -1)
    g2 = np.sum(p * (alpha * P.d2log_prob(spec, f, y[:, None]) + a * a), -1) - g1 * g1
    np.testing.assert_allclose(closed[0], led, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(closed[1], g1, rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(closed[2], g2, rtol=1e-7, atol=1e-7)


@pytest.mark.parametrize("nq", [1, 20, 32])
@pytest.mark.parametrize("name", NAMES)
def test_alpha_one_is_the_predictive_log_density(name, nq):
    spec = L.LIKELIHOODS[name]
    mu, var, y = L.value_grid(name)
    (led, _, _), (mag, _, _) = P.log_expected_density(spec, mu, var, y, 1.0, nq)
    within(f"{name} nq={nq}", led, L.predict_log_density(spec, mu, var, y, nq), mag, k=8.0)


def test_the_unshifted_sum_underflows_where_the_helper_is_finite():
    """Poisson at y = 0, mu = 8, var = 1e-2: every term exp(alpha l_i) w_i is below the smallest double."""
    spec = L.LIKELIHOODS[L.POISSON]
    one = lambda v: np.array([v])                                                               # noqa: E731
    x, w = np.polynomial.hermite.hermgauss(20)
    naive = np.sum(np.exp(L.log_prob(spec, 8.0 + np.sqrt(2e-2) * x, 0.0)) * w / np.sqrt(np.pi))
    assert naive == 0.0
    (led, g1, g2), _ = P.log_expected_density(spec, one(8.0), one(1e-2), one(0.0), 1.0)
    assert np.isfinite(led[0]) and abs(led[0] + 1421.145) < 1e-2 and np.isfinite(g1[0]) and np.isfinite(g2[0])
    (half, _, _), _ = P.log_expected_density(spec, one(8.0), one(1e-2), one(0.0), 0.5)
    assert abs(half[0] + 725.42) < 1e-2


@pytest.mark.parametrize("d", [1, 3, 6])
def test_scalar_cavity_is_the_d_by_d_route(d):
    """Sherman-Morrison: removing alpha x (a site in f = h . s) from a d-dimensional Gaussian and projecting by h is the scalar
    cavity on the marginal of f.  Random SPD covariances with condition numbers of a few hundred: 1e-10 relative."""
    rng = np.random.default_rng(d)
    for trial in range(20):
        a = rng.normal(size=(d, d))
        cov = a @ a.T + 0.1 * np.eye(d)
        mean, h = rng.normal(size=d), rng.normal(size=d)
        alpha = (1.0, 0.5, 0.25)[trial % 3]
        s = h @ cov @ h
        nat1 = rng.normal()
        nat2 = rng.uniform(-0.45, 2.0) / (alpha * s)           # 1 / s + 2 alpha nat2 > 0
        want = P.cavity_dxd(mean, cov, h, nat1, nat2, alpha)
        mc, vc, exists, _ = P.cavity(np.array([h @ mean]), np.array([s]), np.array([nat1]), np.array([nat2]), alpha)
        assert exists[0]
        np.testing.assert_allclose([mc[0], vc[0]], want, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("nq", [1, 20, 32])
@pytest.mark.parametrize("name", NAMES)
def test_torch_log_expected_density_matches_the_helper(name, nq, alpha):
    spec = L.LIKELIHOODS[name]
    mu, var, y = L.value_grid(name)
    lik = make(name, nq)
    want, mags = P.log_expected_density(spec, mu, var, y, alpha, nq)
    got = ML.torch_log_expected_density(lik, col(mu), col(var), col(y), alpha)
    for i, what in enumerate(("I", "g1", "g2")):
        within(f"{name} nq={nq} alpha={alpha} {what}", got[i].numpy()[:, 0], want[i], mags[i])
    value = lik.log_expected_density(col(mu), col(var), col(y), alpha)
    assert tuple(value.shape) == (mu.size,) and torch.equal(value, got[0][:, 0])
    obj, (g1, g2) = lik.grad_log_expected_density(col(mu), col(var), col(y), alpha)
    assert tuple(obj.shape) == (mu.size,) and tuple(g1.shape) == tuple(g2.shape) == (mu.size, 1)
    assert torch.equal(obj, got[0][:, 0]) and torch.equal(g1, got[1]) and torch.equal(g2, got[2])
    bad = col(var).clone()
    bad[3] = 0.0
    out = ML.torch_log_expected_density(lik, col(mu), bad, col(y), alpha)
    assert all(bool(torch.isnan(o[3])) and bool(torch.isfinite(o[4])) for o in out)


@pytest.mark.parametrize("lr", [1.0, 0.3])
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name", NAMES)
def test_torch_pep_site_update_matches_the_helper(name, alpha, lr):
    spec = L.LIKELIHOODS[name]
    m, s, y, nat1, nat2, log_norm = site_inputs(name, alpha)
    lik = make(name)
    t1, t2, tn = col(nat1), col(nat2)[..., None], col(log_norm)
    cav = ML.torch_pep_site_update(lik, col(m), col(s), col(y), alpha, lr, t1, t2, tn)
    own = P.pep_site_update(spec, m, s, y, alpha, lr, nat1, nat2, log_norm)
    assert not own["skipped"].any()
    within(f"{name} cav_mu", cav[0].numpy()[:, 0], own["cav_mu"], own["cav_mags"][0])
    within(f"{name} cav_var", cav[1].numpy()[:, 0], own["cav_var"], own["cav_mags"][1])
    want = P.pep_site_update(spec, m, s, y, alpha, lr, nat1, nat2, log_norm, at_cavity=(cav[0].numpy()[:, 0], cav[1].numpy()[:, 0]))
    for got, key, mag in zip((t1, t2, tn), ("nat1", "nat2", "log_norm"), want["mags"]):
        within(f"{name} alpha={alpha} lr={lr} {key}", got.numpy().reshape(-1), want[key], mag)
    # the method on CPU tensors is this route, in place, with the version counters moved
    u1, u2, un = col(nat1), col(nat2)[..., None], col(log_norm)
    versions = [t._version for t in (u1, u2, un)]
    lik.pep_site_update(col(m), col(s), col(y), alpha, lr, u1, u2, un)
    assert torch.equal(u1, t1) and torch.equal(u2, t2) and torch.equal(un, tn)
    assert all(t._version > v for t, v in zip((u1, u2, un), versions))


def test_torch_pep_site_update_skips_what_the_issue_says_it_skips():
    spec = L.LIKELIHOODS[L.BERNOULLI]
    m, s, y, nat1, nat2, log_norm = (a[:16].copy() for a in site_inputs(L.BERNOULLI, 0.5))
    nat2[1] = -1.0 / s[1]                         # 1 / s + 2 alpha n2 = 0
    s[2] = 0.0
    s[3] = -1.0
    m[4] = np.nan
    nat1[5] = np.nan
    update = np.ones(16, dtype=bool)
    update[7] = False
    skipped = [1, 2, 3, 4, 5, 7]
    t1, t2, tn = col(nat1), col(nat2), col(log_norm)
    before = [t.clone() for t in (t1, t2, tn)]
    make(L.BERNOULLI).pep_site_update(col(m), col(s), col(y), 0.5, 0.3, t1, t2, tn, update=torch.tensor(update).reshape(-1, 1))
    own = P.pep_site_update(spec, m, s, y, 0.5, 0.3, nat1, nat2, log_norm, update=update)
    assert sorted(np.flatnonzero(own["skipped"])) == skipped
    for t, b in zip((t1, t2, tn), before):
        same = (t.view(torch.int64) == b.view(torch.int64))[:, 0].numpy()
        assert same[skipped].all() and not same[[0, 6, 8, 15]].any()


@pytest.mark.parametrize("alpha", ALPHAS)
def test_dense_loop_with_a_gaussian_likelihood_reaches_the_exact_answers(alpha):
    """alpha = 1, lr = 1: one update gives the exact sites and the energy is the log marginal likelihood.  alpha = 0.5, lr = 1:
    nat1 = (1 - 0.5^k) y / variance after k updates, and the energy converges to the log marginal likelihood."""
    spec = L.LIKELIHOODS[L.GAUSSIAN]
    var = spec[1][0]
    t, y = L.draw_series(spec, M32, 33, seed=0, separated=True)
    exact = L.PC.dense_log_marginal(M32, t, y, var)
    if alpha == 1.0:
        rec = P.dense_pep(spec, M32, t, y, 1.0, 1.0, 1, record=(1,))
        np.testing.assert_allclose(rec[1]["nat1"], y / var, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(rec[1]["nat2"], np.full(33, -0.5 / var), rtol=1e-12)
        assert rec[1]["energy"] == pytest.approx(exact, rel=1e-12)
    else:
        rec = P.dense_pep(spec, M32, t, y, 0.5, 1.0, 60, record=(3, 60))
        np.testing.assert_allclose(rec[3]["nat1"], (1 - 0.5 ** 3) * y / var, rtol=1e-12, atol=1e-13)
        assert rec[60]["energy"] == pytest.approx(exact, rel=1e-12)


def test_argument_checks_of_the_likelihood_methods_and_of_the_model():
    lik = mfa.Bernoulli()
    z = torch.zeros(4, 1, dtype=torch.float64)
    one = z + 1
    for alpha in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            lik.log_expected_density(z, one, z, alpha)
        with pytest.raises(ValueError, match="alpha"):
            lik.grad_log_expected_density(z, one, z, alpha)
        with pytest.raises(ValueError, match="alpha"):
            lik.pep_site_update(z, one, z, alpha, 0.5, z.clone(), z.clone(), z.clone())
        with pytest.raises(ValueError, match="alpha"):
            mfa.PowerExpectationPropagation((torch.arange(4.0, dtype=torch.float64), z), mfa.Matern32(1.0, 1.0, device="cpu"), lik,
                                            alpha=alpha)
    for lr in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="learning_rate"):
            lik.pep_site_update(z, one, z, 0.5, lr, z.clone(), z.clone(), z.clone())
    with pytest.raises(ValueError, match="batch \\+ \\[N, 1\\]"):
        lik.log_expected_density(z[:, 0], one[:, 0], z[:, 0])
    with pytest.raises(ValueError, match="fvar has shape"):
        lik.log_expected_density(z, one[:3], z)
    with pytest.raises(ValueError, match="y is torch.float32"):
        lik.grad_log_expected_density(z, one, z.float())
    with pytest.raises(TypeError, match="float32 and float64"):
        lik.log_expected_density(z.long(), one.long(), z.long())
    with pytest.raises(ValueError, match="one element per data point"):
        lik.pep_site_update(z, one, z, 0.5, 0.5, z.clone(), torch.zeros(3, 1, dtype=torch.float64), z.clone())
    with pytest.raises(ValueError, match="log_norm is torch.float32"):
        lik.pep_site_update(z, one, z, 0.5, 0.5, z.clone(), z.clone(), z.clone().float())
    with pytest.raises(ValueError, match="update must be"):
        lik.pep_site_update(z, one, z, 0.5, 0.5, z.clone(), z.clone(), z.clone(), update=torch.ones(4, 1))
    with pytest.raises(ValueError, match="update must be"):
        lik.pep_site_update(z, one, z, 0.5, 0.5, z.clone(), z.clone(), z.clone(), update=torch.ones(3, 1, dtype=torch.bool))
    times = torch.arange(4.0, dtype=torch.float64)
    kern = mfa.Matern32(1.0, 1.0, device="cpu")
    with pytest.raises(ValueError, match="observations must have shape"):
        mfa.PowerExpectationPropagation((times, z[:, 0]), kern, lik)
    with pytest.raises(ValueError, match="time_points must have shape"):
        mfa.PowerExpectationPropagation((times[:3], z), kern, lik)
    with pytest.raises(TypeError, match="Likelihood"):
        mfa.PowerExpectationPropagation((times, z), kern, "bernoulli")
    with pytest.raises(ValueError, match="learning_rate"):
        mfa.PowerExpectationPropagation((times, z), kern, lik, learning_rate=2.0)
    model = mfa.PowerExpectationPropagation((times, z), kern, lik)
    assert model.learning_rate == 1.0 and model.alpha == 1.0 and mfa.models.PowerExpectationPropagation is type(model)
    assert float(model.sites.nat2.max()) == -1e-10 and float(model.sites.log_norm.abs().max()) == 0.0
    with pytest.raises(ValueError, match="1-D integer"):
        model.update_sites(site_indices=torch.tensor([[0]]))
    with pytest.raises(ValueError, match="1-D integer"):
        model.update_sites(site_indices=torch.tensor([0.0]))
    for bad in ([4], [0, 7], [-5], [1, -9]):                 # four data points: -4 <= i < 4, rejected before anything runs
        with pytest.raises(IndexError, match=r"\[-4, 4\)"):
            model.update_sites(site_indices=torch.tensor(bad))
    assert model._update_flags(torch.tensor([0, 3, 3, -3])).tolist() == [1, 1, 0, 1]
    assert model._update_flags(torch.tensor([], dtype=torch.long)).tolist() == [0, 0, 0, 0]
    pair = mfa.PowerExpectationPropagation((torch.stack([times, times]), torch.stack([z, z])), kern, lik)
    assert pair._update_flags(torch.tensor([2], dtype=torch.int32)).tolist() == [[0, 0, 1, 0]] * 2
    t64 = lambda v: torch.tensor(v, dtype=torch.float64)                                          # noqa: E731
    l1, l2 = mfa.models.gradient_correction((t64(0.5), t64(2.0)), (t64(0.3), t64(-0.2)))
    want2 = 0.5 / (2.0 + 1.0 / -0.2)
    assert float(l2) == pytest.approx(want2, rel=1e-14) and float(l1) == pytest.approx(2 * want2 * (0.3 / -0.2 - 0.5), rel=1e-14)


def test_entry_points_return_codes_without_touching_the_gpu():
    """Every argument check of the two entry points returns before a launch: the negative position of the argument."""
    lib = _lib.load()
    arr = lambda *v: (ctypes.c_double * len(v))(*v)       # noqa: E731
    x, w = np.polynomial.hermite.hermgauss(20)
    nodes, weights, var = arr(*x), arr(*w), arr(0.5)
    one = ctypes.c_void_p(8)                               # a non-NULL pointer that is never dereferenced: the checks return first
    for suf in ("_f64", "_f32"):
        led = getattr(lib, "mf_lik_log_expected_density" + suf)
        pep = getattr(lib, "mf_lik_pep_site_update" + suf)
        tail_led = lambda alpha=1.0: (alpha,) + (None,) * 7                                     # noqa: E731
        tail_pep = lambda alpha=1.0, lr=1.0: (alpha, lr) + (None,) * 10                         # noqa: E731
        for fn, tail in ((led, tail_led), (pep, tail_pep)):
            assert fn(-1, 0, var, 20, nodes, weights, *tail()) == -1
            assert fn(4, -1, var, 20, nodes, weights, *tail()) == -2
            assert fn(4, 4, var, 20, nodes, weights, *tail()) == -2
            assert fn(4, 0, None, 20, nodes, weights, *tail()) == -3
            assert fn(4, 3, arr(1.0, 0.0, 0.0), 20, nodes, weights, *tail()) == -3
            assert fn(4, 1, None, 0, nodes, weights, *tail()) == -4
            assert fn(4, 1, None, 33, nodes, weights, *tail()) == -4
            assert fn(4, 1, None, 20, None, weights, *tail()) == -5
            assert fn(4, 1, None, 20, nodes, None, *tail()) == -6
            for alpha in (0.0, -1.0, 1.5, float("nan")):
                assert fn(4, 1, None, 20, nodes, weights, *tail(alpha)) == -7
            assert fn(0, 1, None, 20, nodes, weights, *tail()) == 0               # nothing to do: no launch
        assert led(4, 1, None, 20, nodes, weights, 1.0, None, one, one, None, None, None, None) == -8
        assert led(4, 1, None, 20, nodes, weights, 1.0, one, None, one, None, None, None, None) == -9
        assert led(4, 1, None, 20, nodes, weights, 1.0, one, one, None, None, None, None, None) == -10
        assert led(4, 1, None, 20, nodes, weights, 1.0, one, one, one, None, None, None, None) == 0      # nothing asked for
        for lr in (-0.5, 1.5, float("nan")):
            assert pep(4, 1, None, 20, nodes, weights, *tail_pep(0.5, lr)) == -8
        assert pep(0, 1, None, 20, nodes, weights, *tail_pep(0.5, 2.0)) == -8       # checked before the empty input returns
        ptrs = [one] * 3 + [None] + [one] * 3 + [None, None]                        # fmu fvar y update nat1 nat2 log_norm cav cav
        for pos, code in ((0, -9), (1, -10), (2, -11), (4, -13), (5, -14), (6, -15)):
            args = list(ptrs)
            args[pos] = None
            assert pep(4, 1, None, 20, nodes, weights, 0.5, 0.5, *args, None) == code
