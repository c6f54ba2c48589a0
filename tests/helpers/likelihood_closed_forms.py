"""
numpy / scipy (fp64) reference of the likelihoods and of the CVI iteration - TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Independent of markovflow_amd/likelihoods.py and csrc/mf_lik.hip: the log densities come from scipy.stats / scipy.special, the
quadrature is written once for any callable, and the CVI loop is dense linear algebra on the kernel matrix
(tests/helpers/periodic_closed_forms.py: ``dense_kernel``) - no state space form anywhere.

A likelihood is a tuple ``(name, params)``: ``("gaussian", (variance,))``, ``("bernoulli", ())``, ``("poisson", ())``,
``("studentt", (scale, df))``.  ``dtype`` = numpy.float32 evaluates the same formulas in float32 (the yardstick of the fp32 kernels).
"""
import numpy as np
from scipy import special, stats

from helpers import periodic_closed_forms as PC

GAUSSIAN, BERNOULLI, POISSON, STUDENTT = "gaussian", "bernoulli", "poisson", "studentt"
IDS = {GAUSSIAN: 0, BERNOULLI: 1, POISSON: 2, STUDENTT: 3}
JITTER = 1e-3     # gpflow's inv_probit


def inv_probit(f):
    f = np.asarray(f)
    one = f.dtype.type(1)
    return f.dtype.type(0.5) * (one + special.erf(f / np.sqrt(f.dtype.type(2)))) * f.dtype.type(1 - 2 * JITTER) + f.dtype.type(JITTER)


def log_prob(lik, f, y):
    """log p(y | f), element-wise, in the dtype of f."""
    name, params = lik
    f = np.asarray(f)
    y = np.asarray(y, dtype=f.dtype)
    ty = f.dtype.type
    if name == GAUSSIAN:
        if f.dtype == np.float64:
            return stats.norm.logpdf(y, loc=f, scale=np.sqrt(params[0]))
        v = ty(params[0])
        return ty(-0.5) * (np.log(ty(2 * np.pi)) + np.log(v)) - ty(0.5) * (y - f) ** 2 / v
    if name == BERNOULLI:
        p = inv_probit(f)
        return y * np.log(p) + (ty(1) - y) * np.log1p(-p)
    if name == POISSON:
        if f.dtype == np.float64:
            return stats.poisson.logpmf(y, np.exp(f))
        return y * f - np.exp(f) - special.gammaln(y + ty(1)).astype(f.dtype)
    scale, df = params
    if f.dtype == np.float64:
        return stats.t.logpdf(y, df, loc=f, scale=scale)
    const = ty(special.gammaln(0.5 * (df + 1)) - special.gammaln(0.5 * df) - 0.5 * np.log(df * np.pi) - np.log(scale))
    return const - ty(0.5 * (df + 1)) * np.log1p((y - f) ** 2 / ty(df * scale * scale))


def dlog_prob(lik, f, y):
    """d log p(y | f) / df."""
    name, params = lik
    f = np.asarray(f)
    y = np.asarray(y, dtype=f.dtype)
    ty = f.dtype.type
    if name == GAUSSIAN:
        return (y - f) / ty(params[0])
    if name == BERNOULLI:
        p = inv_probit(f)
        dp = ty(1 - 2 * JITTER) * np.exp(ty(-0.5) * f * f) / np.sqrt(ty(2 * np.pi))
        return dp * (y / p - (ty(1) - y) / (ty(1) - p))
    if name == POISSON:
        return y - np.exp(f)
    scale, df = params
    r = y - f
    return ty(df + 1) * r / (ty(df * scale * scale) + r * r)


def rule(nq, dtype=np.float64):
    """Gauss-Hermite nodes and weights / sqrt(pi) (computed in float64, then cast)."""
    x, w = np.polynomial.hermite.hermgauss(nq)
    return x.astype(dtype), (w / np.sqrt(np.pi)).astype(dtype)


def quadrature(lik, mu, var, y, nq=20, dtype=np.float64):
    """The discretised expectation and its exact derivatives:  VE = sum w_i l(f_i),  dVE/dmu = sum w_i l'(f_i),
    dVE/dvar = sum w_i l'(f_i) x_i / sqrt(2 var)  with f_i = mu + sqrt(2 var) x_i.  Returns ``(ve, g_mu, g_var)`` and the
    magnitudes that scale a rounding-error bound (always float64), the sums of the absolute terms:  sum w_i |l(f_i)|,
    sum w_i |l'(f_i)|  and  sum w_i |l'(f_i)| |x_i| / sqrt(2 var)."""
    mu, var, y = (np.asarray(a, dtype=dtype) for a in (mu, var, y))
    x, w = rule(nq, dtype)
    sd = np.sqrt(dtype(2) * var)
    f = mu[..., None] + sd[..., None] * x
    l, dl = log_prob(lik, f, y[..., None]), dlog_prob(lik, f, y[..., None])
    vals = (np.sum(w * l, -1), np.sum(w * dl, -1), np.sum(w * dl * x, -1) / sd)
    f8, y8, x8, w8 = f.astype(np.float64), y.astype(np.float64)[..., None], x.astype(np.float64), w.astype(np.float64)
    l8, dl8 = np.abs(log_prob(lik, f8, y8)), np.abs(dlog_prob(lik, f8, y8))
    mags = (np.sum(w8 * l8, -1), np.sum(w8 * dl8, -1), np.sum(w8 * dl8 * np.abs(x8), -1) / sd.astype(np.float64))
    return tuple(v.astype(dtype) for v in vals), mags


def closed_form(lik, mu, var, y, dtype=np.float64):
    """(VE, dVE/dmu, dVE/dvar) of the Gaussian and Poisson likelihoods in closed form."""
    name, params = lik
    mu, var, y = (np.asarray(a, dtype=dtype) for a in (mu, var, y))
    if name == GAUSSIAN:
        v = dtype(params[0])
        ve = dtype(-0.5) * np.log(dtype(2 * np.pi) * v) - dtype(0.5) * ((y - mu) ** 2 + var) / v
        return ve, (y - mu) / v, np.full_like(mu, dtype(-0.5) / v)
    assert name == POISSON
    e = np.exp(mu + dtype(0.5) * var)
    return y * mu - e - special.gammaln(y + dtype(1)).astype(dtype), y - e, dtype(-0.5) * e


def expectations(lik, mu, var, y, nq=20, dtype=np.float64):
    """What the library computes: closed forms for Gaussian / Poisson, the quadrature for Bernoulli / Student-t.  Returns
    ``(values, magnitudes)`` as ``quadrature`` does (closed forms: the magnitudes of the terms of each expression)."""
    if lik[0] in (GAUSSIAN, POISSON):
        vals = closed_form(lik, mu, var, y, dtype)
        mu_, var_, y_ = (np.asarray(a, dtype=np.float64) for a in (mu, var, y))
        if lik[0] == GAUSSIAN:
            v = lik[1][0]
            mags = (0.5 * abs(np.log(2 * np.pi * v)) + 0.5 * ((y_ - mu_) ** 2 + var_) / v, np.abs(y_ - mu_) / v, np.full_like(mu_, 0.5 / v))
        else:
            e = np.exp(mu_ + 0.5 * var_)
            mags = (np.abs(y_ * mu_) + e + special.gammaln(y_ + 1), y_ + e, 0.5 * e)
        return vals, mags
    return quadrature(lik, mu, var, y, nq, dtype)


def predict_log_density(lik, mu, var, y, nq=20, dtype=np.float64):
    """log int p(y | f) N(f | mu, var) df: Gaussian in closed form, the others by log-sum-exp over the nodes."""
    mu, var, y = (np.asarray(a, dtype=dtype) for a in (mu, var, y))
    if lik[0] == GAUSSIAN:
        tot = var + dtype(lik[1][0])
        return (dtype(-0.5) * np.log(dtype(2 * np.pi) * tot) - dtype(0.5) * (y - mu) ** 2 / tot).astype(dtype)
    x, w = np.polynomial.hermite.hermgauss(nq)
    logw = np.log(w / np.sqrt(np.pi)).astype(dtype)
    f = mu[..., None] + np.sqrt(dtype(2) * var)[..., None] * x.astype(dtype)
    return special.logsumexp(log_prob(lik, f, y[..., None]) + logw, axis=-1).astype(dtype)


def conditional_mean_var(lik, f):
    """E[y | f] and Var[y | f]."""
    name, params = lik
    if name == GAUSSIAN:
        return f, np.full_like(f, params[0])
    if name == BERNOULLI:
        p = inv_probit(f)
        return p, p - p * p
    if name == POISSON:
        return np.exp(f), np.exp(f)
    scale, df = params
    return f, np.full_like(f, scale * scale * df / (df - 2.0))


def predict_mean_and_var(lik, mu, var, nq=100):
    """Mean and variance of y under f ~ N(mu, var) by an nq-point quadrature (law of total variance)."""
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    x, w = rule(nq)
    m, v = conditional_mean_var(lik, mu[..., None] + np.sqrt(2 * var)[..., None] * x)
    mean = np.sum(w * m, -1)
    return mean, np.sum(w * (v + m * m), -1) - mean * mean


# ---- the dense CVI iteration -----------------------------------------------------------------------------------------------------
def dense_posterior(kmat, nat1, nat2):
    """Sigma = (K^-1 + diag(-2 nat2))^-1, mu = Sigma nat1."""
    sigma = np.linalg.inv(np.linalg.inv(kmat) + np.diag(-2.0 * nat2))
    sigma = 0.5 * (sigma + sigma.T)
    return sigma @ nat1, sigma


def dense_classic_elbo(lik, kmat, nat1, nat2, y, nq=20):
    """sum_i E_q log p(y_i | f_i) - KL[N(mu, Sigma) || N(0, K)]."""
    mu, sigma = dense_posterior(kmat, nat1, nat2)
    (ve, _, _), _ = expectations(lik, mu, np.diag(sigma), y, nq)
    n = len(y)
    kl = 0.5 * (np.trace(np.linalg.solve(kmat, sigma)) + mu @ np.linalg.solve(kmat, mu) - n
                + np.linalg.slogdet(kmat)[1] - np.linalg.slogdet(sigma)[1])
    return np.sum(ve) - kl


def dense_sites_log_marginal(kmat, nat1, nat2):
    """log N(m | 0, K + diag(1 / precision)) with the sites' means m = -nat1 / (2 nat2) and precisions -2 nat2: the marginal
    likelihood of the model whose likelihood terms are the Gaussian sites."""
    prec = -2.0 * nat2
    m = nat1 / prec
    kn = kmat + np.diag(1.0 / prec)
    return -0.5 * m @ np.linalg.solve(kn, m) - 0.5 * np.linalg.slogdet(kn)[1] - 0.5 * len(m) * np.log(2 * np.pi)


def dense_cvi(lik, comps, t, y, lr, iterations, nq=20, jitter=0.0, record=()):
    """The CVI loop on one series with dense matrices.  Sites start at nat1 = 0, nat2 = -1e-10 (variational_cvi.py:98-103); every
    iteration takes the marginals of q, the gradients of the expectations in [mu, var + mu^2] and steps
    nat <- (1 - lr) nat + lr g.  Returns ``{iteration: dict(nat1, nat2, classic_elbo, elbo)}`` for the iterations in ``record``
    (1-based, state AFTER that update) and the final ``(nat1, nat2)``."""
    kmat = PC.dense_kernel(comps, t[:, None] - t[None, :]) + jitter * np.eye(len(t))
    nat1, nat2 = np.zeros(len(t)), np.full(len(t), -1e-10)
    out = {}
    for it in range(1, iterations + 1):
        mu, sigma = dense_posterior(kmat, nat1, nat2)
        (_, g_mu, g_var), _ = expectations(lik, mu, np.diag(sigma), y, nq)
        nat1 = (1 - lr) * nat1 + lr * (g_mu - 2.0 * g_var * mu)
        nat2 = (1 - lr) * nat2 + lr * g_var
        if it in record:
            out[it] = dict(nat1=nat1.copy(), nat2=nat2.copy(), classic_elbo=dense_classic_elbo(lik, kmat, nat1, nat2, y, nq),
                           elbo=dense_sites_log_marginal(kmat, nat1, nat2))
    return out, (nat1, nat2)


def dense_predict(comps, t, nat1, nat2, t_new, jitter=0.0):
    """Mean and variance of f at t_new under q: the GP conditioned on pseudo-observations m with noise 1 / precision."""
    prec = -2.0 * nat2
    kn = PC.dense_kernel(comps, t[:, None] - t[None, :]) + jitter * np.eye(len(t)) + np.diag(1.0 / prec)
    ks = PC.dense_kernel(comps, t_new[:, None] - t[None, :])
    mean = ks @ np.linalg.solve(kn, nat1 / prec)
    var = PC.dense_kernel(comps, np.zeros(len(t_new))) + jitter - np.einsum("ij,ji->i", ks, np.linalg.solve(kn, ks.T))
    return mean, var


def predict_log_density_magnitude(lik, mu, var, y, nq=20):
    """What scales the rounding error of the log-sum-exp: the softmax-weighted mean of |l(f_i) + log w_i| (float64)."""
    mu, var, y = (np.asarray(a, dtype=np.float64) for a in (mu, var, y))
    if lik[0] == GAUSSIAN:
        tot = var + lik[1][0]
        return 0.5 * np.abs(np.log(2 * np.pi * tot)) + 0.5 * (y - mu) ** 2 / tot
    x, w = np.polynomial.hermite.hermgauss(nq)
    v = log_prob(lik, mu[..., None] + np.sqrt(2 * var)[..., None] * x, y[..., None]) + np.log(w / np.sqrt(np.pi))
    return np.sum(special.softmax(v, axis=-1) * np.abs(v), axis=-1)


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------
LIKELIHOODS = {GAUSSIAN: (GAUSSIAN, (0.7,)), BERNOULLI: (BERNOULLI, ()), POISSON: (POISSON, ()), STUDENTT: (STUDENTT, (1.3, 3.5))}
VARIANCES = (1e-6, 1e-2, 1.0, 1e2)
OBSERVED = {GAUSSIAN: (-2.5, -0.3, 0.7, 4.0), STUDENTT: (-2.5, -0.3, 0.7, 4.0), BERNOULLI: (0.0, 1.0), POISSON: (0.0, 1.0, 5.0, 40.0)}


def value_grid(name, variances=VARIANCES):
    """(mu, var, y), flat float64 arrays: mu in [-3, 3] x the variances x the observations of this likelihood - 256 points with the
    four variances, about 1000 over the four likelihoods."""
    ys = OBSERVED[name]
    mus = np.linspace(-3.0, 3.0, 64 // len(ys))
    mu, var, y = np.meshgrid(mus, np.asarray(variances), np.asarray(ys), indexing="ij")
    return mu.ravel(), var.ravel(), y.ravel()


def draw_series(lik, comps, num_points, seed, span=6.0, separated=False):
    """Times uniform on [0, span] (sorted), f ~ N(0, K) and observations drawn from the likelihood given f.  ``separated``: one
    time per cell of an even grid instead, at least 0.4 span / num_points apart - uniform draws put two of 33 points within 1e-3
    of each other, where Q = P - A P A^T at jitter 0 and the inverse of the dense kernel matrix both lose seven digits."""
    rng = np.random.default_rng(seed)
    if separated:
        t = (np.arange(num_points) + 0.5 + rng.uniform(-0.3, 0.3, size=num_points)) * span / num_points
    else:
        t = np.sort(rng.uniform(0.0, span, size=num_points))
    kmat = PC.dense_kernel(comps, t[:, None] - t[None, :])
    f = np.linalg.cholesky(kmat + 1e-10 * np.eye(num_points)) @ rng.normal(size=num_points)
    if lik[0] == BERNOULLI:
        y = (rng.uniform(size=num_points) < inv_probit(f)).astype(np.float64)
    elif lik[0] == POISSON:
        y = rng.poisson(np.exp(f)).astype(np.float64)
    elif lik[0] == GAUSSIAN:
        y = f + np.sqrt(lik[1][0]) * rng.normal(size=num_points)
    else:
        y = f + lik[1][0] * rng.standard_t(lik[1][1], size=num_points)
    return t, y
