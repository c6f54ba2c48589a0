"""
Reference of the SVGP model and of the natural-gradient optimiser - TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Two things, both independent of markovflow_amd/models/ (sparse.py, segmented_ops.py), markovflow_amd/ssm_natgrad.py and csrc/mf_lik.hip:

  * ``segment_expectations``: the per-segment formulas of ``mf_lik_sparse_expectations_*`` for one series in numpy, on
    ``likelihood_closed_forms.expectations``, with the magnitudes that scale a rounding-error bound; ``segment_value_torch`` restates
    the VALUE in torch (float64, CPU) so that autograd can be asked for the adjoints;
  * ``DenseNatGrad``: the natural-gradient loop (markovflow/ssm_natgrad.py) on ONE series in float64 on the CPU with dense matrices:
    the chain's moments from the plain recursion, the joint covariance of the stacked states assembled from them, the KL divergence
    from dense matrices against ``sparse_cvi_closed_forms.dense_state_prior``, the ELBO's data term through
    ``sparse_cvi_closed_forms.conditional_projections``, and the four transforms restated on the dense mean / covariance / precision
    (torch autograd supplies the vector-Jacobian products).  No block-tridiagonal algebra.

A likelihood is the ``(name, params)`` tuple of likelihood_closed_forms.py; a kernel the list of component dicts of
periodic_closed_forms.py.
"""
import math

import numpy as np
import torch

from helpers import likelihood_closed_forms as L
from helpers import sparse_cvi_closed_forms as SC

TILE = 64           # points per tile of mf_lik_sparse_expectations_*: fixes the order of the sums


# ---- the kernel's formulas ---------------------------------------------------------------------------------------------------------
def segment_expectations(lik, w, c, y, offsets, pair_mean, pair_cov, nq=20, dtype=np.float64):
    """One series.  ``w [N, 2d]``, ``c [N]``, ``y [N]``, ``offsets [S + 1]``, ``pair_mean [S, 2d]``, ``pair_cov [S, 2d, 2d]``.  Per
    point k of segment s: fmu = w_k . m_s, fvar = c_k + w_k^T S_s w_k, (ve, gm, gv) the expectations; per segment ve_sum = sum ve,
    g_mean = sum gm w, g_cov = sum gv w w^T, each summed in the kernel's order (tiles of 64 points in ascending order, then the
    tiles).  ``dtype`` = numpy.float32 evaluates everything in float32.  Returns a dict with
    ``ve_sum [S]``, ``g_mean [S, 2d]``, ``g_cov [S, 2d, 2d]`` and the magnitudes (always float64) ``mag_ve_sum`` = the sum of the
    expectations' own magnitudes, ``mag_g_mean`` = sum |gm| |w_i|, ``mag_g_cov`` = sum |gv| |w_i| |w_j| (with the helper's magnitudes
    of the derivatives for |gm| and |gv|)."""
    ty = dtype
    w, c, y, pair_mean, pair_cov = (np.asarray(a, dtype=ty) for a in (w, c, y, pair_mean, pair_cov))
    n, segs, two_d = w.shape[0], len(offsets) - 1, w.shape[1]
    seg = np.repeat(np.arange(segs), np.diff(np.asarray(offsets)))
    assert seg.shape[0] == n and offsets[0] == 0 and offsets[-1] == n
    m, cov = pair_mean[seg], pair_cov[seg]
    # the projection in the kernel's order too: fmu and fvar grow term by term in i, the inner product with row i of S_s in j
    fmu, fvar = np.zeros(n, dtype=ty), c.copy()
    for i in range(two_d):
        row = np.zeros(n, dtype=ty)
        for j in range(two_d):
            row = row + cov[:, i, j] * w[:, j]
        fvar = fvar + w[:, i] * row
        fmu = fmu + w[:, i] * m[:, i]
    if n:
        (ve, gm, gv), mags = L.expectations(lik, fmu, fvar, y, nq, dtype=ty)
    else:
        ve = gm = gv = np.zeros(0, dtype=ty)
        mags = (np.zeros(0),) * 3
    w8 = np.abs(w.astype(np.float64))
    out = dict(ve_sum=np.zeros(segs, dtype=ty), g_mean=np.zeros((segs, two_d), dtype=ty), g_cov=np.zeros((segs, two_d, two_d), dtype=ty),
               mag_ve_sum=np.zeros(segs), mag_g_mean=np.zeros((segs, two_d)), mag_g_cov=np.zeros((segs, two_d, two_d)))
    in_order = lambda terms: np.cumsum(terms, axis=0, dtype=ty)[-1]          # noqa: E731  (numpy accumulates one after the other)
    for s in range(segs):
        # the kernel's order, so that ``dtype`` carries the kernel's rounding: a tile of 64 points is summed in ascending order on its
        # own, then the tiles' sums in ascending order
        tiles = [slice(k0, min(k0 + TILE, offsets[s + 1])) for k0 in range(offsets[s], offsets[s + 1], TILE)]
        if tiles:
            out["ve_sum"][s] = in_order(np.stack([in_order(ve[k]) for k in tiles]))
            out["g_mean"][s] = in_order(np.stack([in_order(gm[k, None] * w[k]) for k in tiles]))
            out["g_cov"][s] = in_order(np.stack([in_order((gv[k, None, None] * w[k][:, None, :]) * w[k][:, :, None]) for k in tiles]))
        k = slice(offsets[s], offsets[s + 1])
        out["mag_ve_sum"][s] = np.sum(mags[0][k])
        out["mag_g_mean"][s] = np.einsum("k,ki->i", mags[1][k], w8[k])
        out["mag_g_cov"][s] = np.einsum("k,ki,kj->ij", mags[2][k], w8[k], w8[k])
    return out


def _t(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64))


def log_prob_torch(lik, f, y):
    """``log p(y | f)`` of likelihood_closed_forms.log_prob in torch (float64)."""
    name, params = lik
    if name == L.GAUSSIAN:
        return -0.5 * math.log(2 * math.pi * params[0]) - 0.5 * (y - f) ** 2 / params[0]
    if name == L.BERNOULLI:
        p = 0.5 * (1.0 + torch.erf(f / math.sqrt(2.0))) * (1 - 2 * L.JITTER) + L.JITTER
        return y * torch.log(p) + (1.0 - y) * torch.log1p(-p)
    if name == L.POISSON:
        return y * f - torch.exp(f) - torch.lgamma(y + 1.0)
    scale, df = params
    const = math.lgamma(0.5 * (df + 1)) - math.lgamma(0.5 * df) - 0.5 * math.log(df * math.pi) - math.log(scale)
    return const - 0.5 * (df + 1) * torch.log1p((y - f) ** 2 / (df * scale * scale))


def expectations_torch(lik, mu, var, y, nq=20):
    """The value of likelihood_closed_forms.expectations in torch: closed forms for Gaussian / Poisson, the quadrature otherwise."""
    name, params = lik
    if name == L.GAUSSIAN:
        return -0.5 * math.log(2 * math.pi * params[0]) - 0.5 * ((y - mu) ** 2 + var) / params[0]
    if name == L.POISSON:
        return y * mu - torch.exp(mu + 0.5 * var) - torch.lgamma(y + 1.0)
    x, wq = (_t(a) for a in L.rule(nq))
    f = mu[..., None] + torch.sqrt(2.0 * var)[..., None] * x
    return torch.sum(wq * log_prob_torch(lik, f, y[..., None]), dim=-1)


def segment_value_torch(lik, w, c, y, offsets, pair_mean, pair_cov, nq=20):
    """``ve_sum [S]`` as a torch (float64, CPU) function of the tensors ``pair_mean`` and ``pair_cov``."""
    segs = len(offsets) - 1
    seg = torch.as_tensor(np.repeat(np.arange(segs), np.diff(np.asarray(offsets))))
    w, c, y = _t(w), _t(c), _t(y)
    fmu = torch.sum(w * pair_mean[seg], dim=-1)
    fvar = c + torch.einsum("ki,kij,kj->k", w, pair_cov[seg], w)
    ve = expectations_torch(lik, fmu, fvar, y, nq)
    return torch.zeros(segs, dtype=torch.float64).index_add(0, seg, ve)


# ---- the dense natural-gradient loop -----------------------------------------------------------------------------------------------
def dense_moments(mu0, chol_p0, a_s, b_s, chol_q):
    """Mean ``[M d]`` and covariance ``[M d, M d]`` of the stacked states from the plain recursion m_{k+1} = A_k m_k + b_k,
    P_{k+1} = A_k P_k A_k^T + Q_k, Cov(x_i, x_j) = A_{i-1} ... A_j P_j for i > j (torch, differentiable)."""
    m = a_s.shape[0] + 1
    means, covs = [mu0], [chol_p0 @ chol_p0.T]
    for k in range(m - 1):
        means.append(a_s[k] @ means[k] + b_s[k])
        covs.append(a_s[k] @ covs[k] @ a_s[k].T + chol_q[k] @ chol_q[k].T)
    rows = [[None] * m for _ in range(m)]
    for j in range(m):
        rows[j][j] = covs[j]
        for i in range(j + 1, m):
            rows[i][j] = a_s[i - 1] @ rows[i - 1][j]
            rows[j][i] = rows[i][j].T
    return torch.cat(means), torch.cat([torch.cat(r, dim=1) for r in rows], dim=0)


def _blocks(mu, sigma, d):
    """``(E x_i [M, d], Cov(x_i) [M, d, d], Cov(x_{i+1}, x_i) [M - 1, d, d])`` of a dense Gaussian."""
    m = mu.shape[0] // d
    lin = mu.reshape(m, d)
    diag = torch.stack([sigma[i * d:(i + 1) * d, i * d:(i + 1) * d] for i in range(m)])
    sub = torch.stack([sigma[(i + 1) * d:(i + 2) * d, i * d:(i + 1) * d] for i in range(m - 1)])
    return lin, diag, sub


def dense_to_expectations(mu, sigma, d):
    """``(eta_linear, eta_diag, eta_subdiag)``: E[x_i], E[x_i x_i^T], E[x_{i+1} x_i^T]."""
    lin, diag, sub = _blocks(mu, sigma, d)
    return lin, diag + lin[:, :, None] * lin[:, None, :], sub + lin[1:, :, None] * lin[:-1, None, :]


def expectations_to_params(eta_lin, eta_diag, eta_sub):
    """``(A_s, b_s, chol P_0, chol Q_s, mu_0)``: A_i = C_i S_i^-1, b_i = m_{i+1} - A_i m_i, Q_i = S_{i+1} - A_i S_i A_i^T with S the
    marginal covariances and C_i = Cov(x_{i+1}, x_i)."""
    covs = eta_diag - eta_lin[:, :, None] * eta_lin[:, None, :]
    covs = 0.5 * (covs + covs.transpose(-1, -2))
    cross = eta_sub - eta_lin[1:, :, None] * eta_lin[:-1, None, :]
    a_s = torch.linalg.solve(covs[:-1], cross.transpose(-1, -2)).transpose(-1, -2)
    b_s = eta_lin[1:] - torch.einsum("kij,kj->ki", a_s, eta_lin[:-1])
    q_s = covs[1:] - a_s @ covs[:-1] @ a_s.transpose(-1, -2)
    q_s = 0.5 * (q_s + q_s.transpose(-1, -2))
    return a_s, b_s, torch.linalg.cholesky(covs[0]), torch.linalg.cholesky(q_s), eta_lin[0]


def dense_to_naturals(mu, sigma, d):
    """``(theta_linear, theta_diag, theta_subdiag)`` of exp(theta^T x + x^T Theta x): K^-1 mu, the diagonal blocks of -1/2 K^-1 and
    the sub-diagonal blocks of -K^-1 (= Q_{i+1}^-1 A_{i+1}, the reference's convention)."""
    prec = torch.linalg.inv(sigma)
    prec = 0.5 * (prec + prec.T)
    lin, diag, sub = _blocks(prec @ mu, prec, d)
    return lin, -0.5 * diag, -sub


def naturals_to_dense(theta_lin, theta_diag, theta_sub):
    """Mean and covariance of the dense Gaussian with these natural parameters."""
    m, d = theta_lin.shape
    rows = [[torch.zeros(d, d, dtype=torch.float64) for _ in range(m)] for _ in range(m)]
    for i in range(m):
        rows[i][i] = -(theta_diag[i] + theta_diag[i].T)
    for i in range(m - 1):
        rows[i + 1][i] = -theta_sub[i]
        rows[i][i + 1] = -theta_sub[i].T
    prec = torch.cat([torch.cat(r, dim=1) for r in rows], dim=0)
    sigma = torch.linalg.inv(prec)
    sigma = 0.5 * (sigma + sigma.T)
    return sigma @ theta_lin.reshape(-1), sigma


def naturals_to_params(theta_lin, theta_diag, theta_sub):
    mu, sigma = naturals_to_dense(theta_lin, theta_diag, theta_sub)
    return expectations_to_params(*dense_to_expectations(mu, sigma, theta_lin.shape[1]))


def pair_marginals_torch(mu, sigma, pinf, d):
    """sparse_cvi_closed_forms.pair_marginals in torch."""
    m = mu.shape[0] // d
    zero_v, zero_m = torch.zeros(d, dtype=torch.float64), torch.zeros(d, d, dtype=torch.float64)
    blk = lambda i, j: sigma[i * d:(i + 1) * d, j * d:(j + 1) * d]          # noqa: E731
    means, covs = [], []
    for s in range(m + 1):
        lo, hi = s - 1, s
        means.append(torch.cat([mu[lo * d:(lo + 1) * d] if lo >= 0 else zero_v, mu[hi * d:(hi + 1) * d] if hi < m else zero_v]))
        c_lo, c_hi = (blk(lo, lo) if lo >= 0 else pinf), (blk(hi, hi) if hi < m else pinf)
        cross = blk(hi, lo) if lo >= 0 and hi < m else zero_m
        covs.append(torch.cat([torch.cat([c_lo, cross.T], dim=1), torch.cat([cross, c_hi], dim=1)], dim=0))
    return torch.stack(means), torch.stack(covs)


def dense_kl_torch(mu, sigma, kuu):
    n = mu.shape[0]
    return 0.5 * (torch.trace(torch.linalg.solve(kuu, sigma)) + mu @ torch.linalg.solve(kuu, mu) - n + torch.linalg.slogdet(kuu)[1]
                  - torch.linalg.slogdet(sigma)[1])


class DenseNatGrad:
    """The dense natural-gradient loop on one series, started at the prior.  The state is the natural parameters ``theta`` (the dense
    precision is never obtained by inverting a covariance: ``theta`` starts from ``inv(K_uu)`` as the dense CVI loop's does and every
    step maps it to the moments with ONE dense inverse); ``params`` = ``(A_s, b_s, chol P_0, chol Q_s, mu_0)`` (float64 torch) is what
    ``naturals_to_params`` makes of it - the optimiser under test re-derives ``theta`` from those, the same iteration.  ``step()`` is
    one ``SSMNaturalGradient.minimize`` on ``loss = -elbo``; ``posterior()``, ``elbo()``, ``predict_f``."""

    def __init__(self, lik, comps, x, y, z, gamma, momentum=False, beta1=0.9, beta2=0.99, epsilon=1e-8, nq=20, num_data=None):
        self.lik, self.comps, self.nq = lik, comps, nq
        order = np.argsort(np.asarray(x), kind="stable")
        self.x, self.y, self.z = np.asarray(x, dtype=np.float64)[order], np.asarray(y, dtype=np.float64)[order], np.asarray(z, dtype=np.float64)
        self.d = SC.state_dim(comps)
        kuu = SC.dense_state_prior(comps, self.z)
        self.kuu = _t(kuu)
        self.pinf = _t(SC._transition(comps, 1.0)[2])
        self.idx, self.w, self.c = SC.conditional_projections(comps, self.x, self.z)
        self.offsets = SC.offsets_of(self.idx, len(self.z) + 1)
        self.scale = 1.0 if num_data is None else float(num_data) / len(self.x)
        self.gamma, self.momentum, self.beta1, self.beta2, self.epsilon = gamma, momentum, beta1, beta2, epsilon
        self.t, self.v, self.ms, self.effective_lr = 1, 0.0, None, gamma
        prec = _t(np.linalg.inv(kuu))
        lin, diag, sub = _blocks(torch.zeros(len(self.z) * self.d, dtype=torch.float64), 0.5 * (prec + prec.T), self.d)
        self.thetas = (lin, -0.5 * diag, -sub)

    @property
    def params(self):
        return naturals_to_params(*self.thetas)

    def posterior(self):
        mu, sigma = naturals_to_dense(*self.thetas)
        return mu.numpy(), sigma.numpy()

    def _elbo(self, mu, sigma):
        pm, pc = pair_marginals_torch(mu, sigma, self.pinf, self.d)
        ve = torch.sum(segment_value_torch(self.lik, self.w, self.c, self.y, self.offsets, pm, pc, self.nq))
        return self.scale * ve - dense_kl_torch(mu, sigma, self.kuu)

    def elbo_of(self, params):
        """The ELBO as a function of the chain's parameters, through the plain recursion."""
        a_s, b_s, cp0, cq, mu0 = params
        return self._elbo(*dense_moments(mu0, cp0, a_s, b_s, cq))

    def elbo(self):
        return float(self._elbo(*naturals_to_dense(*self.thetas)))

    def predict_f(self, t_new):
        mu, sigma = naturals_to_dense(*self.thetas)
        pm, pc = (a.numpy() for a in pair_marginals_torch(mu, sigma, self.pinf, self.d))
        idx, w, c = SC.conditional_projections(self.comps, np.asarray(t_new), self.z)
        return np.einsum("ki,ki->k", w, pm[idx]), c + np.einsum("ki,kij,kj->k", w, pc[idx], w)

    def step(self):
        leaves = tuple(p.detach().clone().requires_grad_(True) for p in self.params)
        grads = list(torch.autograd.grad(-self.elbo_of(leaves), leaves))
        grads[2], grads[3] = torch.tril(grads[2]), torch.tril(grads[3])

        def pulled_back(transform, point):
            point = tuple(p.detach().clone().requires_grad_(True) for p in point)
            return torch.autograd.grad(transform(*point), point, grad_outputs=grads)

        thetas = self.thetas
        etas = dense_to_expectations(*naturals_to_dense(*thetas), self.d)
        g_eta = pulled_back(expectations_to_params, etas)
        if self.momentum:
            g_theta = pulled_back(naturals_to_params, thetas)
            lr = self.gamma * math.sqrt(1.0 - self.beta2 ** self.t) / (1.0 - self.beta1 ** self.t)
            if self.ms is None:
                self.ms = [torch.zeros_like(e) for e in etas]
            self.ms = [m * self.beta1 + (1.0 - self.beta1) * g for m, g in zip(self.ms, g_eta)]
            norm = [float(torch.sum(g * gt)) for g, gt in zip(g_eta, g_theta)]
            self.v = self.v * self.beta2 + (1.0 - self.beta2) * (norm[0] + norm[1] + 2.0 * norm[2])
            self.effective_lr = lr / (math.sqrt(self.v) + self.epsilon)
            new = [th - self.effective_lr * m for th, m in zip(thetas, self.ms)]
            self.t += 1
        else:
            new = [th - self.gamma * g for th, g in zip(thetas, g_eta)]
        self.thetas = tuple(t.detach() for t in new)
