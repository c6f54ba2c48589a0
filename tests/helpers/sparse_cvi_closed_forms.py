"""
numpy (fp64) reference of the sparse CVI model - TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Two things, both independent of markovflow_amd/models/ (sparse.py, segmented_ops.py) and csrc/mf_lik.hip:

  * ``segment_update``: the per-segment formulas of ``mf_lik_sparse_cvi_site_update_*`` for one series, on
    ``likelihood_closed_forms.expectations``, with the magnitudes that scale a rounding-error bound;
  * ``dense_sparse_cvi``: the sparse CVI loop (markovflow/models/sparse_variational_cvi.py) with dense matrices - the prior on the
    stacked inducing states as ONE Gaussian built from the closed-form transitions of tests/helpers/periodic_closed_forms.py, the
    sites added to its precision, a dense inverse, pair marginals read off it, the conditional projections from closed-form
    transitions, the segmented update and ``classic_elbo`` with a dense KL.  No block-tridiagonal algebra, no recursion.

A likelihood is the ``(name, params)`` tuple of likelihood_closed_forms.py; a kernel the list of component dicts of
periodic_closed_forms.py.
"""
import numpy as np

from helpers import likelihood_closed_forms as L
from helpers import periodic_closed_forms as PC


# ---- the kernel's formulas ---------------------------------------------------------------------------------------------------------
def segment_update(lik, w, c, y, offsets, pair_mean, pair_cov, lr, nat1, nat2, nq=20, dtype=np.float64):
    """One series.  ``w [N, 2d]``, ``c [N]``, ``y [N]``, ``offsets [S + 1]``, ``pair_mean [S, 2d]``, ``pair_cov [S, 2d, 2d]``,
    ``nat1 [S, 2d]``, ``nat2 [S, 2d, 2d]``.  Per point k of segment s: fmu = w_k . m_s, fvar = c_k + w_k^T S_s w_k, (ve, gm, gv) the
    expectations, g2 = gv, g1 = gm - 2 gv fmu; per segment nat <- (1 - lr) nat + lr sum_k g (w_k | w_k w_k^T).  ``dtype`` =
    numpy.float32 evaluates everything in float32.  Returns a dict: ``nat1``, ``nat2``, ``fmu``, ``fvar``, ``ve`` and the magnitudes
    (always float64) ``mag_nat1`` = |nat1| + sum_k |g1| |w_i|, ``mag_nat2`` = |nat2| + sum_k |g2| |w_i| |w_j| (with the helper's
    magnitudes of the derivatives for |g|: |g2| -> mag(gv), |g1| -> mag(gm) + 2 mag(gv) |fmu|), ``mag_fmu`` = sum |w_i| |m_i|,
    ``mag_fvar`` = |c| + sum |w_i| |S_ij| |w_j| and ``mag_ve``."""
    ty = dtype
    w, c, y, pair_mean, pair_cov, nat1, nat2 = (np.asarray(a, dtype=ty) for a in (w, c, y, pair_mean, pair_cov, nat1, nat2))
    n, segs = w.shape[0], len(offsets) - 1
    seg = np.repeat(np.arange(segs), np.diff(np.asarray(offsets)))
    assert seg.shape[0] == n and offsets[0] == 0 and offsets[-1] == n
    m, cov = pair_mean[seg], pair_cov[seg]
    fmu = np.einsum("ki,ki->k", w, m).astype(ty)
    fvar = (c + np.einsum("ki,kij,kj->k", w, cov, w)).astype(ty)
    w8, m8, cov8 = w.astype(np.float64), m.astype(np.float64), cov.astype(np.float64)
    mag_fmu = np.einsum("ki,ki->k", np.abs(w8), np.abs(m8))
    mag_fvar = np.abs(c.astype(np.float64)) + np.einsum("ki,kij,kj->k", np.abs(w8), np.abs(cov8), np.abs(w8))
    if n:
        (ve, gm, gv), mags = L.expectations(lik, fmu, fvar, y, nq, dtype=ty)
    else:
        ve = gm = gv = np.zeros(0, dtype=ty)
        mags = (np.zeros(0),) * 3
    g2 = gv
    g1 = gm - ty(2) * gv * fmu
    mg2 = mags[2]
    mg1 = mags[1] + 2.0 * mags[2] * np.abs(fmu.astype(np.float64))
    new1, new2 = np.empty_like(nat1), np.empty_like(nat2)
    mag1, mag2 = np.abs(nat1.astype(np.float64)), np.abs(nat2.astype(np.float64))
    one, lr_t = ty(1), ty(lr)
    for s in range(segs):
        k = slice(offsets[s], offsets[s + 1])
        sum1 = np.einsum("k,ki->i", g1[k], w[k]).astype(ty)
        sum2 = np.einsum("k,ki,kj->ij", g2[k], w[k], w[k]).astype(ty)
        new1[s] = (one - lr_t) * nat1[s] + lr_t * sum1
        new2[s] = (one - lr_t) * nat2[s] + lr_t * sum2
        mag1[s] += np.einsum("k,ki->i", mg1[k], np.abs(w8[k]))
        mag2[s] += np.einsum("k,ki,kj->ij", mg2[k], np.abs(w8[k]), np.abs(w8[k]))
    return dict(nat1=new1, nat2=new2, fmu=fmu, fvar=fvar, ve=ve, mag_nat1=mag1, mag_nat2=mag2, mag_fmu=mag_fmu, mag_fvar=mag_fvar,
                mag_ve=mags[0])


# ---- the dense sparse CVI loop -----------------------------------------------------------------------------------------------------
def state_dim(comps):
    return sum(PC.size(c) for c in comps)


def _transition(comps, dt):
    """(A, Q, Pinf) for ONE gap dt >= 0; dt = inf is the stationary prior's side: A = 0, Q = Pinf."""
    if np.isinf(dt):
        _, _, p = PC.concat_transitions(comps, np.array(1.0))
        return np.zeros_like(p), p.copy(), p
    return PC.concat_transitions(comps, np.array(float(dt)))


def dense_state_prior(comps, z):
    """Covariance [M d, M d] of the stacked states s(z_1) ... s(z_M): Cov(s(z_i), s(z_j)) = A(z_i - z_j) Pinf for i >= j."""
    d, m = state_dim(comps), len(z)
    k = np.zeros((m * d, m * d))
    for i in range(m):
        for j in range(i + 1):
            a, _, p = _transition(comps, z[i] - z[j])
            blk = a @ p
            k[i * d:(i + 1) * d, j * d:(j + 1) * d] = blk
            k[j * d:(j + 1) * d, i * d:(i + 1) * d] = blk.T
    return 0.5 * (k + k.T)


def conditional_projections(comps, x, z):
    """Per data point: the index of the pair it belongs to (z_{m-1} < x <= z_m: pair m, numpy.searchsorted's default side),
    w = H [D E] (``[N, 2d]``) and c = H T H^T (``[N]``) of p(s(x) | s(z_-), s(z_+)) = N(D s_- + E s_+, T) with
    E = Q_mt A_tp^T (Q_tp + A_tp Q_mt A_tp^T)^-1, D = A_mt - E A_tp A_mt, T = Q_mt - E A_tp Q_mt; beyond the ends the neighbour is
    the stationary prior, infinitely far away."""
    d = state_dim(comps)
    h = PC.emission(comps, ())[0]                                        # [d]
    idx = np.searchsorted(z, x)
    aug = np.concatenate([[-np.inf], z, [np.inf]])
    w, c = np.zeros((len(x), 2 * d)), np.zeros(len(x))
    for k, (xk, m) in enumerate(zip(x, idx)):
        a_mt, q_mt, _ = _transition(comps, xk - aug[m])
        gap = aug[m + 1] - xk
        if gap == 0.0:                                                   # the point IS the inducing point
            e_m, d_m, t_m = np.eye(d), np.zeros((d, d)), np.zeros((d, d))
        else:
            a_tp, q_tp, _ = _transition(comps, gap)
            g = a_tp @ q_mt
            e_m = np.linalg.solve(q_tp + g @ a_tp.T, g).T
            d_m = a_mt - e_m @ a_tp @ a_mt
            t_m = q_mt - e_m @ g
        w[k] = np.concatenate([h @ d_m, h @ e_m])
        c[k] = h @ t_m @ h
    return idx, w, c


def offsets_of(idx, segs):
    return np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=segs))]).astype(np.int64)


def dense_posterior(kuu, nat1, nat2, d):
    """q(u) = N(mu, Sigma) from the prior covariance and the sites: pair m = [u_{m-1}, u_m] (0-based states m - 1 and m); the halves
    of sites 0 and M that face the stationary prior, and their cross blocks, do not enter (sparse_variational_cvi.py:154-157).
    Asserts that the precision is positive definite."""
    m = kuu.shape[0] // d
    prec = np.linalg.inv(kuu)
    lin = np.zeros(m * d)
    for s in range(m + 1):
        lo, hi = s - 1, s
        if lo >= 0:
            lin[lo * d:(lo + 1) * d] += nat1[s, :d]
            prec[lo * d:(lo + 1) * d, lo * d:(lo + 1) * d] += -2.0 * nat2[s, :d, :d]
        if hi < m:
            lin[hi * d:(hi + 1) * d] += nat1[s, d:]
            prec[hi * d:(hi + 1) * d, hi * d:(hi + 1) * d] += -2.0 * nat2[s, d:, d:]
        if lo >= 0 and hi < m:
            prec[hi * d:(hi + 1) * d, lo * d:(lo + 1) * d] += -2.0 * nat2[s, d:, :d]
            prec[lo * d:(lo + 1) * d, hi * d:(hi + 1) * d] += -2.0 * nat2[s, d:, :d].T
    prec = 0.5 * (prec + prec.T)
    assert np.linalg.eigvalsh(prec).min() > 0.0, "dist_q of the dense run must stay positive definite"
    sigma = np.linalg.inv(prec)
    sigma = 0.5 * (sigma + sigma.T)
    return sigma @ lin, sigma


def pair_marginals(mu, sigma, pinf, d):
    """([M + 1, 2d], [M + 1, 2d, 2d]): the joint of (u_{m-1}, u_m); the stationary prior N(0, Pinf), uncorrelated, beyond the ends."""
    m = len(mu) // d
    means, covs = np.zeros((m + 1, 2 * d)), np.zeros((m + 1, 2 * d, 2 * d))
    for s in range(m + 1):
        lo, hi = s - 1, s
        covs[s, :d, :d] = sigma[lo * d:(lo + 1) * d, lo * d:(lo + 1) * d] if lo >= 0 else pinf
        covs[s, d:, d:] = sigma[hi * d:(hi + 1) * d, hi * d:(hi + 1) * d] if hi < m else pinf
        if lo >= 0:
            means[s, :d] = mu[lo * d:(lo + 1) * d]
        if hi < m:
            means[s, d:] = mu[hi * d:(hi + 1) * d]
        if lo >= 0 and hi < m:
            covs[s, d:, :d] = sigma[hi * d:(hi + 1) * d, lo * d:(lo + 1) * d]
            covs[s, :d, d:] = covs[s, d:, :d].T
    return means, covs


def dense_kl(mu, sigma, kuu):
    n = len(mu)
    return 0.5 * (np.trace(np.linalg.solve(kuu, sigma)) + mu @ np.linalg.solve(kuu, mu) - n + np.linalg.slogdet(kuu)[1]
                  - np.linalg.slogdet(sigma)[1])


class DenseSparseCVI:
    """The dense loop's state for one series: ``step()`` is one ``update_sites``; ``classic_elbo()``, ``predict_f(t_new)``."""

    def __init__(self, lik, comps, x, y, z, lr, nq=20):
        self.lik, self.comps, self.x, self.y, self.z, self.lr, self.nq = lik, comps, np.asarray(x), np.asarray(y), np.asarray(z), lr, nq
        self.d = state_dim(comps)
        self.kuu = dense_state_prior(comps, self.z)
        self.pinf = _transition(comps, 1.0)[2]
        self.idx, self.w, self.c = conditional_projections(comps, self.x, self.z)
        self.offsets = offsets_of(self.idx, len(self.z) + 1)
        self.nat1 = np.zeros((len(self.z) + 1, 2 * self.d))
        self.nat2 = np.zeros((len(self.z) + 1, 2 * self.d, 2 * self.d))

    def posterior(self):
        return dense_posterior(self.kuu, self.nat1, self.nat2, self.d)

    def step(self):
        mu, sigma = self.posterior()
        pm, pc = pair_marginals(mu, sigma, self.pinf, self.d)
        out = segment_update(self.lik, self.w, self.c, self.y, self.offsets, pm, pc, self.lr, self.nat1, self.nat2, self.nq)
        self.nat1, self.nat2 = out["nat1"], out["nat2"]

    def _project(self, x, y=None):
        mu, sigma = self.posterior()
        pm, pc = pair_marginals(mu, sigma, self.pinf, self.d)
        idx, w, c = conditional_projections(self.comps, x, self.z)
        fmu = np.einsum("ki,ki->k", w, pm[idx])
        fvar = c + np.einsum("ki,kij,kj->k", w, pc[idx], w)
        return fmu, fvar, mu, sigma

    def classic_elbo(self):
        fmu, fvar, mu, sigma = self._project(self.x)
        (ve, _, _), _ = L.expectations(self.lik, fmu, fvar, self.y, self.nq)
        return np.sum(ve) - dense_kl(mu, sigma, self.kuu)

    def predict_f(self, t_new):
        fmu, fvar, _, _ = self._project(np.asarray(t_new))
        return fmu, fvar


def dense_sparse_cvi(lik, comps, x, y, z, lr, iterations, nq=20, record=()):
    """Run the dense loop; ``{iteration: dict(nat1, nat2, classic_elbo)}`` for the (1-based) iterations in ``record`` - the state AFTER
    that update - and the final ``DenseSparseCVI``."""
    run = DenseSparseCVI(lik, comps, x, y, z, lr, nq)
    out = {}
    for it in range(1, iterations + 1):
        run.step()
        if it in record:
            out[it] = dict(nat1=run.nat1.copy(), nat2=run.nat2.copy(), classic_elbo=run.classic_elbo())
    return out, run


def collapsed_bound(comps, x, y, z, noise):
    """Titsias' collapsed bound log N(y | 0, Q_ff + noise I) - tr(K_ff - Q_ff) / (2 noise), Q_ff = K_fu K_uu^-1 K_uf, on the dense
    kernel matrices (for a kernel whose state IS f: Matern-1/2)."""
    kuu = PC.dense_kernel(comps, z[:, None] - z[None, :])
    kfu = PC.dense_kernel(comps, x[:, None] - z[None, :])
    kff_diag = PC.dense_kernel(comps, np.zeros(len(x)))
    qff = kfu @ np.linalg.solve(kuu, kfu.T)
    kn = qff + noise * np.eye(len(x))
    fit = -0.5 * y @ np.linalg.solve(kn, y) - 0.5 * np.linalg.slogdet(kn)[1] - 0.5 * len(x) * np.log(2 * np.pi)
    return fit - 0.5 * np.sum(kff_diag - np.diag(qff)) / noise


def sparse_gp_predict(comps, x, y, z, noise, t_new):
    """The sparse GP predictive of f at t_new with the optimal q(u) (Titsias 2009, eq. 6 with eq. 10)."""
    kuu = PC.dense_kernel(comps, z[:, None] - z[None, :])
    kuf = PC.dense_kernel(comps, z[:, None] - x[None, :])
    ksu = PC.dense_kernel(comps, t_new[:, None] - z[None, :])
    sig = kuu + kuf @ kuf.T / noise
    mean = ksu @ np.linalg.solve(sig, kuf @ y) / noise
    var = (PC.dense_kernel(comps, np.zeros(len(t_new))) - np.einsum("ij,ji->i", ksu, np.linalg.solve(kuu, ksu.T))
           + np.einsum("ij,ji->i", ksu, np.linalg.solve(sig, ksu.T)))
    return mean, var
