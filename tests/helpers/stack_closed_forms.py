"""
Reference of the stacked-chain SVGP data term and model - TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Independent of markovflow_amd/models/, markovflow_amd/likelihoods.py and csrc/mf_lik_stack.hip.  ``K`` latent functions, each on a
chain of its own (markovflow/kernels/sde_kernel.py:945-1279: ``StackKernel``), coupled only by the likelihood of a point:

  * ``MULTISTAGE`` (``K = 3``): the stage functions of tests/helpers/multistage_closed_forms.py, reused;
  * ``HETERO`` (``K = 2``): the heteroscedastic Gaussian ``y ~ N(F0, exp F1)`` in closed form.  With ``e = exp(-m1 + v1 / 2)`` and
    ``E = e ((m0 - y)^2 + v0)``: ``ve = -(log 2 pi + m1 + E) / 2``, ``d/dm0 = -e (m0 - y)``, ``d/dv0 = -e / 2``, ``d/dm1 = -(1 - E) / 2``,
    ``d/dv1 = -E / 4``; the magnitudes are those of the terms of each expression;
  * ``segment_expectations_stack``: the per-segment sums of ``mf_lik_stack_expectations_*`` for one series in the kernel's order
    (points ascending, within a point the latents ascending, tiles of 64 points, then the tiles), with a ``dtype`` switch.  A latent
    that is read outside the domain makes the value and ALL latents' derivatives of the point NaN;
  * ``dense_stack_elbo``: the dense statement of the stacked model at a given block-diagonal ``q`` - ``K`` independent dense
    Gaussians on the (padded) inducing states, their pair marginals and conditional projections, the coupled likelihood, ``K`` dense
    KL terms;
  * ``DenseStackNatGrad``: the dense natural-gradient loop, a ``svgp_closed_forms.DenseNatGrad`` per chain stepped simultaneously.
"""
import numpy as np
import torch

from helpers import multistage_closed_forms as MS
from helpers import sparse_cvi_closed_forms as SC
from helpers import svgp_closed_forms as SV

MULTISTAGE, HETERO = 4, 5           # the likelihood ids of the entry point
LATENTS = {MULTISTAGE: 3, HETERO: 2}
TILE = SV.TILE
LOG_2PI = float(np.log(2.0 * np.pi))


# ---- the heteroscedastic Gaussian ---------------------------------------------------------------------------------------------------
def hetero_log_prob(f, y):
    """``log N(y | F0, exp F1)``, ``f [N, 2]``, ``y [N] -> [N]`` (float64)."""
    f, y = np.asarray(f, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return -0.5 * (LOG_2PI + f[..., 1] + (y - f[..., 0]) ** 2 * np.exp(-f[..., 1]))


def hetero_expectations(mu, var, y, dtype=np.float64):
    """``mu``, ``var`` ``[N, 2]``, ``y [N]``.  Returns ``((ve [N], gm [N, 2], gv [N, 2]), (mag_ve, mag_gm, mag_gv))``: the values in
    ``dtype``, the magnitudes always float64.  Both latents are read: a variance that is not positive gives NaN everywhere."""
    ty = dtype
    mu, var, y = (np.asarray(a, dtype=ty) for a in (mu, var, y))
    with np.errstate(invalid="ignore"):
        ok = (var[..., 0] > 0) & (var[..., 1] > 0)
    r = mu[..., 0] - y
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(ty(0.5) * var[..., 1] - mu[..., 1])
        big = e * (r * r + var[..., 0])
    ve = ty(-0.5) * (ty(LOG_2PI) + mu[..., 1] + big)
    gm = np.stack([-e * r, ty(-0.5) * (ty(1) - big)], axis=-1)
    gv = np.stack([ty(-0.5) * e, ty(-0.25) * big], axis=-1)
    nan = ty(np.nan)
    ve, gm, gv = np.where(ok, ve, nan), np.where(ok[..., None], gm, nan), np.where(ok[..., None], gv, nan)
    m8, v8, y8 = (np.asarray(a, dtype=np.float64) for a in (mu, var, y))
    with np.errstate(over="ignore", invalid="ignore"):
        e8 = np.exp(0.5 * v8[..., 1] - m8[..., 1])
        r8 = np.abs(m8[..., 0] - y8)
        big8 = e8 * (r8 * r8 + np.abs(v8[..., 0]))
    mags = (0.5 * (LOG_2PI + np.abs(m8[..., 1]) + big8), np.stack([e8 * r8, 0.5 * (1.0 + big8)], axis=-1),
            np.stack([0.5 * e8, 0.25 * big8], axis=-1))
    return (ve.astype(ty), gm.astype(ty), gv.astype(ty)), mags


def hetero_expectations_torch(mu, var, y):
    """The value in torch (float64): ``mu``, ``var`` ``[N, 2]`` tensors, ``y [N]`` -> ``[N]``."""
    y = torch.as_tensor(np.array(y, dtype=np.float64)) if not isinstance(y, torch.Tensor) else y          # (a copy: y may be read-only)
    r = mu[..., 0] - y
    return -0.5 * (LOG_2PI + mu[..., 1] + torch.exp(0.5 * var[..., 1] - mu[..., 1]) * (r * r + var[..., 0]))


def gauss_hermite_product(mu, var, y, nq):
    """``E log N(y | F0, exp F1)`` by an ``nq x nq`` Gauss-Hermite product rule (float64): the check of the closed form."""
    x, w = np.polynomial.hermite.hermgauss(nq)
    w = w / np.sqrt(np.pi)
    mu, var, y = (np.asarray(a, dtype=np.float64) for a in (mu, var, y))
    f0 = mu[..., 0, None] + np.sqrt(2.0 * var[..., 0, None]) * x                    # [N, nq]
    f1 = mu[..., 1, None] + np.sqrt(2.0 * var[..., 1, None]) * x
    lp = -0.5 * (LOG_2PI + f1[..., None, :] + (y[..., None, None] - f0[..., :, None]) ** 2 * np.exp(-f1[..., None, :]))
    return np.einsum("...ij,i,j->...", lp, w, w)


# ---- one point on K marginals -------------------------------------------------------------------------------------------------------
def expectations(lik, mu, var, y, nq=20, dtype=np.float64):
    """``mu``, ``var`` ``[N, K]``, ``y [N]``: ``((ve, gm, gv), mags)`` with the stacked term's domain rule."""
    if lik == HETERO:
        return hetero_expectations(mu, var, y, dtype)
    assert lik == MULTISTAGE
    (ve, gm, gv), mags = MS.expectations(mu, var, y, nq, dtype=dtype)
    bad = np.isnan(ve)
    gm, gv = gm.copy(), gv.copy()
    gm[bad], gv[bad] = np.nan, np.nan
    return (ve, gm, gv), mags


def expectations_torch(lik, mu, var, y, nq=20):
    return hetero_expectations_torch(mu, var, y) if lik == HETERO else MS.expectations_torch(mu, var, y, nq)


# ---- the kernel's sums --------------------------------------------------------------------------------------------------------------
def segment_expectations_stack(w, c, y, offsets, pair_mean, pair_cov, lik, nq=20, dtype=np.float64):
    """One series.  ``w [K, N, 2d]``, ``c [K, N]``, ``y [N]``, ``offsets [S + 1]``, ``pair_mean [K, S, 2d]``, ``pair_cov [K, S, 2d, 2d]``.
    Per point n of segment s and latent k: mu_k = w_kn . m_ks, s2_k = c_kn + w_kn^T S_ks w_kn, the expectations; per segment
    ve_sum = sum ve, g_mean[k] = sum gm_k w_kn, g_cov[k] = sum gv_k w_kn w_kn^T in the kernel's order.  Returns ``ve_sum [S]``,
    ``g_mean [K, S, 2d]``, ``g_cov [K, S, 2d, 2d]`` in ``dtype`` and ``mag_*`` in float64."""
    ty = dtype
    w, c, pair_mean, pair_cov = (np.asarray(a, dtype=ty) for a in (w, c, pair_mean, pair_cov))
    lat, n, two_d = w.shape
    segs = len(offsets) - 1
    seg = np.repeat(np.arange(segs), np.diff(np.asarray(offsets)))
    assert seg.shape[0] == n and offsets[0] == 0 and offsets[-1] == n and lat == LATENTS[lik]
    fmu, fvar = np.zeros((n, lat), dtype=ty), c.T.copy()
    for k in range(lat):                        # the kernel's order: term by term in i, the product with row i of S_ks in j
        m, cov = pair_mean[k][seg], pair_cov[k][seg]
        for i in range(two_d):
            row = np.zeros(n, dtype=ty)
            for j in range(two_d):
                row = row + cov[:, i, j] * w[k, :, j]
            fvar[:, k] = fvar[:, k] + w[k, :, i] * row
            fmu[:, k] = fmu[:, k] + w[k, :, i] * m[:, i]
    if n:
        (ve, gm, gv), mags = expectations(lik, fmu, fvar, y, nq, dtype=ty)
    else:
        ve, gm, gv = np.zeros(0, dtype=ty), np.zeros((0, lat), dtype=ty), np.zeros((0, lat), dtype=ty)
        mags = np.zeros(0), np.zeros((0, lat)), np.zeros((0, lat))
    w8 = np.abs(w.astype(np.float64))
    out = dict(ve_sum=np.zeros(segs, dtype=ty), g_mean=np.zeros((lat, segs, two_d), dtype=ty),
               g_cov=np.zeros((lat, segs, two_d, two_d), dtype=ty), mag_ve_sum=np.zeros(segs), mag_g_mean=np.zeros((lat, segs, two_d)),
               mag_g_cov=np.zeros((lat, segs, two_d, two_d)))
    in_order = lambda terms: np.cumsum(terms, axis=0, dtype=ty)[-1]          # noqa: E731  (numpy accumulates one after the other)
    for s in range(segs):
        tiles = [slice(k0, min(k0 + TILE, offsets[s + 1])) for k0 in range(offsets[s], offsets[s + 1], TILE)]
        pts = slice(offsets[s], offsets[s + 1])
        if tiles:
            out["ve_sum"][s] = in_order(np.stack([in_order(ve[t]) for t in tiles]))
        out["mag_ve_sum"][s] = np.sum(mags[0][pts])
        for k in range(lat):
            if tiles:
                out["g_mean"][k, s] = in_order(np.stack([in_order(gm[t, k][:, None] * w[k, t]) for t in tiles]))
                out["g_cov"][k, s] = in_order(np.stack([in_order((gv[t, k][:, None, None] * w[k, t][:, None, :]) * w[k, t][:, :, None])
                                                        for t in tiles]))
            out["mag_g_mean"][k, s] = np.einsum("n,ni->i", mags[1][pts, k], w8[k, pts])
            out["mag_g_cov"][k, s] = np.einsum("n,ni,nj->ij", mags[2][pts, k], w8[k, pts], w8[k, pts])
    return out


# ---- the dense model ----------------------------------------------------------------------------------------------------------------
def _pad_pairs(w, dk, d):
    """``w [N, 2 dk]`` of a chain of dimension ``dk`` in the pair layout of the padded chain, ``[N, 2 d]`` (zeros in the padding)."""
    out = np.zeros((w.shape[0], 2 * d))
    out[:, :dk], out[:, d:d + dk] = w[:, :dk], w[:, dk:]
    return out


def _chain(comp):
    """A chain is one component or a list of them (a Sum)."""
    return list(comp) if isinstance(comp, (list, tuple)) else [comp]


def padded_prior(comp, z, d):
    """``(K_uu [M d, M d], P_inf [d, d])`` of a chain padded to dimension ``d``: the padded states are independent standard normals."""
    cs = _chain(comp)
    dk, m = SC.state_dim(cs), len(z)
    kuu, pinf = np.eye(m * d), np.eye(d)
    real = (np.arange(m)[:, None] * d + np.arange(dk)[None, :]).reshape(-1)
    kuu[np.ix_(real, real)] = SC.dense_state_prior(cs, np.asarray(z))
    pinf[:dk, :dk] = SC._transition(cs, 1.0)[2]
    return kuu, pinf


def dense_stack_elbo(lik, comps, xs, y, zs, qs, nq=20, scale=1.0):
    """The ELBO of the stacked model for ONE series at a block-diagonal ``q``.  ``comps``: the ``K`` components; ``xs [K][N]`` the data
    times of every chain IN THE DATA'S ORDER (row n of every chain is observation ``y[n]``; a chain's times need not be sorted);
    ``zs [K][M]`` its inducing points; ``qs [K]`` its ``(mu0 [d], chol_P0 [d, d], A [M-1, d, d], b [M-1, d], chol_Q [M-1, d, d])`` on
    the padded dimension ``d = max d_k`` (numpy).  Returns a float: ``scale sum_n E_q log p(y_n | f_n) - sum_k KL_k``."""
    d = max(SC.state_dim(_chain(c)) for c in comps)
    fmu, fvar, kl = [], [], 0.0
    for comp, x, z, q in zip(comps, xs, zs, qs):
        mu0, cp0, a_s, b_s, cq = (SV._t(a) for a in q)
        mu, sigma = SV.dense_moments(mu0, cp0, a_s, b_s, cq)
        kuu, pinf = padded_prior(comp, z, d)
        pm, pc = SV.pair_marginals_torch(mu, sigma, SV._t(pinf), d)
        idx, w, c = SC.conditional_projections(_chain(comp), np.asarray(x), np.asarray(z))
        w = SV._t(_pad_pairs(w, SC.state_dim(_chain(comp)), d))
        fmu.append(torch.einsum("ni,ni->n", w, pm[idx]))
        fvar.append(SV._t(c) + torch.einsum("ni,nij,nj->n", w, pc[idx], w))
        kl = kl + SV.dense_kl_torch(mu, sigma, SV._t(kuu))
    ve = expectations_torch(lik, torch.stack(fmu, dim=-1), torch.stack(fvar, dim=-1), np.asarray(y, dtype=np.float64), nq)
    return float(scale * torch.sum(ve) - kl)


class _Chain(SV.DenseNatGrad):
    """One chain of ``DenseStackNatGrad``: its ELBO is the coupled one with the other chains' marginals at the data held fixed."""

    def __init__(self, owner, index, comp, x, y, z, gamma, nq):
        super().__init__(MS.BERN, _chain(comp), x, y, z, gamma, nq=nq)            # (the likelihood slot is not used)
        self.owner, self.index = owner, index
        self.w_t, self.c_t = SV._t(self.w), SV._t(self.c)

    def point_marginals(self, mu, sigma):
        pm, pc = SV.pair_marginals_torch(mu, sigma, self.pinf, self.d)
        return (torch.einsum("ni,ni->n", self.w_t, pm[self.idx]),
                self.c_t + torch.einsum("ni,nij,nj->n", self.w_t, pc[self.idx], self.w_t))

    def _elbo(self, mu, sigma):
        marg = list(self.owner.fixed)
        marg[self.index] = self.point_marginals(mu, sigma)
        return self.owner.data_term(marg) - SV.dense_kl_torch(mu, sigma, self.kuu)


class DenseStackNatGrad:
    """The dense natural-gradient loop of the stacked model on one series, started at the prior: every chain is a dense Gaussian on
    its own (unpadded) inducing states, all chains take ONE simultaneous natural-gradient step on ``loss = -elbo`` (the gradient of a
    chain is taken with the others held at their values before the step, as ``SSMNaturalGradient`` on the batch of chains does).
    ``x`` must be sorted and is shared by the chains; ``zs [K][M]``."""

    def __init__(self, lik, comps, x, y, zs, gamma, nq=20):
        self.lik, self.nq, self.y = lik, nq, np.asarray(y, dtype=np.float64)
        self.chains = [_Chain(self, k, comp, x, y, z, gamma, nq) for k, (comp, z) in enumerate(zip(comps, zs))]
        self.fixed = self._marginals()

    def _marginals(self):
        return [tuple(t.detach() for t in ch.point_marginals(*SV.naturals_to_dense(*ch.thetas))) for ch in self.chains]

    def data_term(self, marg):
        fmu, fvar = torch.stack([m[0] for m in marg], dim=-1), torch.stack([m[1] for m in marg], dim=-1)
        return torch.sum(expectations_torch(self.lik, fmu, fvar, self.y, self.nq))

    def elbo(self):
        self.fixed = self._marginals()
        kl = sum(SV.dense_kl_torch(*SV.naturals_to_dense(*ch.thetas), ch.kuu) for ch in self.chains)
        return float(self.data_term(self.fixed) - kl)

    def step(self):
        self.fixed = self._marginals()
        for ch in self.chains:
            ch.step()
        self.fixed = self._marginals()

    def predict_f(self, t_new):
        parts = [ch.predict_f(t_new) for ch in self.chains]
        return np.stack([p[0] for p in parts], axis=-1), np.stack([p[1] for p in parts], axis=-1)
