"""
numpy (fp64) reference of the sparse power-EP model - TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Two things, both independent of markovflow_amd/models/ (sparse.py, segmented_ops.py) and csrc/mf_lik.hip:

  * ``segment_pep_update``: both passes of ``mf_lik_sparse_pep_site_update_*`` for one series in numpy, in any dtype, on
    ``pep_closed_forms.log_expected_density``, summed in the kernel's order (tiles of 64 points in ascending order, then the tiles),
    with the magnitudes that scale a rounding-error bound;
  * ``DenseSparsePEP``: the sparse power-EP loop (markovflow/models/sparse_pep.py) on ONE Gaussian over the stacked inducing states -
    the dense construction of tests/helpers/sparse_cvi_closed_forms.py (prior covariance from closed-form transitions, sites added to
    its precision, a dense inverse, pair marginals read off it, closed-form conditional projections), the pair cavity by dense
    ``2d x 2d`` inverses, and the site normaliser from ``M + 1`` LEAVE-ONE-OUT posteriors as the reference builds it
    (sparse_pep.py:418-429): ``log Z(q with t_m^(1 - beta_m)) - log Z(q)`` with ``log Z = (log det Sigma + lin^T Sigma lin) / 2`` up to a
    constant that cancels.  No block-tridiagonal algebra, no recursion, no local form of the normaliser.

Magnitudes (always float64; a bound is K eps (magnitude + 1)).  (I, g1, g2) enter with ``pep_closed_forms``' magnitudes + 1; the
correction den, L2, L1 carries a running error bound through its scalar algebra (``pep_closed_forms._add`` ... ``_div``) from an
EXACT (fmu, fvar) - the update may be evaluated at a GIVEN projection (``at=``: the kernel's own, which is checked on its own, so that
the sensitivity of I, g1, g2 to the rounding of fmu and fvar does not have to be bounded).  A segment's sums then have
``mag_sum2 = sum_k bound(L2_k) |w_i| |w_j|``, ``mag_sum1 = sum_k bound(L1_k) |w_i|``, ``mag_led_sum = sum_k (mag_I + 1)``, and the
blended sites ``|(1 - lr) old| + lr (|(1 - alpha) old| + mag_sum (+ |seg_const|)) + |new|``.

A likelihood is the ``(name, params)`` tuple of likelihood_closed_forms.py; a kernel the list of component dicts of
periodic_closed_forms.py.
"""
import numpy as np

from helpers import likelihood_closed_forms as L
from helpers import pep_closed_forms as P
from helpers import sparse_cvi_closed_forms as SC

TILE = 64           # points per tile of pass 1: fixes the order of the sums


def project(w, c, seg, mean, cov, dtype=np.float64):
    """``fmu = w . m``, ``fvar = c + w^T S w`` per point in the kernel's order - fmu and fvar grow term by term in i, the inner
    product with row i of S in j - and their magnitudes ``sum |w_i| |m_i|``, ``|c| + sum |w_i| |S_ij| |w_j|`` (float64)."""
    ty = dtype
    w, c, mean, cov = (np.asarray(a, dtype=ty) for a in (w, c, mean, cov))
    n, two_d = w.shape
    m, s = mean[seg], cov[seg]
    fmu, fvar = np.zeros(n, dtype=ty), c.copy()
    with np.errstate(all="ignore"):
        for i in range(two_d):
            row = np.zeros(n, dtype=ty)
            for j in range(two_d):
                row = row + s[:, i, j] * w[:, j]
            fvar = fvar + w[:, i] * row
            fmu = fmu + w[:, i] * m[:, i]
        w8 = np.abs(w.astype(np.float64))
        mag_fmu = np.einsum("ki,ki->k", w8, np.abs(m.astype(np.float64)))
        mag_fvar = np.abs(c.astype(np.float64)) + np.einsum("ki,kij,kj->k", w8, np.abs(s.astype(np.float64)), w8)
    return fmu, fvar, mag_fmu, mag_fvar


def point_steps(lik, fmu, fvar, y, alpha, nq=20, dtype=np.float64):
    """Per point, from the cavity marginal ``(fmu, fvar)``: ``I, g1, g2``; ``den = 1 + fvar g2`` (Gaussian: ``(var / alpha) /
    (var / alpha + fvar)``, the same number without the cancellation), ``L2 = g2 / (2 den)``, ``L1 = (g1 - fmu g2) / den``.  Returns
    ``(led, l1, l2, defined)`` in ``dtype`` - ``led`` is I wherever fvar > 0 (else NaN), ``l1`` / ``l2`` and the row value of I are NaN
    where the point is undefined - and the running error bounds ``(mag_led, mag_l1, mag_l2)`` (float64, 0 where undefined)."""
    ty = dtype
    fmu, fvar, y = (np.asarray(a, dtype=ty) for a in (fmu, fvar, y))
    inside = fvar > 0
    mu_s, var_s = np.where(inside, fmu, ty(0)).astype(ty), np.where(inside, fvar, ty(1)).astype(ty)
    if len(mu_s) == 0:
        z = np.zeros(0, dtype=ty)
        return z, z, z, np.zeros(0, dtype=bool), (np.zeros(0),) * 3
    (led, g1, g2), led_mags = P.log_expected_density(lik, mu_s, var_s, y, alpha, nq, ty)
    with np.errstate(all="ignore"):
        if lik[0] == L.GAUSSIAN:
            sa = ty(lik[1][0]) / ty(alpha)
            den = sa / (sa + var_s)
        else:
            den = ty(1) + var_s * g2
        l2 = (ty(0.5) * g2 / den).astype(ty)
        l1 = ((g1 - mu_s * g2) / den).astype(ty)
        defined = inside & (den > 0) & np.isfinite(l2) & np.isfinite(l1) & np.isfinite(led)
        # the running error bound of the same algebra in float64, from the (float64 view of the) same fmu, fvar
        e = lambda a: P._exact(np.asarray(a, dtype=np.float64))                                     # noqa: E731
        if ty != np.float64:
            (led8, g18, g28), _ = P.log_expected_density(lik, mu_s.astype(np.float64), var_s.astype(np.float64), y.astype(np.float64),
                                                         alpha, nq)
        else:
            led8, g18, g28 = led, g1, g2
        t1, t2 = ((v, mag + 1.0) for v, mag in zip((g18, g28), led_mags[1:]))
        tm, tv = e(mu_s), e(var_s)
        one, half = e(np.ones_like(tm[0])), e(0.5)
        if lik[0] == L.GAUSSIAN:
            sa8 = e(lik[1][0] / alpha)
            tden = P._div(sa8, P._add(sa8, tv))
        else:
            tden = P._add(one, P._mul(tv, t2))
        tl2 = P._mul(half, P._div(t2, tden))
        tl1 = P._div(P._add(t1, P._mul(tm, t2), -1.0), tden)
    nan = ty(np.nan)
    mags = tuple(np.where(defined, m, 0.0) for m in (led_mags[0] + 1.0, tl1[1], tl2[1]))
    return (np.where(inside, led, nan).astype(ty), np.where(defined, l1, nan).astype(ty), np.where(defined, l2, nan).astype(ty),
            defined, mags)


def segment_pep_update(lik, w, c, y, offsets, cav_mean, cav_cov, alpha, lr, nat1, nat2, log_norm, seg_const=None, nq=20,
                       dtype=np.float64, at=None):
    """One series, both passes.  ``w [N, 2d]``, ``c [N]``, ``y [N]``, ``offsets [S + 1]``, ``cav_mean [S, 2d]``,
    ``cav_cov [S, 2d, 2d]``, ``nat1 [S, 2d]``, ``nat2 [S, 2d, 2d]``, ``log_norm [S]``, ``seg_const [S]`` or None.  ``at`` =
    ``(fmu, fvar)``: the steps at THAT projection instead of the one computed here.  Returns a dict: ``nat1``, ``nat2``, ``log_norm``
    (new values; an undefined segment keeps its old ones), ``led_sum`` (raw, NaN for an undefined segment), ``fmu``, ``fvar`` (NaN
    where fvar is not > 0), ``led``, ``skipped [S]`` and the magnitudes ``mag_nat1``, ``mag_nat2``, ``mag_log_norm``, ``mag_led_sum``,
    ``mag_fmu``, ``mag_fvar``, ``mag_led`` (float64)."""
    ty = dtype
    w, c, y, nat1, nat2, log_norm = (np.asarray(a, dtype=ty) for a in (w, c, y, nat1, nat2, log_norm))
    n, segs, two_d = w.shape[0], len(offsets) - 1, w.shape[1]
    const = np.zeros(segs, dtype=ty) if seg_const is None else np.asarray(seg_const, dtype=ty)
    seg = np.repeat(np.arange(segs), np.diff(np.asarray(offsets)))
    assert seg.shape[0] == n and offsets[0] == 0 and offsets[-1] == n
    fmu, fvar, mag_fmu, mag_fvar = project(w, c, seg, cav_mean, cav_cov, ty)
    if at is not None:
        fmu, fvar = (np.asarray(a, dtype=ty) for a in at)
    led, l1, l2, defined, (mag_led, mag_l1, mag_l2) = point_steps(lik, fmu, fvar, y, alpha, nq, ty)
    row_i = np.where(defined, led, ty(np.nan)).astype(ty)
    inside = fvar > 0
    w8 = np.abs(w.astype(np.float64))
    one, rate, al = ty(1), ty(lr), ty(alpha)
    in_order = lambda terms: np.cumsum(terms, axis=0, dtype=ty)[-1]          # noqa: E731  (numpy accumulates one after the other)
    out = dict(nat1=nat1.copy(), nat2=nat2.copy(), log_norm=log_norm.copy(), led_sum=np.zeros(segs, dtype=ty),
               fmu=np.where(inside, fmu, ty(np.nan)).astype(ty), fvar=np.where(inside, fvar, ty(np.nan)).astype(ty), led=led,
               skipped=np.zeros(segs, dtype=bool), mag_nat1=np.zeros((segs, two_d)), mag_nat2=np.zeros((segs, two_d, two_d)),
               mag_log_norm=np.zeros(segs), mag_led_sum=np.zeros(segs), mag_fmu=mag_fmu, mag_fvar=mag_fvar, mag_led=mag_led)
    with np.errstate(all="ignore"):
        for s in range(segs):
            tiles = [slice(k0, min(k0 + TILE, offsets[s + 1])) for k0 in range(offsets[s], offsets[s + 1], TILE)]
            sum2, sum1, sum_i = np.zeros((two_d, two_d), dtype=ty), np.zeros(two_d, dtype=ty), ty(0)
            if tiles:
                sum2 = in_order(np.stack([in_order((l2[k, None, None] * w[k][:, None, :]) * w[k][:, :, None]) for k in tiles]))
                sum1 = in_order(np.stack([in_order(l1[k, None] * w[k]) for k in tiles]))
                sum_i = in_order(np.stack([in_order(row_i[k]) for k in tiles]))
            out["led_sum"][s] = sum_i
            total = ty(sum_i + const[s])
            k = slice(offsets[s], offsets[s + 1])
            m2 = np.einsum("k,ki,kj->ij", mag_l2[k], w8[k], w8[k])
            m1 = np.einsum("k,ki->i", mag_l1[k], w8[k])
            mi = np.sum(mag_led[k])
            out["mag_led_sum"][s] = mi
            if not (np.all(np.isfinite(sum2)) and np.all(np.isfinite(sum1)) and np.isfinite(total)):
                out["skipped"][s] = True
                continue
            for key, old, step, mag in (("nat2", nat2[s], sum2, m2), ("nat1", nat1[s], sum1, m1),
                                        ("log_norm", log_norm[s], total, mi + abs(float(const[s])))):
                new = (one - rate) * old + rate * ((one - al) * old + step)
                out[key][s] = new
                old8 = np.abs(np.asarray(old, dtype=np.float64))
                out["mag_" + key][s] = (1.0 - lr) * old8 + lr * ((1.0 - alpha) * old8 + mag) + np.abs(np.asarray(new, dtype=np.float64))
    return out


# ---- inputs for the tests of the two passes ----------------------------------------------------------------------------------------
OBSERVED = dict(L.OBSERVED)
OBSERVED[L.POISSON] = (0.0, 1.0, 5.0, 9.0)      # (y = 40 of likelihood_closed_forms.OBSERVED: the 20-node g2 makes 1 + fvar g2 < 0 there)


def random_case(name, two_d, layout, seed=0):
    """Inputs for ``segment_pep_update`` on ``len(layout)`` series whose segment lengths are the rows of ``layout``: projections in
    (-0.7, 0.7), c in (0.02, 0.1), cavities with a mean of order 0.3 and a covariance of order 0.2 / 2d - fvar then stays below about
    0.4 at every 2d, where 1 + fvar g2 is at least 0.1 for the four likelihoods on ``OBSERVED`` (the tests assert it) - and random
    sites (nat2 negative definite), log_norm and seg_const.  A dict of float64 arrays."""
    rng = np.random.default_rng(1000 * two_d + seed)
    bsz, segs, n = len(layout), len(layout[0]), int(np.sum(layout[0]))
    assert all(int(np.sum(ln)) == n for ln in layout)
    d = dict(offsets=np.stack([np.concatenate([[0], np.cumsum(ln)]) for ln in layout]).astype(np.int64))
    d["indices"] = np.stack([np.repeat(np.arange(segs), ln) for ln in layout]).reshape(bsz, n)
    d["w"] = rng.uniform(-0.7, 0.7, size=(bsz, n, two_d))
    d["c"] = rng.uniform(0.02, 0.1, size=(bsz, n))
    a = rng.normal(size=(bsz, segs, two_d, two_d))
    d["cav_cov"] = (0.2 / two_d) * (a @ a.transpose(0, 1, 3, 2) / two_d + 0.1 * np.eye(two_d))
    d["cav_mean"] = 0.3 * rng.normal(size=(bsz, segs, two_d))
    d["y"] = np.resize(np.asarray(OBSERVED[name]), (bsz, n)).astype(np.float64)
    d["nat1"] = rng.normal(size=(bsz, segs, two_d))
    b = rng.normal(size=(bsz, segs, two_d, two_d))
    m = b @ b.transpose(0, 1, 3, 2)
    d["nat2"] = -0.5 * (m + m.transpose(0, 1, 3, 2))
    d["log_norm"] = rng.normal(size=(bsz, segs))
    d["seg_const"] = rng.normal(size=(bsz, segs))
    return d


# ---- the dense sparse power-EP loop ------------------------------------------------------------------------------------------------
def log_partition(kuu, nat1, nat2, d):
    """``log Z`` of ``p(u) prod_m t_m(v_m)`` without the sites' ``log_norm`` and up to the prior's constant:
    ``(log det Sigma - log det K_uu + lin^T Sigma lin) / 2`` with ``q = N(Sigma lin, Sigma)`` (the prior mean is zero)."""
    mu, sigma = SC.dense_posterior(kuu, nat1, nat2, d)
    lin = np.linalg.solve(sigma, mu)
    return 0.5 * (np.linalg.slogdet(sigma)[1] - np.linalg.slogdet(kuu)[1] + lin @ mu)


def pair_cavity(pm, pc, nat1, nat2, beta):
    """The cavity of every pair by dense inverses: precision ``S^-1 + 2 beta nat2``, linear term ``S^-1 m - beta nat1``; and
    ``Gamma = G(m_c, S_c) - G(m, S)``, ``G(m, S) = (log det S + m^T S^-1 m) / 2``."""
    cm, cc, gamma = np.zeros_like(pm), np.zeros_like(pc), np.zeros(len(pm))
    for s in range(len(pm)):
        prec = np.linalg.inv(pc[s])
        cprec = prec + 2.0 * beta[s] * nat2[s]
        cprec = 0.5 * (cprec + cprec.T)
        assert np.linalg.eigvalsh(cprec).min() > 0.0, "the cavity of the dense run must exist"
        cc[s] = np.linalg.inv(cprec)
        cc[s] = 0.5 * (cc[s] + cc[s].T)
        clin = prec @ pm[s] - beta[s] * nat1[s]
        cm[s] = cc[s] @ clin
        gamma[s] = (0.5 * (np.linalg.slogdet(cc[s])[1] + cm[s] @ clin)
                    - 0.5 * (np.linalg.slogdet(pc[s])[1] + pm[s] @ prec @ pm[s]))
    return cm, cc, gamma


class DenseSparsePEP:
    """The dense loop's state for one series: ``step()`` is one ``update_sites``; ``log_norms()`` the per-segment normalisers of the
    current q with the LEAVE-ONE-OUT ratio; ``energy()``, ``predict_f(t_new)``, ``cavity_f()``."""

    def __init__(self, lik, comps, x, y, z, alpha, lr, nq=20):
        self.lik, self.comps, self.alpha, self.lr, self.nq = lik, comps, alpha, lr, nq
        self.x, self.y, self.z = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(z, dtype=np.float64)
        self.d = SC.state_dim(comps)
        self.kuu = SC.dense_state_prior(comps, self.z)
        self.pinf = SC._transition(comps, 1.0)[2]
        self.idx, self.w, self.c = SC.conditional_projections(comps, self.x, self.z)
        segs = len(self.z) + 1
        self.offsets = SC.offsets_of(self.idx, segs)
        self.counts = np.diff(self.offsets).astype(np.float64)
        self.beta = np.where(self.counts > 0, alpha / np.maximum(self.counts, 1.0), 0.0)
        self.nat1, self.nat2 = np.zeros((segs, 2 * self.d)), np.zeros((segs, 2 * self.d, 2 * self.d))
        self.log_norm = np.zeros(segs)

    def posterior(self):
        return SC.dense_posterior(self.kuu, self.nat1, self.nat2, self.d)

    def cavity(self):
        mu, sigma = self.posterior()
        pm, pc = SC.pair_marginals(mu, sigma, self.pinf, self.d)
        return pair_cavity(pm, pc, self.nat1, self.nat2, self.beta)

    def leave_one_out(self):
        """``log Z(q with t_m^(1 - beta_m)) - log Z(q)`` per segment, each from its own dense posterior."""
        full = log_partition(self.kuu, self.nat1, self.nat2, self.d)
        out = np.zeros(len(self.beta))
        for m in range(len(self.beta)):
            n1, n2 = self.nat1.copy(), self.nat2.copy()
            n1[m] *= 1.0 - self.beta[m]
            n2[m] *= 1.0 - self.beta[m]
            out[m] = log_partition(self.kuu, n1, n2, self.d) - full
        return out

    def _update(self, lr, seg_const):
        cm, cc, _ = self.cavity()
        return segment_pep_update(self.lik, self.w, self.c, self.y, self.offsets, cm, cc, self.alpha, lr, self.nat1, self.nat2,
                                  self.log_norm, seg_const, self.nq)

    def step(self):
        out = self._update(self.lr, self.counts * self.leave_one_out())
        assert not out["skipped"].any(), "the reference run skipped a segment"
        self.nat1, self.nat2, self.log_norm = out["nat1"], out["nat2"], out["log_norm"]

    def log_norms(self):
        return self._update(0.0, None)["led_sum"] + self.counts * self.leave_one_out()

    def energy(self):
        return log_partition(self.kuu, self.nat1, self.nat2, self.d) + np.sum(self.log_norms()) / self.alpha

    def cavity_f(self):
        out = self._update(0.0, None)
        return out["fmu"], out["fvar"]

    def predict_f(self, t_new):
        mu, sigma = self.posterior()
        pm, pc = SC.pair_marginals(mu, sigma, self.pinf, self.d)
        idx, w, c = SC.conditional_projections(self.comps, np.asarray(t_new), self.z)
        return np.einsum("ki,ki->k", w, pm[idx]), c + np.einsum("ki,kij,kj->k", w, pc[idx], w)


def dense_sparse_pep(lik, comps, x, y, z, alpha, lr, iterations, nq=20, record=()):
    """Run the dense loop; ``{iteration: dict(nat1, nat2, log_norm, energy)}`` for the (1-based) iterations in ``record`` - the state
    AFTER that update, the energy of the q after it - and the final ``DenseSparsePEP``."""
    run = DenseSparsePEP(lik, comps, x, y, z, alpha, lr, nq)
    out = {}
    for it in range(1, iterations + 1):
        run.step()
        if it in record:
            out[it] = dict(nat1=run.nat1.copy(), nat2=run.nat2.copy(), log_norm=run.log_norm.copy(), energy=run.energy())
    return out, run
