"""
numpy reference of the conditional-prediction kernels (csrc/mf_kernels.hpp: ``sde_cond_stats_kernel``, ``sde_predict_kernel``) -
TEST INFRASTRUCTURE, NOT PRODUCT CODE.

  * ``statistics``: ``(D, E, T)`` of ``p(x_t | x_-, x_+) = N(D x_- + E x_+, T)`` from the transitions ``x_- -> x_t`` (``A_mt, Q_mt``) and
    ``x_t -> x_+`` (``A_tp, Q_tp``):  ``G = A_tp Q_mt``, ``S = Q_tp + G A_tp^T``, ``E = G^T S^-1``, ``D = A_mt - E A_tp A_mt``,
    ``T = Q_mt - G^T S^-1 G``;
  * ``predict``: the marginal of ``x_t`` for one series from the pair marginal of its two neighbours,
    ``mean = D mu_- + E mu_+``, ``cov = T + D P_- D^T + E P_+ E^T + E C D^T + (E C D^T)^T`` with ``C = Cov(x_+, x_-)``; insertion index 0
    pairs (prior, x_0), index N pairs (x_{N-1}, prior), without a cross term at either end;
  * ``draw_statistics_inputs`` / ``draw_predict_inputs``: the random, well-conditioned inputs the host and the GPU tests share.

Everything is evaluated in the numpy ``dtype`` asked for (float32, float64, longdouble) with a hand-written Cholesky - no LAPACK, which
has no long double.  Next to every result comes its magnitude (always float64): the same expression with every factor replaced by
its absolute value, ``|S^-1|`` entrywise - the scale of a rounding-error bound ``K eps (magnitude + 1)``.
tests/test_conditional_closed_forms_host.py pins these functions on direct Gaussian conditioning of the joint of (x_-, x_t, x_+).
"""
import numpy as np


def _t(a):
    return np.swapaxes(a, -1, -2)


def cholesky_lower(s):
    """Lower Cholesky factor of ``s [n, d, d]`` in ``s.dtype``, column by column; a non-positive pivot leaves NaN behind it."""
    n, d, _ = s.shape
    low = np.zeros_like(s)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(d):
            piv = s[:, j, j] - np.sum(low[:, j, :j] * low[:, j, :j], axis=-1, dtype=s.dtype)
            low[:, j, j] = np.sqrt(piv)
            for i in range(j + 1, d):
                low[:, i, j] = (s[:, i, j] - np.sum(low[:, i, :j] * low[:, j, :j], axis=-1, dtype=s.dtype)) / low[:, j, j]
    return low


def inverse_spd(s):
    """``s^-1`` of symmetric positive definite ``s [n, d, d]`` in ``s.dtype``: ``L^-T L^-1`` by forward substitution on the identity."""
    n, d, _ = s.shape
    low = cholesky_lower(s)
    inv_low = np.zeros_like(s)
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in range(d):
            for r in range(c, d):
                rhs = (s.dtype.type(1) if r == c else s.dtype.type(0)) - np.sum(low[:, r, c:r] * inv_low[:, c:r, c], axis=-1, dtype=s.dtype)
                inv_low[:, r, c] = rhs / low[:, r, r]
        return _t(inv_low) @ inv_low


def statistics(a_mt, q_mt, a_tp, q_tp, dtype=np.float64):
    """``(D, E, T), (|D|, |E|, |T|)`` for inputs ``[n, d, d]`` (or one ``[d, d]`` point), evaluated in ``dtype``."""
    single = np.ndim(a_mt) == 2
    a_mt, q_mt, a_tp, q_tp = (np.asarray(x, dtype=dtype).reshape((-1,) + np.shape(x)[-2:]) for x in (a_mt, q_mt, a_tp, q_tp))
    with np.errstate(invalid="ignore"):
        g = a_tp @ q_mt
        s_inv = inverse_spd(q_tp + g @ _t(a_tp))
        e_m = _t(g) @ s_inv
        d_m = a_mt - e_m @ a_tp @ a_mt
        t_m = q_mt - e_m @ g
        t_m = (t_m + _t(t_m)) * dtype(0.5)
        f8 = lambda x: np.abs(x.astype(np.float64))                       # noqa: E731
        mag_g = f8(a_tp) @ f8(q_mt)
        mag_e = _t(mag_g) @ f8(s_inv)
        mag_d = f8(a_mt) + mag_e @ f8(a_tp) @ f8(a_mt)
        mag_t = f8(q_mt) + mag_e @ mag_g
    out, mags = (d_m, e_m, t_m), (mag_d, mag_e, mag_t)
    if single:
        out, mags = tuple(x[0] for x in out), tuple(x[0] for x in mags)
    return out, mags


def predict(idx, a_mt, q_mt, a_tp, q_tp, means, covs, sub, m0, p0, dtype=np.float64):
    """One series: ``idx [Np]`` (0 .. N), transitions ``[Np, d, d]``, ``means [N, d]``, ``covs [N, d, d]``, ``sub [N - 1, d, d]`` =
    ``Cov(x_{k+1}, x_k)`` (None for N = 1), the prior ``m0 [d]``, ``p0 [d, d]``.  Returns ``(mean, cov), (|mean|, |cov|)``; with
    ``covs = None`` the covariance and its magnitude are None."""
    idx = np.asarray(idx, dtype=np.int64)
    n = np.shape(means)[0]
    assert idx.ndim == 1 and idx.min(initial=0) >= 0 and idx.max(initial=0) <= n
    (d_m, e_m, t_m), (mag_d, mag_e, mag_t) = statistics(a_mt, q_mt, a_tp, q_tp, dtype)
    means, m0 = np.asarray(means, dtype=dtype), np.asarray(m0, dtype=dtype)
    has_m, has_p = idx > 0, idx < n
    left, right = np.clip(idx - 1, 0, n - 1), np.clip(idx, 0, n - 1)
    f8 = lambda x: np.abs(x.astype(np.float64))                           # noqa: E731
    mu_m = np.where(has_m[:, None], means[left], m0[None])
    mu_p = np.where(has_p[:, None], means[right], m0[None])
    mean = (d_m @ mu_m[..., None] + e_m @ mu_p[..., None])[..., 0]
    mag_mean = (mag_d @ f8(mu_m)[..., None] + mag_e @ f8(mu_p)[..., None])[..., 0]
    if covs is None:
        return (mean, None), (mag_mean, None)
    covs, p0 = np.asarray(covs, dtype=dtype), np.asarray(p0, dtype=dtype)
    p_m = np.where(has_m[:, None, None], covs[left], p0[None])
    p_p = np.where(has_p[:, None, None], covs[right], p0[None])
    cross = np.zeros_like(p_m)                                            # C = Cov(x_+, x_-), zero at both ends
    both = has_m & has_p
    if both.any():
        cross[both] = np.asarray(sub, dtype=dtype)[idx[both] - 1]
    ecd = e_m @ cross @ _t(d_m)
    cov = t_m + d_m @ p_m @ _t(d_m) + e_m @ p_p @ _t(e_m) + ecd + _t(ecd)
    mag_ecd = mag_e @ f8(cross) @ _t(mag_d)
    mag_cov = mag_t + mag_d @ f8(p_m) @ _t(mag_d) + mag_e @ f8(p_p) @ _t(mag_e) + mag_ecd + _t(mag_ecd)
    return (mean, cov), (mag_mean, mag_cov)


# ---- shared inputs -----------------------------------------------------------------------------------------------------------------
def _spd(rng, lead, d):
    w = rng.normal(size=lead + (d, d))
    s = w @ _t(w) / d + 0.5 * np.eye(d)
    return 0.5 * (s + _t(s))                                              # (a batched product is symmetric only to rounding)


def draw_statistics_inputs(rng, n, d):
    """``(A_mt, Q_mt, A_tp, Q_tp)``, each ``[n, d, d]``, well conditioned on purpose: ``A = 0.7 randn / sqrt(d)``, ``Q = W W^T / d + I / 2``."""
    a = lambda: 0.7 * rng.normal(size=(n, d, d)) / np.sqrt(d)             # noqa: E731
    a_mt, q_mt = a(), _spd(rng, (n,), d)
    a_tp, q_tp = a(), _spd(rng, (n,), d)
    return a_mt, q_mt, a_tp, q_tp


def draw_predict_inputs(rng, bsz, n, n_new, d):
    """A dict of the fused kernel's inputs for ``bsz`` series: ``idx [B, Np]`` (every series covers 0 .. N when Np > N, in shuffled
    order), the four transitions ``[B, Np, d, d]``, and moments that differ from series to series: ``means [B, N, d]``, ``covs``, ``sub``
    (``[B, N - 1, d, d]``, None for N = 1) cut from one random SPD ``2d x 2d`` pair marginal per (series, k): ``P_- = covs[k]`` from the
    upper block, ``P_+`` from the lower, ``C`` the lower left - and the prior ``m0 [B, d]``, ``p0 [B, d, d]``."""
    idx = np.stack([rng.permutation(np.concatenate([np.arange(n + 1), rng.integers(0, n + 1, size=max(0, n_new - n - 1))]))[:n_new]
                    for _ in range(bsz)]).astype(np.int64).reshape(bsz, n_new)
    a_mt, q_mt, a_tp, q_tp = (x.reshape(bsz, n_new, d, d) for x in draw_statistics_inputs(rng, bsz * n_new, d))
    # chain the pair marginals: pair k = (x_k, x_{k+1}) is a random SPD 2d x 2d matrix whose upper block is rescaled onto the lower
    # block of pair k - 1 by a congruence, which keeps every pair positive definite and every block generic
    covs = np.empty((bsz, n, d, d))
    sub = np.empty((bsz, n - 1, d, d)) if n > 1 else None
    covs[:, 0] = _spd(rng, (bsz,), d)
    for k in range(n - 1):
        pair = _spd(rng, (bsz,), 2 * d)
        # M = chol(covs[k]) chol(pair_11)^-1 maps pair_11 onto covs[k]; apply diag(M, I) to the pair
        m = np.linalg.cholesky(covs[:, k]) @ np.linalg.inv(np.linalg.cholesky(pair[:, :d, :d]))
        sub[:, k] = pair[:, d:, :d] @ _t(m)
        covs[:, k + 1] = pair[:, d:, d:]
    return dict(idx=idx, a_mt=a_mt, q_mt=q_mt, a_tp=a_tp, q_tp=q_tp, means=rng.normal(size=(bsz, n, d)), covs=covs, sub=sub,
                m0=rng.normal(size=(bsz, d)), p0=_spd(rng, (bsz,), d))


PREDICT_KEYS = ("a_mt", "q_mt", "a_tp", "q_tp", "means", "covs", "sub", "m0", "p0")


def predict_series(case, b, dtype=np.float64, with_cov=True):
    """``predict`` on series ``b`` of a ``draw_predict_inputs`` dict."""
    args = [None if case[k] is None else case[k][b] for k in PREDICT_KEYS]
    if not with_cov:
        args[5] = args[6] = args[8] = None
    return predict(case["idx"][b], *args, dtype=dtype)
