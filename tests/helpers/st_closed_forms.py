"""
Reference of the spatio-temporal sparse variational model - TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Independent of markovflow_amd/models/spatio_temporal.py, markovflow_amd/kernels.py and csrc/mf_st.hip:

  * ``st_expectations``: the formulas of ``mf_lik_st_expectations_*`` for one series in numpy, in the kernel's summation order
    (include/markovflow_amd.h), in any numpy float type, with the magnitude ``sum |terms|`` of every output.  The likelihood's own
    expectations come from ``likelihood_closed_forms.expectations``, which scipy evaluates in float64 at most: with
    ``dtype = numpy.longdouble`` the projection, the contractions and every sum run in long double and the three expectations of a
    point are float64 numbers of long-double arguments;
  * ``reference_route``: what the reference's ``space_time_predict_f`` computes - the marginal of the state at ``t_k``, the
    covariance of the ``Ms`` outputs, its Cholesky factor and the base conditional - written from the formulas;
  * ``dense_gpr``: the exact log marginal likelihood and predictive mean of GP regression with a product kernel, dense.

A likelihood is the ``(name, params)`` tuple of likelihood_closed_forms.py.
"""
import numpy as np

from helpers import likelihood_closed_forms as L

TILE = 256          # points per workspace row of mf_lik_st_expectations_*: fixes the order of the segment sums


def kron_rows(a, wt):
    """``W [N, 2 Ms d_t]`` with ``W[k, half D + s d_t + i] = a[k, s] wt[k, half d_t + i]``."""
    n, ms = a.shape
    dt = wt.shape[1] // 2
    return (wt.reshape(n, 2, 1, dt) * a[:, None, :, None]).reshape(n, 2 * ms * dt)


def _in_order(terms, ty):
    return np.cumsum(terms, axis=0, dtype=ty)[-1]           # numpy accumulates one after the other


def st_expectations(lik, a, wt, c, y, offsets, pair_mean, pair_cov, nq=20, dtype=np.float64):
    """One series.  ``a [N, Ms]``, ``wt [N, 2 d_t]``, ``c [N]``, ``y [N]``, ``offsets [S + 1]``, ``pair_mean [S, n]``,
    ``pair_cov [S, n, n]`` with ``n = 2 Ms d_t``.  Returns a dict with ``fmu``, ``fvar``, ``g_a``, ``g_wt``, ``g_c`` per point and
    ``ve_sum``, ``g_mean``, ``g_cov`` per segment, in ``dtype``, and ``mag_<name>`` (float64) for each: the sum of the absolute values
    of the terms the output is made of."""
    ty = dtype
    a, wt, c, y, pair_mean, pair_cov = (np.asarray(v, dtype=ty) for v in (a, wt, c, y, pair_mean, pair_cov))
    npts, ms = a.shape
    dt = wt.shape[1] // 2
    big_d, pair, segs = ms * dt, 2 * ms * dt, len(offsets) - 1
    seg = np.repeat(np.arange(segs), np.diff(np.asarray(offsets)))
    assert seg.shape[0] == npts and offsets[0] == 0 and offsets[-1] == npts
    w = kron_rows(a, wt)
    sbar = ty(0.5) * (pair_cov + pair_cov.transpose(0, 2, 1))
    m = pair_mean[seg]                                       # [N, n]
    absw, abss, absm = (np.abs(v.astype(np.float64)) for v in (w, sbar, pair_mean))
    # V_k[i] = sum_j Sbar[i, j] W_k[j] in j; fmu and W . V in the pair index
    v = np.zeros((npts, pair), dtype=ty)
    mag_v = np.zeros((npts, pair))
    for s in range(segs):
        k = slice(offsets[s], offsets[s + 1])
        for j in range(pair):
            v[k] = v[k] + sbar[s, :, j][None, :] * w[k, j][:, None]
        mag_v[k] = absw[k] @ abss[s].T
    fmu, quad = np.zeros(npts, dtype=ty), np.zeros(npts, dtype=ty)
    for j in range(pair):
        fmu = fmu + w[:, j] * m[:, j]
        quad = quad + w[:, j] * v[:, j]
    fvar = c + quad
    out = dict(fmu=fmu, fvar=fvar, mag_fmu=np.sum(absw * absm[seg], axis=1),
               mag_fvar=np.abs(c.astype(np.float64)) + np.sum(absw * mag_v, axis=1))
    if npts:
        args = (fmu, fvar, y) if ty != np.longdouble else tuple(x.astype(np.float64) for x in (fmu, fvar, y))
        (ve, gm, gv), mags = L.expectations(lik, *args, nq, dtype=ty if ty != np.longdouble else np.float64)
        ve, gm, gv = (x.astype(ty) for x in (ve, gm, gv))
    else:
        ve = gm = gv = np.zeros(0, dtype=ty)
        mags = (np.zeros(0),) * 3
    # the contractions of m and V with wt (onto a) and with a (onto wt), each in the pair index of its terms
    m4, v4 = m.reshape(npts, 2, ms, dt), v.reshape(npts, 2, ms, dt)
    wt3 = wt.reshape(npts, 2, dt)
    contract_a = lambda x: _sum_axes(x * wt3[:, :, None, :], (1, 3), ty)           # noqa: E731  [N, Ms]
    contract_wt = lambda x: _sum_axes(x * a[:, None, :, None], (2,), ty).reshape(npts, 2 * dt)      # noqa: E731
    ma, va, mwt, vwt = contract_a(m4), contract_a(v4), contract_wt(m4), contract_wt(v4)
    two = ty(2)
    out["g_a"] = (two * gv)[:, None] * va + (gm[:, None] * ma)
    out["g_wt"] = (two * gv)[:, None] * vwt + (gm[:, None] * mwt)
    out["g_c"] = gv
    am4, av4 = absm[seg].reshape(npts, 2, ms, dt), mag_v.reshape(npts, 2, ms, dt)
    awt3, aa = np.abs(wt3.astype(np.float64)), np.abs(a.astype(np.float64))
    mag_a = lambda x: np.sum(x * awt3[:, :, None, :], axis=(1, 3))                 # noqa: E731
    mag_wt = lambda x: np.sum(x * aa[:, None, :, None], axis=2).reshape(npts, 2 * dt)          # noqa: E731
    out["mag_g_a"] = mags[1][:, None] * mag_a(am4) + 2 * mags[2][:, None] * mag_a(av4)
    out["mag_g_wt"] = mags[1][:, None] * mag_wt(am4) + 2 * mags[2][:, None] * mag_wt(av4)
    out["mag_g_c"] = mags[2]
    out.update(ve_sum=np.zeros(segs, dtype=ty), g_mean=np.zeros((segs, pair), dtype=ty), g_cov=np.zeros((segs, pair, pair), dtype=ty),
               mag_ve_sum=np.zeros(segs), mag_g_mean=np.zeros((segs, pair)), mag_g_cov=np.zeros((segs, pair, pair)))
    lower = np.tril(np.ones((pair, pair), dtype=bool))
    for s in range(segs):
        rows = [slice(k0, min(k0 + TILE, offsets[s + 1])) for k0 in range(offsets[s], offsets[s + 1], TILE)]
        if rows:
            out["ve_sum"][s] = _in_order(np.stack([_in_order(ve[k], ty) for k in rows]), ty)
            out["g_mean"][s] = _in_order(np.stack([_in_order(gm[k, None] * w[k], ty) for k in rows]), ty)
            # (gv W_i) W_j for i >= j, mirrored
            tri = _in_order(np.stack([_in_order((gv[k, None] * w[k])[:, :, None] * w[k][:, None, :], ty) for k in rows]), ty)
            out["g_cov"][s] = np.where(lower, tri, tri.T)
        k = slice(offsets[s], offsets[s + 1])
        out["mag_ve_sum"][s] = np.sum(mags[0][k])
        out["mag_g_mean"][s] = np.einsum("k,ki->i", mags[1][k], absw[k])
        out["mag_g_cov"][s] = np.einsum("k,ki,kj->ij", mags[2][k], absw[k], absw[k])
    assert big_d * 2 == pair
    return out


def _sum_axes(x, axes, ty):
    """Sum over ``axes`` term after term, the first of them outermost."""
    x = np.moveaxis(x, axes, tuple(range(len(axes))))
    x = x.reshape((-1,) + x.shape[len(axes):])
    return _in_order(x, ty)


def reference_route(kmm, kmn, knn, h, proj, cov, pair_mean, pair_cov):
    """The reference's route for ONE point: ``kmm [Ms, Ms]``, ``kmn [Ms]``, ``knn`` the spatial kernel; ``h [d_t]``, ``proj [d_t,
    2 d_t]``, ``cov [d_t, d_t]`` the temporal emission row and conditional statistics of the point; ``pair_mean [n]``, ``pair_cov
    [n, n]`` the marginal of the pair of chain states (copy ``s`` of the temporal state in columns ``s d_t ...``).  The marginal of
    the state at the point, the ``Ms`` outputs ``u = L (I (x) h) s``, the Cholesky factor of their covariance and the base
    conditional.  Returns ``(mean, variance)``."""
    ms, dt = kmm.shape[0], h.shape[0]
    big_d = ms * dt
    eye = np.eye(ms)
    # the pair is [left state; right state], each Ms copies: the conditional acts copy by copy
    big_p = np.concatenate([np.kron(eye, proj[:, :dt]), np.kron(eye, proj[:, dt:])], axis=1)          # [D, 2D]
    assert big_p.shape == (big_d, 2 * big_d)
    sym = 0.5 * (pair_cov + pair_cov.T)
    mean_s = big_p @ pair_mean
    cov_s = np.kron(eye, cov) + big_p @ sym @ big_p.T
    chol_mm = np.linalg.cholesky(kmm)
    emit = chol_mm @ np.kron(eye, h[None, :])                # [Ms, D]
    mean_u, cov_u = emit @ mean_s, emit @ cov_s @ emit.T
    q_sqrt = np.linalg.cholesky(0.5 * (cov_u + cov_u.T))
    amat = np.linalg.solve(chol_mm, kmn)                     # L^-1 K_mn
    var = knn - amat @ amat
    amat = np.linalg.solve(chol_mm.T, amat)                  # K_mm^-1 K_mn
    return amat @ mean_u, var + np.sum((q_sqrt.T @ amat) ** 2)


def dense_gpr(kmat, y, noise, kstar=None):
    """Exact GP regression: the log marginal likelihood of ``y`` under ``N(0, kmat + noise I)`` and, with ``kstar [N*, N]``, the
    predictive mean."""
    n = len(y)
    chol = np.linalg.cholesky(kmat + noise * np.eye(n))
    alpha = np.linalg.solve(chol.T, np.linalg.solve(chol, y))
    lml = -0.5 * y @ alpha - np.sum(np.log(np.diag(chol))) - 0.5 * n * np.log(2 * np.pi)
    return lml, (None if kstar is None else kstar @ alpha)
