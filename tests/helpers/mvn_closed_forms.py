"""
Reference of the SVGP data term under a MultivariateGaussian likelihood - TEST INFRASTRUCTURE, independent of the product code.
Per point k of pair s, with w_k [P, 2d], the full C_k [P, P] and ONE precision Lam [P, P]:
    mu = w m_s      F = C + w S_s w^T      r = y - mu      v = Lam r      quad_k = r . v + <Lam, F>
    quad_sum[s] = sum_k quad_k     g_mean[s] = sum_k w^T v     g_cov[s] = -1/2 sum_k w^T Lam w     m_sum[s] = sum_k (r r^T + F)
"""
import numpy as np

TILE = 64


def segment_expectations_mvn(w, c, y, prec, offsets, pair_mean, pair_cov, dtype=np.float64):
    """One series (``w [N, P, 2d]``, ``c [N, P, P]``, ``y [N, P]``, ``prec [P, P]``, ``offsets [S + 1]``, ``pair_mean [S, 2d]``,
    ``pair_cov [S, 2d, 2d]``) in float64 or, ``dtype=np.float32``, in numpy float32 in the kernel's order of summation (points ascending
    in tiles of 64, then the tiles).  Returns the four sums in ``dtype`` and ``mag_*``, the sums of the absolute values of their terms."""
    ty = dtype
    w, c, y, prec, pair_mean, pair_cov = (np.asarray(a, dtype=ty) for a in (w, c, y, prec, pair_mean, pair_cov))
    n, outs, two_d = w.shape
    segs = len(offsets) - 1
    seg = np.repeat(np.arange(segs), np.diff(np.asarray(offsets)))
    assert seg.shape[0] == n and offsets[0] == 0 and offsets[-1] == n and c.shape == (n, outs, outs) and y.shape == (n, outs)
    m, cov = pair_mean[seg], pair_cov[seg]
    mu, f = np.zeros((n, outs), dtype=ty), c.copy()
    for i in range(two_d):                       # the kernel's walk over the rows of S_s
        for p in range(outs):
            acc = np.zeros(n, dtype=ty)
            for col in range(two_d):
                acc = acc + cov[:, i, col] * w[:, p, col]
            mu[:, p] = mu[:, p] + w[:, p, i] * m[:, i]
            for q in range(outs):
                f[:, p, q] = f[:, p, q] + w[:, q, i] * acc
    f = np.tril(f) + np.tril(f, -1).transpose(0, 2, 1)           # the lower triangle is the one the kernel keeps
    r = y - mu
    v = np.zeros((n, outs), dtype=ty)
    for q in range(outs):
        v = v + prec[None, :, q] * r[:, q, None]
    pairs = [(p, q) for p in range(outs) for q in range(p + 1)]
    quad_terms = np.stack([r[:, p] * v[:, p] for p in range(outs)]
                          + [(prec[p, q] if p == q else ty(2) * prec[p, q]) * f[:, p, q] for p, q in pairs], axis=1)
    in_order = lambda terms: np.cumsum(terms, axis=0, dtype=ty)[-1]          # noqa: E731  (numpy accumulates one after the other)
    quad = in_order(quad_terms.T) if n else np.zeros(0, dtype=ty)
    mm = r[:, :, None] * r[:, None, :] + f                                   # [N, P, P]
    half = ty(-0.5)
    cov_terms = np.stack([(half * prec[p, p]) * (w[:, p, :, None] * w[:, p, None, :]) if p == q else
                          (half * prec[p, q]) * (w[:, p, :, None] * w[:, q, None, :] + w[:, q, :, None] * w[:, p, None, :])
                          for p, q in pairs], axis=1)                        # [N, pairs, 2d, 2d]
    mean_terms = v[:, :, None] * w                                           # [N, P, 2d]
    flat = lambda x: x.reshape((-1,) + x.shape[2:])                          # noqa: E731  ([points, terms, ...] -> point-major)
    w8, l8, r8 = np.abs(w.astype(np.float64)), np.abs(prec.astype(np.float64)), np.abs(y.astype(np.float64))
    r8 = r8 + np.einsum("kpi,ki->kp", w8, np.abs(m.astype(np.float64)))                               # |y| + |w| |m|
    f8 = np.abs(c.astype(np.float64)) + np.einsum("kpi,kij,kqj->kpq", w8, np.abs(cov.astype(np.float64)), w8)
    m8 = r8[:, :, None] * r8[:, None, :] + f8
    out = dict(quad_sum=np.zeros(segs, dtype=ty), g_mean=np.zeros((segs, two_d), dtype=ty), g_cov=np.zeros((segs, two_d, two_d), dtype=ty),
               m_sum=np.zeros((segs, outs, outs), dtype=ty), mag_quad_sum=np.zeros(segs), mag_g_mean=np.zeros((segs, two_d)),
               mag_g_cov=np.zeros((segs, two_d, two_d)), mag_m_sum=np.zeros((segs, outs, outs)))
    lower = np.tril(np.ones((two_d, two_d), dtype=bool))
    for s in range(segs):
        tiles = [slice(k0, min(k0 + TILE, offsets[s + 1])) for k0 in range(offsets[s], offsets[s + 1], TILE)]
        if tiles:
            out["quad_sum"][s] = in_order(np.stack([in_order(quad[k]) for k in tiles]))
            out["g_mean"][s] = in_order(np.stack([in_order(flat(mean_terms[k])) for k in tiles]))
            tri = in_order(np.stack([in_order(flat(cov_terms[k])) for k in tiles]))
            out["g_cov"][s] = np.where(lower, tri, tri.T)                    # the kernel sums the lower triangle and mirrors it
            out["m_sum"][s] = in_order(np.stack([in_order(mm[k]) for k in tiles]))
        k = slice(offsets[s], offsets[s + 1])
        out["mag_quad_sum"][s] = np.einsum("kp,pq,kq->", r8[k], l8, r8[k]) + np.einsum("pq,kpq->", l8, f8[k])
        out["mag_g_mean"][s] = np.einsum("kpi,pq,kq->i", w8[k], l8, r8[k])
        out["mag_g_cov"][s] = 0.5 * np.einsum("kpi,pq,kqj->ij", w8[k], l8, w8[k])
        out["mag_m_sum"][s] = np.sum(m8[k], axis=0)
    return out
