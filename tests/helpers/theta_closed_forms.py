"""
Reference of the SVGP data term with the adjoint onto the likelihood's parameter theta (Gaussian: the variance, Student-t: the scale)
- TEST INFRASTRUCTURE, independent of the product code.  Per point  fmu = w . m_s,  fvar = c + w^T S_s w,  (ve, gm, gv, gt = d ve / d theta);
per segment  ve_sum = sum ve,  g_mean = sum gm w,  g_cov = sum gv w w^T,  g_theta = sum gt.
"""
import math

import numpy as np

TILE = 64


def segment_expectations_theta(lik, theta, w, c, y, offsets, pair_mean, pair_cov, dtype=np.float64, df=3.0, nq=20):
    """One series (``w [N, 2d]``, ``c``, ``y [N]``, ``offsets [S + 1]``, ``theta`` a number; ``lik``: 0 Gaussian, 3 Student-t) in
    ``dtype``, the sums in the kernel's order (points ascending in tiles of 64, then the tiles).  Returns the four sums, ``mag_*`` -
    the sums of the absolute values of their per-point terms - and ``fvar``."""
    ty = dtype
    w, c, y, pair_mean, pair_cov = (np.asarray(a, dtype=ty) for a in (w, c, y, pair_mean, pair_cov))
    th = ty(theta)
    n, two_d = w.shape
    segs = len(offsets) - 1
    seg = np.repeat(np.arange(segs), np.diff(np.asarray(offsets)))
    assert seg.shape[0] == n
    m, cov = pair_mean[seg], pair_cov[seg]
    fmu = np.einsum("ki,ki->k", w, m).astype(ty)
    fvar = (c + np.einsum("ki,kij,kj->k", w, cov, w)).astype(ty)
    r = y - fmu
    if lik == 0:
        ve = ty(-0.5) * (ty(math.log(2 * math.pi)) + np.log(th)) - ty(0.5) * (r * r + fvar) / th
        gm, gv = r / th, np.full(n, ty(-0.5) / th, dtype=ty)
        gt = ty(0.5) / th * ((r * r + fvar) / th - ty(1))
    else:
        x, wq = np.polynomial.hermite.hermgauss(nq)
        x, wq = x.astype(ty), (wq / math.sqrt(math.pi)).astype(ty)
        const = ty(math.lgamma(0.5 * (df + 1)) - math.lgamma(0.5 * df) - 0.5 * math.log(df * math.pi)) - np.log(th)
        sd = np.sqrt(ty(2) * fvar)
        ri = y[:, None] - (fmu[:, None] + sd[:, None] * x)                   # [N, nq]
        a = ty(df) * th * th
        l = const - ty(0.5 * (df + 1)) * np.log1p(ri * ri / a)
        dl = ty(df + 1) * ri / (a + ri * ri)
        ve, gm = (l * wq).sum(-1, dtype=ty), (dl * wq).sum(-1, dtype=ty)
        gv = (dl * x * wq).sum(-1, dtype=ty) / sd
        gt = ((dl * ri - ty(1)) * wq).sum(-1, dtype=ty) / th
    terms = dict(ve_sum=ve, g_mean=gm[:, None] * w, g_cov=gv[:, None, None] * w[:, :, None] * w[:, None, :], g_theta=gt)
    in_order = lambda t: np.cumsum(t, axis=0, dtype=ty)[-1]                  # noqa: E731  (numpy accumulates one after the other)
    out = dict(fvar=fvar)
    for key, t in terms.items():
        out[key] = np.zeros((segs,) + t.shape[1:], dtype=ty)
        out["mag_" + key] = np.zeros((segs,) + t.shape[1:])
        for s in range(segs):
            tiles = [slice(k0, min(k0 + TILE, offsets[s + 1])) for k0 in range(offsets[s], offsets[s + 1], TILE)]
            if tiles:
                out[key][s] = in_order(np.stack([in_order(t[k]) for k in tiles]))
            out["mag_" + key][s] = np.abs(t[offsets[s]:offsets[s + 1]].astype(np.float64)).sum(axis=0)
    return out
