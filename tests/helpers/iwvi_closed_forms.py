"""
Reference of the data term of the importance weights - TEST INFRASTRUCTURE, NOT PRODUCT CODE.

``iw_log_weights``: the formulas of ``mf_lik_iw_log_weights_*`` for ONE series in numpy, on ``likelihood_closed_forms.log_prob`` /
``dlog_prob`` and the second derivatives stated here, independent of markovflow_amd/models/sparse.py and csrc/mf_lik.hip.  The sums run in
the kernel's order - the points of a tile of 64 ascending, then the tiles ascending, then the two segments of ``g_u`` in the stated
order - so that ``dtype`` = numpy.float32 carries the kernel's rounding.  ``dense_gaussian_logpdf`` evaluates a chain's density from
its dense moments.

A likelihood is the ``(name, params)`` tuple of likelihood_closed_forms.py.
"""
import numpy as np

from helpers import likelihood_closed_forms as L

TILE = 64           # points per tile of mf_lik_iw_log_weights_*: fixes the order of the sums


def d2log_prob(lik, f, y):
    """The second derivative of log p(y | f) in f (float64)."""
    name, params = lik
    f, y = np.asarray(f, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if name == L.GAUSSIAN:
        return np.full_like(f, -1.0 / params[0])
    if name == L.BERNOULLI:
        p = L.inv_probit(f)
        dp = (1 - 2 * L.JITTER) * np.exp(-0.5 * f * f) / np.sqrt(2 * np.pi)
        return -f * L.dlog_prob(lik, f, y) - dp * dp * (y / (p * p) + (1.0 - y) / ((1.0 - p) * (1.0 - p)))
    if name == L.POISSON:
        return -np.exp(f)
    scale, df = params
    a, r2 = df * scale * scale, (y - f) ** 2
    return -(df + 1) * (a - r2) / (a + r2) ** 2


def rows_of(offsets):
    """``(segment of every point [N], row of every point [N], row of every inducing point [M])`` in the merged layout: data point n
    of segment s at row n + s, inducing point m at row offsets[m + 1] + m."""
    offsets = np.asarray(offsets)
    segs = len(offsets) - 1
    seg = np.repeat(np.arange(segs), np.diff(offsets))
    return seg, np.arange(seg.shape[0]) + seg, offsets[1:-1] + np.arange(segs - 1)


def in_order(terms, dtype):
    """The sum of ``terms`` along axis 0, one after the other (numpy's cumsum does not reassociate)."""
    return np.cumsum(terms, axis=0, dtype=dtype)[-1]


def iw_log_weights(lik, h, w, y, offsets, states, u_post, dtype=np.float64):
    """One series.  ``h [d]``, ``w [N, 2d]``, ``y [N]``, ``offsets [S + 1]``, ``states [K, N + M, d]`` (a prior draw on the merged time
    points) and ``u_post [K, M, d]`` - or ``u_post`` None and ``states [K, N, d]``, final samples.  Returns a dict with
    ``log_lik [K, S]``, ``g_u [K, M, d]``, ``f``, ``l``, ``dl`` ``[K, N]`` and the magnitudes (always float64) that scale a rounding-error
    bound, with ``fmag_n = sum_i |h_i s_i| + sum_i |w_i| (|prior_i| + |u_i|)``:
    ``mag_log_lik = sum_n (|l_n| + |l'_n| fmag_n)``, ``mag_g_u = sum_n (|l'_n| + |l''_n| fmag_n) |w_n,.|``."""
    ty = dtype
    h, y, states = (np.asarray(a, dtype=ty) for a in (h, y, states))
    offsets = np.asarray(offsets)
    k, d, n, segs = states.shape[0], states.shape[-1], y.shape[0], len(offsets) - 1
    m = segs - 1
    seg, rows_x, rows_z = rows_of(offsets)
    assert seg.shape[0] == n and offsets[0] == 0 and offsets[-1] == n
    if u_post is None:
        prior = states
        w = np.zeros((n, 2 * d), dtype=ty)
        delta = np.zeros((k, m + 2, d), dtype=ty)
        u_mag = np.zeros((k, m + 2, d))
    else:
        w, u_post = np.asarray(w, dtype=ty), np.asarray(u_post, dtype=ty)
        prior = states[:, rows_x]
        zero = np.zeros((k, 1, d), dtype=ty)
        delta = np.concatenate([zero, states[:, rows_z] - u_post, zero], axis=1)
        u_mag = np.concatenate([zero, np.abs(states[:, rows_z]) + np.abs(u_post), zero], axis=1).astype(np.float64)
    # the kernel's order of evaluation: (h . prior - w_left . dL) - w_right . dR, each inner product term by term
    a, cl, cr = (np.zeros((k, n), dtype=ty) for _ in range(3))
    for i in range(d):
        a = a + h[i] * prior[:, :, i]
        cl = cl + w[None, :, i] * delta[:, seg, i]
        cr = cr + w[None, :, d + i] * delta[:, seg + 1, i]
    f = (a - cl) - cr if u_post is not None else a
    yk = np.broadcast_to(y, (k, n))
    with np.errstate(all="ignore"):
        if lik[0] == L.POISSON and ty == np.float64:
            from scipy import special
            l = yk * f - np.exp(f) - special.gammaln(yk + 1.0)          # (scipy's logpmf rejects a NaN rate)
        else:
            l = L.log_prob(lik, f, yk).astype(ty)
        dl = L.dlog_prob(lik, f, yk).astype(ty)
        d2l = d2log_prob(lik, f, yk)
    w8, h8, p8 = np.abs(w.astype(np.float64)), np.abs(h.astype(np.float64)), np.abs(prior.astype(np.float64))
    fmag = p8 @ h8 + np.einsum("ni,kni->kn", w8[:, :d], u_mag[:, seg]) + np.einsum("ni,kni->kn", w8[:, d:], u_mag[:, seg + 1])
    l8, dl8 = np.abs(l.astype(np.float64)), np.abs(dl.astype(np.float64))
    mag_l = l8 + dl8 * fmag
    mag_dl = dl8 + np.abs(d2l) * fmag
    out = dict(f=f, l=l, dl=dl, log_lik=np.zeros((k, segs), dtype=ty), g_u=np.zeros((k, m, d), dtype=ty),
               mag_log_lik=np.zeros((k, segs)), mag_g_u=np.zeros((k, m, d)))
    tile_sums = {}
    for s in range(segs):
        tiles = [slice(k0, min(k0 + TILE, offsets[s + 1])) for k0 in range(offsets[s], offsets[s + 1], TILE)]
        tile_sums[s] = tiles
        if tiles:
            out["log_lik"][:, s] = in_order(np.stack([in_order(l[:, t].T, ty) for t in tiles]), ty)
        pts = slice(offsets[s], offsets[s + 1])
        out["mag_log_lik"][:, s] = np.sum(mag_l[:, pts], axis=1)
    for mi in range(m):
        terms = [in_order(np.swapaxes(dl[:, t, None] * w[None, t, d:], 0, 1), ty) for t in tile_sums[mi]]
        terms += [in_order(np.swapaxes(dl[:, t, None] * w[None, t, :d], 0, 1), ty) for t in tile_sums[mi + 1]]
        if terms:
            out["g_u"][:, mi] = in_order(np.stack(terms), ty)
        a, b = slice(offsets[mi], offsets[mi + 1]), slice(offsets[mi + 1], offsets[mi + 2])
        out["mag_g_u"][:, mi] = np.einsum("kn,ni->ki", mag_dl[:, a], w8[a, d:]) + np.einsum("kn,ni->ki", mag_dl[:, b], w8[b, :d])
    return out


def random_case(name, two_d, layout, k, seed, f32=False, h=None):
    """Inputs of a batch of ``len(layout)`` series whose segments have the lengths ``layout[b]`` (rounded to float32 when ``f32``, held
    in float64): ``states ~ 0.8 N(0, 1)`` on the merged rows, ``u_post`` = the prior at the inducing rows + ``0.3 N(0, 1)``,
    ``w ~ U(-0.7, 0.7)``, ``h = e_0`` unless given, ``y`` cycling through ``likelihood_closed_forms.OBSERVED``."""
    rng = np.random.default_rng(seed)
    dt = np.float32 if f32 else np.float64
    rnd = lambda a: np.asarray(a).astype(dt).astype(np.float64)          # noqa: E731
    bsz, segs, n, d = len(layout), len(layout[0]), int(np.sum(layout[0])), two_d // 2
    assert all(int(np.sum(ln)) == n and len(ln) == segs for ln in layout)
    case = dict(offsets=np.stack([np.concatenate([[0], np.cumsum(ln)]) for ln in layout]).astype(np.int64))
    case["states"] = rnd(0.8 * rng.normal(size=(k, bsz, n + segs - 1, d)))
    rows_z = np.stack([rows_of(case["offsets"][b])[2] for b in range(bsz)])
    prior_z = np.stack([case["states"][:, b, rows_z[b]] for b in range(bsz)], axis=1)
    case["prior_z"] = prior_z
    case["u_post"] = rnd(prior_z + 0.3 * rng.normal(size=prior_z.shape))
    case["w"] = rnd(rng.uniform(-0.7, 0.7, size=(bsz, n, two_d)))
    case["h"] = rnd(np.eye(d)[0] if h is None else h)
    case["y"] = rnd(np.resize(np.asarray(L.OBSERVED[name]), (bsz, n)))
    case["indices"] = np.stack([rows_of(case["offsets"][b])[0] for b in range(bsz)]).astype(np.int64)
    return case


def dense_gaussian_logpdf(x, mean, cov):
    """log N(x | mean, cov) of a dense Gaussian (float64)."""
    r = np.asarray(x, dtype=np.float64) - mean
    return float(-0.5 * (r @ np.linalg.solve(cov, r) + np.linalg.slogdet(cov)[1] + r.shape[0] * np.log(2 * np.pi)))
