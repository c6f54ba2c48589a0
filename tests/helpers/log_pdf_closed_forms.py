"""
References for ``mf_ssm_log_pdf_*`` / ``mf_ssm_log_pdf_grad_*`` (csrc/mf_logpdf.hip) - TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Value and the six
adjoints by the closed formulas in ``numpy.longdouble`` from the ROUNDED inputs (reference) and in the working dtype in the kernel's
documented order (yardstick: ``m = b + sum_l A_il x_l`` ascending, substitution with the reciprocal diagonal, steps and samples added in
ascending order; the chunk and sample-block associations differ by a few sums of the same magnitude, inside the bound's floor).
Magnitude: the sum of the absolute terms of each output on the reference's ``z`` and ``u``.  Chains: ``sample_closed_forms.ORDERS`` with
time gaps from U(0.3, 1.0) (``chol Q`` is inverted here); states: the sampler helper's reference draws, rounded.  Bound:
``sde_closed_forms.allowed``, 8 x the yardstick's largest scaled error with a floor of 8 eps, per output.
"""
import functools
import math

import numpy as np

from helpers import periodic_closed_forms as PC
from helpers import sample_closed_forms as SF
from helpers import sde_closed_forms as SC

LD = SC.LD
OUTPUTS = ("out", "g_x", "g_mu0", "g_cp0", "g_a", "g_b", "g_cq")


def evaluate(mu0, cp0, a, b, cq, x, g, dtype, magnitude_of=None):
    """Every output in ``dtype``; with ``magnitude_of = (z, u)`` of the reference: the sums of absolute terms instead."""
    mu0, cp0, a, b, cq, x, g = (np.asarray(t, dtype=dtype) for t in (mu0, cp0, a, b, cq, x, g))
    s, bsz, t, d = x.shape
    mag = magnitude_of is not None
    if mag:
        a, g = np.abs(a), np.abs(g)
    tri = np.concatenate([cp0[:, None], cq], axis=1)                               # [B, T, d, d]: only the lower triangle is used
    rinv = dtype(1) / np.stack([tri[..., i, i] for i in range(d)], axis=-1)
    z, u = (np.abs(np.asarray(v, dtype=dtype)) for v in magnitude_of) if mag else (np.zeros_like(x), np.zeros_like(x))
    if not mag:
        for i in range(d):
            m = np.broadcast_to(b[None, :, :, i], (s, bsz, t - 1)).copy()
            for l in range(d):
                m = m + a[None, :, :, i, l] * x[:, :, :-1, l]
            v = x[..., i] - np.concatenate([np.broadcast_to(mu0[None, :, None, i], (s, bsz, 1)), m], axis=2)
            for l in range(i):
                v = v - tri[None, :, :, i, l] * z[..., l]
            z[..., i] = v * rinv[None, ..., i]
        for i in reversed(range(d)):
            v = z[..., i].copy()
            for l in range(i + 1, d):
                v = v - tri[None, :, :, l, i] * u[..., l]
            u[..., i] = v * rinv[None, ..., i]
    quad, logdet = np.zeros(x.shape[:3], dtype=dtype), np.zeros((bsz, t), dtype=dtype)
    for i in range(d):
        quad = quad + z[..., i] * z[..., i]
        logdet = logdet + (np.abs(np.log(np.abs(tri[..., i, i]))) if mag else np.log(np.abs(tri[..., i, i])))
    terms = dtype(0.5) * quad + logdet[None] if mag else dtype(-0.5) * quad - logdet[None]
    out = np.zeros((s, bsz), dtype=dtype)
    for k in range(t):
        out = out + terms[:, :, k]
    cst = dtype(0.5 * t * d * math.log(2 * math.pi))
    res = {"out": out + cst if mag else out - cst, "z": z, "u": u}
    gu = g[:, :, None, None] * u
    g_x = gu.copy() if mag else -gu
    for l in range(d):
        for i in range(d):
            g_x[:, :, :-1, l] = g_x[:, :, :-1, l] + a[None, :, :, i, l] * gu[:, :, 1:, i]
    res["g_x"] = g_x
    g_b, g_sum = np.zeros((bsz, t, d), dtype=dtype), np.zeros(bsz, dtype=dtype)
    g_a, g_l = np.zeros((bsz, t - 1, d, d), dtype=dtype), np.zeros((bsz, t, d, d), dtype=dtype)
    xa = np.abs(x) if mag else x
    for smp in range(s):                                                           # the samples in ascending order
        g_b = g_b + gu[smp]
        g_sum = g_sum + g[smp]
        g_a = g_a + gu[smp, :, 1:, :, None] * xa[smp, :, :-1, None, :]
        g_l = g_l + gu[smp, :, :, :, None] * z[smp, :, :, None, :]
    g_l = np.tril(g_l)
    for i in range(d):
        diag = g_sum[:, None] / (np.abs(tri[..., i, i]) if mag else tri[..., i, i])
        g_l[..., i, i] = g_l[..., i, i] + diag if mag else g_l[..., i, i] - diag
    res.update(g_mu0=g_b[:, 0], g_b=g_b[:, 1:], g_a=g_a, g_cp0=g_l[:, 0], g_cq=g_l[:, 1:])
    return res


@functools.lru_cache(maxsize=None)
def make_case(bsz, s, t, d, dtype_name):
    """Inputs rounded to the working dtype with reference, magnitude, yardstick and bound per output; computed once per case and shared."""
    npd = np.dtype(dtype_name).type
    rng = np.random.default_rng(100000 * bsz + 1000 * s + 10 * t + d)
    comps = [dict(order=o, ls=float(rng.uniform(0.6, 1.6)), var=float(rng.uniform(0.5, 1.5)), period=None, osc=0) for o in SF.ORDERS[d]]
    a, q, pinf = PC.concat_transitions(comps, rng.uniform(0.3, 1.0, (bsz, max(t - 1, 1))), jitter=1e-6)
    cp0 = np.broadcast_to(np.linalg.cholesky(pinf + 1e-6 * np.eye(d)), (bsz, d, d))
    case = dict(mu0=rng.standard_normal((bsz, d)), cp0=cp0, a=a[:, :t - 1], b=rng.standard_normal((bsz, t - 1, d)),
                cq=np.linalg.cholesky(q)[:, :t - 1], g=rng.standard_normal((s, bsz)))
    case = {k: np.ascontiguousarray(v, dtype=npd) for k, v in case.items()}
    chain = [case[k] for k in ("mu0", "cp0", "a", "b", "cq")]
    case["x"] = np.ascontiguousarray(SF.recursion(*chain, rng.standard_normal((s, bsz, t, d)).astype(npd), LD), dtype=npd)
    args = chain + [case["x"], case["g"]]
    ref, yard = evaluate(*args, LD), evaluate(*args, npd)
    mag = evaluate(*args, LD, magnitude_of=(ref["z"], ref["u"]))
    case["ref"], case["mag"], case["bound"] = ref, mag, {}
    for name in OUTPUTS:
        assert yard[name].dtype == npd and np.all(np.isfinite(ref[name].astype(np.float64)))
        yard_err = SC.scaled_error(yard[name], ref[name], mag[name], npd)
        case["bound"][name] = SC.allowed(yard_err, npd)
        assert float(np.max(yard_err, initial=0.0)) <= case["bound"][name]         # the yardstick alone is inside the bound
    return case
