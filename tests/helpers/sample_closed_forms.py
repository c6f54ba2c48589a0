"""
References for ``mf_ssm_sample_*`` (csrc/mf_sample.hip) - TEST INFRASTRUCTURE, NOT PRODUCT CODE.  The plain recursion with the full stored
blocks in ``numpy.longdouble`` from the ROUNDED inputs (reference) and in the working dtype (yardstick), the magnitude recursion
``mag_k = |A| mag_{k-1} + |b| + |cholQ| |eps|`` and the magnitude of one step, on Sums of Matern components (contractive chains).  Bound:
tests/helpers/sde_closed_forms.py's, 8 x the yardstick's largest scaled error with a floor of 8 eps, under either magnitude.
"""
import functools

import numpy as np

from helpers import periodic_closed_forms as PC
from helpers import sde_closed_forms as SC

LD = SC.LD
ORDERS = {1: [1], 2: [3], 3: [5], 4: [5, 1], 5: [5, 3], 6: [5, 5], 7: [5, 5, 1], 8: [5, 5, 3], 9: [5, 5, 5]}


def recursion(mu0, cp0, a, b, cq, eps, dtype):
    """``[S, B, T, d]`` draws from ``eps [S, B, T, d]``, every product and sum in ``dtype``."""
    mu0, cp0, a, b, cq, eps = (np.asarray(t, dtype=dtype) for t in (mu0, cp0, a, b, cq, eps))
    x = mu0[None] + np.einsum("bij,sbj->sbi", cp0, eps[:, :, 0])
    out = [x]
    for k in range(1, eps.shape[2]):
        x = np.einsum("bij,sbj->sbi", a[:, k - 1], x) + b[None, :, k - 1] + np.einsum("bij,sbj->sbi", cq[:, k - 1], eps[:, :, k])
        out.append(x)
    return np.stack(out, axis=2)


def local_magnitude(mu0, cp0, a, b, cq, eps, ref):
    """``|A| |x_{k-1}| + |b| + |cholQ| |eps_k|`` on the reference's states: ``mag`` above reaches 10^16 after 200 steps at d = 6."""
    mu0, cp0, a, b, cq, eps, ref = (np.abs(np.asarray(t, dtype=LD)) for t in (mu0, cp0, a, b, cq, eps, ref))
    first = mu0[None] + np.einsum("bij,sbj->sbi", cp0, eps[:, :, 0])
    rest = np.einsum("bkij,sbkj->sbki", a, ref[:, :, :-1]) + b[None] + np.einsum("bkij,sbkj->sbki", cq, eps[:, :, 1:])
    return np.concatenate([first[:, :, None], rest], axis=2)


@functools.lru_cache(maxsize=None)
def make_case(bsz, s, t, d, dtype_name, full_block=False):
    """Inputs rounded to the working dtype with reference, magnitude and yardstick; computed once per case and shared."""
    npd = np.dtype(dtype_name).type
    rng = np.random.default_rng(100000 * bsz + 1000 * s + 10 * t + d + (7 if full_block else 0))
    comps = [dict(order=o, ls=float(rng.uniform(0.6, 1.6)), var=float(rng.uniform(0.5, 1.5)), period=None, osc=0) for o in ORDERS[d]]
    gaps = rng.uniform(0.1, 0.6, (bsz, max(t - 1, 1)))
    a, q, pinf = PC.concat_transitions(comps, gaps, jitter=1e-6)
    cq = np.linalg.cholesky(q)
    if full_block:                                                  # another factor of the same Q: an orthogonal matrix from the right
        rot, _ = np.linalg.qr(rng.standard_normal((d, d)))
        cq = cq @ rot
    cp0 = np.broadcast_to(np.linalg.cholesky(pinf + 1e-6 * np.eye(d)), (bsz, d, d))
    case = dict(mu0=rng.standard_normal((bsz, d)), cp0=cp0, a=a[:, :t - 1], b=rng.standard_normal((bsz, t - 1, d)), cq=cq[:, :t - 1],
                eps=rng.standard_normal((s, bsz, t, d)))
    case = {k: np.ascontiguousarray(v, dtype=npd) for k, v in case.items()}
    args = [case[k] for k in ("mu0", "cp0", "a", "b", "cq", "eps")]
    case["ref"], case["mag"], case["yard"] = recursion(*args, LD), recursion(*[np.abs(t) for t in args], LD), recursion(*args, npd)
    assert case["yard"].dtype == npd and np.all(np.isfinite(case["ref"]))
    assert float(np.max(np.abs(case["ref"]))) < 200.0
    case["local"] = local_magnitude(*args, case["ref"])
    for mag, bound in (("mag", "bound"), ("local", "local_bound")):
        yard_err = SC.scaled_error(case["yard"], case["ref"], case[mag], npd)
        case[bound] = SC.allowed(yard_err, npd)
        assert float(np.max(yard_err)) <= case[bound]               # the yardstick alone is inside the bound
    return case
