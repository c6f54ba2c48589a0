"""
numpy (fp64) closed forms of the periodic and quasi-periodic SDE kernels - TEST INFRASTRUCTURE, NOT PRODUCT CODE.

A component is a dict ``{"order": 0 | 1 | 3 | 5, "ls": lengthscale, "var": variance, "period": period or None, "osc": 0 | 1 | 2}``:
order 0 is the constant factor (markovflow/kernels/constant.py), ``osc`` says whether and on which side the rotation of
markovflow/kernels/periodic.py enters the Kronecker product of markovflow/kernels/sde_kernel.py:691-822 (1: Matern (x) R,
2: R (x) Matern); ``var`` is the product of the factors' variances.  The Matern factor comes from oracle/numpy_kernels.py.
The dense side - k(r) = sum_c var_c k_c(r) cos(omega_c r) - is independent of any state space form.
"""
import numpy as np

from oracle import numpy_kernels as K


def _kron(a, b):
    out = np.einsum("...ij,...kl->...ikjl", a, b)
    return out.reshape(out.shape[:-4] + (out.shape[-4] * out.shape[-3], out.shape[-2] * out.shape[-1]))


def size(comp):
    return (1 if comp["order"] == 0 else K.ORDER_SIZE[comp["order"]]) * (2 if comp["osc"] else 1)


def component_transitions(comp, dt, jitter=0.0):
    """(A [..., n, k, k], Q [..., n, k, k], Pinf [k, k]) of one component for time gaps dt [..., n]."""
    dt = np.asarray(dt, dtype=np.float64)
    if comp["order"] == 0:
        a, p = np.ones(dt.shape + (1, 1)), np.array([[comp["var"]]])
    else:
        a, _, p = K.matern_transitions(comp["order"], comp["ls"], comp["var"], dt)
    if comp["osc"]:
        th = 2.0 * np.pi / comp["period"] * dt
        rot = np.stack([np.stack([np.cos(th), -np.sin(th)], -1), np.stack([np.sin(th), np.cos(th)], -1)], -2)
        a, p = (_kron(a, rot), _kron(p, np.eye(2))) if comp["osc"] == 1 else (_kron(rot, a), _kron(np.eye(2), p))
    k = p.shape[-1]
    if comp["order"] == 0:
        q = np.broadcast_to(jitter * np.eye(k), dt.shape + (k, k)).copy()       # a constant / a rotation adds no noise
    else:
        q = p - a @ p @ np.swapaxes(a, -1, -2) + jitter * np.eye(k)
    return a, q, p


def concat_transitions(comps, dt, jitter=0.0):
    """Block-diagonal (A, Q, Pinf) of a Sum of components."""
    d = sum(size(c) for c in comps)
    dt = np.asarray(dt, dtype=np.float64)
    a, q, p = np.zeros(dt.shape + (d, d)), np.zeros(dt.shape + (d, d)), np.zeros((d, d))
    off = 0
    for c in comps:
        ai, qi, pi = component_transitions(c, dt, jitter)
        k = size(c)
        a[..., off:off + k, off:off + k] = ai
        q[..., off:off + k, off:off + k] = qi
        p[off:off + k, off:off + k] = pi
        off += k
    return a, q, p


def emission(comps, num_points_shape):
    """H [..., T, 1, d] of a Sum: the first state of every component."""
    d = sum(size(c) for c in comps)
    h = np.zeros((1, d))
    off = 0
    for c in comps:
        h[0, off] = 1.0
        off += size(c)
    return np.broadcast_to(h, tuple(num_points_shape) + (1, d)).copy()


def dense_kernel(comps, r):
    """k(r) = sum_c var_c k_c(|r|) cos(omega_c r)."""
    r = np.abs(r)
    out = np.zeros_like(r)
    for c in comps:
        if c["order"] == 0:
            k = np.ones_like(r)
        else:
            lam = np.sqrt(c["order"]) / c["ls"]
            k = {1: 1.0, 3: 1.0 + lam * r, 5: 1.0 + lam * r + (lam * r) ** 2 / 3.0}[c["order"]] * np.exp(-lam * r)
        if c["osc"]:
            k = k * np.cos(2.0 * np.pi / c["period"] * r)
        out += c["var"] * k
    return out


def dense_log_marginal(comps, t, y, noise):
    """-1/2 y^T K^-1 y - 1/2 log|K| - N/2 log 2 pi with K = k(t, t) + noise I, one series."""
    kn = dense_kernel(comps, t[:, None] - t[None, :]) + noise * np.eye(len(t))
    return -0.5 * y @ np.linalg.solve(kn, y) - 0.5 * np.linalg.slogdet(kn)[1] - 0.5 * len(t) * np.log(2 * np.pi)


def dense_predict(comps, t, y, noise, t_new):
    """Dense GP posterior (mean, variance) of f at t_new (Rasmussen & Williams eq. 2.25-2.26)."""
    kn = dense_kernel(comps, t[:, None] - t[None, :]) + noise * np.eye(len(t))
    ks = dense_kernel(comps, t_new[:, None] - t[None, :])
    mean = ks @ np.linalg.solve(kn, y)
    var = dense_kernel(comps, np.zeros(len(t_new))) - np.einsum("ij,ji->i", ks, np.linalg.solve(kn, ks.T))
    return mean, var
