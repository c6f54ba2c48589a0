"""
numpy (fp64) closed forms of the piecewise-stationary kernel - TEST INFRASTRUCTURE, NOT PRODUCT CODE.

A piecewise kernel is ``(segments, change_points)``: ``segments[k]`` is the component list (tests/helpers/periodic_closed_forms.py)
of the kernel active on segment ``k``, ``change_points`` the ``len(segments) - 1`` sorted times between them.  A step belongs to the
segment its START TIME lies in - the number of change points ``<=`` it, so a start time on a change point belongs to the segment
after it - and its ``A``, ``P-infinity`` and ``Q`` all come from that one segment (markovflow/kernels/piecewise_stationary.py).

The dense side is the joint covariance of the chain by recursion, ``P_{k+1} = A_k P_k A_k^T + Q_k`` with the cross terms
``Cov(x_j, x_i) = A_{j-1} ... A_i P_i``; from it ``K_ff``, the log marginal likelihood and the GP prediction on a merged grid.  It is
the exact law of the process whenever no transition crosses a change point.  None of it touches Kalman code.

``first`` (the chain functions): the process is conditioned at points of which ``first`` is the earliest, and before it it is
stationary under the kernel active AT ``first`` - the segment of a time ``t < first`` is looked up at ``first``
(``max(t, first)``), for the initial covariance as for the transitions.  ``dense_predict`` applies the rule with
``first = t[0]``; with every point in the segment of ``t[0]`` or later it changes nothing.
"""
import numpy as np

from helpers import periodic_closed_forms as PC


def segment_index(t, change_points, dtype=np.float64):
    """Number of change points <= t, the comparison done after casting both sides to ``dtype`` (the dtype under test)."""
    cp = np.asarray(change_points, dtype=np.float64).astype(dtype)
    return np.searchsorted(cp, np.asarray(t, dtype=np.float64).astype(dtype), side="right").astype(np.int64)


def transitions(segments, change_points, t_start, dt, jitter=0.0, dtype=np.float64):
    """Per-step ``(A, Q, Pinf, seg)`` for start times ``t_start [..., n]`` and gaps ``dt [..., n]``: ``[..., n, d, d]`` x 3 and the
    segment index ``[..., n]``."""
    dt = np.asarray(dt, dtype=np.float64)
    seg = segment_index(t_start, change_points, dtype)
    d = sum(PC.size(c) for c in segments[0])
    a, q, p = (np.zeros(dt.shape + (d, d)) for _ in range(3))
    for k, comps in enumerate(segments):
        ak, qk, pk = PC.concat_transitions(comps, dt, jitter=jitter)
        here = seg == k
        a[here], q[here], p[here] = ak[here], qk[here], pk
    return a, q, p, seg


def lookup(t, first=None):
    """The times at which the dynamics at ``t`` are looked up (module docstring: ``first``)."""
    t = np.asarray(t, dtype=np.float64)
    return t if first is None else np.maximum(t, first)


def steady_state(segments, change_points, t, dtype=np.float64):
    """``Pinf`` of the segment of every time point, ``[..., n, d, d]``."""
    t = np.asarray(t, dtype=np.float64)
    return transitions(segments, change_points, t, np.ones_like(t), dtype=dtype)[2]


def state_marginals(segments, change_points, t, jitter=0.0, first=None):
    """Marginal state covariances ``[n, d, d]`` of the chain on the sorted time points ``t [n]`` (one series)."""
    a, q, _, _ = transitions(segments, change_points, lookup(t[:-1], first), np.diff(t), jitter=jitter)
    d = a.shape[-1]
    out = np.zeros((len(t), d, d))
    out[0] = steady_state(segments, change_points, lookup(t[:1], first))[0] + jitter * np.eye(d)
    for k in range(len(t) - 1):
        out[k + 1] = a[k] @ out[k] @ a[k].T + q[k]
    return out


def joint_state_covariance(segments, change_points, t, jitter=0.0, first=None):
    """``Cov(x_i, x_j)`` of the chain on the sorted time points ``t [n]``: ``[n, n, d, d]``."""
    a = transitions(segments, change_points, lookup(t[:-1], first), np.diff(t), jitter=jitter)[0]
    marg = state_marginals(segments, change_points, t, jitter, first)
    n, d = len(t), marg.shape[-1]
    cov = np.zeros((n, n, d, d))
    for i in range(n):
        cov[i, i] = marg[i]
        prop = np.eye(d)
        for j in range(i + 1, n):
            prop = a[j - 1] @ prop                       # A_{j-1} ... A_i
            cov[j, i] = prop @ marg[i]
            cov[i, j] = cov[j, i].T
    return cov


def dense_kff(segments, change_points, t, jitter=0.0, first=None):
    """``K_ff [n, n]`` of ``f = H x`` on the sorted time points ``t``."""
    h = PC.emission(segments[0], ())[0]
    return np.einsum("a,ijab,b->ij", h, joint_state_covariance(segments, change_points, t, jitter, first), h)


def dense_log_marginal(segments, change_points, t, y, noise, jitter=0.0):
    """-1/2 y^T K^-1 y - 1/2 log|K| - N/2 log 2 pi with K = K_ff + noise I, one series."""
    kn = dense_kff(segments, change_points, t, jitter) + noise * np.eye(len(t))
    return -0.5 * y @ np.linalg.solve(kn, y) - 0.5 * np.linalg.slogdet(kn)[1] - 0.5 * len(t) * np.log(2 * np.pi)


def dense_predict(segments, change_points, t, y, noise, t_new, jitter=0.0):
    """Dense GP posterior (mean, variance) of f at ``t_new`` given ``y`` at ``t``: the chain on the merged grid of both, stationary
    before ``t[0]`` under the kernel active at ``t[0]``."""
    grid = np.unique(np.concatenate([t, t_new]))
    k = dense_kff(segments, change_points, grid, jitter, first=t[0])
    it, inew = np.searchsorted(grid, t), np.searchsorted(grid, t_new)
    kn = k[np.ix_(it, it)] + noise * np.eye(len(t))
    ks = k[np.ix_(inew, it)]
    mean = ks @ np.linalg.solve(kn, y)
    var = np.diagonal(k)[inew] - np.einsum("ij,ji->i", ks, np.linalg.solve(kn, ks.T))
    return mean, var
