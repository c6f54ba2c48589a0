"""
Independent reference for the impulse / step mean functions, written from the mathematics in numpy.

A kernel is a list of components ``(order, osc, lam, omega)`` (order 0, 1, 3, 5 = Matern-order/2 with ``lam = sqrt(order) / lengthscale``;
osc 0: none, 1: Matern (x) R, 2: R (x) Matern; ``omega = 2 pi / period``) whose states are concatenated, and an output map (the output
that every component's first state is added to).  ``E(D) = exp(F D)`` is the closed form ``e^{-lam D}(I + N D + N^2 D^2 / 2)`` with
``N = F_Matern + lam I`` nilpotent, Kronecker-multiplied with the rotation ``R(omega D)``.

* The REFERENCE runs in ``numpy.longdouble`` and does NOT use the recurrence of the code under test: it uses the direct sums over the
  actions with ``tau_k < t``,

      impulse:  s(t) = sum_k E(t - tau_k) u_k
      step:     s(t) = sum_k F^-1 [E(t - tau_k) - E(t - min(t, tau_{k+1}))] u_k,   tau_K = +inf,

  and, for the entry points that take the right-hand sides ``r`` and the constants ``a`` of the recurrence themselves, the explicit
  matrix of the linear map ``(r, a) -> s``:  ``s(t) = a_k + sum_{i <= k} E(t - tau_i) r_i`` with ``k`` the last action before ``t``
  (``linear_map``; its transpose is the reference of the reverse mode).
* The YARDSTICK is the recurrence ``c_k = E(tau_k - tau_{k-1}) c_{k-1} + r_k``, ``s = a_k + E(t - tau_k) c_k`` (and its reverse)
  restated in numpy in the working dtype; its error against the reference is what the code under test is measured against.

Errors are SCALED: the absolute error of an entry over the summed magnitudes of the terms that make it up (``|a_k| + sum_i |E| |r_i|``),
so that a sum that cancels is not asked for more digits than its terms have (plus an underflow allowance, see ``scaled_error``).
``allowed`` is built like ``leg_closed_forms.allowed``: the code under test gets FACTOR x the yardstick's largest scaled error, with a
floor of FACTOR d eps(dtype).
"""
import numpy as np

LD = np.longdouble
FACTOR = 8.0


def longdouble_ok() -> bool:
    return bool(np.finfo(LD).eps < 2e-19)


def state_dim(comps) -> int:
    return sum((1 if o == 0 else (o + 1) // 2) * (2 if r else 1) for o, r, _, _ in comps)


def offsets(comps):
    out, off = [], 0
    for o, r, _, _ in comps:
        out.append(off)
        off += (1 if o == 0 else (o + 1) // 2) * (2 if r else 1)
    return out


def _nilpotent(order, lam, dt):
    if order <= 1:
        return np.zeros((1, 1), dtype=dt)
    one, zero = dt.type(1), dt.type(0)
    if order == 3:
        return np.array([[lam, one], [-lam * lam, -lam]], dtype=dt)
    return np.array([[lam, one, zero], [zero, lam, one], [-lam * lam * lam, -dt.type(3) * lam * lam, -dt.type(2) * lam]], dtype=dt)


def component_feedback(order, osc, lam, omega, dtype=LD):
    dt = np.dtype(dtype)
    lam = dt.type(0 if order == 0 else lam)
    nil = _nilpotent(order, lam, dt)
    k = nil.shape[0]
    f_m = nil - lam * np.eye(k, dtype=dt)
    if not osc:
        return f_m
    w = dt.type(omega)
    rot = np.array([[0, -w], [w, 0]], dtype=dt)
    eye2, eyek = np.eye(2, dtype=dt), np.eye(k, dtype=dt)
    return np.kron(f_m, eye2) + np.kron(eyek, rot) if osc == 1 else np.kron(eye2, f_m) + np.kron(rot, eyek)


def component_transition(order, osc, lam, omega, delta, dtype=LD):
    """``exp(F delta)`` of one component for gaps ``delta [n]``: ``[n, k, k]``."""
    dt = np.dtype(dtype)
    delta = np.asarray(delta, dtype=dt)
    lam = dt.type(0 if order == 0 else lam)
    nil = _nilpotent(order, lam, dt)
    k = nil.shape[0]
    x = delta[:, None, None]
    mat = np.eye(k, dtype=dt) + nil * x
    if order == 5:
        mat = mat + (nil @ nil) * (dt.type(0.5) * x * x)
    mat = (np.exp(-lam * delta)[:, None, None] * mat).astype(dt)
    if not osc:
        return mat
    th = dt.type(omega) * delta
    c, s = np.cos(th), np.sin(th)
    rot = np.stack([np.stack([c, -s], axis=-1), np.stack([s, c], axis=-1)], axis=-2).astype(dt)
    n = delta.shape[0]
    if osc == 1:
        return np.einsum("nij,npq->nipjq", mat, rot).reshape(n, 2 * k, 2 * k).astype(dt)
    return np.einsum("npq,nij->npiqj", rot, mat).reshape(n, 2 * k, 2 * k).astype(dt)


def feedback(comps, dtype=LD):
    d = state_dim(comps)
    out = np.zeros((d, d), dtype=dtype)
    for (o, r, lam, om), off in zip(comps, offsets(comps)):
        blk = component_feedback(o, r, lam, om, dtype)
        out[off:off + blk.shape[0], off:off + blk.shape[0]] = blk
    return out


def transition(comps, delta, dtype=LD):
    """``exp(F delta)`` block diagonal over the components: ``[n, d, d]``."""
    delta = np.asarray(delta, dtype=dtype)
    d = state_dim(comps)
    out = np.zeros((delta.shape[0], d, d), dtype=dtype)
    for (o, r, lam, om), off in zip(comps, offsets(comps)):
        blk = component_transition(o, r, lam, om, delta, dtype)
        out[:, off:off + blk.shape[-1], off:off + blk.shape[-1]] = blk
    return out


def emission(comps, out_map, m, dtype=LD):
    h = np.zeros((m, state_dim(comps)), dtype=dtype)
    for off, o in zip(offsets(comps), out_map):
        h[o, off] = 1
    return h


def solve(mat, rhs):
    """``mat^-1 rhs`` by Gaussian elimination with partial pivoting in the dtype of ``mat`` (numpy.linalg has no long double)."""
    a = np.array(mat, copy=True)
    b = np.array(rhs, dtype=a.dtype, copy=True)
    n = a.shape[0]
    for c in range(n):
        p = c + int(np.argmax(np.abs(a[c:, c])))
        if p != c:
            a[[c, p]] = a[[p, c]]
            b[[c, p]] = b[[p, c]]
        for r in range(c + 1, n):
            f = a[r, c] / a[c, c]
            a[r, c:] = a[r, c:] - f * a[c, c:]
            b[r] = b[r] - f * b[c]
    x = np.zeros_like(b)
    for r in range(n - 1, -1, -1):
        acc = b[r]
        for c in range(r + 1, n):
            acc = acc - a[r, c] * x[c]
        x[r] = acc / a[r, r]
    return x


def bins(tau, t):
    """``j - 1`` with ``j = #{k : tau_k < t}`` (-1: before the first action), compared in the dtype of the inputs."""
    return np.searchsorted(np.asarray(tau), np.asarray(t), side="left").astype(np.int64) - 1


# ---- the reference: direct sums -------------------------------------------------------------------------------------------------------
def impulse_state(comps, tau, u, t):
    """``s(t) = sum over tau_k < t of E(t - tau_k) u_k``: ``[N, d]`` in long double."""
    tau_l, t_l, u_l = np.asarray(tau, dtype=LD), np.asarray(t, dtype=LD), np.asarray(u, dtype=LD)
    out = np.zeros((t_l.shape[0], state_dim(comps)), dtype=LD)
    for k in range(tau_l.shape[0]):
        seen = np.asarray(tau)[k] < np.asarray(t)
        e = transition(comps, np.where(seen, t_l - tau_l[k], 0), LD)
        out += np.where(seen[:, None], np.einsum("nij,j->ni", e, u_l[k]), 0)
    return out


def step_state(comps, tau, u, t):
    """``s(t) = sum over tau_k < t of F^-1 [E(t - tau_k) - E(t - min(t, tau_{k+1}))] u_k`` with ``tau_K = +inf``."""
    tau_l, t_l, u_l = np.asarray(tau, dtype=LD), np.asarray(t, dtype=LD), np.asarray(u, dtype=LD)
    f = feedback(comps, LD)
    num = tau_l.shape[0]
    out = np.zeros((t_l.shape[0], state_dim(comps)), dtype=LD)
    for k in range(num):
        seen = np.asarray(tau)[k] < np.asarray(t)
        end = t_l if k == num - 1 else np.minimum(t_l, tau_l[k + 1])
        diff = transition(comps, np.where(seen, t_l - tau_l[k], 0), LD) - transition(comps, np.where(seen, t_l - end, 0), LD)
        term = solve(f, np.einsum("nij,j->in", diff, u_l[k])).T
        out += np.where(seen[:, None], term, 0)
    return out


def linear_map(comps, tau, t):
    """The explicit matrices of ``(r, a) -> s``: ``(M_r, M_a)``, each ``[N, d, K, d]`` in long double:
    ``s(t_n) = a_k + sum_{i <= k} E(t_n - tau_i) r_i`` with ``k = bins(tau, t)[n]``, zero rows for ``k = -1``."""
    tau_l, t_l = np.asarray(tau, dtype=LD), np.asarray(t, dtype=LD)
    d, num, n = state_dim(comps), tau_l.shape[0], t_l.shape[0]
    which = bins(tau, t)
    m_r, m_a = np.zeros((n, d, num, d), dtype=LD), np.zeros((n, d, num, d), dtype=LD)
    for i in range(num):
        seen = i <= which
        e = transition(comps, np.where(seen, t_l - tau_l[i], 0), LD)
        m_r[:, :, i, :] = np.where(seen[:, None, None], e, 0)
    for p in range(n):
        if which[p] >= 0:
            m_a[p, :, which[p], :] = np.eye(d, dtype=LD)
    return m_r, m_a


def step_sources(comps, u, dtype=LD):
    """``(r, a)`` of a step: ``a_k = -F^-1 u_k``, ``r_0 = -a_0``, ``r_k = a_{k-1} - a_k``."""
    u = np.asarray(u, dtype=dtype)
    a = -solve(feedback(comps, dtype), u.T).T
    return np.concatenate([-a[:1], a[:-1] - a[1:]], axis=0), a


# ---- the yardstick: the recurrence in the working dtype ---------------------------------------------------------------------------------
def recurrence(comps, tau, r, a, t, dtype):
    """``[N, d]``: ``c_0 = r_0``, ``c_k = E(tau_k - tau_{k-1}) c_{k-1} + r_k``; ``s = a_k + E(t - tau_k) c_k``, zero before ``tau_0``."""
    dt = np.dtype(dtype)
    tau_w, t_w, r_w = np.asarray(tau, dtype=dt), np.asarray(t, dtype=dt), np.asarray(r, dtype=dt)
    num = tau_w.shape[0]
    coef = np.zeros_like(r_w)
    coef[0] = r_w[0]
    if num > 1:
        a_s = transition(comps, tau_w[1:] - tau_w[:-1], dt)
        for k in range(1, num):
            coef[k] = (a_s[k - 1] @ coef[k - 1] + r_w[k]).astype(dt)
    which = bins(tau_w, t_w)
    k = np.maximum(which, 0)
    e = transition(comps, np.where(which >= 0, t_w - tau_w[k], 0).astype(dt), dt)
    s = np.einsum("nij,nj->ni", e, coef[k]).astype(dt)
    if a is not None:
        s = (np.asarray(a, dtype=dt)[k] + s).astype(dt)
    return np.where((which >= 0)[:, None], s, 0).astype(dt)


def reverse_recurrence(comps, tau, t, g_state, dtype):
    """The adjoint in the working dtype: ``(g_r, g_a)``, each ``[K, d]``, from ``g_state [N, d]`` (= ``H^T g_f``)."""
    dt = np.dtype(dtype)
    tau_w, t_w, g_w = np.asarray(tau, dtype=dt), np.asarray(t, dtype=dt), np.asarray(g_state, dtype=dt)
    num = tau_w.shape[0]
    which = bins(tau_w, t_w)
    k = np.maximum(which, 0)
    e = transition(comps, np.where(which >= 0, t_w - tau_w[k], 0).astype(dt), dt)
    v = np.einsum("nij,ni->nj", e, g_w).astype(dt)
    g_c, g_a = np.zeros((num, g_w.shape[-1]), dtype=dt), np.zeros((num, g_w.shape[-1]), dtype=dt)
    for p in range(t_w.shape[0]):
        if which[p] >= 0:
            g_c[which[p]] += v[p]
            g_a[which[p]] += g_w[p]
    if num > 1:
        a_s = transition(comps, tau_w[1:] - tau_w[:-1], dt)
        for i in range(num - 1, 0, -1):
            g_c[i - 1] = (g_c[i - 1] + a_s[i - 1].T @ g_c[i]).astype(dt)
    return g_c, g_a


# ---- measured tolerances ----------------------------------------------------------------------------------------------------------------
def forward_magnitude(m_r, m_a, r, a):
    """Per entry of the state the summed magnitudes of its terms: ``|M_r| |r| + |M_a| |a|``, ``[N, d]``."""
    mag = np.einsum("nikj,kj->ni", np.abs(m_r), np.abs(np.asarray(r, dtype=LD)))
    if a is not None:
        mag = mag + np.einsum("nikj,kj->ni", np.abs(m_a), np.abs(np.asarray(a, dtype=LD)))
    return mag


def reverse_magnitude(mat, g_state):
    """``|M|^T |g|``, ``[K, d]``."""
    return np.einsum("nikj,ni->kj", np.abs(mat), np.abs(np.asarray(g_state, dtype=LD)))


def scaled_error(x, ref, magnitude, dtype):
    """``|x - ref| / (magnitude + tiny(dtype) / eps(dtype))`` entry by entry, as float64.  The second term of the denominator is
    the underflow allowance: a value whose terms lie below the smallest normal number of the working dtype (a response that has
    decayed to 1e-700 exists in long double only) cannot carry a relative accuracy; with it an error bound of ``c eps`` admits an
    absolute error of ``c tiny``.  It also makes an entry without any term (magnitude zero) an absolute comparison."""
    info = np.finfo(dtype)
    err = np.abs(np.asarray(x, dtype=LD) - ref)
    return (err / (magnitude + LD(info.tiny) / LD(info.eps))).astype(np.float64)


def allowed(yardstick_scaled_error, d, dtype):
    """The bound for a scaled error of the code under test: FACTOR x the yardstick's largest scaled error over the same inputs,
    with a floor of FACTOR d eps(dtype)."""
    y = float(np.max(np.asarray(yardstick_scaled_error, dtype=np.float64), initial=0.0))
    return max(FACTOR * y, FACTOR * d * float(np.finfo(dtype).eps))
