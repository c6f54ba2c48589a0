"""
Independent reference for the LatentExponentiallyGenerated transition generator, written from the mathematics in numpy.

    F = -(N N^T + R - R^T) / 2,   A = expm(dt F),   Q = I - A A^T + jitter I,   L = chol Q

Everything is batched over a leading axis of steps and runs in a requested dtype:

* ``numpy.longdouble`` with a long Taylor series (degree 30) is the REFERENCE (``longdouble_ok()`` says whether the platform's long
  double is wider than a double);
* float32 / float64 with the degrees of the device code (8 / 15) is the YARDSTICK: the same chain of operations restated in the
  working precision, whose error against the reference is what the device kernels are measured against.

The matrix exponential is scaling and squaring of ``E = expm(X) - I`` (``E <- 2 E + E E``), ``Q = -(E + E^T + E E^T)`` (the carried
form), the Cholesky factorisation and the triangular solves are hand loops, the Frechet derivative comes from the block-triangular
identity ``expm([[X, G], [0, X]]) = [[e^X, L_exp(X; G)], [0, e^X]]``.
"""
import numpy as np

LD = np.longdouble
DEGREE = {np.dtype(np.float32): 8, np.dtype(np.float64): 15, np.dtype(LD): 30}
THETA = 0.5


def longdouble_ok() -> bool:
    return bool(np.finfo(LD).eps < 2e-19)


def feedback(n_mat, r_mat, dtype=LD):
    n_mat, r_mat = np.asarray(n_mat, dtype=dtype), np.asarray(r_mat, dtype=dtype)
    half = np.asarray(0.5, dtype=dtype)
    return -half * (n_mat @ np.swapaxes(n_mat, -1, -2) + r_mat - np.swapaxes(r_mat, -1, -2))


def grad_to_leaves(n_mat, g_f, dtype=LD):
    """``(gN, gR)`` from the gradient with respect to ``F``."""
    n_mat, g_f = np.asarray(n_mat, dtype=dtype), np.asarray(g_f, dtype=dtype)
    half = np.asarray(0.5, dtype=dtype)
    g_t = np.swapaxes(g_f, -1, -2)
    return -half * (g_f + g_t) @ n_mat, -half * (g_f - g_t)


def scale_counts(x):
    """Per step the smallest ``s >= 0`` with ``||X||_1 2^-s <= 1/2``."""
    norm = np.abs(x).sum(axis=-2).max(axis=-1)
    _, e = np.frexp(norm.astype(np.float64))
    return np.where(norm > THETA, e + 1, 0).astype(np.int64)


def expm1(x, dtype, degree=None, counts=None):
    """``expm(x) - I`` for ``x`` of shape ``[K, m, m]``."""
    dt = np.dtype(dtype)
    x = np.asarray(x, dtype=dt)
    degree = DEGREE[dt] if degree is None else degree
    s = scale_counts(x) if counts is None else counts
    y = np.ldexp(x, -s[:, None, None].astype(np.int32)).astype(dt)
    term, e = y.copy(), y.copy()
    for k in range(2, degree + 1):
        term = (y @ term) / np.asarray(k, dtype=dt)
        e = e + term
    two = np.asarray(2, dtype=dt)
    for t in range(int(s.max()) if s.size else 0):
        e = np.where((t < s)[:, None, None], two * e + e @ e, e)
    return e.astype(dt)


def cholesky(q):
    """Lower factor by hand loops; an all-zero block passes through as zero, a non-positive pivot gives NaN."""
    k, d, _ = q.shape
    low = np.zeros_like(q)
    zero = np.all(q == 0, axis=(-1, -2))
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(d):
            s = q[:, j, j].copy()
            for l in range(j):
                s = s - low[:, j, l] * low[:, j, l]
            ljj = np.sqrt(s)
            low[:, j, j] = ljj
            for i in range(j + 1, d):
                v = q[:, i, j].copy()
                for l in range(j):
                    v = v - low[:, i, l] * low[:, j, l]
                low[:, i, j] = v / ljj
    low[zero] = 0
    return low, zero


def solve_lower_right(low, b):
    """``b L^-1``: rows solve ``u L = b`` from the last column back."""
    d = low.shape[-1]
    b = b.copy()
    u = np.zeros_like(b)
    for j in range(d - 1, -1, -1):
        u[:, :, j] = b[:, :, j] / low[:, j, j][:, None]
        for c in range(j):
            b[:, :, c] = b[:, :, c] - u[:, :, j] * low[:, j, c][:, None]
    return u


def solve_lower_transposed_left(low, b):
    """``L^-T b`` by back substitution over the rows."""
    d = low.shape[-1]
    out = np.zeros_like(b)
    for i in range(d - 1, -1, -1):
        acc = b[:, i, :].copy()
        for c in range(i + 1, d):
            acc = acc - low[:, c, i][:, None] * out[:, c, :]
        out[:, i, :] = acc / low[:, i, i][:, None]
    return out


def forward(f_mat, gaps, jitter, dtype=LD, degree=None):
    """``(A, Q, L, zero)`` for feedback matrices ``[K, d, d]`` (or ``[d, d]``) and gaps ``[K]``."""
    dt = np.dtype(dtype)
    gaps = np.asarray(gaps, dtype=dt)
    f_mat = np.broadcast_to(np.asarray(f_mat, dtype=dt), (gaps.shape[0],) + tuple(np.shape(f_mat)[-2:]))
    d = f_mat.shape[-1]
    eye = np.eye(d, dtype=dt)
    e = expm1(gaps[:, None, None] * f_mat, dt, degree)
    half = np.asarray(0.5, dtype=dt)
    m = e + half * (e @ np.swapaxes(e, -1, -2))
    q = -(m + np.swapaxes(m, -1, -2)) + np.asarray(jitter, dtype=dt) * eye
    low, zero = cholesky(q)
    return e + eye, q, low, zero


def reverse_terms(f_mat, gaps, jitter, g_a, g_c, dtype=LD, degree=None):
    """Per step ``dt L_exp(dt F^T; G)`` with ``G = gA - 2 gQ A`` and ``gQ`` the Cholesky adjoint of the lower triangle of ``gC``:
    ``[K, d, d]``, the terms whose sum over the steps is the gradient with respect to ``F``."""
    dt = np.dtype(dtype)
    gaps = np.asarray(gaps, dtype=dt)
    a, _, low, zero = forward(f_mat, gaps, jitter, dt, degree)
    k, d, _ = a.shape
    f_mat = np.broadcast_to(np.asarray(f_mat, dtype=dt), (k, d, d))
    g_a = np.zeros((k, d, d), dtype=dt) if g_a is None else np.asarray(g_a, dtype=dt)
    g_q = np.zeros((k, d, d), dtype=dt)
    if g_c is not None:
        half = np.asarray(0.5, dtype=dt)
        safe = np.where(zero[:, None, None], np.eye(d, dtype=dt), low)
        p = np.swapaxes(safe, -1, -2) @ np.tril(np.asarray(g_c, dtype=dt))
        p = np.tril(p, -1) + half * p * np.eye(d, dtype=dt)
        s = solve_lower_transposed_left(safe, solve_lower_right(safe, p))
        g_q = np.where(zero[:, None, None], 0, half * (s + np.swapaxes(s, -1, -2))).astype(dt)
    g = g_a - np.asarray(2, dtype=dt) * (g_q @ a)
    xt = gaps[:, None, None] * np.swapaxes(f_mat, -1, -2)
    big = np.zeros((k, 2 * d, 2 * d), dtype=dt)
    big[:, :d, :d], big[:, d:, d:], big[:, :d, d:] = xt, xt, g
    lx = expm1(big, dt, degree, counts=scale_counts(xt))[:, :d, d:]
    return gaps[:, None, None] * lx


def dense_covariance(f_mat, h_mat, times):
    """``H expm(F |t_i - t_j|) H^T`` arranged for the stationary process with ``P_inf = I``: ``[T m, T m]`` in float64
    (``cov(x_i, x_j) = expm(F (t_i - t_j))`` for ``t_i >= t_j``)."""
    t = np.asarray(times, dtype=np.float64)
    n, m = t.shape[0], h_mat.shape[0]
    f_mat = np.asarray(f_mat, dtype=LD)
    lag = np.abs(t[:, None] - t[None, :]).reshape(-1)
    a = (expm1(lag.astype(LD)[:, None, None] * f_mat, LD) + np.eye(f_mat.shape[-1], dtype=LD)).astype(np.float64)
    a = a.reshape(n, n, f_mat.shape[-1], f_mat.shape[-1])
    out = np.zeros((n * m, n * m))
    for i in range(n):
        for j in range(n):
            blk = a[i, j] if t[i] >= t[j] else a[i, j].T
            out[i * m:(i + 1) * m, j * m:(j + 1) * m] = h_mat @ blk @ h_mat.T
    return out


# ---- measured tolerances --------------------------------------------------------------------------------------------------------------
# The code under test is allowed FACTOR x the error of the yardstick (the same chain in the same dtype on the same inputs; in float64
# the larger of that and scipy.linalg.expm's error where the caller supplies it), with a floor of FACTOR d eps(dtype): another
# degree, another scaling threshold, contraction to FMA and another summation order do not change the error's order of magnitude.
FACTOR = 8.0


def forward_errors(a, q, low, ref):
    """Per step: ``A`` and ``Q`` as the largest absolute error over the largest absolute reference entry, ``chol Q`` as the
    reconstruction error ``||L L^T - Q_ref|| / ||Q_ref||`` (Frobenius).  ``ref = (A, Q, L, zero)`` in long double.  A step whose
    reference ``Q`` is all zero has nothing to divide by: its errors are absolute."""
    a_r, q_r = ref[0], ref[1]
    out = {}
    for name, x, r in (("A", a, a_r), ("Q", q, q_r)):
        if x is None:
            continue
        scale = np.abs(r).max(axis=(-1, -2))
        out[name] = (np.abs(np.asarray(x, dtype=LD) - r).max(axis=(-1, -2)) / np.where(scale > 0, scale, 1)).astype(np.float64)
    if low is not None:
        l_ld = np.asarray(low, dtype=LD)
        rec = l_ld @ np.swapaxes(l_ld, -1, -2) - q_r
        scale = np.sqrt((q_r * q_r).sum(axis=(-1, -2)))
        out["L"] = (np.sqrt((rec * rec).sum(axis=(-1, -2))) / np.where(scale > 0, scale, 1)).astype(np.float64)
    return out


def allowed(yardstick_error, d, dtype, other_error=None):
    """The bound for an error of the code under test, elementwise over the steps."""
    y = np.asarray(yardstick_error, dtype=np.float64)
    if other_error is not None:
        y = np.maximum(y, np.asarray(other_error, dtype=np.float64))
    return np.maximum(FACTOR * y, FACTOR * d * float(np.finfo(dtype).eps))


def reverse_allowed(terms_ref, yardstick_sum, d, dtype):
    """The bound for the absolute error of a summed reverse-mode result: FACTOR x the yardstick's absolute error, with the floor
    scaled by the summed magnitudes of the per-step terms."""
    ref_sum = terms_ref.sum(axis=0)
    y_err = float(np.abs(np.asarray(yardstick_sum, dtype=LD) - ref_sum).max())
    magnitude = float(np.abs(terms_ref).max(axis=(-1, -2)).sum())
    return max(FACTOR * y_err, FACTOR * d * float(np.finfo(dtype).eps) * magnitude)
