"""
The local step of the backward of ``KalmanFilter.log_likelihood`` as plain torch on the CPU, parametric in the dtype, and an exact
smoother to feed it - the reference of tests/test_gpu_loglik_grad_float32.py and the float32 yardstick of its kernels
(tests/helpers/loglik_fp32_cases.py).  Nothing here imports the package: tests/test_loglik_grad_closed_forms_host.py pins these
forms against torch autograd of the dense log-likelihood.

Fisher's identity, grad log p(y) = E_{x|y}[grad log p(x, y)], from the smoothed moments m_k, S_k, X_k = Cov(x_{k+1}, x_k), as the
comment above kf_grad_kernel states it (markovflow_amd/csrc/mf_kernels.hpp):

    e_k = x_{k+1} - A_k x_k - b_k:   E[e] = m_{k+1} - A m_k - b,
                                     Psi = E[e e^T] = E[e] E[e]^T + S_{k+1} - A X^T - X A^T + A S_k A^T
    d/dA_k = Q^-1 (E[e] m_k^T + X - A S_k),   d/db_k = Q^-1 E[e],   d/dcholQ_k = tril(C^-T (C^-1 Psi C^-T - I)),   Q = C C^T
    d/dmu0 = P0^-1 (m_0 - mu0),   d/dcholP0 likewise with Psi_0 = (m_0 - mu0)(m_0 - mu0)^T + S_0
    r_k = y_k - H_k x_k:   d/dH_k = R^-1 (E[r] m_k^T - H S_k),   d/dy_k = -R^-1 E[r],   Omega_k = E[r] E[r]^T + H S_k H^T

each weighted by the series' incoming gradient w_s.  Omega is what the kernels hand back for the precision: the gradient of
R^-1 through the quadratic forms is -1/2 Omega (summed over the points that share the precision); the log-determinant of R^-1
is the caller's.
"""
import numpy as np
import torch

NAMES = ("mu0", "cholP0", "A", "b", "cholQ", "H", "y", "Omega")


def _tr(x):
    return x.transpose(-1, -2)


def _outer(u, v):
    return u[..., :, None] * v[..., None, :]


def _mv(mat, vec):
    return (mat @ vec[..., None])[..., 0]


def _cov_inv(chol, rhs, explicit):
    """``(C C^T)^-1 rhs``: two triangular solves, or (``explicit``, as the kernels do it) products with the inverse factor."""
    if explicit:
        inv = torch.linalg.solve_triangular(chol, torch.eye(chol.shape[-1], dtype=chol.dtype).expand(chol.shape), upper=False)
        return _tr(inv) @ (inv @ rhs)
    half = torch.linalg.solve_triangular(chol, rhs, upper=False)
    return torch.linalg.solve_triangular(_tr(chol), half, upper=True)


def _factor_gradient(chol, psi, explicit):
    """``tril(C^-T (C^-1 Psi C^-T - I))``: the gradient of -1/2 tr(Q^-1 Psi) - log|C| with respect to the lower factor C."""
    if explicit:
        eye = torch.eye(chol.shape[-1], dtype=chol.dtype)
        inv = torch.linalg.solve_triangular(chol, eye.expand(chol.shape), upper=False)
        return torch.tril(_tr(inv) @ (inv @ psi @ _tr(inv) - eye))
    left = torch.linalg.solve_triangular(chol, psi, upper=False)                      # C^-1 Psi
    inner = torch.linalg.solve_triangular(chol, _tr(left), upper=False)               # C^-1 Psi^T C^-T (Psi is symmetric)
    inner = inner - torch.eye(chol.shape[-1], dtype=chol.dtype)
    return torch.tril(torch.linalg.solve_triangular(_tr(chol), inner, upper=True))


def local_gradients(mu0, chol_p0, a_s, b_s, chol_q, h, y, r_inv, means, covs, cross, weights=None, explicit_inverse=False):
    """``(g_mu0, g_cholP0, g_A, g_b, g_cholQ, g_H, g_y, Omega)`` of ``sum_s w_s log p(y_s)`` in the dtype of the arguments.

    ``mu0 [B,d]``, ``chol_p0 [B,d,d]``, ``a_s, chol_q [B,T-1,d,d]``, ``b_s [B,T-1,d]``, ``h [B,T,m,d]``, ``y [B,T,m]``,
    ``r_inv [m,m]`` (shared) or ``[B,T,m,m]`` (per step); the smoothed ``means [B,T,d]``, ``covs [B,T,d,d]``,
    ``cross [B,T-1,d,d]``; ``weights [B]`` (None: 1).  Without an emission model (``h`` None) the last three are None.
    ``explicit_inverse``: C^-1 is formed once and Q^-1 (.), C^-1 Psi C^-T are products with it - the order of operations of
    kf_grad_kernel (tri_inv_lower) and row_kf_grad_kernel (row_qinv) - instead of triangular solves; the same numbers in exact
    arithmetic."""
    ex = explicit_inverse
    w = torch.ones(mu0.shape[0], dtype=mu0.dtype) if weights is None else weights
    w1, w2, w3 = w[:, None], w[:, None, None], w[:, None, None, None]
    # the first state
    dev0 = means[:, 0] - mu0
    g_mu0 = w1 * _cov_inv(chol_p0, dev0[..., None], ex)[..., 0]
    g_chol_p0 = w2 * _factor_gradient(chol_p0, _outer(dev0, dev0) + covs[:, 0], ex)
    # the transitions k -> k + 1
    m_k, m_n, s_k, s_n = means[:, :-1], means[:, 1:], covs[:, :-1], covs[:, 1:]
    e_bar = m_n - _mv(a_s, m_k) - b_s
    a_s_k = a_s @ s_k
    g_a = w3 * _cov_inv(chol_q, _outer(e_bar, m_k) + cross - a_s_k, ex)
    g_b = w2 * _cov_inv(chol_q, e_bar[..., None], ex)[..., 0]
    a_xt = a_s @ _tr(cross)
    psi = _outer(e_bar, e_bar) + s_n - a_xt - _tr(a_xt) + a_s_k @ _tr(a_s)
    g_chol_q = w3 * _factor_gradient(chol_q, psi, ex)
    if h is None:
        return g_mu0, g_chol_p0, g_a, g_b, g_chol_q, None, None, None
    # the observations
    r_bar = y - _mv(h, means)
    h_s = h @ covs
    g_h = w3 * (r_inv @ (_outer(r_bar, means) - h_s))
    g_y = -w2 * _mv(r_inv, r_bar)
    omega = w3 * (_outer(r_bar, r_bar) + h_s @ _tr(h))
    return g_mu0, g_chol_p0, g_a, g_b, g_chol_q, g_h, g_y, omega


def exact_moments_one_series(mu0, chol_p0, a_s, b_s, chol_q, h, y, r_inv):
    """``(means [n,d], covariance blocks [n,d,d], Cov(x_{k+1}, x_k) [n-1,d,d])`` of x | y for ONE series by dense Gaussian
    conditioning in float64 torch (the construction of tests/test_gpu_gradients.py: dense_posterior_moments): the chain's dense
    precision plus H^T R^-1 H, inverted.  ``r_inv [m,m]`` or per point ``[n,m,m]``."""
    n, d = a_s.shape[0] + 1, mu0.shape[0]
    eye = torch.eye(d, dtype=mu0.dtype)
    q_inv = [torch.cholesky_solve(eye, chol_p0)] + [torch.cholesky_solve(eye, chol_q[k]) for k in range(n - 1)]
    prec = torch.zeros(n * d, n * d, dtype=mu0.dtype)
    prior_means = [mu0]
    for k in range(n):
        block = q_inv[k]
        if k < n - 1:
            below = q_inv[k + 1] @ a_s[k]
            block = block + a_s[k].T @ below
            prec[(k + 1) * d:(k + 2) * d, k * d:(k + 1) * d] = -below
            prec[k * d:(k + 1) * d, (k + 1) * d:(k + 2) * d] = -below.T
            prior_means.append(a_s[k] @ prior_means[k] + b_s[k])
        prec[k * d:(k + 1) * d, k * d:(k + 1) * d] = block
    h_all = torch.block_diag(*[h[k] for k in range(n)])
    r_all = torch.block_diag(*[r_inv if r_inv.dim() == 2 else r_inv[k] for k in range(n)])
    cov = torch.linalg.inv(prec + h_all.T @ r_all @ h_all)
    cov = 0.5 * (cov + cov.T)
    mean = cov @ (h_all.T @ r_all @ y.reshape(-1) + prec @ torch.cat(prior_means))
    blocks = torch.stack([cov[k * d:(k + 1) * d, k * d:(k + 1) * d] for k in range(n)])
    cross = (torch.stack([cov[(k + 1) * d:(k + 2) * d, k * d:(k + 1) * d] for k in range(n - 1)]) if n > 1
             else cov.new_zeros(0, d, d))
    return mean.reshape(n, d), blocks, cross


def exact_moments(kw, r_inv):
    """The same for a batch: ``kw`` a dict of numpy arrays with a leading series axis (mu0, chol_p0, a_s, b_s, chol_q, h, y),
    ``r_inv [m,m]`` or ``[B,T,m,m]``; three float64 numpy arrays."""
    keys = ("mu0", "chol_p0", "a_s", "b_s", "chol_q", "h", "y")
    ins = [torch.tensor(np.ascontiguousarray(kw[k]), dtype=torch.float64) for k in keys]
    ri = torch.tensor(np.ascontiguousarray(r_inv), dtype=torch.float64)
    per = [exact_moments_one_series(*(x[s] for x in ins), ri[s] if ri.dim() > 2 else ri) for s in range(ins[0].shape[0])]
    return tuple(torch.stack([p[i] for p in per]).numpy() for i in range(3))


def local_gradients_numpy(kw, r_inv, moments, weights, dtype, explicit_inverse=False):
    """``local_gradients`` on numpy inputs, evaluated in ``dtype``; a list of eight CPU tensors."""
    cast = lambda x: None if x is None else torch.tensor(np.ascontiguousarray(x), dtype=dtype)      # noqa: E731
    keys = ("mu0", "chol_p0", "a_s", "b_s", "chol_q", "h", "y")
    return list(local_gradients(*(cast(kw[k]) for k in keys), cast(r_inv), *(cast(x) for x in moments), cast(weights),
                                explicit_inverse))
