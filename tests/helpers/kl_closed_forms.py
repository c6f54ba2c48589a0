"""
Closed forms of ``StateSpaceModel.kl_divergence`` and ``StateSpaceModel.marginals`` (reference: markovflow/state_space_model.py:232-262
and :528-593) in plain torch on the CPU, with the dtype as an argument: the float64 evaluation is the reference of the GPU tests,
the float32 evaluation of the SAME arithmetic is the yardstick their float32 errors are measured against
(tests/helpers/kl_fp32_cases.py).  Nothing here comes from ``markovflow_amd.state_space_model``.

A chain is the tuple ``(mu0 [B,d], chol_p0 [B,d,d], a_s [B,T-1,d,d], b_s [B,T-1,d], chol_q [B,T-1,d,d])`` of one dtype.

Two formulations, the two the kernels evaluate:
  * the LOCAL form (include/markovflow_amd.h, mf_ssm_kl_divergence; csrc/mf_kl_grad.hpp): q1's moment recursion, then per
    transition ``1/2 [|C2^-1 C1|^2 + tr(W S W^T) + |C2^-1 eps|^2] + log|C2| - log|C1|`` with ``W = C2^-1 (A1 - A2)``,
    ``eps = (A1 - A2) m + (b1 - b2)``, the same for the initial state, minus ``T d / 2``;
  * the OPERATOR form (csrc/mf_wave.hpp, wave_ssm_kl_terms_kernel; the reference's own): per block
    ``tr(D_k Sigma_kk) + 2 tr(S_k^T C_k) + delta_k^T D_k delta_k + 2 delta_{k+1}^T S_k delta_k + 2 log|chol2_k| - 2 log|chol1_k| - d``
    from given moments, ``D_k = Q_k^-1 + A_{k+1}^T Q_{k+1}^-1 A_{k+1}``, ``S_k = -Q_{k+1}^-1 A_{k+1}`` the block row of q2's precision.
The moment recursion comes sequentially and as a Hillis-Steele scan in time (the kernels scan on long chains).
"""
import numpy as np
import torch

CHAIN = ("mu0", "chol_p0", "a_s", "b_s", "chol_q")


def chain(kw, dtype=torch.float64, requires_grad=False):
    """The five tensors of a chain from a dict of numpy arrays, as CPU leaves of ``dtype``."""
    return tuple(torch.tensor(np.ascontiguousarray(kw[k]), dtype=dtype).requires_grad_(requires_grad) for k in CHAIN)


def _tr(x):
    return x.transpose(-1, -2)


def _mv(mat, vec):
    return (mat @ vec[..., None])[..., 0]


def _lower_solve(low, rhs):
    return torch.linalg.solve_triangular(low, rhs, upper=False)


def _log_abs_diag(low):
    return torch.sum(torch.log(torch.abs(torch.diagonal(low, dim1=-2, dim2=-1))), dim=-1)


# ---- q's moments: m_{k+1} = A_k m_k + b_k, S_{k+1} = A_k S_k A_k^T + Q_k ----------------------------------------------------------
def moments_sequential(q):
    """``(means [B,T,d], covs [B,T,d,d])`` by the recursion as written."""
    mu0, cp0, a_s, b_s, cq = q
    means, covs = [mu0], [cp0 @ _tr(cp0)]
    for k in range(a_s.shape[1]):
        a_k, c_k = a_s[:, k], cq[:, k]
        means.append(_mv(a_k, means[-1]) + b_s[:, k])
        covs.append(a_k @ covs[-1] @ _tr(a_k) + c_k @ _tr(c_k))
    return torch.stack(means, dim=1), torch.stack(covs, dim=1)


def moments_scan(q):
    """The same by an inclusive Hillis-Steele scan over the T affine maps ``(Phi, beta, Sig): (m, S) -> (Phi m + beta,
    Phi S Phi^T + Sig)``.  Element 0 is the constant map onto the initial state (Phi = 0), element k the transition k - 1, so
    after ceil(log2 T) rounds element k IS the marginal of step k: (beta, Sig)."""
    mu0, cp0, a_s, b_s, cq = q
    n = a_s.shape[1] + 1
    phi = torch.cat([torch.zeros_like(cp0)[:, None], a_s], dim=1)
    beta = torch.cat([mu0[:, None], b_s], dim=1)
    sig = torch.cat([(cp0 @ _tr(cp0))[:, None], cq @ _tr(cq)], dim=1)
    off = 1
    while off < n:
        late_p, late_b, late_s = phi[:, off:], beta[:, off:], sig[:, off:]               # element k ...
        early_p, early_b, early_s = phi[:, :-off], beta[:, :-off], sig[:, :-off]         # ... applied after element k - off
        phi = torch.cat([phi[:, :off], late_p @ early_p], dim=1)
        beta = torch.cat([beta[:, :off], _mv(late_p, early_b) + late_b], dim=1)
        sig = torch.cat([sig[:, :off], late_p @ early_s @ _tr(late_p) + late_s], dim=1)
        off *= 2
    return beta, sig


def moments(q, scan=False):
    return moments_scan(q) if scan else moments_sequential(q)


def cross_covariances(q, covs):
    """``Cov(x_{k+1}, x_k) = A_k S_k`` [B,T-1,d,d]."""
    return q[2] @ covs[:, :-1]


# ---- KL(q1 || q2), local form -----------------------------------------------------------------------------------------------------
def kl_local(q1, q2, scan=False):
    """Per series [B]; differentiable with respect to all ten tensors."""
    mu1, c01, a1, b1, c1 = q1
    mu2, c02, a2, b2, c2 = q2
    means, covs = moments(q1, scan)
    n, d = a1.shape[1] + 1, mu1.shape[-1]
    u0 = _lower_solve(c02, (mu1 - mu2)[..., None])
    out = 0.5 * (torch.sum(_lower_solve(c02, c01) ** 2, dim=(-2, -1)) + torch.sum(u0 ** 2, dim=(-2, -1))) \
        + _log_abs_diag(c02) - _log_abs_diag(c01)
    if n > 1:
        m_k, s_k = means[:, :-1], covs[:, :-1]
        d_a = a1 - a2
        eps = _mv(d_a, m_k) + (b1 - b2)
        w = _lower_solve(c2, d_a)
        u = _lower_solve(c2, eps[..., None])
        terms = 0.5 * (torch.sum(_lower_solve(c2, c1) ** 2, dim=(-2, -1)) + torch.sum((w @ s_k) * w, dim=(-2, -1))
                       + torch.sum(u ** 2, dim=(-2, -1))) + _log_abs_diag(c2) - _log_abs_diag(c1)
        out = out + torch.sum(terms, dim=-1)
    return out - 0.5 * n * d


# ---- KL(q1 || q2), operator form --------------------------------------------------------------------------------------------------
def kl_operator(chol_p0_1, chol_q_1, chol_p0_2, a_2, chol_q_2, covs_1, cross_1, mean_diff):
    """Per series [B] from q1's moments: ``covs_1 [B,T,d,d]``, ``cross_1 [B,T-1,d,d] = Cov(x_{k+1}, x_k)`` and
    ``mean_diff [B,T,d] = mu_2 - mu_1``.  q1's factors enter through their diagonals only.  With T = 1 the tensors over the
    transitions may be None."""
    n, d = covs_1.shape[1], covs_1.shape[-1]
    chol_1 = chol_p0_1[:, None] if n == 1 else torch.cat([chol_p0_1[:, None], chol_q_1], dim=1)
    chol_2 = chol_p0_2[:, None] if n == 1 else torch.cat([chol_p0_2[:, None], chol_q_2], dim=1)
    inv_2 = _lower_solve(torch.tril(chol_2), torch.eye(d, dtype=chol_2.dtype).expand(chol_2.shape))
    q_inv = _tr(inv_2) @ inv_2                                                            # Q_k^-1, k = 0 .. T-1 (Q_0 = P0)
    quad = lambda mat, vec: torch.sum(vec * _mv(mat, vec), dim=-1)                        # noqa: E731
    terms = torch.sum(q_inv * covs_1, dim=(-2, -1)) + quad(q_inv, mean_diff) \
        + 2.0 * _log_abs_diag(chol_2) - 2.0 * _log_abs_diag(chol_1) - d
    if n > 1:
        sub = -(q_inv[:, 1:] @ a_2)                                                       # S_k
        ata = -(_tr(a_2) @ sub)                                                           # A^T Q_{k+1}^-1 A
        delta, delta_next = mean_diff[:, :-1], mean_diff[:, 1:]
        coupled = torch.sum(ata * covs_1[:, :-1], dim=(-2, -1)) + quad(ata, delta) \
            + 2.0 * torch.sum(sub * cross_1, dim=(-2, -1)) + 2.0 * torch.sum(delta_next * _mv(sub, delta), dim=-1)
        terms = terms + torch.cat([coupled, torch.zeros_like(terms[:, :1])], dim=1)
    return 0.5 * torch.sum(terms, dim=-1)


def kl_operator_from_chains(q1, q2, scan=False):
    """The operator form with q1's moments and both chains' means from the recursion in the chains' own dtype."""
    means_1, covs_1 = moments(q1, scan)
    means_2 = moments(q2, scan)[0]
    cross_1 = cross_covariances(q1, covs_1) if q1[2].shape[1] > 0 else None
    return kl_operator(q1[1], q1[4], q2[1], q2[2], q2[4], covs_1, cross_1, means_2 - means_1)


# ---- the marginals and a linear functional of them ---------------------------------------------------------------------------------
def marginals_functional(q, w_means, w_covs, scan=False):
    """``sum(w_means * means) + sum(w_covs * covs)``: autograd gives the adjoint of the moment recursion."""
    means, covs = moments(q, scan)
    return torch.sum(w_means * means) + torch.sum(w_covs * covs)


# ---- the metrics of the float32 checks ---------------------------------------------------------------------------------------------
def tensor_error(got, want):
    """``max|got - want| / max|want|`` of one tensor (a tensor that is exactly zero has to be met exactly)."""
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    diff, scale = float((got.reshape(want.shape) - want).abs().max()), float(want.abs().max())
    if scale == 0.0:
        return 0.0 if diff == 0.0 else float("inf")
    return diff / scale


def value_error(got, want, t, d):
    """``max_s |got_s - want_s| / max(|want_s|, T d / 2)``: T d / 2 is the constant every formulation subtracts, i.e. the scale
    rounding acts on (and what keeps KL(q || q) = 0 well defined)."""
    got, want = torch.as_tensor(got).double().cpu().reshape(-1), torch.as_tensor(want).double().cpu().reshape(-1)
    return float(((got - want).abs() / torch.clamp(want.abs(), min=0.5 * t * d)).max())
