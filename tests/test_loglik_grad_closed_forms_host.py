"""
The reference of the float32 log-likelihood gradient tests pinned on the CPU, independently of the package: the local forms of
Fisher's identity (tests/helpers/loglik_grad_closed_forms.py) on the EXACT smoothed moments (dense Gaussian conditioning) equal
torch autograd of the dense log-likelihood (tests/test_post_host_sim.py: _dense_log_likelihood) in float64, to 1e-9 of every
gradient tensor's size - state dimensions on both sides of the kernels' lane / row split, one to four outputs, shared and per-step
precisions, series weighted differently, a single time point.
"""
import numpy as np
import pytest
import torch

from helpers import loglik_grad_closed_forms as LC
from test_post_host_sim import _dense_log_likelihood

KEYS = ("mu0", "chol_p0", "a_s", "b_s", "chol_q", "h", "y")


def draw(rng, bsz, t, d, m, per_step):
    kw = dict(mu0=rng.normal(size=(bsz, d)), chol_p0=np.tril(0.2 * rng.normal(size=(bsz, d, d))) + np.eye(d),
              a_s=0.5 / np.sqrt(d) * rng.normal(size=(bsz, t - 1, d, d)), b_s=0.3 * rng.normal(size=(bsz, t - 1, d)),
              chol_q=np.tril(0.2 * rng.normal(size=(bsz, t - 1, d, d))) + np.eye(d), h=rng.normal(size=(bsz, t, m, d)),
              y=rng.normal(size=(bsz, t, m)))
    root = rng.normal(size=((bsz, t, m, m) if per_step else (m, m)))
    r_inv = root @ np.swapaxes(root, -1, -2) + np.eye(m)
    return kw, r_inv, rng.uniform(0.5, 1.5, size=bsz)


def max_norm_error(got, want):
    return float((got - want).abs().max()) / float(want.abs().max())


@pytest.mark.parametrize("per_step", [False, True])
@pytest.mark.parametrize("d,m,t,bsz", [(1, 1, 6, 2), (1, 2, 1, 3), (3, 2, 7, 2), (3, 4, 5, 1), (7, 1, 5, 2), (7, 4, 1, 2),
                                       (12, 2, 4, 2), (12, 4, 6, 1), (3, 1, 1, 2), (7, 2, 9, 1), (12, 1, 3, 1), (1, 4, 4, 2)])
def test_local_forms_on_exact_moments_are_the_gradients_of_the_dense_log_likelihood(d, m, t, bsz, per_step):
    rng = np.random.default_rng(1000 * d + 100 * m + 10 * t + bsz + int(per_step))
    kw, r_inv, w = draw(rng, bsz, t, d, m, per_step)
    got = LC.local_gradients_numpy(kw, r_inv, LC.exact_moments(kw, r_inv), w, torch.float64)
    leaves = [torch.tensor(kw[k], requires_grad=True) for k in KEYS] + [torch.tensor(r_inv, requires_grad=True)]
    total = 0.0
    for s in range(bsz):
        total = total + w[s] * _dense_log_likelihood(*[v[s] for v in leaves[:7]], leaves[7][s] if per_step else leaves[7])
    total.backward()
    want = [v.grad for v in leaves]
    for name, g, ref in zip(LC.NAMES[:7], got[:7], want[:7]):
        if t == 1 and name in ("A", "b", "cholQ"):
            assert g.numel() == 0
            continue
        ref = torch.tril(ref) if name in ("cholP0", "cholQ") else ref
        assert max_norm_error(g, ref) <= 1e-9, name
        if name in ("cholP0", "cholQ"):
            assert float(torch.triu(g, diagonal=1).abs().max()) == 0.0, name
    # d/dR^-1: -1/2 Omega through the quadratic forms, + 1/2 w R from the log-determinant (which the kernels leave to the caller)
    cov_r = torch.linalg.inv(torch.tensor(r_inv))
    if per_step:
        got_r = -0.5 * got[7] + 0.5 * torch.tensor(w)[:, None, None, None] * cov_r
    else:
        got_r = -0.5 * got[7].sum(dim=(0, 1)) + 0.5 * float(w.sum()) * t * cov_r
    assert max_norm_error(got_r, 0.5 * (want[7] + want[7].transpose(-1, -2))) <= 1e-9


def test_unit_weights_are_the_default():
    rng = np.random.default_rng(5)
    kw, r_inv, _ = draw(rng, 2, 4, 3, 2, False)
    moments = LC.exact_moments(kw, r_inv)
    for a, b in zip(LC.local_gradients_numpy(kw, r_inv, moments, None, torch.float64),
                    LC.local_gradients_numpy(kw, r_inv, moments, np.ones(2), torch.float64)):
        assert torch.equal(a, b)
