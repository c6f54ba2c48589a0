"""
CPU tests of ``kernels.LatentExponentiallyGenerated`` (the torch restatement and the public surface), of the numpy reference
tests/helpers/leg_closed_forms.py against ``scipy.linalg.expm``, and of the new symbols' presence in the C header and the ctypes table.
"""
import os
import re

import numpy as np
import pytest
import scipy.linalg
import torch

from markovflow_amd import _lib
from markovflow_amd import kernels as K
from helpers import leg_closed_forms as LC

DIMS = [1, 2, 3, 6, 8, 13, 16]
GAPS = np.array([1e-5, 1e-3, 0.1, 1.0, 10.0, 40.0])
NEW_SYMBOLS = ["mf_sde_leg_transitions_f64", "mf_sde_leg_transitions_f32", "mf_sde_leg_transitions_grad_f64",
               "mf_sde_leg_transitions_grad_f32", "mf_sde_leg_transitions_grad_workspace_bytes"]


def draw(d, seed, batch=()):
    rng = np.random.default_rng(seed)
    return rng, rng.standard_normal(batch + (d, d)), rng.standard_normal(batch + (d, d))


@pytest.mark.parametrize("d", DIMS)
def test_reference_against_scipy(d):
    """A sanity bound on the helper, not a tolerance on the kernel."""
    _, n_mat, r_mat = draw(d, d)
    f = LC.feedback(n_mat, r_mat).astype(np.float64)
    a = LC.forward(f, GAPS, 0.0)[0].astype(np.float64)
    for k, g in enumerate(GAPS):
        assert np.max(np.abs(a[k] - scipy.linalg.expm(g * f))) < 1e-12


def test_feedback_matrix_and_steady_state_covariance():
    _, n_mat, r_mat = draw(5, 1, (3,))
    kern = K.LatentExponentiallyGenerated(torch.tensor(n_mat), torch.tensor(r_mat))
    want = -0.5 * (n_mat @ np.swapaxes(n_mat, -1, -2) + r_mat - np.swapaxes(r_mat, -1, -2))
    np.testing.assert_allclose(kern.feedback_matrix.numpy(), want, rtol=1e-14, atol=1e-15)
    assert np.array_equal(kern.steady_state_covariance.numpy(), np.broadcast_to(np.eye(5), (3, 5, 5)))
    assert kern.state_dim == 5 and kern._components() == [kern] and len(kern._leaves()) == 2
    kern.invalidate_cache()
    sym = kern.feedback_matrix + kern.feedback_matrix.transpose(-1, -2)            # F + F^T = -N N^T: negative semi-definite
    assert float(torch.linalg.eigvalsh(sym).max()) <= 1e-12


@pytest.mark.parametrize("batch", [(), (2,)])
def test_shapes_and_output_dim(batch):
    d, n = 4, 7
    rng, n_mat, r_mat = draw(d, 2, batch)
    t = torch.tensor(np.sort(rng.uniform(0, 5, batch + (n,)), axis=-1))
    for output_dim, m in ((None, d), (1, 1)):
        kern = K.LatentExponentiallyGenerated(torch.tensor(n_mat), torch.tensor(r_mat), jitter=1e-6, output_dim=output_dim)
        assert kern.output_dim == m
        h = kern.generate_emission_model(t).emission_matrix
        assert tuple(h.shape) == batch + (n, m, d)
        assert bool((h[..., 0] == 1).all()) and bool((h[..., 1:] == 0).all())       # every row is [1, 0, ...]
        a_s, q_s = kern.transition_statistics(t[..., :-1], K.to_delta_time(t))
        assert tuple(a_s.shape) == batch + (n - 1, d, d) and tuple(q_s.shape) == batch + (n - 1, d, d)
        assert tuple(kern.state_transitions(t[..., :-1], K.to_delta_time(t)).shape) == batch + (n - 1, d, d)
        assert tuple(kern.process_covariances(t[..., :-1], K.to_delta_time(t)).shape) == batch + (n - 1, d, d)
        p0 = kern.initial_covariance(t[..., :1])
        assert tuple(p0.shape) == batch + (d, d)
        np.testing.assert_allclose(p0.numpy(), np.broadcast_to((1 + 1e-6) * np.eye(d), batch + (d, d)))
        ssm = kern.state_space_model(t)
        assert tuple(ssm.state_transitions.shape) == batch + (n - 1, d, d)
        chol0 = kern._initial_cholesky(batch, t.dtype, t.device)                     # the closed-form factor of (1 + jitter) I
        np.testing.assert_allclose((chol0 @ chol0.transpose(-1, -2)).numpy(), p0.numpy(), rtol=1e-14)
        assert tuple(kern.initial_mean(batch).shape) == batch + (d,)
        assert tuple(kern.jitter_matrix.shape) == (d, d)


@pytest.mark.parametrize("d", [1, 3, 6])
def test_torch_route_against_reference(d):
    rng, n_mat, r_mat = draw(d, 30 + d)
    gaps = rng.uniform(0.05, 3.0, 9)
    kern = K.LatentExponentiallyGenerated(torch.tensor(n_mat), torch.tensor(r_mat), jitter=1e-6)
    a_s, chol, q_s = kern._device_transitions(torch.tensor(gaps), True, True)            # CPU tensors: the torch restatement
    ref = LC.forward(LC.feedback(n_mat, r_mat), gaps, 1e-6)
    np.testing.assert_allclose(a_s.numpy(), ref[0].astype(np.float64), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(q_s.numpy(), ref[1].astype(np.float64), rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(chol.numpy(), ref[2].astype(np.float64), rtol=1e-9, atol=1e-12)


def test_torch_route_without_process_noise():
    d = 4
    rng, _, r_mat = draw(d, 40)
    kern = K.LatentExponentiallyGenerated(torch.zeros((d, d), dtype=torch.float64), torch.tensor(r_mat))
    a_s, chol, q_s = kern._device_transitions(torch.tensor([0.3, 2.0]), True, True)
    assert bool((q_s == 0).all()) and bool((chol == 0).all()) and bool(torch.isfinite(a_s).all())


def test_torch_route_autograd_against_reference():
    d, n = 5, 7
    rng, n_mat, r_mat = draw(d, 50)
    n_mat = np.eye(d) + 0.3 * n_mat
    gaps = rng.uniform(0.05, 3.0, n)
    g_a, g_c = rng.standard_normal((n, d, d)), np.tril(rng.standard_normal((n, d, d)))
    n_t, r_t = torch.tensor(n_mat, requires_grad=True), torch.tensor(r_mat, requires_grad=True)
    kern = K.LatentExponentiallyGenerated(n_t, r_t, jitter=1e-6)
    a_s, chol, _ = kern._device_transitions(torch.tensor(gaps), True, False)
    ((torch.tensor(g_a) * a_s).sum() + (torch.tensor(g_c) * chol).sum()).backward()
    terms = LC.reverse_terms(LC.feedback(n_mat, r_mat), gaps, 1e-6, g_a, g_c)
    g_n, g_r = LC.grad_to_leaves(n_mat, terms.sum(axis=0))
    np.testing.assert_allclose(n_t.grad.numpy(), g_n.astype(np.float64), rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(r_t.grad.numpy(), g_r.astype(np.float64), rtol=1e-9, atol=1e-11)


def test_refused_as_a_child():
    leg = K.LatentExponentiallyGenerated(torch.eye(2, dtype=torch.float64), torch.zeros((2, 2), dtype=torch.float64), output_dim=1)
    m32 = K.Matern32(1.0, 1.0)
    for build in (lambda: K.Sum([leg, m32]), lambda: K.Product([leg, m32]), lambda: K.IndependentMultiOutput([leg, m32]),
                  lambda: leg + m32, lambda: leg * m32,
                  lambda: K.PiecewiseKernel([leg, leg], torch.tensor([1.0], dtype=torch.float64))):
        with pytest.raises(NotImplementedError):
            build()


def test_refused_as_the_temporal_kernel_of_a_spatio_temporal_kernel():
    from markovflow_amd import spatial_kernels as S
    leg = K.LatentExponentiallyGenerated(torch.eye(2, dtype=torch.float64), torch.zeros((2, 2), dtype=torch.float64), output_dim=1)
    space = [c for c in vars(S).values() if isinstance(c, type) and hasattr(c, "_leaves") and not getattr(c, "__abstractmethods__", None)]
    if not space:
        pytest.skip("no concrete spatial kernel found")
    with pytest.raises(NotImplementedError):
        K.SparseSpatioTemporalKernel(space[0](1.0, 1.0), leg, torch.zeros((3, 1), dtype=torch.float64))


def test_bad_arguments():
    with pytest.raises(ValueError):
        K.LatentExponentiallyGenerated(torch.zeros((2, 3)), torch.zeros((2, 3)))
    with pytest.raises(ValueError):
        K.LatentExponentiallyGenerated(torch.zeros((2, 2)), torch.zeros((3, 3)))


def test_new_symbols_in_header_and_table():
    header = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "markovflow_amd.h")
    text = open(header).read()
    names = set(_lib.exported_symbols())
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b" + sym + r"\(", text), sym
        assert sym in names, sym
