"""
GPU tests of ``kernels.LatentExponentiallyGenerated`` inside the models: ``GaussianProcessRegression`` (log marginal likelihood, its
backward onto ``N`` and ``R``, posterior prediction) against the dense Gaussian of the joint covariance
``k(t_i, t_j) = [expm(F |t_i − t_j|)]_00`` (``P∞ = I``, ``H = [1, 0, …]``), and ``SparseVariationalGaussianProcess`` with
``output_dim=1`` against the same model on the torch route.  Tolerances are those tests/test_gpu_piecewise.py applies to the same
comparisons: log-likelihood rel 1e-8, gradients rtol 1e-6 / atol 1e-9, prediction rtol 1e-6 (mean) and 1e-5 (variance) / atol 1e-7.
"""
import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BSZ, T, NOISE = 3, 40, 0.1


def tt(x, **kw):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV, **kw)


def draw(d, seed):
    rng = np.random.default_rng(seed)
    n_mat, r_mat = np.eye(d) + 0.3 * rng.standard_normal((d, d)), rng.standard_normal((d, d))
    t = np.sort(rng.uniform(0.0, 8.0, (BSZ, T)), axis=-1) + 0.01 * np.arange(T)
    return rng, n_mat, r_mat, t, rng.standard_normal((BSZ, T, 1))


def dense_kernel(n_mat, r_mat, t1, t2):
    """``[expm(F |t1_i − t2_j|)]_00`` in differentiable torch ops (CPU)."""
    f = -0.5 * (n_mat @ n_mat.T + r_mat - r_mat.T)
    lag = (t1[:, None] - t2[None, :]).abs()
    return torch.linalg.matrix_exp(f * lag[..., None, None])[..., 0, 0]


def dense_log_marginal(n_mat, r_mat, t, y):
    kn = dense_kernel(n_mat, r_mat, t, t) + NOISE * torch.eye(t.shape[0], dtype=t.dtype)
    return -0.5 * (y @ torch.linalg.solve(kn, y) + torch.linalg.slogdet(kn)[1] + t.shape[0] * np.log(2 * np.pi))


def gpr_of(n_dev, r_dev, t, y):
    kern = K.LatentExponentiallyGenerated(n_dev, r_dev, output_dim=1)
    return mfa.GaussianProcessRegression((tt(t), tt(y)), kern, chol_obs_covariance=tt(np.sqrt(NOISE) * np.eye(1)))


def refuse_torch_route(monkeypatch):
    def boom(self, *a, **k):
        raise AssertionError("the torch restatement ran")
    monkeypatch.setattr(K.LatentExponentiallyGenerated, "_torch_transitions", boom)


@pytest.mark.parametrize("d", [2, 6])
def test_gpr_log_likelihood_and_backward_vs_dense_gp(d, monkeypatch):
    _, n_mat, r_mat, t, y = draw(d, 10 + d)
    n_c, r_c = torch.tensor(n_mat, requires_grad=True), torch.tensor(r_mat, requires_grad=True)
    want = sum(dense_log_marginal(n_c, r_c, torch.tensor(t[s]), torch.tensor(y[s, :, 0])) for s in range(BSZ))
    want.backward()
    n_d, r_d = tt(n_mat, requires_grad=True), tt(r_mat, requires_grad=True)
    refuse_torch_route(monkeypatch)                       # forward AND backward below are the HIP kernel pair
    gpr = gpr_of(n_d, r_d, t, y)
    assert gpr._fused_log_likelihood_per_series() is None
    loss = gpr.loss()
    loss.backward()
    got = -float(loss.detach())
    print(f"d={d}: state space {got!r}, dense {float(want.detach())!r}, rel {abs(got - float(want.detach())) / abs(float(want.detach())):.2e}")
    assert got == pytest.approx(float(want.detach()), rel=1e-8)
    for name, g, c in (("N", n_d, n_c), ("R", r_d, r_c)):
        assert g.grad is not None
        np.testing.assert_allclose(-g.grad.cpu().numpy(), c.grad.numpy(), rtol=1e-6, atol=1e-9, err_msg=name)
    with torch.no_grad():
        assert float(gpr.log_likelihood()) == pytest.approx(float(want.detach()), rel=1e-8)


def test_posterior_prediction_vs_dense_conditioning(monkeypatch):
    d = 6
    rng, n_mat, r_mat, t, y = draw(d, 21)
    refuse_torch_route(monkeypatch)
    gpr = gpr_of(tt(n_mat), tt(r_mat), t, y)
    t_new = np.stack([np.sort(np.concatenate([[t[s, 0] - 0.7, t[s, 0] - 0.05], 0.5 * (t[s, 5:9] + t[s, 6:10]), [t[s, -1] + 0.1, t[s, -1] + 2.0]]))
                      for s in range(BSZ)])
    f_mean, f_var = gpr.posterior.predict_f(tt(t_new))
    assert tuple(f_mean.shape) == (BSZ, t_new.shape[1], 1)
    n_c, r_c = torch.tensor(n_mat), torch.tensor(r_mat)
    for s in range(BSZ):
        ts, tn = torch.tensor(t[s]), torch.tensor(t_new[s])
        kn = dense_kernel(n_c, r_c, ts, ts) + NOISE * torch.eye(T, dtype=torch.float64)
        ks = dense_kernel(n_c, r_c, tn, ts)
        mean = ks @ torch.linalg.solve(kn, torch.tensor(y[s, :, 0]))
        var = 1.0 - (ks * torch.linalg.solve(kn, ks.T).T).sum(-1)
        np.testing.assert_allclose(f_mean.cpu().numpy()[s, :, 0], mean.numpy(), rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(f_var.cpu().numpy()[s, :, 0], var.numpy(), rtol=1e-5, atol=1e-7)


def test_svgp_elbo_and_gradient_vs_torch_route(monkeypatch):
    d = 3
    rng, n_mat, r_mat, t, y = draw(d, 33)
    z = np.stack([np.linspace(-0.5, 9.0, 12)] * BSZ)
    results = []
    for route in ("torch", "hip"):
        n_d, r_d = tt(n_mat, requires_grad=True), tt(r_mat, requires_grad=True)
        kern = K.LatentExponentiallyGenerated(n_d, r_d, jitter=1e-6, output_dim=1)
        if route == "torch":
            kern._device_transitions = lambda dt, want_chol, want_cov, transition_times=None, k=kern: k._torch_transitions(dt, want_chol, want_cov)
        seen = []
        real = K._lib.call
        monkeypatch.setattr(K._lib, "call", lambda name, *a, _real=real, _seen=seen: _seen.append(name) or _real(name, *a))
        model = mfa.SparseVariationalGaussianProcess(kern, mfa.Gaussian(NOISE), tt(z))
        elbo = model.elbo((tt(t), tt(y)))
        elbo.backward()
        # the prior chain on the inducing points comes from the kernel pair; the conditionals ask for Q under a gradient, which is
        # the torch restatement's by design
        ran = ("mf_sde_leg_transitions" in seen, "mf_sde_leg_transitions_grad" in seen)
        assert ran == ((True, True) if route == "hip" else (False, False)), (route, seen)
        results.append((float(elbo.detach()), n_d.grad.cpu().numpy(), r_d.grad.cpu().numpy()))
    (e_t, gn_t, gr_t), (e_h, gn_h, gr_h) = results
    print(f"SVGP elbo: torch route {e_t!r}, HIP route {e_h!r}")
    assert e_h == pytest.approx(e_t, rel=1e-8)
    assert np.abs(gn_t).max() > 0
    np.testing.assert_allclose(gn_h, gn_t, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(gr_h, gr_t, rtol=1e-6, atol=1e-9)


def test_shared_gradient_is_the_sum_of_per_series_gradients():
    d = 6
    rng, n_mat, r_mat, t, _ = draw(d, 44)
    w_a, w_c = tt(rng.standard_normal((BSZ, T - 1, d, d))), tt(rng.standard_normal((BSZ, T - 1, d, d)))
    grads = []
    for per_series in (False, True):
        n_d = tt(np.broadcast_to(n_mat, (BSZ, d, d)) if per_series else n_mat, requires_grad=True)
        r_d = tt(np.broadcast_to(r_mat, (BSZ, d, d)) if per_series else r_mat, requires_grad=True)
        kern = K.LatentExponentiallyGenerated(n_d, r_d, jitter=1e-6)
        ssm = kern.state_space_model(tt(t))
        ((w_a * ssm.state_transitions).sum() + (w_c * ssm.cholesky_process_covariances).sum()).backward()
        grads.append((n_d.grad.cpu().numpy(), r_d.grad.cpu().numpy()))
    (gn, gr), (gn_b, gr_b) = grads
    assert gn_b.shape == (BSZ, d, d) and np.abs(gn).max() > 0
    np.testing.assert_allclose(gn, gn_b.sum(axis=0), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(gr, gr_b.sum(axis=0), rtol=1e-12, atol=1e-13)
