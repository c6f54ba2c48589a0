"""
GPU tests of ``markovflow_amd.mean_function`` through the public API: the fused route (``mf_mean_response_*``) against the torch route
and the long double reference of tests/helpers/mean_function_closed_forms.py, autograd, and ``GaussianProcessRegression`` /
``AnalyticPosteriorProcess`` with a mean function.
"""
import numpy as np
import pytest
import scipy.linalg
import torch

import markovflow_amd as mfa
from markovflow_amd import mean_function as MF
from helpers import mean_function_closed_forms as MC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NP = {torch.float64: np.float64, torch.float32: np.float32}
LS32, LS52 = 0.9, 1.6
COMPS = [(3, 0, np.sqrt(3.0) / LS32, 0.0), (5, 0, np.sqrt(5.0) / LS52, 0.0)]
CLASSES = {"impulse": MF.ImpulseMeanFunction, "step": MF.StepMeanFunction}


def nn(x):
    return x.detach().cpu().numpy()


def sum_kernel(dtype=torch.float64, device=DEV, jitter=1e-9):
    return mfa.Sum([mfa.Matern32(LS32, 1.0, device=device, dtype=dtype), mfa.Matern52(LS52, 1.3, device=device, dtype=dtype)],
                   jitter=jitter)


def draw(batch, num, n, seed, npd=np.float64):
    rng = np.random.default_rng(seed)
    tau = np.sort(rng.uniform(0.0, 6.0, size=batch + (num,)), axis=-1).astype(npd)
    u = rng.standard_normal(batch + (num, 5)).astype(npd)
    t = rng.uniform(-1.0, 9.0, size=batch + (n,)).astype(npd)
    t[..., 0] = tau[..., 0] - 1e6                                                  # long before the first action
    t[..., 1] = tau[..., 1]                                                        # exactly on an action
    return tau, u, t


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("mode", list(CLASSES))
def test_fused_route_against_torch_route(mode, dtype):
    if dtype == torch.float64 and not MC.longdouble_ok():
        pytest.skip("numpy.longdouble is no wider than a double here: no reference for the float64 accuracy")
    npd = NP[dtype]
    batch = (2, 3)
    tau, u, t = draw(batch, 6, 41, 1, npd)
    kernel = sum_kernel(dtype)
    mean = CLASSES[mode](torch.tensor(tau, device=DEV), torch.tensor(u, device=DEV), kernel)
    tp = torch.tensor(t, device=DEV)
    fused = nn(mean(tp))
    MF.fused = False
    try:
        plain = nn(mean(tp))
    finally:
        MF.fused = True
    assert fused.shape == plain.shape == batch + (41, 1) and fused.dtype == npd
    # (the components as the kernels see them: sqrt(order) / lengthscale formed in the working dtype)
    comps = [(o, r, float(k._lambda), om) for (o, r, _, om), k in zip(COMPS, kernel.kernels)]
    h = MC.emission(comps, [0, 0], 1)
    worst = 0.0
    for idx in np.ndindex(*batch):
        m_r, m_a = MC.linear_map(comps, tau[idx], t[idx])
        if mode == "impulse":
            ref = MC.impulse_state(comps, tau[idx], u[idx], t[idx])
            (r_l, a_l), (r_w, a_w) = (u[idx], None), (u[idx], None)
        else:
            ref = MC.step_state(comps, tau[idx], u[idx], t[idx])
            r_l, a_l = MC.step_sources(comps, u[idx])
            r_w, a_w = MC.step_sources(comps, u[idx], npd)
        mag = MC.forward_magnitude(m_r, m_a, r_l, a_l) @ h.T
        yard = MC.recurrence(comps, tau[idx], r_w, a_w, t[idx], npd).astype(MC.LD) @ h.T
        bound = MC.allowed(MC.scaled_error(yard, ref @ h.T, mag, npd), 5, npd)
        for got in (fused[idx], plain[idx]):
            err = MC.scaled_error(got, ref @ h.T, mag, npd)
            assert err.max() <= bound, (idx, err.max(), bound)
            worst = max(worst, err.max() / bound)
        assert fused[idx][0, 0] == 0.0 and plain[idx][0, 0] == 0.0                 # exactly zero, not NaN, 1e6 before the actions
    print(f"mean function {mode} routes, largest error / allowed: {worst:.3f}")


@pytest.mark.parametrize("order", ["matern_x_oscillator", "oscillator_x_matern"])
def test_independent_multi_output_and_oscillator(order):
    """Two outputs, and a quasi-periodic component in either order of the Kronecker product: the fused route against the torch route."""
    factors = [mfa.Matern32(1.3, 1.0, device=DEV), mfa.HarmonicOscillator(1.0, 2.5, device=DEV)]
    product = mfa.Product(factors if order == "matern_x_oscillator" else factors[::-1])
    assert product._osc == (1 if order == "matern_x_oscillator" else 2)
    kern = mfa.IndependentMultiOutput([mfa.Matern12(0.7, 1.0, device=DEV), product])
    rng = np.random.default_rng(3)
    tau = torch.tensor(np.sort(rng.uniform(0, 5, size=(2, 4)), axis=-1), device=DEV)
    u = torch.tensor(rng.standard_normal((2, 4, 5)), device=DEV)
    t = torch.tensor(rng.uniform(-1, 8, size=(2, 70)), device=DEV)
    for cls in CLASSES.values():
        mean = cls(tau, u, kern)
        fused = mean(t)
        MF.fused = False
        try:
            plain = mean(t)
        finally:
            MF.fused = True
        assert fused.shape == (2, 70, 2)
        np.testing.assert_allclose(nn(fused), nn(plain), rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("mode", list(CLASSES))
def test_nan_time_point_and_mixed_dtypes(mode):
    """A NaN query time gives NaN on both routes (it is not hidden behind the zero before the first action), and a float64 kernel
    with float32 data runs on both routes: the hyper-parameters are cast to the data's dtype."""
    tau, u, t = draw((2,), 4, 20, 21, np.float32)
    t[:, 5] = np.nan
    kern = mfa.Sum([mfa.Constant(2.0, device=DEV), mfa.Matern32(LS32, 1.0, device=DEV)], jitter=1e-6) if mode == "impulse" \
        else sum_kernel()
    u = u[..., :kern.state_dim]
    mean = CLASSES[mode](torch.tensor(tau, device=DEV), torch.tensor(u, device=DEV), kern)
    fused = nn(mean(torch.tensor(t, device=DEV)))
    MF.fused = False
    try:
        plain = nn(mean(torch.tensor(t, device=DEV)))
    finally:
        MF.fused = True
    assert fused.dtype == plain.dtype == np.float32
    for got in (fused, plain):
        assert np.isnan(got[:, 5]).all() and np.isfinite(np.delete(got, 5, axis=1)).all() and (got[:, 0] == 0).all()
    np.testing.assert_allclose(np.delete(fused, 5, axis=1), np.delete(plain, 5, axis=1), rtol=2e-4, atol=2e-5)


def test_leg_kernel_takes_the_torch_route():
    rng = np.random.default_rng(5)
    n_mat, r_mat = rng.standard_normal((3, 3)), rng.standard_normal((3, 3))
    kern = mfa.LatentExponentiallyGenerated(torch.tensor(n_mat, device=DEV), torch.tensor(r_mat, device=DEV), output_dim=1)
    f = -0.5 * (n_mat @ n_mat.T + r_mat - r_mat.T)
    u = rng.standard_normal((2, 3))
    tau = np.array([0.5, 1.5])
    t = np.array([0.2, 0.5, 0.9, 1.5, 1.7, 3.0])
    got = nn(MF.ImpulseMeanFunction(torch.tensor(tau, device=DEV), torch.tensor(u, device=DEV), kern)(torch.tensor(t, device=DEV)))
    want = np.zeros((6, 3))
    for k in range(2):
        for i, x in enumerate(t):
            if tau[k] < x:
                want[i] += scipy.linalg.expm(f * (x - tau[k])) @ u[k]
    np.testing.assert_allclose(got[:, 0], want[:, 0], rtol=1e-9, atol=1e-12)
    assert got[0, 0] == 0.0 and got[1, 0] == 0.0


@pytest.mark.parametrize("mode", list(CLASSES))
def test_autograd_state_perturbations(mode):
    tau, u, t = draw((2,), 5, 90, 7)
    w = np.random.default_rng(8).standard_normal((2, 90, 1))
    grads = []
    for dev in (DEV, "cpu"):
        leaf = torch.tensor(u, device=dev, requires_grad=True)
        out = CLASSES[mode](torch.tensor(tau, device=dev), leaf, sum_kernel(device=dev))(torch.tensor(t, device=dev))
        (g,) = torch.autograd.grad((out * torch.tensor(w, device=dev)).sum(), leaf)
        grads.append(nn(g))
    np.testing.assert_allclose(grads[0], grads[1], rtol=1e-10, atol=1e-12)
    leaf = torch.tensor(u, device=DEV, requires_grad=True)
    out = CLASSES[mode](torch.tensor(tau, device=DEV), leaf, sum_kernel())(torch.tensor(t, device=DEV))
    with pytest.raises(RuntimeError, match="differentiable once"):
        torch.autograd.grad(out.sum(), leaf, create_graph=True)


@pytest.mark.parametrize("mode", list(CLASSES))
def test_autograd_lengthscale(mode):
    tau, u, t = draw((2,), 4, 30, 9)
    grads = []
    for dev in (DEV, "cpu"):
        ell = torch.tensor(1.1, dtype=torch.float64, device=dev, requires_grad=True)
        kern = mfa.Sum([mfa.Matern32(ell, 1.0, device=dev), mfa.Matern52(LS52, 1.3, device=dev)])
        out = CLASSES[mode](torch.tensor(tau, device=dev), torch.tensor(u[..., :5], device=dev), kern)(torch.tensor(t, device=dev))
        (g,) = torch.autograd.grad((out ** 2).sum(), ell)
        grads.append(float(g))
    assert grads[0] == pytest.approx(grads[1], rel=1e-8)


def gpr_setup(batch, n, seed):
    rng = np.random.default_rng(seed)
    t = np.cumsum(0.05 + rng.exponential(0.1, size=batch + (n,)), axis=-1)
    y = rng.standard_normal(batch + (n, 1))
    tau = np.sort(rng.uniform(0.0, t[..., -1:].min(), size=batch + (3,)), axis=-1)
    u = rng.standard_normal(batch + (3, 5))
    dev = lambda x: torch.tensor(x, device=DEV)                                     # noqa: E731
    return dev(t), dev(y), dev(tau), dev(u), dev(np.sqrt(0.1) * np.eye(1))


@pytest.mark.parametrize("batch,n,fused", [((), 15, False), ((2,), 130, True)], ids=["materialised", "fused"])
def test_gpr_log_likelihood_and_posterior(batch, n, fused):
    t, y, tau, u, chol_r = gpr_setup(batch, n, 11)
    kernel = sum_kernel()
    mean = MF.ImpulseMeanFunction(tau, u, kernel)
    with_mean = mfa.GaussianProcessRegression((t, y), kernel, chol_obs_covariance=chol_r, mean_function=mean)
    mean_free = mfa.GaussianProcessRegression((t, y - mean(t)), kernel, chol_obs_covariance=chol_r)
    with_mean.fused = mean_free.fused = fused
    assert (with_mean._fused_log_likelihood_per_series() is not None) == fused
    assert float(with_mean.log_likelihood().cpu()) == pytest.approx(float(mean_free.log_likelihood().cpu()), rel=1e-9)
    new = torch.sort(torch.rand(batch + (20,), dtype=torch.float64, device=DEV) * (float(t.max()) + 1.0), dim=-1)[0]
    f_mean, f_var = with_mean.posterior.predict_f(new)
    f_mean0, f_var0 = mean_free.posterior.predict_f(new)
    np.testing.assert_allclose(nn(f_mean), nn(f_mean0 + mean(new)), rtol=1e-9, atol=1e-12)
    assert torch.equal(f_var, f_var0)
    y_mean, y_var = with_mean.posterior.predict_y(new)
    np.testing.assert_allclose(nn(y_mean), nn(f_mean), rtol=0, atol=0)
    np.testing.assert_allclose(nn(y_var), nn(f_var) + 0.1, rtol=1e-12)
    torch.manual_seed(0)
    s1 = with_mean.posterior.sample_f(new, 2)
    torch.manual_seed(0)
    s0 = mean_free.posterior.sample_f(new, 2)
    np.testing.assert_allclose(nn(s1), nn(s0 + mean(new)), rtol=1e-9, atol=1e-10)


def test_gpr_without_mean_function_hands_on_the_observations():
    t, y, _, _, chol_r = gpr_setup((2,), 15, 12)
    model = mfa.GaussianProcessRegression((t, y), sum_kernel(), chol_obs_covariance=chol_r, mean_function=None)
    assert model.mean_function is None and model._kalman._observations is y


@pytest.mark.parametrize("batch,n", [((), 15), ((2,), 130)], ids=["n15", "n130"])
def test_gpr_gradient_in_state_perturbations(batch, n):
    t, y, tau, u, chol_r = gpr_setup(batch, n, 13)
    kernel = sum_kernel()
    leaf = u.clone().requires_grad_(True)
    model = mfa.GaussianProcessRegression((t, y), kernel, chol_obs_covariance=chol_r,
                                          mean_function=MF.ImpulseMeanFunction(tau, leaf, kernel))
    (g_fused,) = torch.autograd.grad(model.log_likelihood(), leaf)
    # the same likelihood with the mean from the CPU float64 torch route
    leaf_cpu = u.cpu().clone().requires_grad_(True)
    mu = MF.ImpulseMeanFunction(tau.cpu(), leaf_cpu, sum_kernel(device="cpu"))(t.cpu())
    ll = mfa.GaussianProcessRegression((t, y - mu.to(DEV)), kernel, chol_obs_covariance=chol_r).log_likelihood()
    (g_cpu,) = torch.autograd.grad(ll, leaf_cpu)
    np.testing.assert_allclose(nn(g_fused), nn(g_cpu), rtol=1e-8, atol=1e-10)


def test_in_place_update_is_seen():
    t, y, tau, u, chol_r = gpr_setup((2,), 130, 17)
    kernel = sum_kernel()
    model = mfa.GaussianProcessRegression((t, y), kernel, chol_obs_covariance=chol_r,
                                          mean_function=MF.StepMeanFunction(tau, u, kernel))
    before = float(model.log_likelihood().cpu())
    with torch.no_grad():
        u.mul_(-0.5)
    after = float(model.log_likelihood().cpu())
    fresh = mfa.GaussianProcessRegression((t, y), kernel, chol_obs_covariance=chol_r,
                                          mean_function=MF.StepMeanFunction(tau, u.clone(), kernel))
    assert after != before and after == pytest.approx(float(fresh.log_likelihood().cpu()), rel=1e-12)


@pytest.mark.parametrize("mode", list(CLASSES))
def test_non_contiguous_inputs(mode):
    tau, u, t = draw((3,), 5, 50, 19)
    kernel = sum_kernel()
    wide_u = torch.tensor(np.concatenate([u, u], axis=-1), device=DEV)[..., :5]       # a strided view
    wide_t = torch.tensor(np.stack([t, t], axis=-1), device=DEV)[..., 0]
    assert not wide_u.is_contiguous() and not wide_t.is_contiguous()
    got = CLASSES[mode](torch.tensor(tau, device=DEV), wide_u, kernel)(wide_t)
    want = CLASSES[mode](torch.tensor(tau, device=DEV), wide_u.contiguous(), kernel)(wide_t.contiguous())
    assert torch.equal(got, want)
