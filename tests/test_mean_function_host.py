"""
CPU tests of ``markovflow_amd.mean_function`` (float64, the torch route): ports of the reference's unit tests
(tests/unit/test_mean_function.py), the numpy reference tests/helpers/mean_function_closed_forms.py against ``scipy.linalg.expm``, the
edge cases of the bin rule, gradients, the error cases, the ``GaussianProcessRegression`` constructor, and the presence of the new
symbols in the C header, the ctypes table and ``__all__``.
"""
import os
import re

import numpy as np
import pytest
import scipy.linalg
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from markovflow_amd import kernels as K
from markovflow_amd import mean_function as MF
from helpers import mean_function_closed_forms as MC

EXPECTED_RANGE = 12.0
BATCHES = [(), (3,), (2, 2)]
NEW_SYMBOLS = ["mf_mean_response_f64", "mf_mean_response_f32", "mf_mean_response_grad_f64", "mf_mean_response_grad_f32",
               "mf_mean_response_grad_workspace_bytes"]


def setup_actions(batch, seed=0, num=5):
    rng = np.random.default_rng(seed)
    kernel = K.Matern32(lengthscale=1.0, variance=1.0)
    u = torch.tensor(rng.standard_normal(batch + (num, 2)))
    tau = torch.tensor(np.sort(rng.uniform(0.0, EXPECTED_RANGE, size=batch + (num,)), axis=-1))
    return kernel, tau, u


def project(kernel, tau, u):
    return kernel.generate_emission_model(tau).project_state_to_f(u)


# ---- ports of the reference's unit tests ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", BATCHES, ids=str)
def test_around_impulse(batch):
    kernel, tau, u = setup_actions(batch)
    mean = MF.ImpulseMeanFunction(tau, u, kernel)
    np.testing.assert_allclose(mean(tau - 1e-15) + project(kernel, tau, u), mean(tau + 1e-15), atol=1e-10)


@pytest.mark.parametrize("batch", BATCHES, ids=str)
def test_on_impulse(batch):
    kernel, tau, u = setup_actions(batch)
    mean = MF.ImpulseMeanFunction(tau, u, kernel)
    np.testing.assert_allclose(mean(tau - 1e-15), mean(tau), atol=1e-10)


@pytest.mark.parametrize("batch", BATCHES, ids=str)
def test_far_from_impulse(batch):
    kernel, tau, u = setup_actions(batch)
    np.testing.assert_allclose(MF.ImpulseMeanFunction(tau, u, kernel)(tau + 10 * EXPECTED_RANGE), 0.0, atol=1e-10)


@pytest.mark.parametrize("cls", [MF.ImpulseMeanFunction, MF.StepMeanFunction], ids=["impulse", "step"])
@pytest.mark.parametrize("batch", BATCHES, ids=str)
def test_before_first_action_is_exactly_zero(batch, cls):
    kernel, tau, u = setup_actions(batch)
    out = cls(tau, u, kernel)(tau[..., :1] - 1e-6)
    assert out.shape == batch + (1, 1) and bool(torch.all(out == 0.0))


@pytest.mark.parametrize("batch", BATCHES, ids=str)
def test_around_step(batch):
    kernel, tau, u = setup_actions(batch)
    mean = MF.StepMeanFunction(tau, u, kernel)
    np.testing.assert_allclose(mean(tau - 1e-15), mean(tau + 1e-15), atol=1e-10)


@pytest.mark.parametrize("batch", BATCHES, ids=str)
def test_far_from_step(batch):
    rng = np.random.default_rng(3)
    tau = torch.tensor(np.broadcast_to(np.array([-10.0, 90.0, 190.0]), batch + (3,)).copy())
    kernel = K.Matern32(lengthscale=3.0, variance=1.0)
    u = torch.tensor(rng.standard_normal(batch + (3, 2)))
    expect = project(kernel, tau, torch.einsum("ij,...j->...i", -torch.linalg.inv(kernel.feedback_matrix), u))
    np.testing.assert_allclose(MF.StepMeanFunction(tau, u, kernel)(tau + 99.0), expect, atol=1e-10)


def test_single_impulse_against_expm():
    u = np.array([[2.3, 1.2]])
    kernel = K.Matern32(lengthscale=3.0, variance=1.0)
    mean = MF.ImpulseMeanFunction(torch.tensor([0.0], dtype=torch.float64), torch.tensor(u), kernel)
    t = np.linspace(0.01, 12.0, 100)
    f = kernel.feedback_matrix.numpy()
    expect = np.stack([scipy.linalg.expm(f * x) @ u[0] for x in t])[:, :1]
    np.testing.assert_allclose(mean(torch.tensor(t)).numpy(), expect, rtol=1e-7, atol=1e-12)


def test_single_step_against_expm():
    u = np.array([[2.3, 1.2]])
    kernel = K.Matern32(lengthscale=3.0, variance=1.0)
    mean = MF.StepMeanFunction(torch.tensor([0.0], dtype=torch.float64), torch.tensor(u), kernel)
    t = np.linspace(0.0, 12.0, 1001)
    f = kernel.feedback_matrix.numpy()
    f_inv_u = np.linalg.solve(f, u[0])
    expect = np.stack([scipy.linalg.expm(f * x) @ f_inv_u - f_inv_u for x in t])[:, :1]
    np.testing.assert_allclose(mean(torch.tensor(t)).numpy(), expect, rtol=1e-7, atol=1e-12)


@pytest.mark.parametrize("batch", BATCHES, ids=str)
def test_zero_function(batch):
    t = torch.tensor(np.random.default_rng(0).uniform(0, EXPECTED_RANGE, size=batch + (7,)))
    out = MF.ZeroMeanFunction(obs_dim=3)(t)
    assert out.shape == batch + (7, 3) and out.dtype == t.dtype and bool(torch.all(out == 0))


@pytest.mark.parametrize("batch", BATCHES, ids=str)
def test_linear_function(batch):
    t = torch.tensor(np.random.default_rng(0).uniform(0, EXPECTED_RANGE, size=batch + (7,)))
    coef = torch.tensor(3.1, dtype=torch.float64, requires_grad=True)
    out = MF.LinearMeanFunction(coefficient=coef, obs_dim=3)(t)
    np.testing.assert_allclose(out.detach().numpy(), np.broadcast_to(3.1 * t.numpy()[..., None], batch + (7, 3)))
    (grad,) = torch.autograd.grad(out.sum(), coef)
    np.testing.assert_allclose(float(grad), 3.0 * float(t.sum()))
    np.testing.assert_allclose(MF.LinearMeanFunction(2.0)(t).numpy(), 2.0 * t.numpy()[..., None])


# ---- the helper ---------------------------------------------------------------------------------------------------------------------
SIGNATURES = {
    "m12": [(1, 0, 0.7, 0.0)],
    "m32": [(3, 0, 1.3, 0.0)],
    "m52": [(5, 0, 0.9, 0.0)],
    "m32xosc": [(3, 1, 1.1, 2.0)],
    "oscxm52": [(5, 2, 0.8, 1.5)],
    "constxosc": [(0, 1, 0.0, 0.6)],
    "const+m32": [(0, 0, 0.0, 0.0), (3, 0, 1.3, 0.0)],
}


@pytest.mark.parametrize("name", list(SIGNATURES))
def test_helper_against_scipy(name):
    """A sanity bound on the helper, not a tolerance on the code under test."""
    comps = SIGNATURES[name]
    f = MC.feedback(comps).astype(np.float64)
    gaps = np.array([0.0, 1e-3, 0.3, 2.0, 9.0])
    e = MC.transition(comps, gaps).astype(np.float64)
    for k, g in enumerate(gaps):
        assert np.max(np.abs(e[k] - scipy.linalg.expm(g * f))) < 1e-12
    assert np.array_equal(MC.transition(comps, np.zeros(1))[0], np.eye(MC.state_dim(comps)))


def test_helper_direct_sums_agree_with_the_linear_map():
    comps = [(3, 0, 1.3, 0.0), (5, 0, 0.9, 0.0)]
    rng = np.random.default_rng(5)
    tau = np.array([0.5, 1.0, 1.0, 2.5])
    u = rng.standard_normal((4, 5))
    t = np.array([0.1, 0.5, 0.7, 1.0, 1.2, 2.5, 3.0, 40.0])
    m_r, m_a = MC.linear_map(comps, tau, t)
    np.testing.assert_allclose(np.einsum("nikj,kj->ni", m_r, u).astype(float), MC.impulse_state(comps, tau, u, t).astype(float),
                               rtol=1e-15, atol=1e-17)
    r, a = MC.step_sources(comps, u)
    via_map = np.einsum("nikj,kj->ni", m_r, r) + np.einsum("nikj,kj->ni", m_a, a)
    np.testing.assert_allclose(via_map.astype(float), MC.step_state(comps, tau, u, t).astype(float), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(MC.recurrence(comps, tau, r, a, t, np.float64), via_map.astype(float), rtol=1e-12, atol=1e-14)
    g = rng.standard_normal((8, 5))
    g_r, g_a = MC.reverse_recurrence(comps, tau, t, g, np.float64)
    np.testing.assert_allclose(g_r, np.einsum("nikj,ni->kj", m_r, g).astype(float), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(g_a, np.einsum("nikj,ni->kj", m_a, g).astype(float), rtol=1e-12, atol=1e-14)


def build_kernel(name):
    two_pi = 2.0 * np.pi
    if name == "m12":
        return K.Matern12(1.0 / 0.7, 1.0)
    if name == "m32":
        return K.Matern32(np.sqrt(3.0) / 1.3, 1.0)
    if name == "m52":
        return K.Matern52(np.sqrt(5.0) / 0.9, 1.0)
    if name == "m32xosc":
        return K.Product([K.Matern32(np.sqrt(3.0) / 1.1, 1.0), K.HarmonicOscillator(1.0, two_pi / 2.0)])
    if name == "oscxm52":
        return K.Product([K.HarmonicOscillator(1.0, two_pi / 1.5), K.Matern52(np.sqrt(5.0) / 0.8, 1.0)])
    if name == "constxosc":
        return K.Product([K.Constant(2.0), K.HarmonicOscillator(1.0, two_pi / 0.6)])
    return K.Sum([K.Constant(2.0), K.Matern32(np.sqrt(3.0) / 1.3, 1.0)], jitter=1e-6)


@pytest.mark.parametrize("name", list(SIGNATURES))
def test_torch_route_against_the_helper(name):
    comps = SIGNATURES[name]
    kernel = build_kernel(name)
    d = MC.state_dim(comps)
    assert kernel.state_dim == d
    np.testing.assert_allclose(kernel.feedback_matrix.numpy(), MC.feedback(comps).astype(float), rtol=1e-13, atol=1e-15)
    rng = np.random.default_rng(11)
    tau = np.array([0.5, 1.0, 1.0, 2.5])
    u = rng.standard_normal((4, d))
    t = np.array([3.0, 0.1, 0.5, 0.7, 1.0, 1.2, 2.5, 40.0])                       # (unsorted)
    h = MC.emission(comps, [0] * len(comps), 1)
    got = MF.ImpulseMeanFunction(torch.tensor(tau), torch.tensor(u), kernel)(torch.tensor(t)).numpy()
    np.testing.assert_allclose(got, (MC.impulse_state(comps, tau, u, t) @ h.T).astype(float), rtol=1e-11, atol=1e-13)
    if name != "const+m32":
        got = MF.StepMeanFunction(torch.tensor(tau), torch.tensor(u), kernel)(torch.tensor(t)).numpy()
        np.testing.assert_allclose(got, (MC.step_state(comps, tau, u, t) @ h.T).astype(float), rtol=1e-10, atol=1e-12)


# ---- edge cases of the bin rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [MF.ImpulseMeanFunction, MF.StepMeanFunction], ids=["impulse", "step"])
def test_long_before_the_first_action_is_zero_not_nan(cls):
    kernel = K.Matern32(0.5, 1.0)
    mean = cls(torch.tensor([0.0, 1.0], dtype=torch.float64), torch.ones(2, 2, dtype=torch.float64), kernel)
    out = mean(torch.tensor([-1e6, -1.0, 0.0], dtype=torch.float64))
    assert bool(torch.all(out == 0.0)) and not bool(torch.isnan(out).any())


def test_two_impulses_at_one_time_add():
    kernel = K.Matern32(0.8, 1.0)
    u = torch.tensor([[1.0, -0.5], [0.25, 2.0]], dtype=torch.float64)
    t = torch.tensor([0.9, 1.0, 1.3, 4.0], dtype=torch.float64)
    both = MF.ImpulseMeanFunction(torch.tensor([1.0, 1.0], dtype=torch.float64), u, kernel)(t)
    one = MF.ImpulseMeanFunction(torch.tensor([1.0], dtype=torch.float64), u.sum(dim=0, keepdim=True), kernel)(t)
    np.testing.assert_allclose(both.numpy(), one.numpy(), rtol=1e-14, atol=1e-16)


def test_unsorted_time_points():
    kernel, tau, u = setup_actions((2,), seed=4)
    mean = MF.StepMeanFunction(tau, u, kernel)
    t = torch.tensor(np.random.default_rng(1).uniform(-1.0, 15.0, size=(2, 9)))
    perm = torch.tensor([4, 0, 8, 2, 6, 1, 7, 3, 5])
    assert torch.equal(mean(t[:, perm]), mean(t)[:, perm])


# ---- gradients ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [MF.ImpulseMeanFunction, MF.StepMeanFunction], ids=["impulse", "step"])
def test_gradcheck_state_perturbations(cls):
    kernel, tau, u = setup_actions((2,), seed=7, num=3)
    t = torch.tensor(np.random.default_rng(2).uniform(-1.0, 14.0, size=(2, 6)))
    u = u.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: cls(tau, x, kernel)(t), (u,))


@pytest.mark.parametrize("cls", [MF.ImpulseMeanFunction, MF.StepMeanFunction], ids=["impulse", "step"])
def test_gradcheck_lengthscale(cls):
    _, tau, u = setup_actions((), seed=8, num=3)
    t = torch.tensor(np.random.default_rng(3).uniform(-1.0, 14.0, size=(6,)))
    ell = torch.tensor(1.3, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda x: cls(tau, u, K.Matern32(x, 1.0))(t), (ell,))


@pytest.mark.parametrize("cls", [MF.ImpulseMeanFunction, MF.StepMeanFunction], ids=["impulse", "step"])
def test_nan_time_point_and_mixed_dtypes(cls):
    """A NaN query time gives a NaN mean; a float64 kernel with float32 data is cast to the data's dtype."""
    kernel = K.Sum([K.Matern32(1.0, 1.0), K.Product([K.Constant(2.0), K.HarmonicOscillator(1.0, 2.0)])], jitter=1e-6)
    tau = torch.tensor([0.5, 1.0], dtype=torch.float32)
    t = torch.tensor([0.0, float("nan"), 0.7, 3.0], dtype=torch.float32)
    out = cls(tau, torch.ones(2, 4, dtype=torch.float32), kernel)(t)
    assert out.dtype == torch.float32 and out[0, 0] == 0 and bool(torch.isnan(out[1, 0])) and bool(torch.isfinite(out[2:]).all())
    one = K.Sum([K.Constant(2.0), K.Matern12(1.0, 1.0)], jitter=1e-6)                # (an order-0 block [1] does not carry a NaN gap)
    out = MF.ImpulseMeanFunction(tau.double(), torch.ones(2, 2, dtype=torch.float64), one)(t.double())
    assert bool(torch.isnan(out[1, 0])) and bool(torch.isfinite(out[2:]).all())


def test_in_place_update_is_seen():
    kernel, tau, u = setup_actions(())
    mean = MF.StepMeanFunction(tau, u, kernel)
    t = tau + 0.3
    before = mean(t).clone()
    with torch.no_grad():
        u.mul_(2.0)
    np.testing.assert_allclose(mean(t).numpy(), 2.0 * before.numpy(), rtol=1e-13)


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def test_error_cases():
    kernel, tau, u = setup_actions((2,))
    for cls in (MF.ImpulseMeanFunction, MF.StepMeanFunction):
        with pytest.raises(ValueError, match="action_times has shape"):
            cls(tau[:, :4], u, kernel)
        with pytest.raises(ValueError, match="state dimension"):
            cls(tau, u[..., :1], kernel)
        with pytest.raises(ValueError, match="at least one action"):
            cls(tau[:, :0], u[:, :0], kernel)
        with pytest.raises(ValueError):
            cls(tau.float(), u, kernel)
        with pytest.raises(TypeError):
            cls(tau, u, "kernel")
        with pytest.raises((ValueError, TypeError)):
            cls(tau, u, kernel)(tau.float())
        with pytest.raises(ValueError, match="batch shape"):
            cls(tau, u, kernel)(tau[0])
        with pytest.raises(NotImplementedError):
            cls(tau, u, K.PiecewiseKernel([K.Matern32(1.0, 1.0), K.Matern32(2.0, 1.0)], torch.tensor([5.0], dtype=torch.float64)))
    t1, u1 = tau[0], torch.ones(5, 1, dtype=torch.float64)
    with pytest.raises(ValueError, match="singular"):
        MF.StepMeanFunction(t1, u1, K.Constant(1.0))
    with pytest.raises(ValueError, match="singular"):
        MF.StepMeanFunction(t1, torch.ones(5, 3, dtype=torch.float64), K.Sum([K.Constant(1.0), K.Matern32(1.0, 1.0)], jitter=1e-6))
    with pytest.raises(ValueError, match="singular"):
        MF.StepMeanFunction(t1, u1, K.Product([K.Constant(1.0), K.Constant(2.0)]))
    MF.ImpulseMeanFunction(t1, u1, K.Constant(1.0))                               # (an impulse needs no inverse)
    MF.StepMeanFunction(t1, torch.ones(5, 2, dtype=torch.float64), K.Product([K.Constant(1.0), K.HarmonicOscillator(1.0, 2.0)]))


def test_spatio_temporal_kernel_is_refused():
    from markovflow_amd import spatial_kernels
    st = K.SparseSpatioTemporalKernel(spatial_kernels.SquaredExponential(1.0, 1.0), K.Matern32(1.0, 1.0),
                                      torch.zeros(2, 1, dtype=torch.float64))
    with pytest.raises(NotImplementedError):
        MF.ImpulseMeanFunction(torch.zeros(1, dtype=torch.float64), torch.zeros(1, st.state_dim, dtype=torch.float64), st)


# ---- GaussianProcessRegression ------------------------------------------------------------------------------------------------------------
def test_gpr_constructor():
    kernel, tau, u = setup_actions(())
    t = torch.linspace(0.0, 10.0, 12, dtype=torch.float64)
    y = torch.zeros(12, 1, dtype=torch.float64)
    model = mfa.GaussianProcessRegression((t, y), kernel)
    assert model.mean_function is None and model._residuals() is y
    model = mfa.GaussianProcessRegression((t, y), kernel, mean_function=None)
    assert model._residuals() is y
    # _kalman on CPU tensors: the kernel's chain comes from the HIP generator, so the torch restatement stands in for it
    a_s, chol, _ = kernel._torch_transitions(K.to_delta_time(t), True, False)
    kernel.state_space_model = lambda tp: mfa.StateSpaceModel(torch.zeros(2, dtype=tp.dtype), torch.eye(2, dtype=tp.dtype), a_s,
                                                              torch.zeros(11, 2, dtype=tp.dtype), chol)
    assert model._kalman._observations is y
    del kernel.state_space_model
    mean = MF.ImpulseMeanFunction(tau, u, kernel)
    model = mfa.GaussianProcessRegression((t, y), kernel, None, mean)
    assert model.mean_function is mean
    np.testing.assert_allclose(model._residuals().numpy(), -mean(t).numpy())
    with pytest.raises(ValueError, match="output dimension"):
        mfa.GaussianProcessRegression((t, y), kernel, mean_function=MF.ZeroMeanFunction(2))
    with pytest.raises(ValueError, match="output dimension"):
        mfa.GaussianProcessRegression((t, y), kernel, mean_function=lambda x: torch.zeros(tuple(x.shape) + (3,)))
    with pytest.raises(TypeError):
        mfa.GaussianProcessRegression((t, y), kernel, mean_function=3.0)


def test_posterior_processes_take_a_mean_function():
    import inspect
    from markovflow_amd import posterior
    for cls in (posterior.ConditionalProcess, posterior.AnalyticPosteriorProcess):
        params = list(inspect.signature(cls.__init__).parameters.values())
        assert params[-1].name == "mean_function" and params[-1].default is None


# ---- the public surface -------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_everywhere():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "markovflow_amd.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.exported_symbols()
    for name in ("MeanFunction", "ZeroMeanFunction", "LinearMeanFunction", "ImpulseMeanFunction", "StepMeanFunction", "mean_function"):
        assert name in mfa.__all__ and hasattr(mfa, name)
    assert mfa.mean_function is MF and MF.fused is True
