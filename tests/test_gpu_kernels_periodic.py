"""
GPU parity tests of the periodic and quasi-periodic kernels (markovflow_amd/kernels.py: Constant, HarmonicOscillator, Product;
csrc/mf_sde.hip: mf_sde_transitions_*, mf_sde_transitions_grad_*): the device-generated tensors against the numpy closed forms
of tests/helpers/periodic_closed_forms.py, the GPR log marginal likelihood, its gradients and its predictions against a dense GP
with k(r) = sum_c var_c k_c(r) cos(omega_c r), and the filter on order-0 components against the numpy oracle.
Tolerances are those of tests/test_gpu_kernels.py and tests/test_gpu_gpr_grad.py.
"""
import ctypes

import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from oracle import numpy_oracle as O
from helpers import periodic_closed_forms as PC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MATERN = {1: mfa.Matern12, 3: mfa.Matern32, 5: mfa.Matern52}
BSZ, T = 3, 40


def tt(x, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device=DEV)


def nn(x):
    return x.detach().cpu().numpy().astype(np.float64)


def times(rng, bsz=BSZ, n=T):
    return np.cumsum(0.05 + rng.exponential(0.2, size=(bsz, n)), axis=-1)


def build(comps, jitter=0.0, dtype=torch.float64):
    """The kernel a list of component descriptions (tests/helpers/periodic_closed_forms.py) stands for: a Sum of Constant,
    HarmonicOscillator, Matern and Matern * HarmonicOscillator (Product in the list order `osc` says); a factor's variances multiply
    to the component's."""
    parts = []
    for c in comps:
        if c["order"] == 0:
            k = (mfa.HarmonicOscillator(c["var"], c["period"], device=DEV, dtype=dtype) if c["osc"]
                 else mfa.Constant(c["var"], device=DEV, dtype=dtype))
        elif not c["osc"]:
            k = MATERN[c["order"]](c["ls"], c["var"], device=DEV, dtype=dtype)
        else:
            pair = [MATERN[c["order"]](c["ls"], c["var"] / 0.8, device=DEV, dtype=dtype),
                    mfa.HarmonicOscillator(0.8, c["period"], device=DEV, dtype=dtype)]
            k = mfa.Product(pair if c["osc"] == 1 else pair[::-1], jitter=jitter)
        parts.append(k)
    if len(parts) == 1 and isinstance(parts[0], mfa.Product):
        return parts[0]
    return mfa.Sum(parts, jitter=jitter)


def qp(order, osc=1, ls=0.7, var=1.3, period=1.7):
    return {"order": order, "ls": ls, "var": var, "period": period, "osc": osc}


HO = {"order": 0, "var": 0.8, "period": 1.7, "osc": 1}
CONST = {"order": 0, "var": 1.5, "osc": 0}
M32 = {"order": 3, "ls": 0.9, "var": 0.6, "osc": 0}

GENERATOR_CASES = {"oscillator": [HO], "constant": [CONST], "sum9": [CONST, qp(5, 2), M32]}
for _o in (1, 3, 5):
    for _r in (1, 2):
        GENERATOR_CASES[f"m{_o}2xho_osc{_r}"] = [qp(_o, _r)]


def check_generated(kern, comps_per_series, t, jitter, dtype):
    """A, chol Q chol Q^T and Q, P-infinity, P0 and the emission matrix of `kern` on the time points t [B, T] against the closed
    forms (one component list per series).  The reference is evaluated at the time gaps the device sees: those of the time points
    rounded to `dtype`."""
    tol = dict(rtol=1e-10, atol=1e-12) if dtype == torch.float64 else dict(rtol=2e-5, atol=2e-6)
    tol_q = dict(rtol=tol["rtol"] * 100, atol=tol["atol"] * 100)
    tdev = tt(t, dtype)
    dt = np.diff(nn(tdev), axis=-1)
    ssm = kern.state_space_model(tdev)
    a_s, q_s = kern.transition_statistics_from_time_points(tdev)
    assert torch.equal(a_s, ssm.state_transitions)
    chol = nn(ssm.cholesky_process_covariances)
    assert np.all(np.triu(chol, 1) == 0) and np.all(np.isfinite(chol))
    d = kern.state_dim
    pinf = nn(kern.steady_state_covariance)
    for s, comps in enumerate(comps_per_series):
        a_ref, q_ref, p_ref = PC.concat_transitions(comps, dt[s], jitter=jitter)
        assert a_ref.shape[-1] == d
        np.testing.assert_allclose(nn(a_s)[s], a_ref, **tol)
        np.testing.assert_allclose(chol[s] @ np.swapaxes(chol[s], -1, -2), q_ref, **tol_q)
        np.testing.assert_allclose(nn(q_s)[s], q_ref, **tol_q)
        np.testing.assert_allclose(pinf[s] if pinf.ndim == 3 else pinf, p_ref, **tol)
        np.testing.assert_allclose(nn(ssm.initial_covariance)[s], p_ref + jitter * np.eye(d), **tol)
    np.testing.assert_array_equal(nn(kern.generate_emission_model(tdev).emission_matrix), PC.emission(comps_per_series[0], t.shape))


# ---- 1. generator against the closed forms ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", sorted(GENERATOR_CASES))
def test_generator_vs_closed_forms(rng, case, dtype):
    comps = GENERATOR_CASES[case]
    kern = build(comps, jitter=1e-6, dtype=dtype)
    assert kern.state_dim == sum(PC.size(c) for c in comps)
    check_generated(kern, [comps] * BSZ, times(rng), 1e-6, dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_generator_per_series_period_and_variance(rng, dtype):
    per, var = 0.9 + 1.5 * rng.random(BSZ), 0.5 + rng.random(BSZ)
    kern = mfa.Product([mfa.Matern52(0.7, 1.3, device=DEV, dtype=dtype), mfa.HarmonicOscillator(tt(var, dtype), tt(per, dtype))],
                       jitter=1e-6)
    per, var = nn(kern.kernels[1].period), nn(kern.kernels[1].variance)          # (as rounded to dtype)
    check_generated(kern, [[qp(5, 1, var=1.3 * var[s], period=per[s])] for s in range(BSZ)], times(rng), 1e-6, dtype)


# ---- 2. zero time gap ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("osc", [1, 2])
def test_zero_time_gap_gives_identity_and_zero_cholesky(osc):
    """dt = 0: cos 0 = 1, sin 0 = 0 exactly, so A = I, Q = 0 and the all-zero covariance passes through as a zero factor."""
    kern = build([qp(3, osc)])
    ssm = kern.state_space_model(tt(np.array([[0.0, 0.5, 0.5, 1.0]])))
    assert np.all(nn(ssm.state_transitions)[0, 1] == np.eye(4))
    assert np.all(nn(ssm.cholesky_process_covariances)[0, 1] == 0)
    assert np.all(np.isfinite(nn(ssm.cholesky_process_covariances)))
    assert np.all(np.diagonal(nn(ssm.cholesky_process_covariances)[0, 0]) > 0)


# ---- 3. / 4. log marginal likelihood against a dense GP ------------------------------------------------------------------------------
def dense_total(comps, t, y, noise):
    return sum(PC.dense_log_marginal(comps, t[s], y[s, :, 0], noise) for s in range(t.shape[0]))


@pytest.mark.parametrize("case,bsz", [("m32xho_d4", 3), ("m52xho_d6", 3), ("sum_d8", 3), ("sum_d16", 2)])
def test_gpr_log_likelihood_vs_dense_gp(rng, case, bsz):
    """d = 4: register kernels, d = 6: the headline kernel's dimension, d = 8: row kernels, d = 16: wave kernels."""
    comps = {"m32xho_d4": [qp(3, 1)], "m52xho_d6": [qp(5, 2)], "sum_d8": [qp(5, 1), M32],
             "sum_d16": [qp(5, 1), qp(5, 2, ls=1.1, var=0.7, period=0.9), qp(3, 1, ls=0.5, var=0.4, period=3.1)]}[case]
    noise = 0.1
    t, y = times(rng, bsz), rng.normal(size=(bsz, T, 1))
    kern = build(comps)
    assert kern.state_dim == int(case.rsplit("_d", 1)[1])
    gpr = mfa.GaussianProcessRegression((tt(t), tt(y)), kern, chol_obs_covariance=tt(np.sqrt(noise) * np.eye(1)))
    assert gpr._fused_log_likelihood_per_series() is None            # the fused GPR kernels are Matern-only
    want = dense_total(comps, t, y, noise)
    got = float(gpr.log_likelihood().cpu())
    print(f"{case}: state space {got!r}, dense {want!r}, rel {abs(got - want) / abs(want):.2e}")
    assert got == pytest.approx(want, rel=1e-9)


# ---- 5. order-0 components through the filter ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [HO, CONST], ids=["oscillator", "constant"])
def test_order0_components_through_the_filter(rng, first):
    comps, jitter, noise = [first, M32], 1e-6, 0.1
    t, y = times(rng), rng.normal(size=(BSZ, T, 1))
    kern = build(comps, jitter=jitter)
    kf = mfa.KalmanFilter(kern.state_space_model(tt(t)), kern.generate_emission_model(tt(t)), tt(y), tt(np.sqrt(noise) * np.eye(1)))
    a_s, q_s, pinf = PC.concat_transitions(comps, np.diff(t, axis=-1), jitter=jitter)
    d = pinf.shape[-1]
    chol_p0 = np.broadcast_to(np.linalg.cholesky(pinf + jitter * np.eye(d)), (BSZ, d, d)).copy()
    want = float(O.kf_log_likelihood(np.zeros((BSZ, d)), chol_p0, a_s, np.zeros((BSZ, T - 1, d)), np.linalg.cholesky(q_s),
                                     PC.emission(comps, t.shape), y, np.eye(1) / noise))
    got = float(kf.log_likelihood().cpu())
    print(f"{first}: filter {got!r}, oracle {want!r}, rel {abs(got - want) / abs(want):.2e}")
    assert got == pytest.approx(want, rel=1e-9)


# ---- 6. gradients -----------------------------------------------------------------------------------------------------------------
def count_calls(monkeypatch):
    seen = []
    real = _lib.call

    def spy(name, *args):
        seen.append(name)
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", spy)
    return seen


@pytest.mark.parametrize("per_series", [False, True], ids=["shared", "per-series"])
@pytest.mark.parametrize("osc", [1, 2])
def test_generator_backward_equals_autograd_through_the_closed_forms(rng, monkeypatch, osc, per_series):
    """state_space_model(t) through the HIP Function (mf_sde_transitions_* forward, mf_sde_transitions_grad_* backward) and through
    the torch restatement of the closed forms (time points that require a gradient take that route): the gradients of a random
    linear functional of (A, chol Q) with respect to lengthscale, both variances and period."""
    shape = (BSZ,) if per_series else ()
    leaves = [tt(lo + rng.random(shape)).requires_grad_(True) for lo in (0.5, 0.5, 0.5, 1.0)]    # lengthscale, variances, period
    pair = [mfa.Matern52(leaves[0], leaves[1]), mfa.HarmonicOscillator(leaves[2], leaves[3])]
    kern = mfa.Product(pair if osc == 1 else pair[::-1], jitter=1e-8)
    t = tt(times(rng))
    w_a, w_c = tt(rng.normal(size=(BSZ, T - 1, 6, 6))), torch.tril(tt(rng.normal(size=(BSZ, T - 1, 6, 6))))
    seen = count_calls(monkeypatch)
    ssm = kern.state_space_model(t)
    (torch.sum(w_a * ssm.state_transitions) + torch.sum(w_c * ssm.cholesky_process_covariances)).backward()
    assert seen.count("mf_sde_transitions") == 1 and seen.count("mf_sde_transitions_grad") == 1
    got = [x.grad.clone() for x in leaves]
    for x in leaves:
        x.grad = None
    del seen[:]
    ssm_t = kern.state_space_model(t.clone().requires_grad_(True))
    assert "mf_sde_transitions" not in seen
    np.testing.assert_allclose(nn(ssm.state_transitions), nn(ssm_t.state_transitions), rtol=1e-12, atol=1e-14)
    # The two factors are compared through chol chol^T = Q, not entry by entry: at these gaps and jitter the smallest pivots of a
    # Matern-5/2 block are ~1e-4 and the entries that are zero in exact arithmetic (Q = Q^M (x) I2) are rounding noise of Q divided
    # by them, 1e-10 in either route.  Q = Pinf - A Pinf A^T is a sum of 36 products per entry, each bounded by max|A|^2 max|Pinf|,
    # and a Cholesky factor reproduces its matrix to a few eps of the same size: 100 eps max|A|^2 max|Pinf| covers both routes.
    c_hip, c_torch = nn(ssm.cholesky_process_covariances), nn(ssm_t.cholesky_process_covariances)
    assert np.all(np.triu(c_hip, 1) == 0) and np.all(np.isfinite(c_hip))
    bound = 100 * np.finfo(np.float64).eps * np.abs(nn(ssm.state_transitions)).max() ** 2 * np.abs(nn(kern.steady_state_covariance)).max()
    np.testing.assert_allclose(c_hip @ np.swapaxes(c_hip, -1, -2), c_torch @ np.swapaxes(c_torch, -1, -2), rtol=0, atol=bound)
    (torch.sum(w_a * ssm_t.state_transitions) + torch.sum(w_c * ssm_t.cholesky_process_covariances)).backward()
    for g, x in zip(got, leaves):
        np.testing.assert_allclose(nn(g), nn(x.grad), rtol=1e-8, atol=1e-10)


def test_gpr_backward_vs_dense_gp(rng, monkeypatch):
    """GaussianProcessRegression.log_likelihood().backward() for Matern32 * HarmonicOscillator against torch autograd through the
    dense marginal likelihood on the CPU."""
    t, y = times(rng), rng.normal(size=(BSZ, T))
    vals = {"l": 0.7, "vm": 1.3, "vo": 0.8, "p": 1.7, "s": 0.3}
    cpu = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in vals.items()}
    tc, yc = torch.tensor(t), torch.tensor(y)
    total = 0.0
    for s in range(BSZ):
        r = (tc[s][:, None] - tc[s][None, :]).abs()
        lam = np.sqrt(3.0) / cpu["l"]
        kmat = cpu["vm"] * cpu["vo"] * (1 + lam * r) * torch.exp(-lam * r) * torch.cos(2 * np.pi / cpu["p"] * r)
        kn = kmat + cpu["s"] ** 2 * torch.eye(T, dtype=torch.float64)
        total = total - 0.5 * (yc[s] @ torch.linalg.solve(kn, yc[s]) + torch.linalg.slogdet(kn)[1] + T * np.log(2 * np.pi))
    total.backward()
    dev = {k: torch.tensor(v, dtype=torch.float64, device=DEV, requires_grad=True) for k, v in vals.items()}
    kern = mfa.Matern32(dev["l"], dev["vm"]) * mfa.HarmonicOscillator(dev["vo"], dev["p"])
    gpr = mfa.GaussianProcessRegression((tt(t), tt(y[..., None])), kern, chol_obs_covariance=dev["s"].reshape(1, 1))
    seen = count_calls(monkeypatch)
    ll = gpr.log_likelihood()
    ll.backward()
    assert seen.count("mf_sde_transitions_grad") == 1, "the generator's HIP backward should have run"
    assert float(ll.detach()) == pytest.approx(float(total.detach()), rel=1e-9)
    for k in vals:
        np.testing.assert_allclose(nn(dev[k].grad), cpu[k].grad.numpy(), rtol=1e-6, atol=1e-9, err_msg=k)


# ---- 7. prediction ------------------------------------------------------------------------------------------------------------------
def test_posterior_predict_f_vs_dense_gp(rng):
    comps, noise = [qp(3, 1)], 0.05
    t, y = times(rng), rng.normal(size=(BSZ, T, 1))
    t_new = np.sort(np.concatenate([t[:, :1] - 0.1 - rng.random((BSZ, 2)), t[:, -1:] + 0.1 + rng.random((BSZ, 2)),
                                    t[:, :1] + rng.random((BSZ, 3)) * (t[:, -1:] - t[:, :1])], axis=-1), axis=-1)
    gpr = mfa.GaussianProcessRegression((tt(t), tt(y)), build(comps), chol_obs_covariance=tt(np.sqrt(noise) * np.eye(1)))
    post = gpr.posterior_state_space_model()
    assert post.state_dim == 4
    f_mean, f_var = gpr.posterior.predict_f(tt(t_new))
    assert tuple(f_mean.shape) == (BSZ, 7, 1) and tuple(f_var.shape) == (BSZ, 7, 1)
    for s in range(BSZ):
        mean, var = PC.dense_predict(comps, t[s], y[s, :, 0], noise, t_new[s])
        np.testing.assert_allclose(nn(f_mean)[s, :, 0], mean, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(nn(f_var)[s, :, 0], var, rtol=1e-5, atol=1e-7)


# ---- 8. unchanged behaviour ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_no_oscillator_is_bitwise_the_matern_generator(rng, dtype):
    """mf_sde_transitions_* with every oscillator flag 0 against mf_sde_matern_transitions_* for Sum(Matern52, Matern52)."""
    dt = tt(0.05 + rng.exponential(0.2, size=(BSZ, T - 1)), dtype)
    lam, var = tt(np.sqrt(5.0) / np.array([0.7, 1.8]), dtype), tt([1.3, 1.1], dtype)
    orders, oscs = (ctypes.c_int * 2)(5, 5), (ctypes.c_int * 2)(0, 0)
    old = [torch.full((BSZ, T - 1, 6, 6), float("nan"), dtype=dtype, device=DEV) for _ in range(3)]
    new = [x.clone() for x in old]
    _lib.call("mf_sde_matern_transitions", dtype, BSZ, T - 1, 2, orders, _lib.ptr(lam), _lib.ptr(var), 0, _lib.ptr(dt), 1e-6,
              *[_lib.ptr(x) for x in old], _lib.stream_ptr(dt.device))
    _lib.call("mf_sde_transitions", dtype, BSZ, T - 1, 2, orders, oscs, _lib.ptr(lam), _lib.ptr(var), None, 0, _lib.ptr(dt), 1e-6,
              *[_lib.ptr(x) for x in new], _lib.stream_ptr(dt.device))
    for a, b in zip(old, new):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def test_plain_matern_gpr_still_takes_the_fused_route(rng, monkeypatch):
    t, y = times(rng), rng.normal(size=(BSZ, T, 1))
    kern = mfa.Sum([mfa.Matern52(0.7, 1.3, device=DEV), mfa.Matern52(1.8, 1.1, device=DEV)])
    gpr = mfa.GaussianProcessRegression((tt(t), tt(y)), kern, chol_obs_covariance=tt(np.sqrt(0.1) * np.eye(1)))
    assert gpr._fused_log_likelihood_per_series() is not None
    seen = count_calls(monkeypatch)
    kern.state_space_model(tt(t))
    assert "mf_sde_matern_transitions" in seen and "mf_sde_transitions" not in seen     # ... and the Matern generator
