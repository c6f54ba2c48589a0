"""
GPU tests of ``markovflow_amd.sde`` through its public functions on HIP tensors: the fused routes against the torch routes on the same
device and against the long double closed forms of tests/helpers/sde_closed_forms.py, both dtypes, both drifts; the linearised chain
through ``StateSpaceModel``'s operators; the reference's ``test_KL_sde`` through ``StateSpaceModel.kl_divergence`` on the device; the
backward of the drift difference; and the routing of custom drifts and trainable parameters.
"""
import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import sde as S
from helpers import sde_closed_forms as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float64, torch.float32]
NP = {torch.float64: np.float64, torch.float32: np.float32}
LAM, Q = 2.0, 0.5


def tt(x, dtype):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device=DEV)


def make_sde(drift_id, q=((Q,),), nq=10):
    return S.OrnsteinUhlenbeckSDE(LAM, q, num_gauss_hermite_points=nq) if drift_id == 0 else S.DoubleWellSDE(q, num_gauss_hermite_points=nq)


class PythonDrift(S.SDE):
    """A user subclass with the built-ins' drift written in Python: no kernel stands for it."""

    def __init__(self, drift_id, q):
        super().__init__(1)
        self.drift_id, self.q = drift_id, torch.tensor([[q]], dtype=torch.float64)

    def drift(self, x, t):
        return -LAM * x if self.drift_id == 0 else 4.0 * x * (1.0 - x * x)

    def diffusion(self, x, t):
        return torch.ones_like(x[..., None]) * float(np.sqrt(float(self.q)))


def path(rng, shape, npd):
    return rng.uniform(-1.5, 1.5, shape + (1,)).astype(npd), rng.uniform(0.05, 0.6, shape + (1, 1)).astype(npd)


# ---- Euler-Maruyama --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("drift_id", [0, 1], ids=["ou", "double_well"])
def test_euler_maruyama_against_the_torch_route_and_long_double(drift_id, dtype):
    """Along a trajectory a rounding error of one step, at most 4 eps of the step's terms (below 4 in magnitude here), is amplified by
    at most ``exp(4 t)`` (the double well's largest slope) over ``t <= 37 * 0.02``: the routes may differ by
    ``2 * 37 * 16 eps * exp(2.96)`` and each from long double by half of that."""
    npd = NP[dtype]
    rng = np.random.default_rng(40 + drift_id)
    bsz, tn, d = 70, 37, 2
    q = np.array([[1.0, 0.3], [0.3, 0.5]])
    grid = np.concatenate([[0.0], np.cumsum(rng.uniform(0.002, 0.02, tn - 1))]).astype(npd)
    x0, noise = rng.uniform(-1.5, 1.5, (bsz, d)).astype(npd), rng.standard_normal((bsz, tn - 1, d)).astype(npd)
    sde = make_sde(drift_id, q)
    fused = S.euler_maruyama(sde, tt(x0, dtype), tt(grid, dtype), noise=tt(noise, dtype))
    plain = S.euler_maruyama_torch(sde, tt(x0, dtype), tt(grid, dtype), tt(noise, dtype))
    assert tuple(fused.shape) == (bsz, tn, d) and torch.equal(fused[:, 0], tt(x0, dtype))
    ref = SC.em_path(drift_id, npd(LAM), x0, grid, noise, np.linalg.cholesky(q).astype(npd))
    tol = 37 * 16 * float(np.finfo(npd).eps) * float(np.exp(2.96))
    e_f, e_p = (float(np.max(np.abs(t.cpu().numpy().astype(SC.LD) - ref))) for t in (fused, plain))
    print(f"fused - long double {e_f:.3e}, torch - long double {e_p:.3e}, allowed {tol:.3e}")
    assert e_f <= tol and e_p <= tol


def test_euler_maruyama_generator_routing_and_refusal():
    sde = make_sde(1)
    x0, grid = torch.zeros((5, 1), dtype=torch.float64, device=DEV), torch.linspace(0.0, 0.5, 26, dtype=torch.float64, device=DEV)
    runs = [S.euler_maruyama(sde, x0, grid, generator=torch.Generator(device=DEV).manual_seed(seed)) for seed in (7, 7, 8)]
    assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0], runs[2])
    with pytest.raises(NotImplementedError, match="not differentiable"):
        S.euler_maruyama(sde, x0.clone().requires_grad_(True), grid)
    with torch.no_grad():
        assert tuple(S.euler_maruyama(sde, x0.clone().requires_grad_(True), grid).shape) == (5, 26, 1)
    # a custom drift, a trainable decay and D > 4 take the torch route and agree with the kernel
    noise = torch.randn((5, 25, 1), dtype=torch.float64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    x1 = torch.full((5, 1), 0.7, dtype=torch.float64, device=DEV)
    for drift_id in (0, 1):
        fused = S.euler_maruyama(make_sde(drift_id), x1, grid, noise=noise)
        custom = S.euler_maruyama(PythonDrift(drift_id, Q), x1, grid, noise=noise)
        np.testing.assert_allclose(custom.cpu().numpy(), fused.cpu().numpy(), rtol=1e-12, atol=1e-13)
    decay = torch.tensor(LAM, dtype=torch.float64, device=DEV, requires_grad=True)
    trained = S.euler_maruyama(S.OrnsteinUhlenbeckSDE(decay, [[Q]]), x1, grid, noise=noise)
    np.testing.assert_allclose(trained.detach().cpu().numpy(), S.euler_maruyama(make_sde(0), x1, grid, noise=noise).cpu().numpy(), rtol=1e-12,
                               atol=1e-13)
    trained[:, -1].sum().backward()
    assert decay.grad is not None and bool(torch.isfinite(decay.grad))
    wide = S.euler_maruyama(S.DoubleWellSDE(np.eye(5)), torch.zeros((2, 5), dtype=torch.float64, device=DEV), grid)
    assert tuple(wide.shape) == (2, 26, 5) and bool(torch.isfinite(wide).all())


# ---- linearisation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("drift_id", [0, 1], ids=["ou", "double_well"])
def test_linearize_sde_against_the_torch_route_and_closed_forms(drift_id, dtype):
    npd = NP[dtype]
    rng = np.random.default_rng(50 + drift_id)
    bsz, n, nq = 3, 130, 10
    m, s = path(rng, (bsz, n), npd)
    times = np.concatenate([[0.5], 0.5 + np.cumsum(rng.uniform(0.002, 0.02, n))]).astype(npd)
    sde = make_sde(drift_id, nq=nq)
    args = (tt(times, dtype), (tt(m, dtype), tt(s, dtype)), (tt(m[:, 0], dtype), tt(s[:, 0], dtype)))
    ssm = S.linearize_sde(sde, *args)
    assert isinstance(ssm, mfa.StateSpaceModel) and ssm.state_dim == 1 and ssm.num_transitions == n
    plain = S.linearize_torch(sde, args[0], args[1][0][..., 0], args[1][1][..., 0, 0])
    got = (ssm.state_transitions[..., 0, 0], ssm.state_offsets[..., 0], ssm.cholesky_process_covariances[..., 0, 0])
    zeros = np.zeros((bsz, n), dtype=npd)
    ref7 = SC.reference_sums(drift_id, npd(LAM), nq, m[..., 0], s[..., 0, 0], zeros, zeros)
    mag7 = SC.gh_magnitudes(drift_id, npd(LAM), nq, m[..., 0], s[..., 0, 0], zeros, zeros)
    yard7 = SC.gh_sums(drift_id, npd(LAM), nq, m[..., 0], s[..., 0, 0], zeros, zeros, npd)
    dts = np.broadcast_to((times[1:] - times[:-1])[None, :], (bsz, n))
    chol_l = npd(np.sqrt(Q))
    refs = SC.linearize_from_sums(ref7[0], ref7[1], m[..., 0], dts, chol_l, SC.LD)
    mags = SC.linearize_magnitudes(mag7[0], mag7[1], m[..., 0], dts, chol_l)
    yards = SC.linearize_from_sums(yard7[0], yard7[1], m[..., 0], dts, chol_l, npd)
    worst = 0.0
    for fused_t, plain_t, ref, mag, yard in zip(got, plain, refs, mags, yards):
        bound = SC.allowed(SC.scaled_error(yard, ref, mag, npd), npd)
        for t in (fused_t, plain_t):
            err = float(np.max(SC.scaled_error(t.cpu().numpy(), ref, np.broadcast_to(mag, (bsz, n)), npd)))
            worst = max(worst, err / bound)
            assert err <= bound
    print(f"largest error / bound: {worst:.3f}")
    np.testing.assert_array_equal(ssm.initial_mean.cpu().numpy(), m[:, 0])
    # the chain runs through the operators every model here is built on
    states = torch.zeros((bsz, n + 1, 1), dtype=dtype, device=DEV)
    means, covs = ssm.marginals
    assert tuple(means.shape) == (bsz, n + 1, 1) and tuple(covs.shape) == (bsz, n + 1, 1, 1)
    assert bool(torch.isfinite(ssm.log_pdf(states)).all()) and bool(torch.isfinite(means).all()) and bool((covs > 0).all())
    other = S.linearize_sde(make_sde(1 - drift_id, nq=nq), *args)
    kl = ssm.kl_divergence(other)
    assert tuple(kl.shape) == (bsz,) and bool((kl > 0).all()) and bool(torch.isfinite(kl).all())


def test_linearize_sde_routing_of_custom_drifts_and_trainable_parameters():
    """A Python drift and a trainable ``decay`` take ``linearize_torch`` on HIP tensors and agree with the kernel; so does a path that
    requires a gradient, which the torch route differentiates."""
    rng = np.random.default_rng(55)
    bsz, n = 2, 37
    m, s = path(rng, (bsz, n), np.float64)
    times = tt(np.concatenate([[0.5], 0.5 + np.cumsum(rng.uniform(0.002, 0.02, n))]), torch.float64)
    args = (times, (tt(m, torch.float64), tt(s, torch.float64)), (tt(m[:, 0], torch.float64), tt(s[:, 0], torch.float64)))

    def parts(ssm):
        return [t.detach().cpu().numpy() for t in (ssm.state_transitions, ssm.state_offsets, ssm.cholesky_process_covariances)]

    for drift_id in (0, 1):
        builtin = make_sde(drift_id)
        assert builtin._fusable()
        custom = PythonDrift(drift_id, Q)
        assert not custom._fusable()
        for got, want in zip(parts(S.linearize_sde(custom, *args)), parts(S.linearize_sde(builtin, *args))):
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-14)
    decay = torch.tensor(LAM, dtype=torch.float64, device=DEV, requires_grad=True)
    trained = S.linearize_sde(S.OrnsteinUhlenbeckSDE(decay, [[Q]]), *args)
    for got, want in zip(parts(trained), parts(S.linearize_sde(make_sde(0), *args))):
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-14)
    trained.state_transitions.sum().backward()
    want_grad = -float((times[1:] - times[:-1]).sum().cpu()) * bsz                      # A = 1 - decay dt
    assert abs(float(decay.grad.cpu()) - want_grad) <= 1e-12 * abs(want_grad)
    leaf = args[1][0].clone().requires_grad_(True)
    under_tape = S.linearize_sde(make_sde(1), times, (leaf, args[1][1]), args[2])
    for got, want in zip(parts(under_tape), parts(S.linearize_sde(make_sde(1), *args))):
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-14)
    under_tape.state_offsets.sum().backward()
    assert leaf.grad is not None and bool(torch.isfinite(leaf.grad).all())


# ---- drift difference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_kl_sde_through_the_chain_operators(dtype):
    """``test_KL_sde`` of the reference on the device: an OU prior (linearised: exact for a linear drift), a linear q, 1000 transitions
    of 1e-3, P0 = 0.1; ``q.kl_divergence(p)`` of the two chains against the drift difference along q's marginals, to the reference's
    ``decimal=2`` (|difference| < 1.5e-2)."""
    n, dt, decay, a_q = 1000, 1e-3, 1.3, -0.6
    times = torch.arange(n + 1, dtype=torch.float64, device=DEV).mul(dt).to(dtype)
    x0, chol0 = torch.full((1, 1), 0.4, dtype=dtype, device=DEV), torch.full((1, 1, 1), float(np.sqrt(0.1)), dtype=dtype, device=DEV)
    drift = S.LinearDrift(torch.full((1, n, 1, 1), a_q, dtype=dtype, device=DEV), torch.zeros((1, n, 1), dtype=dtype, device=DEV))
    q_ssm = drift.to_ssm(torch.ones((1, n, 1, 1), dtype=dtype, device=DEV), times, x0, chol0)
    means, covs = q_ssm.marginals
    ou = S.OrnsteinUhlenbeckSDE(decay)
    p_ssm = S.linearize_sde(ou, times, (means[:, :-1], covs[:, :-1]), (x0, chol0 * chol0))
    kl = float(q_ssm.kl_divergence(p_ssm)[0].cpu())
    val = S.squared_drift_difference_along_Gaussian_path(ou, drift, (means[:, :-1], covs[:, :-1]), dt)
    assert tuple(val.shape) == (1,)
    print(f"KL of the chains {kl:.6f}, drift difference {float(val[0].cpu()):.6f}")
    assert abs(kl - float(val[0].cpu())) < 1.5e-2


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("drift_id", [0, 1], ids=["ou", "double_well"])
def test_drift_difference_and_backward_against_the_torch_route_and_closed_forms(drift_id, dtype):
    npd = NP[dtype]
    rng = np.random.default_rng(60 + drift_id)
    batch, n, nq, dt = (2, 2), 300, 20, 0.01
    m, s = path(rng, batch + (n,), npd)
    a, b = rng.standard_normal(batch + (n, 1, 1)).astype(npd), rng.standard_normal(batch + (n, 1)).astype(npd)
    weights = rng.standard_normal(batch).astype(npd)
    sde = make_sde(drift_id)
    fused = [tt(t, dtype).requires_grad_(True) for t in (m, s, a, b)]
    plain = [tt(t, dtype).requires_grad_(True) for t in (m, s, a, b)]
    v_f = S.squared_drift_difference_along_Gaussian_path(sde, S.LinearDrift(fused[2], fused[3]), (fused[0], fused[1]), dt, nq)
    v_p = S.squared_drift_difference_torch(sde, plain[0][..., 0], plain[1][..., 0, 0], plain[2][..., 0, 0], plain[3][..., 0], dt, nq)
    assert tuple(v_f.shape) == batch
    (v_f * tt(weights, dtype)).sum().backward()
    (v_p * tt(weights, dtype)).sum().backward()
    flat = [t.reshape(batch + (n,)) for t in (m, s, a, b)]
    ref = SC.reference_sums(drift_id, npd(LAM), nq, *flat)
    mag = SC.gh_magnitudes(drift_id, npd(LAM), nq, *flat)
    yard = SC.gh_sums(drift_id, npd(LAM), nq, *flat, npd)
    scale = SC.LD(dt) / SC.LD(Q)
    worst = 0.0
    # the value: per series, the yardstick sums its points in the working dtype
    ref_v, mag_v = (ref[2] * scale).sum(axis=-1), (mag[2] * scale).sum(axis=-1)
    yard_v = np.sum((yard[2] * npd(scale)).astype(npd), axis=-1, dtype=npd)
    bound = SC.allowed(SC.scaled_error(yard_v, ref_v, mag_v, npd), npd)
    for v in (v_f, v_p):
        err = float(np.max(SC.scaled_error(v.detach().cpu().numpy(), ref_v, mag_v, npd)))
        worst = max(worst, err / bound)
        assert err <= bound
    # the gradients: the four derivatives per point times the series' weight (the yardstick multiplies too).  The kernel's are held to
    # the bound against long double; autograd through the torch route, entitled to the same bound, must lie within two of them
    for idx, f_leaf, p_leaf in zip((3, 4, 5, 6), fused, plain):
        w = weights[..., None].astype(SC.LD)
        ref_g, mag_g = ref[idx] * scale * w, mag[idx] * scale * np.abs(w)
        yard_g = ((yard[idx] * npd(scale)).astype(npd) * weights[..., None]).astype(npd)
        bound = SC.allowed(SC.scaled_error(yard_g, ref_g, mag_g, npd), npd)
        got = f_leaf.grad.cpu().numpy().reshape(batch + (n,))
        err = float(np.max(SC.scaled_error(got, ref_g, mag_g, npd)))
        worst = max(worst, err / bound)
        assert err <= bound
        apart = float(np.max(SC.scaled_error(p_leaf.grad.cpu().numpy().reshape(batch + (n,)), got.astype(SC.LD), mag_g, npd)))
        assert apart <= 2 * bound
    print(f"largest error / bound: {worst:.3f}")


def test_drift_difference_routing_once_differentiable_and_nan():
    rng = np.random.default_rng(70)
    m, s = path(rng, (2, 40), np.float64)
    a, b = rng.standard_normal((2, 40, 1, 1)), rng.standard_normal((2, 40, 1))
    ts = [tt(t, torch.float64) for t in (m, s, a, b)]
    for drift_id in (0, 1):
        builtin = S.squared_drift_difference_along_Gaussian_path(make_sde(drift_id), S.LinearDrift(ts[2], ts[3]), (ts[0], ts[1]), 0.01)
        custom = S.squared_drift_difference_along_Gaussian_path(PythonDrift(drift_id, Q), S.LinearDrift(ts[2], ts[3]), (ts[0], ts[1]), 0.01)
        np.testing.assert_allclose(custom.cpu().numpy(), builtin.cpu().numpy(), rtol=1e-12)
    decay = torch.tensor(LAM, dtype=torch.float64, device=DEV, requires_grad=True)
    trained = S.squared_drift_difference_along_Gaussian_path(S.OrnsteinUhlenbeckSDE(decay, [[Q]]), S.LinearDrift(ts[2], ts[3]), (ts[0], ts[1]), 0.01)
    builtin = S.squared_drift_difference_along_Gaussian_path(make_sde(0), S.LinearDrift(ts[2], ts[3]), (ts[0], ts[1]), 0.01)
    np.testing.assert_allclose(trained.detach().cpu().numpy(), builtin.cpu().numpy(), rtol=1e-12)
    trained.sum().backward()
    assert decay.grad is not None and bool(torch.isfinite(decay.grad))
    leaf = ts[0].clone().requires_grad_(True)
    bad = ts[1].clone()
    bad[1, 7] = float("nan")
    val = S.squared_drift_difference_along_Gaussian_path(make_sde(1), S.LinearDrift(ts[2], ts[3]), (leaf, bad), 0.01)
    assert np.isnan(val.detach().cpu().numpy()).tolist() == [False, True]
    with pytest.raises(RuntimeError, match="differentiable once"):
        torch.autograd.grad(val[0], leaf, create_graph=True)
