"""
CPU tests of ``markovflow_amd.sde`` (the torch routes and the public surface), of the kernels' arithmetic built for the host
(tests/host_sim/nlsde_sim.cpp, a stand-alone program over markovflow_amd/csrc/mf_nlsde_math.hpp) and of the new symbols' presence in
the C header and the ctypes table.  References: tests/helpers/sde_closed_forms.py (long double closed forms) and, for the one number
taken from the reference's own test (``test_KL_sde``), ``oracle.numpy_oracle.ssm_kl_divergence``.

The double well is a polynomial, so a rule with ``nq >= 4`` integrates every expectation here exactly and the comparisons with the
closed forms carry rounding only.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from markovflow_amd import sde as S
from oracle import numpy_oracle as O
from helpers import sde_closed_forms as SC

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_SRC = os.path.join(HERE, "host_sim", "nlsde_sim.cpp")
NEW_SYMBOLS = ["mf_nlsde_euler_maruyama_f64", "mf_nlsde_euler_maruyama_f32", "mf_nlsde_linearize_f64", "mf_nlsde_linearize_f32",
               "mf_nlsde_drift_difference_f64", "mf_nlsde_drift_difference_f32", "mf_nlsde_drift_difference_workspace_bytes"]
F64 = torch.float64


def t64(x):
    return torch.tensor(np.asarray(x, dtype=np.float64))


def nonuniform_grid(rng, n, t0=0.3, lo=0.002, hi=0.02):
    return np.concatenate([[t0], t0 + np.cumsum(rng.uniform(lo, hi, n - 1))])


# ---- Euler-Maruyama, torch route -------------------------------------------------------------------------------------------------
def test_euler_maruyama_ou_without_noise_is_the_product():
    rng = np.random.default_rng(1)
    lam, grid = 0.9, nonuniform_grid(rng, 41)
    x0 = rng.standard_normal((3, 2))
    sde = S.OrnsteinUhlenbeckSDE(lam, np.eye(2))
    out = S.euler_maruyama(sde, t64(x0), t64(grid), noise=torch.zeros((3, 40, 2), dtype=F64))
    assert tuple(out.shape) == (3, 41, 2)
    assert np.array_equal(out[:, 0].numpy(), x0)                                      # bitwise
    want = x0[:, None, :] * np.concatenate([[1.0], np.cumprod(1.0 - lam * np.diff(grid))])[None, :, None]
    np.testing.assert_allclose(out.numpy(), want, rtol=1e-13, atol=0)


def test_euler_maruyama_against_the_long_double_recurrence():
    rng = np.random.default_rng(2)
    grid = nonuniform_grid(rng, 30)
    x0, noise = rng.uniform(-1.5, 1.5, (4, 3)), rng.standard_normal((4, 29, 3))
    q = np.array([[1.0, 0.2, 0.1], [0.2, 0.8, 0.3], [0.1, 0.3, 0.6]])
    for sde, drift_id, lam in ((S.DoubleWellSDE(q), 1, 0.0), (S.OrnsteinUhlenbeckSDE(0.7, q), 0, 0.7)):
        out = S.euler_maruyama(sde, t64(x0), t64(grid), noise=t64(noise))
        ref = SC.em_path(drift_id, lam, x0, grid, noise, np.linalg.cholesky(q))
        np.testing.assert_allclose(out.numpy(), ref.astype(np.float64), rtol=1e-12, atol=1e-13)


def test_euler_maruyama_generator():
    sde = S.DoubleWellSDE()
    x0, grid = torch.zeros((5, 1), dtype=F64), torch.linspace(0.0, 0.5, 26, dtype=F64)
    runs = [S.euler_maruyama(sde, x0, grid, generator=torch.Generator().manual_seed(seed)) for seed in (7, 7, 8)]
    assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0], runs[2])
    assert tuple(runs[0].shape) == (5, 26, 1)


def test_euler_maruyama_grid_deviation_on_the_reference_setting():
    """The reference's test setting: 1000 steps on [0, 1], its grid ``linspace(dt, 1, 1000)``.  Its output on that grid starts its clock
    at 0: entry k is the state at ``grid[k] - dt``, which is our output on ``[0, grid[:-1]]``; the deterministic value test of
    the reference (``a <- a - decay a dt``) pins the numbers."""
    n, decay = 1000, 0.8
    dt = 1.0 / n
    ref_grid = np.linspace(dt, 1.0, n)
    ours = np.concatenate([[0.0], ref_grid[:-1]])
    x0 = np.array([[0.7], [-1.1], [0.2]])
    sde = S.OrnsteinUhlenbeckSDE(decay, 1e-20 * np.eye(1))
    out = S.euler_maruyama(sde, t64(x0), t64(ours), generator=torch.Generator().manual_seed(0))
    assert tuple(out.shape) == (3, n, 1)                                               # num_transitions + 1 values, as the reference
    want = x0[:, None, :] * ((1.0 - decay * dt) ** np.arange(n))[None, :, None]
    np.testing.assert_allclose(out.numpy(), want, atol=1e-5)                           # the reference's own tolerance
    np.testing.assert_allclose(out.numpy(), want, atol=1e-8)                           # 1e-10 sqrt(dt) noise: far below


def test_euler_maruyama_torch_route_is_differentiable_and_arguments_are_checked():
    decay = torch.tensor(0.5, dtype=F64, requires_grad=True)
    sde = S.OrnsteinUhlenbeckSDE(decay)
    assert not sde._fusable()
    out = S.euler_maruyama(sde, torch.ones((2, 1), dtype=F64), torch.linspace(0, 1, 5, dtype=F64), noise=torch.zeros((2, 4, 1), dtype=F64))
    out[:, -1].sum().backward()
    assert abs(float(decay.grad) - 2 * 4 * (-0.25) * (1 - 0.125) ** 3) < 1e-12
    with pytest.raises(ValueError):
        S.euler_maruyama(S.DoubleWellSDE(), torch.ones((2, 1), dtype=F64), t64([0.0, 0.2, 0.1]))
    with pytest.raises(ValueError):
        S.euler_maruyama(S.DoubleWellSDE(), torch.ones((2, 2), dtype=F64), t64([0.0, 0.2]))
    with pytest.raises(ValueError):
        S.euler_maruyama(S.DoubleWellSDE(), torch.ones((2, 1), dtype=F64), t64([0.0, 0.2]), noise=torch.zeros((2, 2, 1), dtype=F64))


# ---- linearisation ---------------------------------------------------------------------------------------------------------------
def path(rng, bsz, n):
    return rng.uniform(-1.5, 1.5, (bsz, n, 1)), rng.uniform(0.05, 0.6, (bsz, n, 1, 1))


def test_linearize_ou_is_exact():
    rng = np.random.default_rng(3)
    lam, q = 1.7, 0.4
    times = nonuniform_grid(rng, 12)
    m, s = path(rng, 3, 11)
    ssm = S.linearize_sde(S.OrnsteinUhlenbeckSDE(lam, [[q]]), t64(times), (t64(m), t64(s)), (t64(m[:, 0]), t64(s[:, 0])))
    assert isinstance(ssm, mfa.StateSpaceModel)
    dts = np.diff(times)
    np.testing.assert_allclose(ssm.state_transitions.numpy(), np.broadcast_to((1 - lam * dts)[None, :, None, None], (3, 11, 1, 1)), rtol=1e-14)
    np.testing.assert_allclose(ssm.state_offsets.numpy(), 0.0, atol=1e-16)
    np.testing.assert_allclose(ssm.cholesky_process_covariances.numpy(), np.broadcast_to(np.sqrt(q * dts)[None, :, None, None], (3, 11, 1, 1)),
                               rtol=1e-14)
    np.testing.assert_allclose(ssm.initial_mean.numpy(), m[:, 0], rtol=0)
    np.testing.assert_allclose(ssm.cholesky_initial_covariance.numpy(), np.sqrt(s[:, 0]), rtol=1e-15)


@pytest.mark.parametrize("nq", [4, 10, 20])
def test_linearize_double_well_against_closed_forms(nq):
    rng = np.random.default_rng(4)
    times = nonuniform_grid(rng, 9)
    m, s = path(rng, 2, 8)
    ssm = S.linearize_sde(S.DoubleWellSDE([[0.5]], num_gauss_hermite_points=nq), t64(times), (t64(m), t64(s)), (t64(m[:, 0]), t64(s[:, 0])))
    ref = SC.reference_sums(1, 0.0, nq, m[..., 0], s[..., 0, 0], 0 * m[..., 0], 0 * m[..., 0])
    assert np.max(np.abs(ref[0] - (4 * m[..., 0] - 4 * (m[..., 0] ** 3 + 3 * m[..., 0] * s[..., 0, 0])))) < 1e-14     # the issue's forms
    assert np.max(np.abs(ref[1] - (4 - 12 * (m[..., 0] ** 2 + s[..., 0, 0])))) < 1e-14
    a_ref, b_ref, c_ref = SC.linearize_from_sums(ref[0], ref[1], m[..., 0], np.diff(times), np.sqrt(0.5), SC.LD)
    np.testing.assert_allclose(ssm.state_transitions.numpy()[..., 0, 0], a_ref.astype(np.float64), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(ssm.state_offsets.numpy()[..., 0], b_ref.astype(np.float64), rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(ssm.cholesky_process_covariances.numpy()[..., 0, 0], np.broadcast_to(c_ref.astype(np.float64), (2, 8)), rtol=1e-14)


def test_linearize_refuses_other_dimensions_and_marks_bad_variances():
    with pytest.raises(NotImplementedError, match="state_dim == 1"):
        S.linearize_sde(S.DoubleWellSDE(np.eye(2)), t64([0.0, 0.1]), (torch.zeros((1, 1, 2), dtype=F64), torch.ones((1, 1, 2, 2), dtype=F64)),
                        (torch.zeros((1, 2), dtype=F64), torch.ones((1, 2, 2), dtype=F64)))
    m, s = np.zeros((1, 3, 1)), np.array([0.2, 0.0, np.nan]).reshape(1, 3, 1, 1)
    ssm = S.linearize_sde(S.DoubleWellSDE(), t64([0.0, 0.1, 0.2, 0.3]), (t64(m), t64(s)), (t64(m[:, 0]), t64([[[0.2]]])))
    bad = np.isnan(ssm.state_transitions.numpy()[0, :, 0, 0])
    assert bad.tolist() == [False, True, True] and np.isnan(ssm.state_offsets.numpy()[0, :, 0]).tolist() == [False, True, True]
    assert np.all(np.isfinite(ssm.cholesky_process_covariances.numpy()))


def test_expected_drift_shapes_and_a_custom_drift():
    class Cubic(S.SDE):                                   # an arbitrary Python drift: f' by autograd
        def drift(self, x, t):
            return 4.0 * x * (1.0 - x * x)

        def diffusion(self, x, t):
            return torch.ones_like(x[..., None])

    rng = np.random.default_rng(5)
    m, s = path(rng, 2, 6)
    custom, builtin = Cubic(1), S.DoubleWellSDE()
    assert not custom._fusable() and builtin._fusable()
    for name in ("expected_drift", "expected_gradient_drift"):
        a, b = getattr(custom, name)(t64(m), t64(s)), getattr(builtin, name)(t64(m), t64(s))
        assert tuple(a.shape) == (2, 6, 1)
        np.testing.assert_allclose(a.detach().numpy(), b.numpy(), rtol=1e-13, atol=1e-14)
    m2, s2 = rng.standard_normal((2, 3, 2)), np.broadcast_to(np.array([[0.3, 0.1], [0.1, 0.2]]), (2, 3, 2, 2)).copy()
    e2 = S.DoubleWellSDE(np.eye(2)).expected_drift(t64(m2), t64(s2)).numpy()            # element-wise drift: the marginals decide
    for i in range(2):
        np.testing.assert_allclose(e2[..., i], 4 * m2[..., i] - 4 * (m2[..., i] ** 3 + 3 * m2[..., i] * s2[..., i, i]), rtol=1e-12, atol=1e-13)


# ---- LinearDrift -----------------------------------------------------------------------------------------------------------------
def test_linear_drift_round_trip_and_the_reference_identities():
    rng = np.random.default_rng(6)
    n, dt, decay = 50, 1e-3, 0.9
    times = t64(np.arange(n + 1) * dt)
    a_d, b_d = t64(rng.standard_normal((2, n, 1, 1))), t64(rng.standard_normal((2, n, 1)))
    diffusion = torch.full((2, n, 1, 1), 0.7, dtype=F64)
    drift = S.LinearDrift(a_d, b_d)
    ssm = drift.to_ssm(diffusion, times, torch.zeros((2, 1), dtype=F64), torch.ones((2, 1, 1), dtype=F64))
    np.testing.assert_allclose(ssm.state_transitions.numpy(), 1 + a_d.numpy() * dt, rtol=1e-13)
    np.testing.assert_allclose(ssm.cholesky_process_covariances.numpy(),
                               np.broadcast_to(0.7 * np.sqrt(np.diff(times.numpy()))[None, :, None, None], (2, n, 1, 1)), rtol=1e-15)
    back = S.LinearDrift()
    back.set_from_ssm(ssm, dt)
    np.testing.assert_allclose(back.A.numpy(), a_d.numpy(), rtol=1e-9, atol=1e-12)      # (1 + A dt - 1) / dt: eps / dt
    np.testing.assert_allclose(back.b.numpy(), b_d.numpy(), rtol=1e-12)
    # test_ssm_to_linear_drift of the reference: the chain of an OU process gives A = -decay, b = 0
    a_p = torch.full((1, n, 1, 1), 1.0 - decay * dt, dtype=F64)
    p_ssm = mfa.StateSpaceModel(torch.zeros((1, 1), dtype=F64), torch.full((1, 1, 1), np.sqrt(0.1), dtype=F64), a_p,
                                torch.zeros((1, n, 1), dtype=F64), torch.full((1, n, 1, 1), np.sqrt(dt), dtype=F64))
    got = S.LinearDrift()
    got.set_from_ssm(p_ssm, dt)
    np.testing.assert_allclose(got.A.numpy(), -decay * np.ones((1, n, 1, 1)))
    np.testing.assert_allclose(got.b.numpy(), np.zeros((1, n, 1)))
    with pytest.raises(ValueError):
        S.LinearDrift().to_ssm(diffusion, times, torch.zeros((2, 1), dtype=F64), torch.ones((2, 1, 1), dtype=F64))


# ---- drift difference ------------------------------------------------------------------------------------------------------------
def test_kl_sde_at_the_reference_shape():
    """``test_KL_sde`` of the reference: an OU prior, a linear q, 1000 transitions of 1e-3, P0 = 0.1; the drift difference along q's
    marginals against the KL of the two chains, to the reference's ``decimal=2`` (|difference| < 1.5e-2)."""
    n, dt, decay, a_q = 1000, 1e-3, 1.3, -0.6
    x0 = np.array([0.4])
    cq = np.full((n, 1, 1), np.sqrt(dt))
    p = (x0, np.array([[np.sqrt(0.1)]]), np.full((n, 1, 1), 1 - decay * dt), np.zeros((n, 1)), cq)
    q = (x0, np.array([[np.sqrt(0.1)]]), np.full((n, 1, 1), 1 + a_q * dt), np.zeros((n, 1)), cq)
    kl = float(O.ssm_kl_divergence(q, p))
    means = O.ssm_marginal_means(q[0], q[2], q[3])
    covs = O.ssm_marginal_covariances(q[1], q[2], q[4])
    drift = S.LinearDrift(torch.full((n, 1, 1), a_q, dtype=F64), torch.zeros((n, 1), dtype=F64))
    val = S.squared_drift_difference_along_Gaussian_path(S.OrnsteinUhlenbeckSDE(decay), drift, (t64(means[:-1]), t64(covs[:-1])), dt)
    assert val.shape == ()
    print(f"KL of the chains {kl:.6f}, drift difference {float(val):.6f}")
    assert abs(kl - float(val)) < 1.5e-2


def dd_inputs(rng, batch, n):
    m, s = rng.uniform(-1.5, 1.5, batch + (n, 1)), rng.uniform(0.05, 0.6, batch + (n, 1, 1))
    return m, s, rng.standard_normal(batch + (n, 1, 1)), rng.standard_normal(batch + (n, 1))


@pytest.mark.parametrize("nq", [4, 10, 20])
@pytest.mark.parametrize("drift_id", [0, 1], ids=["ou", "double_well"])
def test_drift_difference_and_its_backward_against_closed_forms(drift_id, nq):
    rng = np.random.default_rng(10 + nq)
    lam, q, dt = 0.8, 0.5, 0.01
    sde = S.OrnsteinUhlenbeckSDE(lam, [[q]]) if drift_id == 0 else S.DoubleWellSDE([[q]])
    m, s, a, b = dd_inputs(rng, (2, 3), 7)
    leaves = [t64(t).requires_grad_(True) for t in (m, s, a, b)]
    val = S.squared_drift_difference_along_Gaussian_path(sde, S.LinearDrift(leaves[2], leaves[3]), (leaves[0], leaves[1]), dt, nq)
    assert tuple(val.shape) == (2, 3)
    weights = rng.standard_normal((2, 3))
    (val * t64(weights)).sum().backward()
    ref = SC.reference_sums(drift_id, lam, nq, m[..., 0], s[..., 0, 0], a[..., 0, 0], b[..., 0])
    scale = SC.LD(dt) / SC.LD(q)
    np.testing.assert_allclose(val.detach().numpy(), (ref[2].sum(axis=-1) * scale).astype(np.float64), rtol=1e-12)
    for leaf, part in zip(leaves, (ref[3], ref[4], ref[5], ref[6])):
        want = (part * scale * weights[..., None]).astype(np.float64)
        np.testing.assert_allclose(leaf.grad.numpy().reshape(want.shape), want, rtol=1e-10, atol=1e-12)


def test_drift_difference_backward_against_autograd_on_the_torch_route():
    rng = np.random.default_rng(20)
    m, s, a, b = dd_inputs(rng, (3,), 9)
    for sde in (S.OrnsteinUhlenbeckSDE(0.8, [[0.5]]), S.DoubleWellSDE([[0.5]])):
        fused = [t64(t).requires_grad_(True) for t in (m, s, a, b)]
        plain = [t64(t).requires_grad_(True) for t in (m, s, a, b)]
        v1 = S.squared_drift_difference_along_Gaussian_path(sde, S.LinearDrift(fused[2], fused[3]), (fused[0], fused[1]), 0.02)
        v2 = S.squared_drift_difference_torch(sde, plain[0][..., 0], plain[1][..., 0, 0], plain[2][..., 0, 0], plain[3][..., 0], 0.02, 20)
        np.testing.assert_allclose(v1.detach().numpy(), v2.detach().numpy(), rtol=1e-13)
        v1.sum().backward()
        v2.sum().backward()
        for f, p in zip(fused, plain):
            np.testing.assert_allclose(f.grad.numpy(), p.grad.numpy(), rtol=1e-11, atol=1e-13)


def test_drift_difference_trainable_and_custom_take_autograd_and_agree():
    class MyOU(S.SDE):
        def __init__(self):
            super().__init__(1)
            self.q = torch.tensor([[0.5]], dtype=F64)

        def drift(self, x, t):
            return -0.8 * x

        def diffusion(self, x, t):
            return torch.ones_like(x[..., None]) * np.sqrt(0.5)

    rng = np.random.default_rng(21)
    m, s, a, b = (t64(t) for t in dd_inputs(rng, (2,), 6))
    builtin = S.squared_drift_difference_along_Gaussian_path(S.OrnsteinUhlenbeckSDE(0.8, [[0.5]]), S.LinearDrift(a, b), (m, s), 0.01)
    custom = S.squared_drift_difference_along_Gaussian_path(MyOU(), S.LinearDrift(a, b), (m, s), 0.01)
    decay = torch.tensor(0.8, dtype=F64, requires_grad=True)
    trained = S.squared_drift_difference_along_Gaussian_path(S.OrnsteinUhlenbeckSDE(decay, [[0.5]]), S.LinearDrift(a, b), (m, s), 0.01)
    np.testing.assert_allclose(custom.numpy(), builtin.numpy(), rtol=1e-13)
    np.testing.assert_allclose(trained.detach().numpy(), builtin.numpy(), rtol=1e-13)
    trained.sum().backward()
    assert decay.grad is not None and np.isfinite(float(decay.grad))


def test_drift_difference_once_differentiable_and_nan_series():
    rng = np.random.default_rng(22)
    m, s, a, b = dd_inputs(rng, (2,), 5)
    s[1, 2] = 0.0
    leaves = [t64(t).requires_grad_(True) for t in (m, s, a, b)]
    val = S.squared_drift_difference_along_Gaussian_path(S.DoubleWellSDE(), S.LinearDrift(leaves[2], leaves[3]), (leaves[0], leaves[1]), 0.01)
    assert np.isnan(val.detach().numpy()).tolist() == [False, True]
    with pytest.raises(RuntimeError, match="differentiable once"):
        torch.autograd.grad(val[0], leaves[0], create_graph=True)
    with pytest.raises(NotImplementedError, match="state_dim == 1"):
        S.squared_drift_difference_along_Gaussian_path(S.DoubleWellSDE(np.eye(2)), S.LinearDrift(leaves[2], leaves[3]), (leaves[0], leaves[1]), 0.01)


# ---- the kernels' arithmetic on the host --------------------------------------------------------------------------------------------
def build_sim(tmp_path_factory, flags, name):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no system C++ compiler")
    exe = str(tmp_path_factory.mktemp("nlsde_sim") / name)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags + ["-o", exe, SIM_SRC])
    return exe


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return build_sim(tmp_path_factory, [], "nlsde_sim")


def hexes(values):
    return " ".join(float(v).hex() for v in np.ravel(values))


def sim_commands(npd):
    """Commands for the host program with what the torch route gives for each, in the working dtype, and long double references."""
    rng = np.random.default_rng(30)
    tt = lambda x: torch.tensor(np.asarray(x, dtype=npd))                              # noqa: E731
    lines, expect = [], []
    lam = float(npd(0.7))
    for d in (1, 2, 3, 4):
        base = rng.standard_normal((d, d))
        qmat = base @ base.T / d + 0.2 * np.eye(d)
        for drift_id in (0, 1):
            sde = S.OrnsteinUhlenbeckSDE(lam, qmat) if drift_id == 0 else S.DoubleWellSDE(qmat)
            chol = np.linalg.cholesky(qmat).astype(npd)                                # what the kernel holds
            x, xi, dt = rng.uniform(-1.5, 1.5, d).astype(npd), rng.standard_normal(d).astype(npd), npd(rng.uniform(0.002, 0.02))
            packed = [chol[i, j] for i in range(d) for j in range(i + 1)]
            step_dt = npd(npd(0.25) + dt) - npd(0.25)                                    # the step the grid holds
            lines.append(f"em {d} {drift_id} {hexes([lam, step_dt])} {hexes(packed)} {hexes(x)} {hexes(xi)}")
            got = S.euler_maruyama(sde, tt(x[None]), tt([0.25, npd(0.25) + dt]), noise=tt(xi[None, None]))[0, 1].numpy()
            ref, mag = SC.em_step(drift_id, lam, x, xi, step_dt, chol)
            yard, _ = SC.em_step(drift_id, lam, x, xi, step_dt, chol, npd)
            expect.append((got, [ref], [mag], [yard]))
    for nq in (4, 10, 20):
        nodes, weights = np.polynomial.hermite.hermgauss(nq)
        lines.append(f"rule {nq} {hexes(nodes)} {hexes(weights)}")
        expect.append(None)
        for drift_id in (0, 1):
            q = 0.5
            sde = (S.OrnsteinUhlenbeckSDE(lam, [[q]], num_gauss_hermite_points=nq) if drift_id == 0
                   else S.DoubleWellSDE([[q]], num_gauss_hermite_points=nq))
            for _ in range(3):
                m, s, a, b = npd(rng.uniform(-1.5, 1.5)), npd(rng.uniform(0.05, 0.6)), npd(rng.standard_normal()), npd(rng.standard_normal())
                t0, dt = npd(0.5), npd(rng.uniform(0.002, 0.02))
                step_dt = npd(t0 + dt) - t0
                ref7 = SC.reference_sums(drift_id, lam, nq, m, s, a, b)
                mag7 = SC.gh_magnitudes(drift_id, lam, nq, m, s, a, b)
                yard7 = SC.gh_sums(drift_id, lam, nq, m, s, a, b, npd)
                chol_l = float(np.sqrt(q))
                lines.append(f"lin {drift_id} {hexes([lam, chol_l, m, s, step_dt])}")
                ssm = S.linearize_sde(sde, tt([t0, t0 + dt]), (tt([[[m]]]), tt([[[[s]]]])), (tt([[m]]), tt([[[s]]])))
                got = np.array([ssm.state_transitions.numpy().ravel()[0], ssm.state_offsets.numpy().ravel()[0],
                                ssm.cholesky_process_covariances.numpy().ravel()[0]])
                expect.append((got, SC.linearize_from_sums(ref7[0], ref7[1], m, step_dt, npd(chol_l), SC.LD),
                               SC.linearize_magnitudes(mag7[0], mag7[1], m, step_dt, npd(chol_l)),
                               SC.linearize_from_sums(yard7[0], yard7[1], m, step_dt, npd(chol_l), npd)))
                scale = float(npd(0.01 / q))
                lines.append(f"dd {drift_id} {hexes([lam, m, s, a, b, scale])}")
                parts = S._drift_difference_parts(sde, tt([[m]]), tt([[s]]), tt([[a]]), tt([[b]]), scale, nq)
                got = np.array([float(p.ravel()[0]) for p in parts], dtype=npd)
                expect.append((got, [r * SC.LD(scale) for r in ref7[2:]], [g * SC.LD(scale) for g in mag7[2:]],
                               [y * npd(scale) for y in yard7[2:]]))
    return lines, expect


@pytest.mark.parametrize("npd", [np.float64, np.float32], ids=["f64", "f32"])
def test_host_program_against_the_torch_route(sim, npd):
    """The program's outputs and the torch route's are both held to the yardstick bound against long double, and to each other within
    the sum of the two bounds."""
    if npd == np.float64 and not SC.longdouble_ok():
        pytest.skip("numpy.longdouble is no wider than a double here: no reference for the float64 accuracy")
    lines, expect = sim_commands(npd)
    res = subprocess.run([sim, "f64" if npd == np.float64 else "f32"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    outs = iter(res.stdout.strip().split("\n"))
    worst = 0.0
    for line, exp in zip(lines, expect):
        if exp is None:
            continue
        sim_vals = np.array([float.fromhex(tok) for tok in next(outs).split()])
        torch_vals, refs, mags, yards = exp
        refs, mags, yards = (np.ravel(np.array([np.ravel(np.asarray(v, dtype=SC.LD)) for v in part])) for part in (refs, mags, yards))
        bound = SC.allowed(SC.scaled_error(yards, refs, mags, npd), npd)
        for vals in (sim_vals, np.ravel(torch_vals)):
            err = float(np.max(SC.scaled_error(vals, refs, mags, npd)))
            worst = max(worst, err / bound)
            assert err <= bound, (line, err, bound)
    print(f"largest error / bound: {worst:.3f}")


def test_host_program_under_the_sanitizers(tmp_path_factory):
    """The same program built with -fsanitize=address,undefined and run on its own, with the environment it inherits (no Python code
    runs under a sanitizer): it must exit clean.  Where the environment preloads a library into every process, the sanitizer's runtime
    would not come first in the program's library list and refuses to start: the run is skipped there, on the check below."""
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("a library is preloaded into every process here: the sanitizer run belongs on a machine without one")
    exe = build_sim(tmp_path_factory, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"], "nlsde_sim_san")
    for npd in (np.float64, np.float32):
        lines, _ = sim_commands(npd)
        res = subprocess.run([exe, "f64" if npd == np.float64 else "f32"], input="\n".join(lines) + "\n", capture_output=True, text=True,
                             timeout=60)
        assert res.returncode == 0, res.stderr
        assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
        assert len(res.stdout.strip().split("\n")) == sum(1 for line in lines if not line.startswith("rule"))
    assert subprocess.run([exe, "f64"], input="em 9 0 0x1p0\n", capture_output=True, text=True, timeout=60).returncode == 2


# ---- symbols ---------------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_table_and_library():
    header = os.path.join(HERE, "..", "include", "markovflow_amd.h")
    text = open(header).read()
    names = set(_lib.exported_symbols())
    lib = _lib.load()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b" + sym + r"\(", text), sym
        assert sym in names, sym
        assert getattr(lib, sym) is not None
    assert lib.mf_nlsde_drift_difference_workspace_bytes(3, 300) == 3 * 2 * 8 and lib.mf_nlsde_drift_difference_workspace_bytes(0, 5) == 0
    for name in ("sde", "SDE", "OrnsteinUhlenbeckSDE", "DoubleWellSDE", "LinearDrift", "euler_maruyama", "linearize_sde",
                 "squared_drift_difference_along_Gaussian_path"):
        assert name in mfa.__all__ and hasattr(mfa, name)


def test_argument_errors_without_touching_the_gpu():
    lib = _lib.load()
    null = None
    assert lib.mf_nlsde_euler_maruyama_f64(-1, 5, 1, 1, null, null, null, null, null, null, null) == -1
    assert lib.mf_nlsde_euler_maruyama_f64(1, 0, 1, 1, null, null, null, null, null, null, null) == -2
    assert lib.mf_nlsde_euler_maruyama_f32(1, 5, 5, 1, null, null, null, null, null, null, null) == -100
    assert lib.mf_nlsde_euler_maruyama_f32(1, 5, 1, 2, null, null, null, null, null, null, null) == -4
    assert lib.mf_nlsde_euler_maruyama_f32(1, 5, 1, 0, null, null, null, null, null, null, null) == -5
    assert lib.mf_nlsde_euler_maruyama_f32(1, 5, 1, 1, null, null, null, null, null, null, null) == -6
    assert lib.mf_nlsde_linearize_f64(1, 1, 1, null, 1.0, 33, null, null, null, null, null, null, null, null, null) == -6
    assert lib.mf_nlsde_linearize_f64(1, 1, 1, null, 1.0, 3, null, null, null, null, null, null, null, null, null) == -7
    assert lib.mf_nlsde_drift_difference_f32(1, 1, 7, null, 3, null, null, 1.0, *([null] * 10), 0, null) == -3
    assert lib.mf_nlsde_drift_difference_f32(1, 1, 1, null, 0, null, null, 1.0, *([null] * 10), 0, null) == -5
