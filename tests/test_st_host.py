"""
CPU tests of the spatio-temporal sparse variational model's host side (markovflow_amd/spatial_kernels.py,
``kernels.SparseSpatioTemporalKernel``, ``models.st_expected_log_likelihood_torch`` / ``st_point_marginals`` /
``SpatioTemporalSparseVariational``), of the entry points' declarations and of the reference the GPU tests lean on
(tests/helpers/st_closed_forms.py): the helper's projection against an independent statement of the reference's route, its five
adjoints against central differences, the torch composition and its autograd gradients against the helper, a batch against its series,
the spatial kernels against their closed forms, the Kronecker chain against the dense product kernel, the error paths, the symbols,
the workspace formula and every argument error code.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from markovflow_amd import models as MM
from markovflow_amd import spatial_kernels as SK
from conftest import ROOT
from helpers import likelihood_closed_forms as L
from helpers import st_closed_forms as ST

NAMES = [L.GAUSSIAN, L.BERNOULLI, L.POISSON, L.STUDENTT]
SIZES = [(1, 1), (3, 2), (5, 3), (21, 3)]


def tt(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=torch.float64).requires_grad_(grad)


def _likelihood(name):
    params = L.LIKELIHOODS[name][1]
    return {L.GAUSSIAN: lambda: mfa.Gaussian(params[0]), L.BERNOULLI: mfa.Bernoulli, L.POISSON: mfa.Poisson,
            L.STUDENTT: lambda: mfa.StudentT(*params)}[name]()


def _case(seed, ms, dt, name, lengths=(0, 3, 7, 1), skew=0.0):
    rng = np.random.default_rng(seed)
    n, segs, pair = int(np.sum(lengths)), len(lengths), 2 * ms * dt
    root = rng.normal(size=(segs, pair, pair))
    anti = rng.normal(size=(segs, pair, pair))
    return dict(a=rng.uniform(-1, 1, size=(n, ms)) / np.sqrt(ms), wt=rng.uniform(-0.7, 0.7, size=(n, 2 * dt)) / np.sqrt(dt),
                c=rng.uniform(0.05, 0.5, size=n), y=np.resize(np.asarray(L.OBSERVED[name]), n),
                offsets=np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), pair_mean=rng.normal(size=(segs, pair)),
                pair_cov=root @ root.transpose(0, 2, 1) / pair + 0.1 * np.eye(pair) + skew * (anti - anti.transpose(0, 2, 1)))


def _helper(name, case, dtype=np.float64):
    return ST.st_expectations(L.LIKELIHOODS[name], case["a"], case["wt"], case["c"], case["y"], case["offsets"], case["pair_mean"],
                              case["pair_cov"], 20, dtype)


# ---- the helper ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ms,dt", SIZES)
def test_the_kronecker_projection_is_the_references_conditional(ms, dt):
    """fmu = W . m and fvar = c + W^T S W with c = K_s(x, x) - |a|^2 (1 - ct) against the state marginal at t_k, cov_u, its
    Cholesky factor and the base conditional."""
    rng = np.random.default_rng(100 * ms + dt)
    pair, n = 2 * ms * dt, 6
    z, x = rng.uniform(-1, 1, size=(ms, 2)), rng.uniform(-1, 1, size=(n, 2))
    sq = lambda p, q: np.exp(-0.5 * np.sum((p[:, None, :] - q[None, :, :]) ** 2, axis=-1) / 0.8 ** 2)          # noqa: E731
    kmm, kmn = 1.3 * sq(z, z) + 1e-9 * np.eye(ms), 1.3 * sq(z, x)
    chol = np.linalg.cholesky(kmm)
    a = np.linalg.solve(chol, kmn).T                          # [N, Ms]
    h = rng.normal(size=dt)
    proj = rng.normal(size=(n, dt, 2 * dt)) * 0.5
    root = rng.normal(size=(n, dt, dt))
    cov = root @ root.transpose(0, 2, 1) / dt + 0.05 * np.eye(dt)
    wt, ct = np.einsum("i,kij->kj", h, proj), np.einsum("i,kij,j->k", h, cov, h)
    c = 1.3 - np.sum(a * a, axis=1) * (1.0 - ct)
    big = rng.normal(size=(pair, pair))
    pair_mean, pair_cov = rng.normal(size=pair), big @ big.T / pair + 0.1 * np.eye(pair)
    got = ST.st_expectations(L.LIKELIHOODS[L.GAUSSIAN], a, wt, c, np.zeros(n), np.array([0, n]), pair_mean[None], pair_cov[None])
    for k in range(n):
        mean, var = ST.reference_route(kmm, kmn[:, k], 1.3, h, proj[k], cov[k], pair_mean, pair_cov)
        np.testing.assert_allclose(got["fmu"][k], mean, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(got["fvar"][k], var, rtol=1e-12)


@pytest.mark.parametrize("name", NAMES)
def test_the_helpers_five_adjoints_against_central_differences(name):
    case = _case(3, 3, 2, name, skew=0.02)
    base = _helper(name, case)
    total = lambda cs: float(np.sum(_helper(name, cs)["ve_sum"]))          # noqa: E731
    rng = np.random.default_rng(0)
    seg = np.repeat(np.arange(len(case["offsets"]) - 1), np.diff(case["offsets"]))
    adjoint = dict(a=base["g_a"], wt=base["g_wt"], c=base["g_c"], pair_mean=base["g_mean"], pair_cov=base["g_cov"])
    assert seg.shape[0] == case["a"].shape[0]
    for key, grad in adjoint.items():
        for _ in range(6):
            index = tuple(int(rng.integers(0, s)) for s in case[key].shape)
            if key in ("pair_mean", "pair_cov") and case["offsets"][index[0] + 1] == case["offsets"][index[0]]:
                assert np.all(grad[index[0]] == 0), "an empty segment has zero adjoints"
                continue
            step = 1e-6
            plus, minus = ({**case, key: case[key].copy()} for _ in range(2))
            plus[key][index] += step
            minus[key][index] -= step
            numeric = (total(plus) - total(minus)) / (2 * step)
            np.testing.assert_allclose(grad[index], numeric, rtol=2e-6, atol=2e-8, err_msg=f"{key}{index}")


# ---- the torch composition -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ms,dt", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_the_torch_composition_and_its_gradients_against_the_helper(name, ms, dt):
    case = _case(11, ms, dt, name, lengths=(2, 0, 9, 1), skew=0.01)
    want = _helper(name, case)
    a, wt, c, pm, pc = (tt(case[k], True) for k in ("a", "wt", "c", "pair_mean", "pair_cov"))
    indices = MM._segments_of(torch.tensor(case["offsets"]), a.shape[0])
    ve = MM.st_expected_log_likelihood_torch(_likelihood(name), a, wt, c, tt(case["y"]), indices, pm, pc)
    grads = torch.autograd.grad(ve.sum(), (pm, pc, a, wt, c))
    fmu, fvar = MM.st_point_marginals(a.detach(), wt.detach(), c.detach(), torch.tensor(case["offsets"]), pm.detach(), pc.detach())
    got = dict(zip(("ve_sum", "g_mean", "g_cov", "g_a", "g_wt", "g_c", "fmu", "fvar"), (ve.detach(),) + grads + (fmu, fvar)))
    for key, value in got.items():
        np.testing.assert_allclose(value.numpy(), want[key], rtol=1e-12, atol=1e-12 * float(np.max(want["mag_" + key]) + 1e-300),
                                   err_msg=key)


def test_a_batch_is_its_series_one_by_one():
    name, ms, dt = L.BERNOULLI, 3, 2
    cases = [_case(seed, ms, dt, name, lengths=lengths) for seed, lengths in ((1, (4, 0, 5, 3)), (2, (0, 6, 6, 0)))]
    stack = lambda k: tt(np.stack([cs[k] for cs in cases]))          # noqa: E731
    offsets = torch.tensor(np.stack([cs["offsets"] for cs in cases]))
    indices = MM._segments_of(offsets, 12)
    args = [stack(k) for k in ("a", "wt", "c", "y")]
    both = MM.st_expected_log_likelihood_torch(_likelihood(name), *args, indices, stack("pair_mean"), stack("pair_cov"))
    for b, cs in enumerate(cases):
        one = MM.st_expected_log_likelihood_torch(_likelihood(name), *[x[b] for x in args], indices[b], tt(cs["pair_mean"]),
                                                  tt(cs["pair_cov"]))
        assert torch.equal(one, both[b])
    fmu, fvar = MM.st_point_marginals(*args[:3], offsets, stack("pair_mean"), stack("pair_cov"))
    assert tuple(fmu.shape) == tuple(fvar.shape) == (2, 12)


# ---- the spatial kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,rho", [(SK.SquaredExponential, lambda r: np.exp(-0.5 * r * r)), (SK.Matern12, lambda r: np.exp(-r)),
                                     (SK.Matern32, lambda r: (1 + np.sqrt(3) * r) * np.exp(-np.sqrt(3) * r)),
                                     (SK.Matern52, lambda r: (1 + np.sqrt(5) * r + 5 * r * r / 3) * np.exp(-np.sqrt(5) * r))])
def test_spatial_kernels_against_their_closed_forms(cls, rho):
    rng = np.random.default_rng(4)
    x, x2 = rng.normal(size=(7, 3)), rng.normal(size=(5, 3))
    ls = np.array([0.7, 1.9])
    kern = cls(variance=1.7, lengthscales=tt(ls, True), active_dims=[0, 2])
    assert isinstance(kern, SK.SpatialKernel) and len(kern.trainable_variables) == 2
    dist = lambda p, q: np.sqrt(np.sum(((p[:, None, [0, 2]] - q[None, :, [0, 2]]) / ls) ** 2, axis=-1))          # noqa: E731
    np.testing.assert_allclose(kern.K(tt(x), tt(x2)).detach().numpy(), 1.7 * rho(dist(x, x2)), rtol=1e-13, atol=1e-15)
    kxx = kern.K(tt(x))
    np.testing.assert_allclose(kxx.detach().numpy(), 1.7 * rho(dist(x, x)), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(kern.K_diag(tt(x)).detach().numpy(), np.full(7, 1.7), rtol=0, atol=0)
    assert float(np.linalg.eigvalsh(kxx.detach().numpy()).min()) > 0, "positive definite on distinct points"
    (grad,) = torch.autograd.grad(kxx.sum(), kern.lengthscales)
    assert bool(torch.isfinite(grad).all()) and float(grad.abs().sum()) > 0, "differentiable, also through the zero distances"
    scalar = cls(variance=0.5, lengthscales=2.0)
    np.testing.assert_allclose(scalar.K(tt(x)).numpy(), 0.5 * rho(np.sqrt(np.sum((x[:, None] - x[None]) ** 2, -1)) / 2.0), rtol=1e-13)
    with pytest.raises(ValueError):
        cls(variance=-1.0)
    with pytest.raises(ValueError):
        cls(lengthscales=[1.0, 2.0], active_dims=[0])
    with pytest.raises(ValueError):
        cls(lengthscales=[1.0, 2.0]).K(tt(x))


# ---- the spatio-temporal kernel ---------------------------------------------------------------------------------------------------
def _time_kernel(cls=mfa.Matern32, grad=True):
    # (a hyper-parameter under the tape: the chain comes from the differentiable torch forms, which run on CPU tensors)
    return cls(lengthscale=tt(0.8, grad), variance=tt(1.0))


@pytest.mark.parametrize("cls,k_t", [(mfa.Matern12, lambda r: np.exp(-r / 0.8)),
                                     (mfa.Matern32, lambda r: (1 + np.sqrt(3) * r / 0.8) * np.exp(-np.sqrt(3) * r / 0.8))])
def test_the_kronecker_chain_reproduces_the_product_kernel(cls, k_t):
    rng = np.random.default_rng(8)
    z = tt(rng.normal(size=(4, 2)))
    space = SK.Matern32(variance=1.4, lengthscales=0.9)
    kern = mfa.SparseSpatioTemporalKernel(space, _time_kernel(cls), z, jitter=0.0)
    d_t = kern.kernel_time.state_dim
    assert kern.state_dim == 4 * d_t and kern.output_dim == 4 and kern.num_inducing_space == 4
    times = tt(np.array([0.0, 0.3, 1.1, 1.15, 2.5]))
    h = kern.generate_emission_model(times).emission_matrix.detach().numpy()
    assert h.shape == (5, 4, 4 * d_t)
    chol = np.linalg.cholesky(space.K(z).numpy())
    base = np.kron(np.eye(4), np.eye(1, d_t))                 # I (x) h, h = [1, 0, ...]
    np.testing.assert_allclose(h[0], chol @ base, rtol=1e-13, atol=1e-15)
    a_s, q_s = (x.detach().numpy() for x in kern.transition_statistics(times[:-1], times[1:] - times[:-1]))
    direct = kern._torch_transitions(times[1:] - times[:-1], True, True)          # (the inherited entry replicates the blocks too)
    assert tuple(direct[1].shape) == (4, 4 * d_t, 4 * d_t)
    np.testing.assert_allclose(direct[0].detach().numpy(), a_s, rtol=0, atol=0)
    np.testing.assert_allclose(direct[2].detach().numpy(), q_s, rtol=0, atol=0)
    p_inf = kern.initial_covariance(times[:1]).detach().numpy()
    # Cov(f(Z, t_i), f(Z, t_j)) from the chain, densely, against K_s (x) k_t
    covs = [p_inf]
    for k in range(4):
        covs.append(a_s[k] @ covs[k] @ a_s[k].T + q_s[k])
    dense = space.K(z).numpy()
    for i in range(5):
        cross = covs[i]
        for j in range(i, 5):
            if j > i:
                cross = a_s[j - 1] @ cross
            want = dense * k_t(abs(float(times[j] - times[i])))
            np.testing.assert_allclose(h[j] @ cross @ h[i].T, want, rtol=1e-10, atol=1e-12)
    proj = kern.state_to_space_conditional_projection(torch.cat([z, times[:4, None]], dim=-1)).detach().numpy()
    assert proj.shape == (4, 1, 4 * d_t)
    np.testing.assert_allclose(proj[:, 0, :], h[0], rtol=1e-9, atol=1e-11, err_msg="at Z_s the projection is the emission row")


def test_thirty_two_copies_never_reach_the_generators_component_limit(monkeypatch):
    z = tt(np.random.default_rng(0).normal(size=(32, 2)))
    kern = mfa.SparseSpatioTemporalKernel(SK.SquaredExponential(), _time_kernel(mfa.Matern32, grad=False), z)
    assert kern.state_dim == 64 and len(kern._components()) == 1, "ONE copy of the temporal components"
    calls = []

    def fake(deltas, want_chol, want_cov):
        calls.append(tuple(deltas.shape))
        block = torch.arange(4.0, dtype=deltas.dtype).reshape(2, 2).expand(tuple(deltas.shape) + (2, 2))
        return block, (block if want_chol else None), (block if want_cov else None)

    monkeypatch.setattr(kern.kernel_time, "_device_transitions", fake)
    a_s, chol, cov = kern._device_transitions(torch.ones(3, 5, dtype=torch.float64), True, False)
    assert calls == [(3, 5)] and tuple(a_s.shape) == tuple(chol.shape) == (3, 5, 64, 64) and cov is None
    want = torch.kron(torch.eye(32, dtype=torch.float64), torch.arange(4.0, dtype=torch.float64).reshape(2, 2))
    assert torch.equal(a_s[1, 2], want)


def test_constructor_and_function_error_paths():
    z = tt(np.zeros((3, 2)) + np.arange(3)[:, None])
    space, time = SK.Matern32(), _time_kernel()
    with pytest.raises(TypeError):
        mfa.SparseSpatioTemporalKernel(time, time, z)
    with pytest.raises(TypeError):
        mfa.SparseSpatioTemporalKernel(space, space, z)
    with pytest.raises(ValueError):
        mfa.SparseSpatioTemporalKernel(space, time, z[0])
    with pytest.raises(ValueError):
        mfa.SparseSpatioTemporalKernel(space, time, z, jitter=-1.0)
    with pytest.raises(NotImplementedError, match="exceeds 64"):
        mfa.SparseSpatioTemporalKernel(space, time, tt(np.zeros((33, 2))))
    case = _case(0, 3, 2, L.GAUSSIAN)
    a, wt, c, y, pm, pc = (tt(case[k]) for k in ("a", "wt", "c", "y", "pair_mean", "pair_cov"))
    offsets = torch.tensor(case["offsets"])
    indices = MM._segments_of(offsets, a.shape[0])
    lik = mfa.Gaussian(1.0)
    with pytest.raises(TypeError):
        MM.st_expected_log_likelihood_torch("gaussian", a, wt, c, y, indices, pm, pc)
    with pytest.raises(ValueError, match="pair_cov"):
        MM.st_expected_log_likelihood_torch(lik, a, wt, c, y, indices, pm, pc[:, :-1])
    with pytest.raises(ValueError, match="wt"):
        MM.st_expected_log_likelihood(lik, a, wt[:-1], c, y, offsets, pm, pc)
    with pytest.raises(NotImplementedError):
        MM.st_expected_log_likelihood_torch(lik, a, wt[:, :3], c, y, indices, pm, pc)
    with pytest.raises(ValueError):
        MM.st_point_marginals(a, wt, c.float(), offsets, pm, pc)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MM.st_expected_log_likelihood(lik, a, wt, c, y, offsets, pm, pc)
    assert MM.ST_EXPECT_TILE == 256
    assert {"SparseSpatioTemporalKernel", "SpatioTemporalSparseVariational", "spatial_kernels"} <= set(mfa.__all__)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "markovflow_amd.h")).read()
    declared = set(re.findall(r"\b(mf_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in ("mf_lik_st_expectations_f64", "mf_lik_st_expectations_f32", "mf_lik_st_expectations_workspace_bytes"):
        assert name in declared and name in _lib.exported_symbols() and getattr(lib, name) is not None


def test_workspace_formula_and_every_argument_error_need_no_gpu():
    lib = _lib.load()
    size = lib.mf_lik_st_expectations_workspace_bytes
    for tiles, ms, two_dt, elem in ((1, 1, 2, 8), (7, 5, 6, 4), (3, 32, 4, 8), (11, 64, 2, 4), (2, 21, 6, 8)):
        n = ms * two_dt
        assert int(size(tiles, ms, two_dt, elem)) == tiles * (n * (n + 1) // 2 + n + 1) * elem
    assert all(int(size(*args)) == 0 for args in ((0, 3, 2, 8), (-1, 3, 2, 8), (2, 0, 2, 8), (2, 3, 3, 8), (2, 33, 4, 8), (2, 3, 2, 2)))
    fn = lib.mf_lik_st_expectations_f64
    x, w = np.polynomial.hermite.hermgauss(20)
    nodes, weights = (ctypes.c_double * 20)(*x), (ctypes.c_double * 20)(*w)
    params = (ctypes.c_double * 1)(0.5)
    p = ctypes.c_void_p(64)                        # never dereferenced: every call below stops at an argument check
    good = [2, 5, 3, 3, 2, 0, params, 20, nodes, weights, p, p, p, p, p, p, p, 2, p, p, p, 1 << 20, p, p, p, p, p, p, p, p, None]
    bad = [(1, -1, -1), (2, -1, -2), (3, 0, -3), (4, 0, -100), (4, 65, -100), (5, 3, -100), (5, 0, -100), (6, 4, -6), (6, -1, -6),
           (7, None, -7), (8, 0, -8), (8, 33, -8), (9, None, -9), (10, None, -10), (11, None, -11), (12, None, -12), (13, None, -13),
           (14, None, -14), (15, None, -15), (16, None, -16), (17, None, -17), (18, -1, -18), (18, 1 << 31, -18), (19, None, -19),
           (20, None, -20), (21, None, -21), (22, 8, -22), (24, None, -24), (25, None, -25), (26, None, -26), (27, None, -27),
           (28, None, -28)]
    for position, value, code in bad:
        args = list(good)
        args[position - 1] = value
        assert fn(*args) == code, f"argument {position} = {value!r}"
    args = list(good)
    args[3], args[4] = 17, 8                       # Ms d_t = 68
    assert fn(*args) == -100
    args = list(good)
    args[1], args[17] = 0, 1                       # tiles without points
    assert fn(*args) == -18
    nothing = list(good)
    nothing[22:30] = [None] * 8
    assert fn(*nothing) == 0, "every output NULL: nothing asked for, nothing launched"
    none = list(good)
    none[0] = 0
    assert fn(*none) == 0, "B = 0: nothing is launched"
    only_projection = list(good)
    only_projection[14] = None                     # y
    only_projection[22:28] = [None] * 6
    only_projection[15] = None                     # pair_mean: the check behind y's is reached
    assert fn(*only_projection) == -16, "projection only: y may be NULL"
