"""
CPU tests of the piecewise-stationary kernel (markovflow_amd/kernels.py: PiecewiseKernel, NonStationaryKernel): construction and
its refusals, shapes, the segment lookup, the differentiable torch restatement of the generator against
tests/helpers/piecewise_closed_forms.py, the argument checks of mf_sde_piecewise_transitions_* / _grad_* (no GPU is touched), the
model classes that refuse a non-stationary kernel, and the reference's two tests (tests/unit/kernels/test_piecewise_stationary.py)
restated.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from markovflow_amd.posterior import APPROX_INF
from helpers import periodic_closed_forms as PC
from helpers import piecewise_closed_forms as PW
from helpers import piecewise_kernels as PK


def qp(order, osc=1, ls=0.7, var=1.3, period=1.7):
    return {"order": order, "ls": ls, "var": var, "period": period, "osc": osc}


def m(order, ls, var):
    return {"order": order, "ls": ls, "var": var, "osc": 0}


CONST = {"order": 0, "var": 1.5, "osc": 0}
QP_SEGMENTS = [[qp(5, 1)], [qp(5, 1, ls=0.3, var=0.5, period=0.9)]]
SUM_SEGMENTS = [[CONST, qp(5, 2), m(3, 0.9, 0.6)], [{"order": 0, "var": 0.7, "osc": 0}, qp(5, 2, ls=0.4, var=2.0, period=0.8), m(3, 0.2, 1.9)],
                [{"order": 0, "var": 0.2, "osc": 0}, qp(5, 2, ls=1.4, var=0.3, period=3.0), m(3, 2.0, 0.1)]]


# ---- construction ------------------------------------------------------------------------------------------------------------------
def test_constructor_validation():
    cp = torch.tensor([1.0], dtype=torch.float64)
    two = lambda: [mfa.Matern32(1.0, 1.0), mfa.Matern32(2.0, 0.5)]                              # noqa: E731
    k = mfa.PiecewiseKernel(two(), cp, jitter=1e-6)
    assert isinstance(k, mfa.NonStationaryKernel) and isinstance(k, mfa.SDEKernel) and not isinstance(k, mfa.StationaryKernel)
    assert k.state_dim == 2 and k.output_dim == 1 and k.num_change_points == 1 and len(k.kernels) == 2
    assert not k.change_points.requires_grad
    with pytest.raises(AssertionError):
        mfa.PiecewiseKernel([], torch.zeros(0, dtype=torch.float64))
    with pytest.raises(AssertionError):                       # one more kernel than change points
        mfa.PiecewiseKernel(two(), torch.tensor([1.0, 2.0], dtype=torch.float64))
    with pytest.raises(TypeError):                            # mismatched classes
        mfa.PiecewiseKernel([mfa.Matern32(1.0, 1.0), mfa.Matern12(1.0, 1.0) * mfa.HarmonicOscillator(1.0, 1.0)], cp)
    with pytest.raises(TypeError):
        mfa.PiecewiseKernel([mfa.Matern32(1.0, 1.0), 3.0], cp)
    with pytest.raises(AssertionError):                       # mismatched state dimensions
        mfa.PiecewiseKernel([mfa.Matern32(1.0, 1.0), mfa.Matern52(1.0, 1.0)], cp)
    with pytest.raises(AssertionError):                       # mismatched output dimensions
        mfa.PiecewiseKernel([mfa.Matern32(1.0, 1.0), mfa.Matern32(1.0, 1.0, output_dim=2)], cp)
    with pytest.raises(TypeError):                            # one class, one state dimension, another signature
        mfa.PiecewiseKernel([mfa.Sum([mfa.Matern12(1.0, 1.0), mfa.Matern32(1.0, 1.0)]),
                             mfa.Sum([mfa.Matern32(1.0, 1.0), mfa.Matern12(1.0, 1.0)])], cp)
    with pytest.raises(TypeError):                            # ... the two Kronecker orders of a product
        mfa.PiecewiseKernel([mfa.Matern32(1.0, 1.0) * mfa.HarmonicOscillator(1.0, 1.0),
                             mfa.HarmonicOscillator(1.0, 1.0) * mfa.Matern32(1.0, 1.0)], cp)
    for bad in ([2.0, 1.0], [float("nan"), 1.0], [0.0, float("inf")]):
        with pytest.raises(ValueError):
            mfa.PiecewiseKernel(two() + [mfa.Matern32(3.0, 1.0)], torch.tensor(bad, dtype=torch.float64))
    with pytest.raises(ValueError):
        mfa.PiecewiseKernel(two(), torch.tensor([[1.0]], dtype=torch.float64))
    with pytest.raises(AssertionError):
        mfa.PiecewiseKernel(two(), cp, jitter=-1.0)
    # the signatures the kernel is meant for
    for make in (lambda: mfa.Matern32(1.0, 1.0), lambda: mfa.Matern52(1.0, 1.0) * mfa.HarmonicOscillator(1.0, 1.0),
                 lambda: mfa.Constant(1.0) + mfa.Matern12(1.0, 1.0)):
        assert mfa.PiecewiseKernel([make(), make()], cp).state_dim == make().state_dim


def test_refusals_of_combinations():
    cp = torch.tensor([1.0], dtype=torch.float64)
    pw = mfa.PiecewiseKernel([mfa.Matern32(1.0, 1.0), mfa.Matern32(2.0, 0.5)], cp)
    multi = lambda: mfa.IndependentMultiOutput([mfa.Matern32(1.0, 1.0)])                         # noqa: E731
    st = lambda: mfa.SparseSpatioTemporalKernel(mfa.spatial_kernels.SquaredExponential(1.0, 1.0),     # noqa: E731
                                                mfa.Matern32(1.0, 1.0), torch.zeros((2, 1), dtype=torch.float64))
    for children in ([multi(), multi()], [st(), st()], [pw, pw]):
        with pytest.raises(NotImplementedError):
            mfa.PiecewiseKernel(children, cp)
    for make in (lambda: mfa.Sum([pw, mfa.Matern32(1.0, 1.0)]), lambda: pw + mfa.Matern32(1.0, 1.0),
                 lambda: mfa.Product([pw, mfa.HarmonicOscillator(1.0, 1.0)]), lambda: pw * mfa.Constant(1.0),
                 lambda: mfa.IndependentMultiOutput([pw]),
                 lambda: mfa.SparseSpatioTemporalKernel(mfa.spatial_kernels.SquaredExponential(1.0, 1.0), pw,
                                                        torch.zeros((2, 1), dtype=torch.float64))):
        with pytest.raises(NotImplementedError, match="non-stationary"):
            make()


def test_every_model_but_gpr_refuses_a_piecewise_kernel():
    cp = torch.tensor([1.0], dtype=torch.float64)
    pw = mfa.PiecewiseKernel([mfa.Matern32(1.0, 1.0), mfa.Matern32(2.0, 0.5)], cp)
    t = torch.linspace(0.0, 2.0, 6, dtype=torch.float64)
    data = (t, torch.zeros((6, 1), dtype=torch.float64))
    z = torch.linspace(0.0, 2.0, 3, dtype=torch.float64)
    lik = mfa.Gaussian(0.1)
    zs, ks = torch.zeros((2, 1), dtype=torch.float64), mfa.spatial_kernels.SquaredExponential(1.0, 1.0)
    makers = {
        "CVIGaussianProcess": lambda: mfa.CVIGaussianProcess(data, pw, lik),
        "PowerExpectationPropagation": lambda: mfa.PowerExpectationPropagation(data, pw, lik),
        "SparseCVIGaussianProcess": lambda: mfa.SparseCVIGaussianProcess(pw, z, lik),
        "SparsePowerExpectationPropagation": lambda: mfa.SparsePowerExpectationPropagation(pw, z, lik),
        "SparseVariationalGaussianProcess": lambda: mfa.SparseVariationalGaussianProcess(pw, lik, z),
        "ImportanceWeightedVI": lambda: mfa.ImportanceWeightedVI(pw, z, lik, 4),
        "VariationalGaussianProcess": lambda: mfa.VariationalGaussianProcess(data, pw, lik),
        "SpatioTemporalSparseVariational": lambda: mfa.SpatioTemporalSparseVariational(zs, z, ks, pw, lik),
        "SpatioTemporalSparseCVI": lambda: mfa.SpatioTemporalSparseCVI(zs, z, ks, pw, lik),
    }
    public = {n for n, c in vars(mfa.models).items()
              if n in mfa.__all__ and isinstance(c, type) and (c.__module__ + ".").startswith(mfa.models.__name__ + ".")}
    assert set(makers) | {"GaussianProcessRegression"} == public        # (a model class added later has to take a stand too)
    for name, make in makers.items():
        with pytest.raises(NotImplementedError, match="non-stationary"):
            make()
    mfa.GaussianProcessRegression(data, pw)                     # the one model that takes it


# ---- the segment lookup and the per-time-point methods ----------------------------------------------------------------------------
def test_split_time_indices():
    cp = torch.tensor([0.0, 1.0, 1.0, 2.5], dtype=torch.float64)          # (a repeated change point: segment 2 is empty)
    k = mfa.PiecewiseKernel([mfa.Matern12(1.0 + i, 1.0) for i in range(5)], cp)
    t = torch.tensor([[-APPROX_INF, -0.1, 0.0, 0.5, 1.0, 1.7, 2.5, 3.0, APPROX_INF],
                      [2.6, 2.5, 2.4, 1.0, 0.99, 0.0, -1e-300, 7.0, -7.0]], dtype=torch.float64)
    want = np.array([[0, 0, 1, 1, 3, 3, 4, 4, 4], [4, 4, 3, 3, 1, 1, 0, 4, 0]])
    got = k.split_time_indices(t)
    assert got.dtype == torch.int64 and tuple(got.shape) == (2, 9)
    np.testing.assert_array_equal(got.numpy(), want)
    np.testing.assert_array_equal(PW.segment_index(t.numpy(), cp.numpy()), want)
    assert 2 not in got.numpy()
    # the comparison runs in the dtype of the times: 1 + 2^-30 is 1 in float32, and a time on a change point goes right
    k2 = mfa.PiecewiseKernel([mfa.Matern12(1.0, 1.0), mfa.Matern12(2.0, 1.0)], torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64))
    one = torch.tensor([1.0], dtype=torch.float64)
    assert int(k2.split_time_indices(one)) == 0 and int(k2.split_time_indices(one.float())) == 1
    assert int(PW.segment_index(1.0, [1.0 + 2.0 ** -30])) == 0 and int(PW.segment_index(1.0, [1.0 + 2.0 ** -30], np.float32)) == 1
    # no change point at all: one segment
    k1 = mfa.PiecewiseKernel([mfa.Matern12(1.0, 1.0)], torch.zeros(0, dtype=torch.float64))
    assert torch.all(k1.split_time_indices(t) == 0)


def test_change_points_are_read_only_and_lookup_times():
    k = mfa.PiecewiseKernel([mfa.Matern12(1.0, 1.0), mfa.Matern12(2.0, 1.0)], torch.tensor([1.0], dtype=torch.float64))
    with pytest.raises(AttributeError):
        k.change_points = torch.tensor([2.0], dtype=torch.float64)
    t = torch.tensor([0.5, 1.5, 2.5], dtype=torch.float64)
    np.testing.assert_array_equal(k.split_time_indices(t).numpy(), [0, 1, 1])
    k.change_points.add_(1.0)                                  # an in-place write is seen by the lookup (the copies carry the version)
    np.testing.assert_array_equal(k.split_time_indices(t).numpy(), [0, 0, 1])
    # before the first conditioning point the dynamics are those active AT it; a stationary kernel takes the times as they are
    train = torch.tensor([[2.5, 3.0], [0.2, 0.4]], dtype=torch.float64)
    times = torch.tensor([[-APPROX_INF, 0.5, 2.7], [-APPROX_INF, 0.1, 0.3]], dtype=torch.float64)
    np.testing.assert_array_equal(k._lookup_times(times, train).numpy(), [[2.5, 2.5, 2.7], [0.2, 0.2, 0.3]])
    assert mfa.Matern12(1.0, 1.0)._lookup_times(times, train) is times


def test_shapes_and_per_time_point_methods():
    cps = [1.0, 2.0]
    kern = PK.build(SUM_SEGMENTS, cps, jitter=1e-6)
    t = torch.tensor([[0.0, 0.5, 1.0, 1.5, 2.0, 2.5], [1.0, 1.1, 1.2, 1.3, 1.4, 3.0]], dtype=torch.float64)
    d = 9
    assert kern.state_dim == d and [(c.order, c._osc) for c in kern._components()] == [(0, 0), (5, 2), (3, 0)]
    p = kern.steady_state_covariances(t)
    f = kern.feedback_matrices(t)
    assert tuple(p.shape) == (2, 6, d, d) and tuple(f.shape) == (2, 6, d, d)
    np.testing.assert_allclose(p.numpy(), PW.steady_state(SUM_SEGMENTS, cps, t.numpy()), rtol=1e-14)
    seg = kern.split_time_indices(t).numpy()
    for s in range(2):
        for i in range(6):
            np.testing.assert_array_equal(f[s, i].numpy(), kern.kernels[seg[s, i]].feedback_matrix.numpy())
    assert tuple(kern.state_means(t).shape) == (2, 6, d) and not kern.state_means(t).any()
    assert tuple(kern.initial_mean((2,)).shape) == (2, d) and not kern.initial_mean((2,)).any()
    dts, starts = t[..., 1:] - t[..., :-1], t[..., :-1]
    assert tuple(kern.state_offsets(starts, dts).shape) == (2, 5, d) and not kern.state_offsets(starts, dts).any()
    # P-infinity of the segment holding EACH series' first point (series 0 starts in segment 0, series 1 in segment 1)
    p0 = kern.initial_covariance(t[..., :1])
    assert tuple(p0.shape) == (2, d, d)
    for s, k in ((0, 0), (1, 1)):
        np.testing.assert_allclose(p0[s].numpy(), PC.concat_transitions(SUM_SEGMENTS[k], np.ones(1))[2] + 1e-6 * np.eye(d), rtol=1e-14)
    assert tuple(kern.jitter_matrix.shape) == (d, d) and float(kern.jitter_matrix[0, 0]) == 1e-6
    h = kern.generate_emission_model(t).emission_matrix
    np.testing.assert_array_equal(h.numpy(), PC.emission(SUM_SEGMENTS[0], t.shape))
    with pytest.raises(ValueError, match="transition_times"):
        kern._device_transitions(dts, True, False)
    # the leaves are all segments' hyper-parameters, and the caches can be told to forget every one of them
    leaves = []
    kern = PK.build(QP_SEGMENTS, [1.0], leaves=leaves)
    assert len(leaves) == 8 and kern._needs_grad()
    got = [x for c in kern._components() for x in c._leaves()]
    assert len(got) == 8 and all(any(x is y for y in leaves) for x in got)
    kern.invalidate_cache()
    mfa.GaussianProcessRegression((t[0], torch.zeros((6, 1), dtype=torch.float64)), kern).invalidate_hyperparameter_cache()
    # per-series hyper-parameters carry their batch shape
    per = [[m(3, np.array([0.5, 0.9]), 1.0)], [m(3, 2.0, np.array([0.3, 0.4]))]]
    kb = PK.build(per, [1.0])
    pb = kb.steady_state_covariances(t)
    assert tuple(pb.shape) == (2, 6, 2, 2)
    for s in range(2):
        one = [[m(3, 0.5 if s == 0 else 0.9, 1.0)], [m(3, 2.0, 0.3 if s == 0 else 0.4)]]
        np.testing.assert_allclose(pb[s].numpy(), PW.steady_state(one, [1.0], t[s].numpy()), rtol=1e-14)


# ---- the torch route against the closed forms ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["qp2", "sum3", "matern12"])
def test_torch_transitions_vs_closed_forms(rng, case):
    segments, cps = {"qp2": (QP_SEGMENTS, [1.0]), "sum3": (SUM_SEGMENTS, [0.8, 1.9]),
                     "matern12": ([[m(1, 0.5, 1.0)], [m(1, 1.5, 0.4)], [m(1, 0.1, 2.0)], [m(1, 3.0, 0.2)]], [0.5, 0.5, 2.0])}[case]
    jit = 1e-6
    t = np.cumsum(0.05 + rng.exponential(0.2, size=(3, 13)), axis=-1)
    t[1] = t[1, rng.permutation(13)]                                    # one series with unsorted start times
    t[2, 4] = cps[0]                                                    # a start time exactly on a change point
    starts, dt = t[:, :-1], 0.05 + rng.exponential(0.2, size=(3, 12))
    starts[0, 0], starts[0, -1] = -APPROX_INF, APPROX_INF
    kern = PK.build(segments, cps, jitter=jit)
    a_ref, q_ref, p_ref, seg = PW.transitions(segments, cps, starts, dt, jitter=jit)
    assert seg[2, 4] == sum(c <= cps[0] for c in cps) and seg[0, 0] == 0 and seg[0, -1] == len(cps)
    np.testing.assert_array_equal(kern.split_time_indices(torch.tensor(starts)).numpy(), seg)
    a_s, chol, q_s = kern._torch_transitions(torch.tensor(dt), True, True, torch.tensor(starts))
    np.testing.assert_allclose(a_s.numpy(), a_ref, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(q_s.numpy(), q_ref, rtol=1e-10, atol=1e-13)
    cc = chol.numpy()
    np.testing.assert_allclose(cc @ np.swapaxes(cc, -1, -2), q_ref, rtol=1e-10, atol=1e-13)
    assert np.all(np.triu(cc, 1) == 0)
    np.testing.assert_allclose(kern.steady_state_covariances(torch.tensor(starts)).numpy(), p_ref, rtol=1e-14)
    # the public methods honour transition_times (CPU tensors under a gradient take this route)
    leaves = []
    kern = PK.build(segments, cps, jitter=jit, leaves=leaves)
    a_p, q_p = kern.transition_statistics(torch.tensor(starts), torch.tensor(dt))
    np.testing.assert_allclose(a_p.detach().numpy(), a_ref, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(q_p.detach().numpy(), q_ref, rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(kern.state_transitions(torch.tensor(starts), torch.tensor(dt)).detach().numpy(), a_ref, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(kern.process_covariances(torch.tensor(starts), torch.tensor(dt)).detach().numpy(), q_ref, rtol=1e-10,
                               atol=1e-13)
    ts = np.sort(t, axis=-1)
    a_t, q_t = kern.transition_statistics_from_time_points(torch.tensor(ts))
    a_r, q_r, _, _ = PW.transitions(segments, cps, ts[:, :-1], np.diff(ts, axis=-1), jitter=jit)
    np.testing.assert_allclose(a_t.detach().numpy(), a_r, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(q_t.detach().numpy(), q_r, rtol=1e-10, atol=1e-13)


def test_torch_transitions_gradcheck():
    """Two segments of Matern52 * HarmonicOscillator: the derivative with respect to every segment's leaves, and with respect to the
    time gaps (gaps at which chol Q is well conditioned, as in test_kernels_periodic_host.py)."""
    starts = torch.tensor([[0.1, 0.4, 1.0, 1.55]], dtype=torch.float64)          # (segments 0, 0, 1, 1)
    dts = torch.tensor([[0.3, 0.55, 0.5, 0.9]], dtype=torch.float64)
    cp = torch.tensor([1.0], dtype=torch.float64)

    def fn(dt, *hyper):
        kernels = [mfa.Matern52(hyper[4 * k], hyper[4 * k + 1]) * mfa.HarmonicOscillator(hyper[4 * k + 2], hyper[4 * k + 3])
                   for k in range(2)]
        return mfa.PiecewiseKernel(kernels, cp, jitter=1e-8)._torch_transitions(dt, True, True, starts)

    vals = (0.7, 1.3, 0.8, 1.7, 0.5, 0.6, 1.1, 0.9)
    leaves = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in vals]
    assert torch.autograd.gradcheck(fn, [dts.clone().requires_grad_(True)] + leaves, eps=1e-6, atol=1e-6, rtol=1e-5)
    # every segment's leaves receive a gradient through the public route, and only from the steps of their segment
    kernels = [mfa.Matern52(leaves[4 * k], leaves[4 * k + 1]) * mfa.HarmonicOscillator(leaves[4 * k + 2], leaves[4 * k + 3])
               for k in range(2)]
    kern = mfa.PiecewiseKernel(kernels, cp)
    a_s, _ = kern.transition_statistics(starts, dts)
    torch.sum(a_s[:, :2]).backward()
    assert all(float(x.grad.abs()) > 0 for x in (leaves[0], leaves[3])) and all(x.grad is None or float(x.grad.abs()) == 0 for x in leaves[4:])


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
FWD, GRAD = "mf_sde_piecewise_transitions", "mf_sde_piecewise_transitions_grad"


def test_symbols_are_declared_bound_and_exported():
    assert len(_lib._SIGS[FWD][1]) == 19 and len(_lib._SIGS[GRAD][1]) == 20
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "markovflow_amd.h")).read()
    lib = _lib.load()
    for base in (FWD, GRAD):
        for suf in ("_f64", "_f32"):
            assert base + suf in _lib.exported_symbols()
            assert re.search(r"\bint " + base + suf + r"\(", header)
            assert getattr(lib, base + suf).restype is ctypes.c_int
    assert GRAD + "_workspace_bytes" in _lib.exported_symbols() and re.search(r"\bsize_t " + GRAD + r"_workspace_bytes\(", header)
    assert "PiecewiseKernel" in mfa.__all__ and "NonStationaryKernel" in mfa.__all__
    # per block of 64 steps: 64 records of 3 ncomp values, their segments, one count
    assert lib.mf_sde_piecewise_transitions_grad_workspace_bytes(3, 65, 2, 8) == 3 * 2 * (64 * 6 * 8 + 64 * 4 + 4)
    assert lib.mf_sde_piecewise_transitions_grad_workspace_bytes(3, 0, 2, 8) == 0
    assert lib.mf_sde_piecewise_transitions_grad_workspace_bytes(3, 65, 2, 2) == 0


def test_generator_argument_errors_without_touching_the_gpu():
    """mf_sde_piecewise_transitions_* / _grad_*: invalid arguments are refused before any launch, by the negative position of the
    argument; -100 when the staging image of 64 d x d blocks exceeds the LDS limit (d = 18 in fp64)."""
    lib = _lib.load()
    ints = lambda *v: (ctypes.c_int * len(v))(*v)                                            # noqa: E731
    some = ctypes.c_void_p(8)                                                                # (never dereferenced)
    o2, r2 = ints(0, 5), ints(1, 2)

    def fwd(fn, b, n, nc, o, r, nseg, cp=None, lam=None, var=None, om=None, ts=None, dt=None, a=None):
        return fn(b, n, nc, o, r, nseg, cp, lam, var, om, 0, ts, dt, 0.0, a, None, None, None, None)

    def grad(fn, b, n, nc, o, r, nseg, cp=None, lam=None, var=None, om=None, ts=None, dt=None, out=None, ws=None, wsb=0):
        return fn(b, n, nc, o, r, nseg, cp, lam, var, om, 0, ts, dt, 0.0, None, None, out, ws, wsb, None)

    for suf in ("_f64", "_f32"):
        for call, fn in ((fwd, getattr(lib, FWD + suf)), (grad, getattr(lib, GRAD + suf))):
            assert call(fn, -1, 4, 1, ints(0), ints(0), 1) == -1
            assert call(fn, 1, -4, 1, ints(0), ints(0), 1) == -2
            assert call(fn, 1, 4, 0, ints(0), ints(0), 1) == -3 and call(fn, 1, 4, 17, ints(*[1] * 17), ints(*[0] * 17), 1) == -3
            assert call(fn, 1, 4, 2, ints(0, 2), r2, 1) == -4 and call(fn, 1, 4, 1, None, ints(0), 1) == -4
            assert call(fn, 1, 4, 2, o2, ints(3, 0), 1) == -5 and call(fn, 1, 4, 1, ints(0), None, 1) == -5
            assert call(fn, 1, 4, 2, o2, r2, 0) == -6 and call(fn, 1, 4, 2, o2, r2, -3) == -6
            assert call(fn, 0, 4, 2, o2, r2, 2) == 0 and call(fn, 1, 0, 2, o2, r2, 2) == 0
            assert call(fn, 1, 4, 2, o2, r2, 2) == -7
            assert call(fn, 1, 4, 2, o2, r2, 1) == -8                     # (one segment: no change points needed)
            assert call(fn, 1, 4, 2, o2, r2, 2, some) == -8
            assert call(fn, 1, 4, 2, o2, r2, 2, some, some) == -9
            assert call(fn, 1, 4, 2, o2, r2, 2, some, some, some) == -10
            assert call(fn, 1, 4, 2, o2, ints(0, 0), 2, some, some, some) == -12     # (no oscillator: omega may be NULL)
            assert call(fn, 1, 4, 2, o2, r2, 2, some, some, some, some) == -12
            assert call(fn, 1, 4, 2, o2, r2, 2, some, some, some, some, some) == -13
        f, g = getattr(lib, FWD + suf), getattr(lib, GRAD + suf)
        assert fwd(f, 1, 4, 2, o2, r2, 2, some, some, some, some, some, some) == -15
        assert grad(g, 1, 4, 2, o2, r2, 2, some, some, some, some, some, some) == -17
        assert grad(g, 1, 4, 2, o2, r2, 2, some, some, some, some, some, some, some) == -18
        need = lib.mf_sde_piecewise_transitions_grad_workspace_bytes(1, 4, 2, 8 if suf == "_f64" else 4)
        assert grad(g, 1, 4, 2, o2, r2, 2, some, some, some, some, some, some, some, some, need - 1) == -19
    big = (ints(5, 5, 5), ints(1, 1, 1))
    assert fwd(lib.mf_sde_piecewise_transitions_f64, 1, 4, 3, *big, 2, some, some, some, some, some, some, some) == -100


# ---- the reference's two tests, restated ---------------------------------------------------------------------------------------------
def chain_marginals(kern, t):
    """Marginal state covariances of kern's chain on t [n] by recursion on the torch-route transitions (CPU)."""
    t = torch.tensor(t)
    a_s, q_s = kern.transition_statistics_from_time_points(t)
    a_s, q_s = a_s.detach().numpy(), q_s.detach().numpy()
    out = [kern.initial_covariance(t[:1]).detach().numpy()]
    for k in range(len(t) - 1):
        out.append(a_s[k] @ out[-1] @ a_s[k].T + q_s[k])
    return np.stack(out)


def grad_leaf(v):
    return torch.tensor(v, dtype=torch.float64, requires_grad=True)       # (CPU tensors under a gradient: the torch route)


def test_equal_parameter_segments_reproduce_the_base_kernel():
    """tests/unit/kernels/test_piecewise_stationary.py::test_piecewise_stationary_matern: with the same hyper-parameters in every
    segment the chain is the base kernel's, whatever the change points."""
    t = np.linspace(0.0, 10.0, 21)
    base = mfa.Matern52(grad_leaf(0.9), grad_leaf(1.4), jitter=1e-9)
    pw = mfa.PiecewiseKernel([mfa.Matern52(grad_leaf(0.9), grad_leaf(1.4)) for _ in range(4)],
                             torch.tensor([2.0, 3.3, 7.5], dtype=torch.float64), jitter=1e-9)
    for got, want in zip(pw.transition_statistics_from_time_points(torch.tensor(t)), base.transition_statistics_from_time_points(torch.tensor(t))):
        np.testing.assert_array_equal(got.detach().numpy(), want.detach().numpy())
    want = chain_marginals(base, t)
    np.testing.assert_allclose(chain_marginals(pw, t), want, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(want, np.broadcast_to(base.steady_state_covariance.detach().numpy(), want.shape), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(PW.state_marginals([[m(5, 0.9, 1.4)]] * 4, [2.0, 3.3, 7.5], t, jitter=1e-9), want, rtol=1e-10, atol=1e-13)


def test_two_segments_equal_two_stitched_chains():
    """tests/unit/kernels/test_piecewise_stationary.py::test_piecewise_stationary_2_kernels: with the change point among the time
    points, the transitions before it are the first kernel's on the first part of the grid and those from it on the second
    kernel's on the second part."""
    t = np.linspace(0.0, 10.0, 21)
    split = 8
    k1, k2 = (mfa.Matern32(grad_leaf(ls), grad_leaf(var), jitter=1e-9) for ls, var in ((0.5, 1.0), (2.5, 3.0)))
    pw = mfa.PiecewiseKernel([k1, k2], torch.tensor([t[split]], dtype=torch.float64), jitter=1e-9)
    a_s, q_s = pw.transition_statistics_from_time_points(torch.tensor(t))
    a_1, q_1 = k1.transition_statistics_from_time_points(torch.tensor(t[:split + 1]))
    a_2, q_2 = k2.transition_statistics_from_time_points(torch.tensor(t[split:]))
    np.testing.assert_array_equal(a_s.detach().numpy(), np.concatenate([a_1.detach().numpy(), a_2.detach().numpy()]))
    np.testing.assert_array_equal(q_s.detach().numpy(), np.concatenate([q_1.detach().numpy(), q_2.detach().numpy()]))
    marg = chain_marginals(pw, t)
    p1, p2 = (k.steady_state_covariance.detach().numpy() for k in (k1, k2))
    np.testing.assert_allclose(marg[:split + 1], np.broadcast_to(p1, (split + 1, 2, 2)), rtol=1e-6, atol=1e-6)     # stationary up to the change
    assert not np.allclose(marg[split + 1], p1, rtol=1e-2) and not np.allclose(marg[split + 1], p2, rtol=1e-2)
    np.testing.assert_allclose(marg[-1], p2, rtol=5e-2, atol=5e-2)                                                  # ... relaxing to the second
    np.testing.assert_allclose(marg, PW.state_marginals([[m(3, 0.5, 1.0)], [m(3, 2.5, 3.0)]], [t[split]], t, jitter=1e-9),
                               rtol=1e-10, atol=1e-13)
