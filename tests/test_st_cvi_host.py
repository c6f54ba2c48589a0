"""
CPU tests of the spatio-temporal sparse CVI model's host side (``models.st_cvi_site_update_torch``, ``SpatioTemporalSparseCVI``'s
projection, the declarations of ``mf_lik_st_cvi_site_update_*``) and of the reference the GPU tests lean on
(tests/helpers/st_cvi_closed_forms.py): the torch composition against the helper's literal statement of the reference's update, the
identity ``theta_1 = g_mean - 2 g_cov m`` against the autograd gradients of ``st_expected_log_likelihood_torch``, the exact decay of an
empty segment, the NaN rule, the dense projection, the error paths, the symbols and every argument error code.
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
from helpers import sparse_cvi_closed_forms as SC
from helpers import st_cvi_closed_forms as STC

NAMES = [L.GAUSSIAN, L.BERNOULLI, L.POISSON, L.STUDENTT]
SIZES = [(2, 1), (5, 3), (21, 3)]
LENGTHS = (2, 0, 9, 1)          # an empty segment and a single point among them


def tt(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def _likelihood(name):
    params = L.LIKELIHOODS[name][1]
    return {L.GAUSSIAN: lambda: mfa.Gaussian(params[0]), L.BERNOULLI: mfa.Bernoulli, L.POISSON: mfa.Poisson,
            L.STUDENTT: lambda: mfa.StudentT(*params)}[name]()


def _case(seed, ms, dt, name, lengths=LENGTHS, zero_sites=False):
    rng = np.random.default_rng(seed)
    n, segs, pair = int(np.sum(lengths)), len(lengths), 2 * ms * dt
    root, site = rng.normal(size=(segs, pair, pair)), rng.normal(size=(segs, pair, pair))
    case = dict(a=rng.uniform(-1, 1, size=(n, ms)) / np.sqrt(ms), wt=rng.uniform(-0.7, 0.7, size=(n, 2 * dt)) / np.sqrt(dt),
                c=rng.uniform(0.05, 0.5, size=n), y=np.resize(np.asarray(L.OBSERVED[name]), n),
                offsets=np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), pair_mean=rng.normal(size=(segs, pair)),
                pair_cov=root @ root.transpose(0, 2, 1) / pair + 0.1 * np.eye(pair),
                nat1=rng.normal(size=(segs, pair)), nat2=-0.5 * (site + site.transpose(0, 2, 1)))
    if zero_sites:
        case["nat1"], case["nat2"] = np.zeros_like(case["nat1"]), np.zeros_like(case["nat2"])
    return case


def _torch_step(name, case, lr):
    """``st_cvi_site_update_torch`` on a copy of the case's sites: ``(nat1, nat2, ve_sum, fmu, fvar)``."""
    nat1, nat2 = tt(case["nat1"]), tt(case["nat2"])
    indices = MM._segments_of(torch.tensor(case["offsets"]), case["a"].shape[0])
    outs = MM.st_cvi_site_update_torch(_likelihood(name), *[tt(case[k]) for k in ("a", "wt", "c", "y")], indices, tt(case["pair_mean"]),
                                       tt(case["pair_cov"]), lr, nat1, nat2)
    return (nat1, nat2) + tuple(outs)


@pytest.mark.parametrize("ms,dt", SIZES)
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("lr,zero_sites", [(1.0, True), (0.3, False)])
def test_the_torch_composition_against_the_helpers_literal_update(name, ms, dt, lr, zero_sites):
    case = _case(7, ms, dt, name, zero_sites=zero_sites)
    want = STC.st_cvi_site_update(L.LIKELIHOODS[name], *[case[k] for k in ("a", "wt", "c", "y", "offsets", "pair_mean", "pair_cov")], lr,
                                  case["nat1"], case["nat2"])
    got = dict(zip(("nat1", "nat2", "ve_sum", "fmu", "fvar"), _torch_step(name, case, lr)))
    for key, value in got.items():
        np.testing.assert_allclose(value.numpy(), want[key], rtol=1e-12, atol=1e-12 * float(np.max(want["mag_" + key]) + 1e-300),
                                   err_msg=key)


@pytest.mark.parametrize("name", NAMES)
def test_theta1_is_g_mean_minus_two_g_cov_m(name):
    """From zero sites at lr = 1 the new sites are the site sums: against the autograd gradients of the data term."""
    case = _case(3, 5, 3, name, zero_sites=True)
    nat1, nat2 = _torch_step(name, case, 1.0)[:2]
    pm, pc = tt(case["pair_mean"]).requires_grad_(True), tt(case["pair_cov"]).requires_grad_(True)
    indices = MM._segments_of(torch.tensor(case["offsets"]), case["a"].shape[0])
    ve = MM.st_expected_log_likelihood_torch(_likelihood(name), *[tt(case[k]) for k in ("a", "wt", "c", "y")], indices, pm, pc)
    g_mean, g_cov = torch.autograd.grad(ve.sum(), (pm, pc))
    theta1 = g_mean - 2.0 * torch.einsum("sij,sj->si", g_cov, pm.detach())
    scale = float(g_mean.abs().max() + 2.0 * torch.einsum("sij,sj->si", g_cov.abs(), pm.detach().abs()).max())
    np.testing.assert_allclose(nat1.numpy(), theta1.numpy(), rtol=0, atol=1e-12 * scale)
    np.testing.assert_allclose(nat2.numpy(), g_cov.numpy(), rtol=1e-12, atol=1e-13 * float(g_cov.abs().max()))


def test_an_empty_segment_decays_by_exactly_one_minus_lr():
    case = _case(5, 5, 3, L.BERNOULLI)
    lr = 0.3
    nat1, nat2 = _torch_step(L.BERNOULLI, case, lr)[:2]
    assert LENGTHS[1] == 0
    assert torch.equal(nat1[1], (1.0 - lr) * tt(case["nat1"])[1]) and torch.equal(nat2[1], (1.0 - lr) * tt(case["nat2"])[1])
    assert not torch.equal(nat1[0], (1.0 - lr) * tt(case["nat1"])[0])
    none = {**case, **{k: case[k][:0] for k in ("a", "wt", "c", "y")}, "offsets": np.zeros(5, dtype=np.int64)}
    nat1, nat2, ve_sum = _torch_step(L.BERNOULLI, none, lr)[:3]
    assert torch.equal(nat1, (1.0 - lr) * tt(case["nat1"])) and torch.equal(nat2, (1.0 - lr) * tt(case["nat2"])), "N = 0: every site"
    assert float(ve_sum.abs().max()) == 0.0


@pytest.mark.parametrize("name", [L.GAUSSIAN, L.BERNOULLI])
def test_a_negative_variance_poisons_its_own_segment_only(name):
    case = _case(9, 2, 1, name)
    clean = _torch_step(name, case, 0.3)
    bad = {**case, "c": case["c"].copy()}
    point = int(case["offsets"][2]) + 4                 # a point of segment 2
    bad["c"][point] = -1e6
    nat1, nat2, ve_sum, fmu, fvar = _torch_step(name, bad, 0.3)
    for got, ref in ((nat1, clean[0]), (nat2, clean[1]), (ve_sum, clean[2])):
        assert bool(torch.isnan(got[2]).all()), "the sites of the poisoned segment are NaN, also for a constant gv"
        keep = torch.tensor([0, 1, 3])
        assert torch.equal(got[keep], ref[keep])
    assert bool(torch.isnan(fmu[point])) and bool(torch.isnan(fvar[point]))
    mask = torch.arange(fmu.shape[0]) != point
    assert torch.equal(fmu[mask], clean[3][mask]) and torch.equal(fvar[mask], clean[4][mask])


def test_a_batch_is_its_series_one_by_one():
    name = L.POISSON
    cases = [_case(seed, 3, 2, name, lengths=lengths) for seed, lengths in ((1, (4, 0, 5, 3)), (2, (0, 6, 6, 0)))]
    stack = lambda k: tt(np.stack([cs[k] for cs in cases]))          # noqa: E731
    indices = MM._segments_of(torch.tensor(np.stack([cs["offsets"] for cs in cases])), 12)
    nat1, nat2 = stack("nat1"), stack("nat2")
    MM.st_cvi_site_update_torch(_likelihood(name), *[stack(k) for k in ("a", "wt", "c", "y")], indices, stack("pair_mean"),
                                stack("pair_cov"), 0.5, nat1, nat2)
    for b, cs in enumerate(cases):
        one = _torch_step(name, cs, 0.5)
        assert torch.equal(one[0], nat1[b]) and torch.equal(one[1], nat2[b])


# ---- the model's host side ----------------------------------------------------------------------------------------------------------
def _model(grad=True, **kwargs):
    rng = np.random.default_rng(12)
    z_space = rng.uniform(-1, 1, size=(3, 2))
    # (a hyper-parameter under the tape: the chain comes from the differentiable torch forms, which run on CPU tensors)
    time = mfa.Matern32(lengthscale=tt(1.1).requires_grad_(grad), variance=tt(1.0))
    model = mfa.SpatioTemporalSparseCVI(tt(z_space), tt([0.5, 1.7, 2.6, 4.0]), SK.Matern32(1.3, [0.8, 1.4]), time, mfa.Gaussian(0.7),
                                        **kwargs)
    return model, z_space


def test_the_projection_is_the_helpers_dense_p():
    model, z_space = _model()
    rng = np.random.default_rng(2)
    n = 17
    x, t = rng.uniform(-1, 1, size=(n, 2)), rng.uniform(0.0, 4.5, size=n)          # not sorted by time
    inputs, obs = tt(np.concatenate([x, t[:, None]], axis=1)), tt(rng.normal(size=(n, 1)))
    got = model.projection_inducing_states_to_observations((inputs, obs))
    assert tuple(got.shape) == (n, 1, 2 * model.kernel.state_dim) and got.requires_grad, "under the tape: differentiable"
    got = got.detach()
    _, wt, _ = SC.conditional_projections([dict(order=3, ls=1.1, var=1.0, period=None, osc=0)], t, np.array([0.5, 1.7, 2.6, 4.0]))
    ls = np.array([0.8, 1.4])
    r = lambda p, q: np.sqrt(3.0) * np.sqrt(np.sum((p[:, None, :] / ls - q[None, :, :] / ls) ** 2, axis=-1))          # noqa: E731
    k32 = lambda p, q: 1.3 * (1.0 + r(p, q)) * np.exp(-r(p, q))          # noqa: E731
    a = np.linalg.solve(np.linalg.cholesky(k32(z_space, z_space) + 1e-6 * np.eye(3)), k32(z_space, x)).T
    np.testing.assert_allclose(got.numpy(), STC.dense_projection(a, wt), rtol=1e-9, atol=1e-11)


def test_constructor_function_and_data_error_paths():
    model, _ = _model(learning_rate=0.5, num_data=40)
    assert model.learning_rate == 0.5 and model.num_data == 40
    assert tuple(model.nat1.shape) == (5, 12) and tuple(model.nat2.shape) == (5, 12, 12) and float(model.nat2.abs().max()) == 0.0
    assert model.inducing_time is model.inducing_inputs and tuple(model.inducing_space.shape) == (3, 2)
    assert "SpatioTemporalSparseCVI" in mfa.__all__
    z, space, time = tt(np.zeros((3, 2)) + np.arange(3)[:, None]), SK.Matern32(), mfa.Matern32(tt(1.0), tt(1.0))
    with pytest.raises(ValueError, match="learning_rate"):
        mfa.SpatioTemporalSparseCVI(z, tt([0.0, 1.0]), space, time, mfa.Gaussian(), learning_rate=1.5)
    with pytest.raises(ValueError, match="num_data"):
        mfa.SpatioTemporalSparseCVI(z, tt([0.0, 1.0]), space, time, mfa.Gaussian(), num_data=0)
    with pytest.raises(ValueError, match="at least two"):
        mfa.SpatioTemporalSparseCVI(z, tt([0.0]), space, time, mfa.Gaussian())
    with pytest.raises(ValueError, match="sorted"):
        mfa.SpatioTemporalSparseCVI(z, tt([1.0, 0.0]), space, time, mfa.Gaussian())
    with pytest.raises(TypeError):
        mfa.SpatioTemporalSparseCVI(z, tt([0.0, 1.0]), space, time, "gaussian")
    with pytest.raises(NotImplementedError, match="exceeds 64"):
        mfa.SpatioTemporalSparseCVI(tt(np.zeros((33, 2))), tt([0.0, 1.0]), space, time, mfa.Gaussian())
    inputs, obs = tt(np.zeros((6, 3))), tt(np.zeros((6, 1)))
    for call in (model.update_sites, model.elbo, model.projection_inducing_states_to_observations):
        with pytest.raises(ValueError, match="time in the last column"):
            call((inputs[..., :2], obs))
        with pytest.raises(ValueError, match="batch shape"):
            call((inputs[None], obs[None]))
        with pytest.raises(ValueError, match="observations"):
            call((inputs, obs[..., 0]))
    case = _case(0, 3, 2, L.GAUSSIAN)
    a, wt, c, y, pm, pc, nat1, nat2 = (tt(case[k]) for k in ("a", "wt", "c", "y", "pair_mean", "pair_cov", "nat1", "nat2"))
    offsets = torch.tensor(case["offsets"])
    indices = MM._segments_of(offsets, a.shape[0])
    lik = mfa.Gaussian(1.0)
    before = nat1.clone(), nat2.clone()
    with pytest.raises(TypeError):
        MM.st_cvi_site_update_torch("gaussian", a, wt, c, y, indices, pm, pc, 0.5, nat1, nat2)
    with pytest.raises(ValueError, match="nat2"):
        MM.st_cvi_site_update_torch(lik, a, wt, c, y, indices, pm, pc, 0.5, nat1, nat2[:, :-1])
    with pytest.raises(ValueError, match="nat1"):
        MM.st_cvi_site_update_hip(lik, a, wt, c, y, offsets, pm, pc, 0.5, None, nat2)
    with pytest.raises(ValueError, match="learning_rate"):
        MM.st_cvi_site_update_torch(lik, a, wt, c, y, indices, pm, pc, -0.1, nat1, nat2)
    with pytest.raises(ValueError, match="learning_rate"):
        MM.st_cvi_site_update_hip(lik, a, wt, c, y, offsets, pm, pc, float("nan"), nat1, nat2)
    with pytest.raises(ValueError, match="contiguous"):
        MM.st_cvi_site_update_hip(lik, a, wt, c, y, offsets, pm, pc, 0.5, nat1, nat2.transpose(-1, -2))
    with pytest.raises(ValueError):
        MM.st_cvi_site_update_torch(lik, a, wt, c, y, indices, pm, pc, 0.5, nat1.float(), nat2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MM.st_cvi_site_update_hip(lik, a, wt, c, y, offsets, pm, pc, 0.5, nat1, nat2)
    assert torch.equal(nat1, before[0]) and torch.equal(nat2, before[1]), "an error leaves the sites alone"


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "markovflow_amd.h")).read()
    declared = set(re.findall(r"\b(mf_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in ("mf_lik_st_cvi_site_update_f64", "mf_lik_st_cvi_site_update_f32", "mf_lik_st_cvi_site_update_workspace_bytes"):
        assert name in declared and name in _lib.exported_symbols() and getattr(lib, name) is not None


@pytest.mark.parametrize("suffix,scalar", [("_f64", ctypes.c_double), ("_f32", ctypes.c_float)])
def test_workspace_formula_and_every_argument_error_need_no_gpu(suffix, scalar):
    lib = _lib.load()
    size = lib.mf_lik_st_cvi_site_update_workspace_bytes
    for tiles, ms, two_dt, elem in ((1, 1, 2, 8), (7, 5, 6, 4), (3, 32, 4, 8), (11, 64, 2, 4), (2, 21, 6, 8)):
        n = ms * two_dt
        assert int(size(tiles, ms, two_dt, elem)) == tiles * (n * (n + 1) // 2 + n + 1) * elem
        assert int(size(tiles, ms, two_dt, elem)) == int(lib.mf_lik_st_expectations_workspace_bytes(tiles, ms, two_dt, elem))
    assert all(int(size(*args)) == 0 for args in ((0, 3, 2, 8), (-1, 3, 2, 8), (2, 0, 2, 8), (2, 3, 3, 8), (2, 33, 4, 8), (2, 3, 2, 2)))
    fn = getattr(lib, "mf_lik_st_cvi_site_update" + suffix)
    x, w = np.polynomial.hermite.hermgauss(20)
    nodes, weights = (ctypes.c_double * 20)(*x), (ctypes.c_double * 20)(*w)
    params = (ctypes.c_double * 1)(0.5)
    p = ctypes.c_void_p(64)                        # never dereferenced: every call below stops at an argument check
    good = [2, 5, 3, 3, 2, 0, params, 20, nodes, weights, p, p, p, p, p, p, p, 2, p, p, p, 1 << 20, 0.5, p, p, p, p, p, None]
    bad = [(1, -1, -1), (2, -1, -2), (3, 0, -3), (4, 0, -100), (4, 65, -100), (5, 3, -100), (5, 0, -100), (6, 4, -6), (6, -1, -6),
           (7, None, -7), (8, 0, -8), (8, 33, -8), (9, None, -9), (10, None, -10), (11, None, -11), (12, None, -12), (13, None, -13),
           (14, None, -14), (15, None, -15), (16, None, -16), (17, None, -17), (18, -1, -18), (18, 1 << 31, -18), (19, None, -19),
           (20, None, -20), (21, None, -21), (22, 8, -22), (23, -0.1, -23), (23, 1.5, -23), (23, float("nan"), -23), (24, None, -24),
           (25, None, -25)]
    for position, value, code in bad:
        args = list(good)
        args[position - 1] = value
        assert fn(*args) == code, f"argument {position} = {value!r}"
    args = list(good)
    args[3], args[4] = 33, 4                       # Ms d_t = 66
    assert fn(*args) == -100
    args = list(good)
    args[1], args[17] = 0, 1                       # tiles without points
    assert fn(*args) == -18
    none = list(good)
    none[0] = 0
    assert fn(*none) == 0, "B = 0: nothing is launched"
    none[23] = None
    assert fn(*none) == -24, "the sites are required also where nothing would be launched"
