"""
GPU tests of ``SpatioTemporalSparseCVI`` (markovflow_amd/models.py): the reference's own model test against exact dense GP regression
with the product kernel and against ``SpatioTemporalSparseVariational`` at its optimum, the fused site update
(``mf_lik_st_cvi_site_update_*``) against the torch composition on the same model, and the model's bookkeeping.

Fused against composed: ``nat1`` and ``nat2`` after one ``update_sites`` on each route, from the same sites and therefore the same
pair marginals, are held to the bounds of tests/test_gpu_st.py's ``assert_close``, whose reasoning is, for float64: "both routes
evaluate the same formulas on the same pair marginals and differ in the order of their sums - N <= 130 points per series, pair
dimension <= 128 [...] A sum of n terms carries at most n eps of its magnitude [...]: rtol 1e-7 with an atol of 1e-9 of the largest
entry"; and for float32, where state dimension 64 runs (the chain operators carry 64 in float32 and 32 in float64): "The adjoints
``g_mean`` / ``g_cov`` of the two routes lie within 75 eps32 of their magnitude of the exact ones for the composition (the largest
float32 yardstick at 20 nodes in tests/golden/st_yardsticks.json) and within 4 x that for the kernel [...], so they differ by at most
5 x 75 eps32 = 4.5e-5 of it [...]: 5e-5 of the largest entry [...], with rtol 1e-4, and no further allowance."  The new sites are
those sums blended with the old sites, which are the same bits on both routes.
"""
import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from markovflow_amd import models as MM
from markovflow_amd import spatial_kernels as SK
from helpers import likelihood_closed_forms as L
import test_gpu_st as G

pytestmark = pytest.mark.gpu
DEV = G.DEV
NAMES = G.NAMES
FN = "mf_lik_st_cvi_site_update"
tt, nn = G.tt, G.nn


# ---- the reference's model test -----------------------------------------------------------------------------------------------------
def test_the_references_model_test_ten_unit_steps_reach_dense_gp_regression():
    inputs, obs = G.reference_data()
    z_space, z_time = np.unique(inputs[:, 0]).reshape(-1, 1), np.unique(inputs[:, 1])
    model = mfa.SpatioTemporalSparseCVI(tt(z_space), tt(z_time), SK.Matern32(1.0, 1.0, device=DEV), mfa.Matern12(1.0, 1.0, device=DEV),
                                        mfa.Gaussian(1.0), learning_rate=1.0)
    assert model.kernel.state_dim == 2 and tuple(model.nat1.shape) == (3, 4) and tuple(model.nat2.shape) == (3, 4, 4)
    xy = (tt(inputs), tt(obs))
    for _ in range(10):
        model.update_sites(xy)
    variational = G.reference_model(z_space, z_time)
    opt = mfa.SSMNaturalGradient(gamma=1.0, momentum=False)          # a unit step reaches the optimum of a Gaussian likelihood
    for _ in range(2):
        opt.minimize(lambda: variational.loss(xy), variational.dist_q)
    lml, mean = G.dense_product_gpr(inputs, obs, inputs)
    elbo, elbo_variational = float(model.elbo(xy).detach()), float(variational.elbo(xy).detach())
    print(f"ELBO sites {elbo:.12f}  ELBO variational {elbo_variational:.12f}  log marginal likelihood {lml:.12f}")
    st_mean, st_var = model.space_time_predict_f(xy[0])
    assert tuple(st_mean.shape) == tuple(st_var.shape) == (4, 1)
    print(f"mean against the dense GP: {float(np.abs(nn(st_mean)[:, 0] - mean).max()):.3e}")
    assert np.allclose(elbo, lml, atol=1e-4, rtol=1e-4)
    assert np.allclose(nn(st_mean)[:, 0], mean, atol=1e-4, rtol=1e-4)
    var_mean, _ = variational.space_time_predict_f(xy[0])
    print(f"mean against the variational model: {float((st_mean - var_mean).abs().max()):.3e}")
    assert np.allclose(elbo, elbo_variational, atol=1e-6, rtol=1e-6)
    assert np.allclose(nn(st_mean), nn(var_mean), atol=1e-6, rtol=1e-6)


# ---- fused against composed --------------------------------------------------------------------------------------------------------
def draw_model(name, ms, time_cls, n, batch=2, seed=0, num_data=None, space_grad=False, time_grad=False, dtype=torch.float64,
               learning_rate=0.3, steps=1):
    """A batch of series on ``Ms`` inducing locations in the plane and 4 inducing times (the data of tests/test_gpu_st.py's
    ``draw_model``), after ``steps`` site updates: a ``q`` that is not the prior."""
    rng = np.random.default_rng(seed + 17 * ms + n)
    z_space = rng.uniform(-1.0, 1.0, size=(ms, 2))
    z_time = np.tile(np.array([0.5, 1.7, 2.6, 4.0]), (batch, 1)) + rng.uniform(0, 0.2, size=(batch, 4))
    inputs = np.concatenate([rng.uniform(-1.0, 1.0, size=(batch, n, 2)), np.sort(rng.uniform(0.0, 4.5, size=(batch, n, 1)), axis=1)],
                            axis=-1)
    obs = np.resize(np.asarray(L.OBSERVED[name]), (batch, n, 1))
    space = SK.Matern32(tt(1.3, dtype).requires_grad_(space_grad), tt([0.8, 1.4], dtype).requires_grad_(space_grad))
    time = time_cls(tt(1.1, dtype).requires_grad_(time_grad), tt(1.0, dtype))
    model = mfa.SpatioTemporalSparseCVI(tt(z_space, dtype), tt(z_time, dtype), space, time, G.build_likelihood(name), num_data=num_data,
                                        learning_rate=learning_rate)
    xy = (tt(inputs, dtype), tt(obs, dtype))
    for _ in range(steps):
        model.update_sites(xy)
    return model, xy


def sites_of(model):
    return model.nat1.clone(), model.nat2.clone()


def restore(model, sites):
    with torch.no_grad():
        model.nat1.copy_(sites[0])
        model.nat2.copy_(sites[1])


@pytest.mark.parametrize("ms,time_cls", G.SIZES, ids=["3x1", "4x2", "16x2", "32x2"])
@pytest.mark.parametrize("name", NAMES)
def test_fused_update_sites_against_the_torch_composition(name, ms, time_cls, monkeypatch):
    n = 33 if name in (L.GAUSSIAN, L.POISSON) else 130          # (every size meets both lengths, a batch of two each)
    dtype = torch.float32 if ms * time_cls(1.0, 1.0).state_dim > 32 else torch.float64          # (state dimension 64: float32)
    model, xy = draw_model(name, ms, time_cls, n, dtype=dtype)
    start = sites_of(model)
    assert float(start[1].abs().max()) > 0, "one step has been taken: dist_q is not the prior"
    model.update_sites(xy)
    fused = sites_of(model)
    restore(model, start)
    monkeypatch.setattr(model, "_fused", lambda inputs: False)
    model.update_sites(xy)
    composed = sites_of(model)
    assert not torch.equal(fused[0], start[0])
    G.assert_close(fused[0], composed[0], "nat1")
    G.assert_close(fused[1], composed[1], "nat2")


# ---- bookkeeping -------------------------------------------------------------------------------------------------------------------
def test_shuffled_data_has_the_bits_of_sorted_data():
    model, (inputs, obs) = draw_model(L.BERNOULLI, 4, mfa.Matern32, 33)
    start = sites_of(model)
    model.update_sites((inputs, obs))
    sorted_sites = sites_of(model)
    perm = torch.stack([torch.randperm(33, generator=torch.Generator().manual_seed(b)) for b in range(2)]).to(DEV)
    shuffled = (torch.gather(inputs, 1, perm[..., None].expand(inputs.shape)).contiguous(), torch.gather(obs, 1, perm[..., None]).contiguous())
    restore(model, start)
    model.update_sites(shuffled)
    assert torch.equal(model.nat1, sorted_sites[0]) and torch.equal(model.nat2, sorted_sites[1])
    assert torch.equal(model.elbo(shuffled), model.elbo((inputs, obs)))
    proj = model.projection_inducing_states_to_observations((inputs, obs))
    proj_s = model.projection_inducing_states_to_observations(shuffled)
    assert tuple(proj.shape) == (2, 33, 1, 16)
    assert torch.equal(torch.gather(proj, 1, perm[..., None, None].expand(proj.shape)), proj_s), "the projection keeps the data's order"


def test_update_sites_is_one_call_and_the_version_counters_advance(monkeypatch):
    model, xy = draw_model(L.BERNOULLI, 4, mfa.Matern32, 33)
    seen = []
    real_rc = _lib.call_rc
    monkeypatch.setattr(_lib, "call_rc", lambda base, *a: (seen.append(base), real_rc(base, *a))[1])

    def no_torch(*a, **k):
        raise AssertionError("the torch route must not run on HIP tensors")

    monkeypatch.setattr(MM.spatio_temporal, "st_cvi_site_update_torch", no_torch)
    versions = model.nat1._version, model.nat2._version
    model.update_sites(xy)
    assert [s for s in seen if s.startswith("mf_lik_")] == [FN], "ONE call of the new entry point, none of mf_lik_st_expectations_*"
    assert model.nat1._version > versions[0] and model.nat2._version > versions[1]


def test_the_elbo_rises_over_three_steps():
    model, xy = draw_model(L.BERNOULLI, 4, mfa.Matern32, 130, learning_rate=0.5, steps=0)
    values = [float(model.elbo(xy))]
    for _ in range(3):
        model.update_sites(xy)
        values.append(float(model.elbo(xy)))
    print("ELBO over the steps:", values)
    assert all(b > a for a, b in zip(values, values[1:]))


def test_num_data_scales_the_data_term_and_leaves_update_sites_alone():
    model, xy = draw_model(L.BERNOULLI, 4, mfa.Matern32, 33)
    scaled, _ = draw_model(L.BERNOULLI, 4, mfa.Matern32, 33, num_data=330)
    assert torch.equal(scaled.nat1, model.nat1) and torch.equal(scaled.nat2, model.nat2), "num_data does not enter the update"
    with torch.no_grad():
        kl = torch.sum(model.dist_q.kl_divergence(model.dist_p))
        ve = model.elbo(xy) + kl
        np.testing.assert_allclose(float(scaled.elbo(xy)), float(10.0 * ve - kl), rtol=1e-12)
        np.testing.assert_allclose(float(model.loss(xy)), -float(model.elbo(xy)), rtol=0)


@pytest.mark.parametrize("name", [L.BERNOULLI, L.GAUSSIAN])
def test_hyper_parameter_gradients_with_the_sites_held_fixed(name, monkeypatch):
    model, xy = draw_model(name, 4, mfa.Matern32, 130, space_grad=True, time_grad=True)
    space, time = model.kernel.kernel_space, model.kernel.kernel_time
    hyper = (space.variance, space.lengthscales, time._leaves()[0])
    assert all(h.requires_grad for h in hyper)
    seen = []
    real_rc = _lib.call_rc
    monkeypatch.setattr(_lib, "call_rc", lambda base, *a: (seen.append(base), real_rc(base, *a))[1])
    fused = model.loss(xy)
    assert seen.count("mf_lik_st_expectations") == 1, "a hyper-parameter under the tape stays on the fused data term"
    fused.backward()
    g_fused = [h.grad.clone() for h in hyper]
    for h in hyper:
        h.grad = None
    monkeypatch.setattr(model, "_fused", lambda inputs: False)
    composed = model.loss(xy)
    composed.backward()
    G.assert_close(fused.detach(), composed.detach(), "loss")
    for what, a, h in zip(("spatial variance", "spatial lengthscales", "temporal lengthscale"), g_fused, hyper):
        assert float(h.grad.abs().max()) > 0
        G.assert_close(a, h.grad, what)


def test_limits_routing_and_errors():
    model, (inputs, obs) = draw_model(L.GAUSSIAN, 3, mfa.Matern12, 33)
    assert model.inducing_time is model.inducing_inputs and tuple(model.inducing_space.shape) == (3, 2)
    assert isinstance(model.kernel, mfa.SparseSpatioTemporalKernel) and isinstance(model.posterior, mfa.ConditionalProcess)
    assert model.dist_p.state_dim == model.dist_q.state_dim == 3 and model.learning_rate == 0.3
    fmu, fvar = model.space_time_predict_f(inputs)
    value, (g1, g2) = model.local_objective_and_gradients(fmu, fvar, obs)
    assert tuple(g1.shape) == tuple(g2.shape) == tuple(fmu.shape) and value.dim() == 0
    np.testing.assert_allclose(float(value), float(torch.sum(model.local_objective(fmu, fvar, obs))), rtol=1e-12)
    density = model.predict_log_density((inputs, obs))
    assert tuple(density.shape) == (2, 33) and bool(torch.isfinite(density).all())
    for call in (model.update_sites, model.elbo):
        with pytest.raises(ValueError, match="time in the last column"):
            call((inputs[..., :2], obs))
        with pytest.raises(ValueError, match="batch shape"):
            call((inputs[0], obs[0]))
        with pytest.raises(ValueError, match="observations"):
            call((inputs, obs[..., 0]))
        with pytest.raises(ValueError):
            call((inputs.float(), obs.float()))
    with pytest.raises(NotImplementedError):
        model.predict_log_density((inputs, obs), full_output_cov=True)
    with pytest.raises(ValueError, match="num_data"):
        draw_model(L.GAUSSIAN, 3, mfa.Matern12, 33, num_data=0)
    with pytest.raises(ValueError, match="learning_rate"):
        draw_model(L.GAUSSIAN, 3, mfa.Matern12, 33, learning_rate=1.5)
    space, time = SK.Matern32(device=DEV), mfa.Matern32(1.0, 1.0, device=DEV)
    with pytest.raises(ValueError, match="at least two"):
        mfa.SpatioTemporalSparseCVI(tt(np.zeros((3, 2))), tt([0.0]), space, time, mfa.Gaussian())
    with pytest.raises(ValueError, match="sorted"):
        mfa.SpatioTemporalSparseCVI(tt(np.zeros((3, 2))), tt([1.0, 0.0]), space, time, mfa.Gaussian())
    with pytest.raises(NotImplementedError, match="exceeds 64"):
        mfa.SpatioTemporalSparseCVI(tt(np.zeros((33, 2))), tt([0.0, 1.0]), space, time, mfa.Gaussian())
    wide, wide_xy = draw_model(L.GAUSSIAN, 32, mfa.Matern32, 33, steps=0)
    for call in (wide.update_sites, wide.elbo):
        with pytest.raises(NotImplementedError, match="up to 32 in float64"):
            call(wide_xy)
    assert float(wide.nat2.abs().max()) == 0.0
