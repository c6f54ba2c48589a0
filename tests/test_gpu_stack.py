"""
GPU tests of ``SparseVariationalGaussianProcess`` on an ``IndependentMultiOutputStack`` (markovflow_amd/kernels.py,
markovflow_amd/models/sparse.py, segmented_ops.py; the workflow of the reference's docs/notebooks/stacked_kernels.py) against the
dense references of tests/helpers/stack_closed_forms.py and against separate single-output models.

State space against dense: rtol 1e-6 / atol 1e-7, the ``TOL`` of tests/test_gpu_multistage.py, unless a test says otherwise.  Float64
unless said.  Data and inducing points are well separated (one per cell of an even grid), for the reason
tests/test_gpu_sparse_cvi.py gives for its Matern-5/2 cases.
"""
import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from markovflow_amd import models as MM
from helpers import stack_closed_forms as ST

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = dict(rtol=1e-6, atol=1e-7)
SPAN = 10.0
FN = "mf_lik_stack_expectations"


def _comp(order, ls, var):
    return dict(order=order, ls=ls, var=var, period=None, osc=0)


MIXED3 = [_comp(1, 1.5, 0.9), _comp(3, 1.2, 1.1), _comp(5, 1.6, 0.8)]          # d = 3 with padding, 2d = 6
M32X3 = [_comp(3, 1.0, 1.0), _comp(3, 2.0, 0.7), _comp(3, 0.8, 1.3)]           # equal order
HET2 = [_comp(3, 1.2, 1.0), _comp(1, 2.0, 0.6)]                                # the mean on Matern-3/2, the log-variance on Matern-1/2
WIDE2 = [[_comp(5, 1.4, 0.5), _comp(5, 2.0, 0.3), _comp(5, 0.9, 0.2), _comp(3, 1.1, 0.2)], _comp(1, 2.0, 0.6)]      # d = 11: 2d = 22


def tt(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def nn(t):
    return t.detach().cpu().numpy()


def child(comp, dtype=torch.float64, ls=None):
    if isinstance(comp, list):
        return mfa.Sum([child(c, dtype) for c in comp])
    cls = {1: mfa.Matern12, 3: mfa.Matern32, 5: mfa.Matern52}[comp["order"]]
    return cls(comp["ls"] if ls is None else ls, comp["var"], device=DEV, dtype=dtype)


def stack_kernel(comps, dtype=torch.float64, first_ls=None, jitter=0.0):
    return mfa.IndependentMultiOutputStack([child(c, dtype, first_ls if i == 0 else None) for i, c in enumerate(comps)], jitter=jitter)


def likelihood(lik_id):
    return mfa.MultiStageLikelihood() if lik_id == ST.MULTISTAGE else mfa.HeteroscedasticGaussian()


_DATA = {}


def draw(lik_id, n, m, seed, lead=1):
    """``(x [lead, n], y [lead, n], z [lead, m])``, read-only: one time per cell of an even grid on [0, SPAN], the inducing points
    likewise; ``y`` drawn from smooth latents."""
    key = (lik_id, n, m, seed, lead)
    if key not in _DATA:
        rng = np.random.default_rng(seed)
        x = (np.arange(n) + 0.5 + rng.uniform(-0.3, 0.3, size=(lead, n))) * SPAN / n
        z = (np.arange(m) + 0.5 + rng.uniform(-0.2, 0.2, size=(lead, m))) * SPAN / m
        if lik_id == ST.HETERO:
            y = 0.8 * np.sin(0.9 * x) + np.exp(0.5 * (-1.0 + 0.5 * np.cos(0.6 * x))) * rng.normal(size=(lead, n))
        else:
            f = np.stack([0.8 * np.sin(0.9 * x) - 0.2, np.cos(0.6 * x), 0.9 + 0.6 * np.sin(0.4 * x + 1.0)], axis=-1)
            y = mfa.MultiStageLikelihood().sample_y(torch.tensor(f), generator=torch.Generator().manual_seed(seed))[..., 0].numpy()
            assert {0.0, 1.0} <= set(y.reshape(-1).tolist()) and y.max() >= 2.0, "every branch of the likelihood is met"
        for a in (x, y, z):
            a.setflags(write=False)
        _DATA[key] = (x, y, z)
    return _DATA[key]


def chains(a, k):
    """``[lead, n] -> [lead, k, n]``: the same times on every chain."""
    return np.repeat(np.asarray(a)[:, None, :], k, axis=1)


def build(lik_id, comps, z, dtype=torch.float64, **kwargs):
    """The stacked model with inducing points ``z [lead, K, M]``."""
    return mfa.SparseVariationalGaussianProcess(stack_kernel(comps, dtype), likelihood(lik_id), tt(z, dtype), **kwargs)


def data(x, y, k, dtype=torch.float64):
    return tt(chains(x, k), dtype), tt(y, dtype)[..., None]


def perturb(model, seed=3, scale=0.05):
    """Move ``dist_q`` away from the prior, padded dimensions included; the Cholesky leaves stay lower triangular."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for i, leaf in enumerate(model.trainable_variables):             # (mu0, chol_P0, As, offsets, chol_Qs)
            noise = scale * torch.randn(leaf.shape, generator=gen, dtype=torch.float64).to(leaf)
            leaf.add_(torch.tril(noise) if i in (1, 4) else noise)


def q_of(model, b, k):
    q = model.dist_q
    return tuple(nn(t)[b, k] for t in (q.initial_mean, q.cholesky_initial_covariance, q.state_transitions, q.state_offsets,
                                       q.cholesky_process_covariances))


def dense_elbo(lik_id, comps, x, y, z, model, scale=1.0):
    """The dense statement summed over the lead batch: ``x``, ``z`` ``[lead, K, .]``, ``y [lead, n]``."""
    k = len(comps)
    return sum(ST.dense_stack_elbo(lik_id, comps, x[b], y[b], z[b], [q_of(model, b, i) for i in range(k)], scale=scale)
               for b in range(x.shape[0]))


def natgrad_steps(model, xy, steps, gamma):
    opt = mfa.SSMNaturalGradient(gamma=gamma, momentum=False)
    for _ in range(steps):
        opt.minimize(lambda: model.loss(xy), model.dist_q)


def spy(monkeypatch):
    seen = []
    real_rc = _lib.call_rc
    monkeypatch.setattr(_lib, "call_rc", lambda base, *a: (seen.append(base), real_rc(base, *a))[1])
    return seen


# ---- the chain ----------------------------------------------------------------------------------------------------------------------
def test_chain_with_padding_has_the_childs_values_in_the_leading_block_and_a_zero_kl_to_itself():
    jitter = 1e-4
    kids = [mfa.Matern12(1.5, 0.9, jitter=jitter, device=DEV), mfa.Matern32(1.2, 1.1, jitter=jitter, device=DEV)]
    kern = mfa.IndependentMultiOutputStack(kids, jitter=jitter)
    assert kern.state_dim == 2
    t = tt(chains(draw(ST.HETERO, 20, 7, 1)[2], 2))[0]                   # [2, 7]
    ssm = kern.state_space_model(t)
    assert tuple(ssm.batch_shape) == (2,) and ssm.state_dim == 2
    own = kids[0].state_space_model(t[0])
    a, cq, cp0 = nn(ssm.state_transitions), nn(ssm.cholesky_process_covariances), nn(ssm.cholesky_initial_covariance)
    np.testing.assert_array_equal(a[0, :, :1, :1], nn(own.state_transitions))
    np.testing.assert_array_equal(cq[0, :, :1, :1], nn(own.cholesky_process_covariances))
    np.testing.assert_array_equal(cp0[0, :1, :1], nn(own.cholesky_initial_covariance))
    assert not a[0, :, 1, :].any() and not a[0, :, :, 1].any(), "A is padded with zeros"
    np.testing.assert_allclose(cq[0, :, 1, 1], np.sqrt(1.0 + jitter), rtol=1e-15)
    assert not cq[0, :, 1, 0].any() and not cq[0, :, 0, 1].any()
    np.testing.assert_allclose(nn(kern.initial_covariance(t[:, :1]))[0], np.diag([0.9 + jitter, 1.0 + jitter]), rtol=1e-15)
    np.testing.assert_allclose(cp0[0], np.diag(np.sqrt([0.9 + jitter, 1.0 + jitter])), rtol=1e-15)
    second = kids[1].state_space_model(t[1])
    np.testing.assert_array_equal(a[1], nn(second.state_transitions))
    np.testing.assert_array_equal(cq[1], nn(second.cholesky_process_covariances))
    np.testing.assert_allclose(nn(ssm.kl_divergence(kern.state_space_model(t))), 0.0, atol=1e-9)
    with pytest.raises(ValueError, match=r"\(\.\.\., 2\), got \(\)"):
        kern.state_space_model(t[0])


# ---- one series per output ----------------------------------------------------------------------------------------------------------
def test_per_output_route_equals_two_separate_single_output_models(monkeypatch):
    n, m = 100, 8
    rng = np.random.default_rng(4)
    x = (np.arange(n) + 0.5 + rng.uniform(-0.3, 0.3, size=n)) * SPAN / n
    z = np.stack([(np.arange(m) + 0.5 + rng.uniform(-0.2, 0.2, size=m)) * SPAN / m for _ in range(2)])      # per-output inducing points
    y = np.stack([np.sin(x) + 0.3 * rng.normal(size=n), np.cos(0.7 * x) + 0.3 * rng.normal(size=n)], axis=-1)
    comps = [_comp(1, 1.5, 0.9), _comp(3, 1.2, 1.1)]
    lik = mfa.Gaussian(0.09)
    stacked = mfa.SparseVariationalGaussianProcess(stack_kernel(comps), lik, tt(z))
    xy = (tt(np.stack([x, x])), tt(y))
    singles = [mfa.SparseVariationalGaussianProcess(child(c), lik, tt(z[i])) for i, c in enumerate(comps)]       # Matern-1/2 unpadded
    single_xy = [(tt(x), tt(y[:, i:i + 1])) for i in range(2)]
    seen = spy(monkeypatch)
    opt = mfa.SSMNaturalGradient(gamma=0.5, momentum=False)
    opts = [mfa.SSMNaturalGradient(gamma=0.5, momentum=False) for _ in singles]
    for step in range(4):
        with torch.no_grad():
            total = sum(float(s.elbo(d)) for s, d in zip(singles, single_xy))
            np.testing.assert_allclose(float(stacked.elbo(xy)), total, err_msg=f"after {step} steps", **TOL)
        opt.minimize(lambda: stacked.loss(xy), stacked.dist_q)
        for o, s, d in zip(opts, singles, single_xy):
            o.minimize(lambda: s.loss(d), s.dist_q)
    assert "mf_lik_sparse_expectations" in seen and FN not in seen, "K decoupled chains: the single-latent kernel on the batch of chains"
    t_new = np.sort(rng.uniform(-0.5, SPAN + 0.5, size=9))
    f_mean, f_var = stacked.predict_f(tt(np.stack([t_new, t_new])))
    assert tuple(f_mean.shape) == (9, 2) and tuple(f_var.shape) == (9, 2)
    for i, s in enumerate(singles):
        mean, var = s.predict_f(tt(t_new))
        np.testing.assert_allclose(nn(f_mean[:, i]), nn(mean[:, 0]), **TOL)
        np.testing.assert_allclose(nn(f_var[:, i]), nn(var[:, 0]), **TOL)
    with pytest.raises(NotImplementedError):
        stacked.predict_log_density(xy)
    with pytest.raises(ValueError, match="observations must have shape"):
        stacked.elbo((xy[0], xy[1][:, :1]))


# ---- the coupled route --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lik_id,comps", [(ST.MULTISTAGE, MIXED3), (ST.HETERO, HET2)], ids=["multistage", "heteroscedastic"])
def test_fused_elbo_and_gradients_against_the_torch_composition_and_the_dense_statement(lik_id, comps, monkeypatch):
    k = len(comps)
    x, y, z = draw(lik_id, 150, 6, 2, lead=2)
    model = build(lik_id, comps, chains(z, k))
    perturb(model)
    xy = data(x, y, k)
    leaves = model.trainable_variables
    seen = spy(monkeypatch)
    fused = model.elbo(xy)
    assert seen.count(FN) == 1 and not any(s.startswith("mf_lik_") and s != FN for s in seen)
    del seen[:]
    g_fused = torch.autograd.grad(fused, leaves)
    assert not any(s.startswith("mf_lik_") for s in seen), "the backward reuses the forward's adjoints: no second launch"
    monkeypatch.setattr(MM.sparse, "sparse_stack_instantiated", lambda *a: False)
    composed = model.elbo(xy)
    assert FN not in seen
    g_composed = torch.autograd.grad(composed, leaves)
    np.testing.assert_allclose(float(fused.detach()), float(composed.detach()), **TOL)
    for a, b in zip(g_fused, g_composed):
        np.testing.assert_allclose(nn(a), nn(b), **TOL)
    want = dense_elbo(lik_id, comps, chains(x, k), y, chains(z, k), model)
    np.testing.assert_allclose(float(fused.detach()), want, **TOL)
    np.testing.assert_allclose(float(composed.detach()), want, **TOL)
    # the fused function alone: one value with and without the adjoints, differentiable once, refuses w / c under the tape
    _, w, c, _, offsets, tiles, shared = model._projections(xy[0])
    assert shared and tuple(w.shape) == (2, k, 150, 2 * model.kernel.state_dim)
    with torch.no_grad():
        pair_mean, pair_cov = model._pair_marginals()
    args = (model.likelihood, w, c, xy[1][..., 0], offsets[..., 0, :].contiguous())
    plain = MM.sparse_stack_expected_log_likelihood(*args, pair_mean, pair_cov, tiles=tiles)
    pm, pc = pair_mean.clone().requires_grad_(True), pair_cov.clone().requires_grad_(True)
    taped = MM.sparse_stack_expected_log_likelihood(*args, pm, pc)
    assert tuple(plain.shape) == (2, 7) and torch.equal(taped.detach(), plain)
    with pytest.raises(RuntimeError, match="differentiable once"):
        torch.autograd.grad(taped.sum(), (pm, pc), create_graph=True)
    with pytest.raises(NotImplementedError, match="no adjoint onto w and c"):
        MM.sparse_stack_expected_log_likelihood(model.likelihood, w.clone().requires_grad_(True), *args[2:], pm, pc)


def test_stacked_elbo_equals_the_concatenated_model_at_the_block_diagonal_q():
    x, y, z = draw(ST.MULTISTAGE, 150, 6, 2, lead=1)
    model = build(ST.MULTISTAGE, M32X3, chains(z, 3))
    perturb(model)
    q = model.dist_q
    block = lambda t: torch.block_diag(*t) if t.dim() == 3 else torch.stack([torch.block_diag(*t[:, i]) for i in range(t.shape[1])])  # noqa: E731
    cat = lambda t: torch.cat(list(t), dim=-1)                          # noqa: E731
    with torch.no_grad():
        wide = mfa.StateSpaceModel(cat(q.initial_mean[0]), block(q.cholesky_initial_covariance[0]), block(q.state_transitions[0]),
                                   cat(q.state_offsets[0]), block(q.cholesky_process_covariances[0]))
    concat = mfa.SparseVariationalGaussianProcess(mfa.IndependentMultiOutput([child(c) for c in M32X3]), mfa.MultiStageLikelihood(),
                                                  tt(z[0]), initial_distribution=wide)
    with torch.no_grad():
        np.testing.assert_allclose(float(model.elbo(data(x, y, 3))), float(concat.elbo((tt(x[0]), tt(y[0])[:, None]))), **TOL)


# ---- the fallbacks ------------------------------------------------------------------------------------------------------------------
def test_unshared_inducing_points_and_a_wide_state_take_the_torch_route_and_agree_with_the_dense_statement(monkeypatch):
    x, y, z = draw(ST.HETERO, 150, 6, 5, lead=2)
    seen = spy(monkeypatch)
    # chains with inducing points of their own
    z2 = np.stack([z, z + 0.11], axis=1)
    model = build(ST.HETERO, HET2, z2)
    perturb(model)
    xy = data(x, y, 2)
    value = model.elbo(xy)
    assert FN not in seen and not model._projections(xy[0])[6], "the chains do not share a segmentation"
    torch.autograd.grad(value, model.trainable_variables)
    np.testing.assert_allclose(float(value.detach()), dense_elbo(ST.HETERO, HET2, chains(x, 2), y, z2, model), **TOL)
    # 2d = 22 > 18
    wide = build(ST.HETERO, WIDE2, chains(z, 2))
    assert 2 * wide.kernel.state_dim == 22
    natgrad_steps(wide, xy, 1, 0.3)
    with torch.no_grad():
        value = float(wide.elbo(xy))
    assert FN not in seen
    np.testing.assert_allclose(value, dense_elbo(ST.HETERO, WIDE2, chains(x, 2), y, chains(z, 2), wide), **TOL)
    # and the same data on the fused route, for the record of the spy
    with torch.no_grad():
        build(ST.HETERO, HET2, chains(z, 2)).elbo(xy)
    assert FN in seen


def test_elbo_backward_gives_the_lengthscale_gradient_through_the_composed_route(monkeypatch):
    """d elbo / d (lengthscale of the first child) with q held fixed, against the five-point stencil with h = 1e-3 of
    tests/test_gpu_multistage.py::test_elbo_backward_gives_the_lengthscale_gradient_through_the_composed_route, whose error budget
    (|elbo| < 400 and |gradient| > 0.1, both asserted, at rtol 1e-5) is restated there; the data are shuffled, so the branch sorts
    every chain."""
    comps = M32X3
    x, y, z = draw(ST.MULTISTAGE, 100, 10, 1, lead=1)
    perm = np.random.default_rng(9).permutation(100)
    xy, shuffled = data(x, y, 3), data(x[:, perm], y[:, perm], 3)
    trained = build(ST.MULTISTAGE, comps, chains(z, 3))
    natgrad_steps(trained, xy, 3, 0.05)
    seen = spy(monkeypatch)

    def elbo_at(ls, grad=False):
        ls_t = torch.tensor(ls, dtype=torch.float64, device=DEV, requires_grad=grad)
        m = mfa.SparseVariationalGaussianProcess(stack_kernel(comps, first_ls=ls_t), mfa.MultiStageLikelihood(), tt(chains(z, 3)),
                                                 initial_distribution=trained.dist_q)
        return m.elbo(shuffled), ls_t

    ls0 = comps[0]["ls"]
    value, ls_t = elbo_at(ls0, grad=True)
    assert value.requires_grad and FN not in seen, "w and c are under the tape: the composed route"
    with torch.no_grad():
        np.testing.assert_allclose(float(trained.elbo(xy)), float(value.detach()), rtol=1e-10)      # both routes, one value
    assert FN in seen
    (g_ls,) = torch.autograd.grad(value, ls_t)
    h = 1e-3
    with torch.no_grad():
        f = {k: float(elbo_at(ls0 + k * h)[0]) for k in (-2, -1, 1, 2)}
    fd = (8.0 * (f[1] - f[-1]) - (f[2] - f[-2])) / (12.0 * h)
    print(f"GRAD lengthscale: autograd {float(g_ls):.9e}  five-point {fd:.9e}  |elbo| {abs(float(value.detach())):.3f}")
    assert abs(float(value.detach())) < 400.0 and abs(float(g_ls)) > 0.1
    np.testing.assert_allclose(float(g_ls), fd, rtol=1e-5, atol=1e-7)


# ---- training -----------------------------------------------------------------------------------------------------------------------
def test_five_natural_gradient_steps_never_decrease_the_elbo_and_match_the_dense_loop():
    x, y, z = draw(ST.HETERO, 60, 6, 1, lead=1)
    dense = ST.DenseStackNatGrad(ST.HETERO, HET2, x[0], y[0], [z[0], z[0]], gamma=0.5)
    trail = [dense.elbo()]
    for _ in range(5):
        dense.step()
        trail.append(dense.elbo())
    assert np.all(np.diff(trail) >= 0.0), "the dense block-diagonal loop is monotone on these inputs"
    model = build(ST.HETERO, HET2, chains(z, 2))
    xy = data(x, y, 2)
    opt = mfa.SSMNaturalGradient(gamma=0.5, momentum=False)
    with torch.no_grad():
        got = [float(model.elbo(xy))]
    for _ in range(5):
        opt.minimize(lambda: model.loss(xy), model.dist_q)
        with torch.no_grad():
            got.append(float(model.elbo(xy)))
    print("ELBO trail:", np.round(got, 6))
    assert np.all(np.diff(got) >= 0.0)
    np.testing.assert_allclose(got, trail, **TOL)
    t_new = np.sort(np.random.default_rng(11).uniform(-0.5, SPAN + 0.5, size=9))
    mean, var = dense.predict_f(t_new)
    f_mean, f_var = model.predict_f(tt(chains(t_new[None], 2)))
    assert tuple(f_mean.shape) == (1, 9, 2) and tuple(f_var.shape) == (1, 9, 2)
    np.testing.assert_allclose(nn(f_mean)[0], mean, **TOL)
    np.testing.assert_allclose(nn(f_var)[0], var, **TOL)


# ---- unsorted data, minibatches, float32 --------------------------------------------------------------------------------------------
def test_shuffled_data_give_the_sorted_datas_bits_and_num_data_scales_the_data_term():
    x, y, z = draw(ST.MULTISTAGE, 100, 10, 1, lead=2)
    xy = data(x, y, 3)
    plain = build(ST.MULTISTAGE, MIXED3, chains(z, 3))
    natgrad_steps(plain, xy, 2, 0.05)
    scaled = build(ST.MULTISTAGE, MIXED3, chains(z, 3), num_data=100, initial_distribution=plain.dist_q)
    perm = np.random.default_rng(5).permutation(100)
    shuffled = data(x[:, perm], y[:, perm], 3)
    with torch.no_grad():
        full = float(plain.elbo(xy))
        assert float(scaled.elbo(xy)) == full, "num_data = N on the full batch: scale 1"
        pick = np.array([4, 17, 29, 55, 56, 78, 80, 81, 93, 99])
        sub = data(x[:, pick], y[:, pick], 3)
        kl = float(torch.sum(plain.dist_q.kl_divergence(plain.dist_p)))
        np.testing.assert_allclose(float(scaled.elbo(sub)), 10.0 * (float(plain.elbo(sub)) + kl) - kl, rtol=1e-12)
        assert float(plain.elbo(shuffled)) == full, "shuffled data: the bits of the sorted data"
    g_sorted = torch.autograd.grad(plain.elbo(xy), plain.trainable_variables)
    g_shuffled = torch.autograd.grad(plain.elbo(shuffled), plain.trainable_variables)
    assert all(torch.equal(a, b) for a, b in zip(g_sorted, g_shuffled))


def test_a_float32_model_runs_and_its_elbo_agrees_with_the_float64_one():
    """The bound of tests/test_gpu_multistage.py's float32 test, restated for the stacked layout: a segment's float32 sum is within
    4 x the normalised error e32 of the helper evaluated in numpy float32 (on the float32-rounded projections and pair marginals of
    the float64 model, in the kernel's order), times (magnitude + 1); the ELBO adds S = M + 1 of them, so
    |elbo32 - elbo64| <= S x 4 x e32 x (the largest segment magnitude + 1)."""
    x, y, z = draw(ST.MULTISTAGE, 100, 10, 1, lead=1)
    model64 = build(ST.MULTISTAGE, M32X3, chains(z, 3))
    xy = data(x, y, 3)
    natgrad_steps(model64, xy, 3, 0.05)
    with torch.no_grad():
        exact = float(model64.elbo(xy))
        pair_mean, pair_cov = model64._pair_marginals()
    _, w, c, _, offsets, _, _ = model64._projections(xy[0])
    r32 = lambda t: nn(t)[0].astype(np.float32).astype(np.float64)          # noqa: E731
    args = (r32(w), r32(c), y[0], nn(offsets)[0, 0], r32(pair_mean), r32(pair_cov), ST.MULTISTAGE)
    want, low = ST.segment_expectations_stack(*args), ST.segment_expectations_stack(*args, dtype=np.float32)
    e32 = float((np.abs(low["ve_sum"].astype(np.float64) - want["ve_sum"]) / (want["mag_ve_sum"] + 1.0)).max())
    segs = z.shape[-1] + 1
    bound = segs * 4.0 * e32 * (float(want["mag_ve_sum"].max()) + 1.0)
    q64 = model64.dist_q
    q32 = mfa.StateSpaceModel(*(t.detach().to(torch.float32) for t in (q64.initial_mean, q64.cholesky_initial_covariance,
                                                                        q64.state_transitions, q64.state_offsets,
                                                                        q64.cholesky_process_covariances)))
    model32 = build(ST.MULTISTAGE, M32X3, chains(z, 3), dtype=torch.float32, initial_distribution=q32)
    elbo32 = model32.elbo(data(x, y, 3, torch.float32))
    assert elbo32.dtype == torch.float32
    torch.autograd.grad(elbo32, model32.trainable_variables)
    got = float(elbo32.detach())
    print(f"ERR f32 elbo: |elbo32 - elbo64| {abs(got - exact):.3e}  bound {bound:.3e}  (e32 {e32:.3e}, S {segs}, |elbo| {abs(exact):.3f})")
    assert abs(got - exact) <= bound
