"""
GPU tests of ``SparseVariationalGaussianProcess`` with ``MultiStageLikelihood`` on an ``IndependentMultiOutput`` kernel of three
components (markovflow_amd/models/sparse.py, segmented_ops.py; the workflow of the reference's docs/notebooks/multistage_likelihood.py)
against the dense references of tests/helpers/multistage_closed_forms.py.

State space against dense: rtol 1e-6 / atol 1e-7, the ``TOL`` of tests/test_gpu_svgp.py, unless a test says otherwise.  The kernels
carry jitter 0 and so do the dense loops.  N = 100 data points and M = 10 inducing points as in the notebook (one case has N = 40,
M = 5), the observations drawn with ``sample_y`` from three smooth latents; data and inducing points are well separated, for the
reason tests/test_gpu_sparse_cvi.py gives for its Matern-5/2 cases (Q = P - A P A^T loses digits between close points).

The model's chain operators are HIP kernels, so two checks that would otherwise need no device are here: the ELBO at ``q = prior``
against ``sum_i VE(0, [k_l(0)]_l, y_i)``, and the product's projections against the helper's.
"""
import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from markovflow_amd import likelihoods as ML
from markovflow_amd import models as MM
from helpers import multistage_closed_forms as MS
from helpers import sparse_cvi_closed_forms as SC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = dict(rtol=1e-6, atol=1e-7)
GAMMA = 0.05                    # the notebook's natural-gradient step


def _comp(order, ls, var):
    return dict(order=order, ls=ls, var=var, period=None, osc=0)


KERNELS = {"m32x3": [_comp(3, 1.0, 1.0), _comp(3, 2.0, 0.7), _comp(3, 0.8, 1.3)],              # 2d = 12
           "m12+m32+m52": [_comp(1, 1.5, 0.9), _comp(3, 1.2, 1.1), _comp(5, 1.6, 0.8)],         # 2d = 12, unequal blocks
           "m52x3": [_comp(5, 1.4, 1.0), _comp(5, 2.0, 0.7), _comp(5, 1.7, 1.2)]}               # 2d = 18
SPAN = 10.0


def tt(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def nn(t):
    return t.detach().cpu().numpy()


def build_kernel(comps, dtype=torch.float64, first_ls=None):
    cls = {1: mfa.Matern12, 3: mfa.Matern32, 5: mfa.Matern52}
    parts = [cls[c["order"]](c["ls"] if first_ls is None or i else first_ls, c["var"], device=DEV, dtype=dtype)
             for i, c in enumerate(comps)]
    return mfa.IndependentMultiOutput(parts)


def build_model(comps, z, dtype=torch.float64, **kwargs):
    return mfa.SparseVariationalGaussianProcess(build_kernel(comps, dtype), mfa.MultiStageLikelihood(), tt(z, dtype), **kwargs)


def data(x, y, dtype=torch.float64):
    return tt(x, dtype), tt(y, dtype)[..., None]


_SERIES = {}


def series(n=100, m=10, seed=1):
    """``(x [n], y [n], z [m])``, read-only: one time per cell of an even grid on [0, SPAN], the inducing points likewise (never
    closer than 0.4 of a cell), ``y`` drawn by ``sample_y`` from three smooth latents."""
    if (n, m, seed) not in _SERIES:
        rng = np.random.default_rng(seed)
        x = (np.arange(n) + 0.5 + rng.uniform(-0.3, 0.3, size=n)) * SPAN / n
        z = (np.arange(m) + 0.5 + rng.uniform(-0.2, 0.2, size=m)) * SPAN / m
        f = np.stack([0.8 * np.sin(0.9 * x) - 0.2, np.cos(0.6 * x), 0.9 + 0.6 * np.sin(0.4 * x + 1.0)], axis=-1)
        y = mfa.MultiStageLikelihood().sample_y(torch.tensor(f), generator=torch.Generator().manual_seed(seed))[:, 0].numpy()
        assert {0.0, 1.0} <= set(y.tolist()) and y.max() >= 2.0, "every branch of the likelihood is met"
        for a in (x, y, z):
            a.setflags(write=False)
        _SERIES[(n, m, seed)] = (x, y, z)
    return _SERIES[(n, m, seed)]


def natgrad_steps(model, xy, steps, gamma=GAMMA):
    opt = mfa.SSMNaturalGradient(gamma=gamma, momentum=False)
    for _ in range(steps):
        opt.minimize(lambda: model.loss(xy), model.dist_q)
    return opt


def compare_q_with_dense(model, mu, sigma, where):
    with torch.no_grad():
        means, covs = (nn(a) for a in model.dist_q.marginals)
    m, d = means.shape[-2:]
    np.testing.assert_allclose(means, mu.reshape(m, d), err_msg=f"marginal means {where}", **TOL)
    blocks = np.stack([sigma[i * d:(i + 1) * d, i * d:(i + 1) * d] for i in range(m)])
    np.testing.assert_allclose(covs, blocks, err_msg=f"marginal covariances {where}", **TOL)


# ---- projections and the prior -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(KERNELS))
def test_projections_against_the_helper_and_the_elbo_at_the_prior(key):
    comps = KERNELS[key]
    x, y, z = series()
    kernel = build_kernel(comps)
    w, c, indices, offsets = MM.sparse_multi_site_projections(kernel, tt(x), tt(z))
    idx, w_h, c_h = MS.conditional_projections_multi(comps, x, z)
    two_d = 2 * SC.state_dim(comps)
    assert tuple(w.shape) == (100, 3, two_d) and tuple(c.shape) == (100, 3)
    np.testing.assert_allclose(nn(w), w_h, **TOL)
    np.testing.assert_allclose(nn(c), c_h, **TOL)
    assert nn(indices).tolist() == idx.tolist() and nn(offsets).tolist() == SC.offsets_of(idx, 11).tolist()
    w1, c1, _, _ = MM.sparse_site_projections(kernel, tt(x), tt(z))
    assert torch.equal(w1, w[:, 0]) and torch.equal(c1, c[:, 0]), "the single-latent projection is row 0 of the emission matrix"
    model = build_model(comps, z)
    with torch.no_grad():
        elbo = float(model.elbo(data(x, y)))
        kl = float(torch.sum(model.dist_q.kl_divergence(model.dist_p)))
    k0 = np.tile(np.array([comp["var"] for comp in comps]), (100, 1))
    np.testing.assert_allclose(kl, 0.0, atol=1e-9)
    np.testing.assert_allclose(elbo, MS.expectations(np.zeros((100, 3)), k0, y)[0][0].sum(), **TOL)


# ---- fused against composed --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(KERNELS))
def test_fused_elbo_and_its_gradients_against_the_torch_composition_on_the_same_model(key, monkeypatch):
    x, y, z = series()
    xy = data(x, y)
    model = build_model(KERNELS[key], z)
    natgrad_steps(model, xy, 2)                                         # (a q that is not the prior)
    leaves = model.trainable_variables
    seen = []
    real_rc = _lib.call_rc
    monkeypatch.setattr(_lib, "call_rc", lambda base, *a: (seen.append(base), real_rc(base, *a))[1])
    fused = model.elbo(xy)
    assert seen.count("mf_lik_sparse_multi_expectations") == 1 and not any(s.startswith("mf_lik_") and s != "mf_lik_sparse_multi_expectations"
                                                                           for s in seen)
    del seen[:]
    g_fused = torch.autograd.grad(fused, leaves)
    assert not any(s.startswith("mf_lik_") for s in seen), "the backward reuses the forward's adjoints: no second launch"
    monkeypatch.setattr(model, "_fused", lambda time_points: False)
    composed = model.elbo(xy)
    assert "mf_lik_sparse_multi_expectations" not in seen and "mf_lik_multistage_variational_expectations" in seen
    g_composed = torch.autograd.grad(composed, leaves)
    np.testing.assert_allclose(float(fused.detach()), float(composed.detach()), **TOL)
    for a, b in zip(g_fused, g_composed):
        np.testing.assert_allclose(nn(a), nn(b), **TOL)
    assert float(torch.triu(g_fused[1], 1).abs().max()) == 0.0 and float(torch.triu(g_fused[4], 1).abs().max()) == 0.0


def test_the_fused_function_against_the_helper_is_differentiable_once_and_never_takes_the_torch_route(monkeypatch):
    x, y, z = series()
    model = build_model(KERNELS["m32x3"], z)
    natgrad_steps(model, data(x, y), 1)
    _, w, c, _, offsets, tiles = model._projections(tt(x))
    with torch.no_grad():
        pair_mean, pair_cov = model._pair_marginals()
    lik = model.likelihood

    def no_torch(*a, **k):
        raise AssertionError("the torch route must not run on HIP tensors")

    monkeypatch.setattr(ML, "torch_multistage_variational_expectations", no_torch)
    monkeypatch.setattr(ML, "torch_variational_expectations", no_torch)
    plain = MM.sparse_multi_expected_log_likelihood(lik, w, c, tt(y), offsets, pair_mean, pair_cov, tiles=tiles)
    assert tuple(plain.shape) == (11,) and not plain.requires_grad
    pm, pc = pair_mean.clone().requires_grad_(True), pair_cov.clone().requires_grad_(True)
    taped = MM.sparse_multi_expected_log_likelihood(lik, w, c, tt(y), offsets, pm, pc)
    assert torch.equal(taped.detach(), plain), "the value has the same bits with and without the adjoints"
    g_mean, g_cov = torch.autograd.grad(taped.sum(), (pm, pc))
    assert torch.equal(g_cov, g_cov.transpose(-1, -2))
    want = MS.segment_expectations_multi(nn(w), nn(c), y, nn(offsets), nn(pair_mean), nn(pair_cov))
    np.testing.assert_allclose(nn(plain), want["ve_sum"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(nn(g_mean), want["g_mean"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(nn(g_cov), want["g_cov"], rtol=1e-12, atol=1e-13)
    again = MM.sparse_multi_expected_log_likelihood(lik, w, c, tt(y), offsets, pm, pc)
    with pytest.raises(RuntimeError, match="differentiable once"):
        torch.autograd.grad(again.sum(), (pm, pc), create_graph=True)
    # the element-wise kernel behind ``variational_expectations`` on HIP tensors: value and the six derivatives
    fmu, fvar = tt(np.linspace(-1.0, 1.0, 21).reshape(7, 3)).requires_grad_(True), tt(np.linspace(0.2, 2.0, 21).reshape(7, 3)).requires_grad_(True)
    obs = np.asarray(MS.OBSERVED)
    ve = lik.variational_expectations(fmu, fvar, tt(obs)[:, None])
    torch.sum(ve).backward()
    (ve_h, gm_h, gv_h), _ = MS.expectations(nn(fmu), nn(fvar), obs)
    np.testing.assert_allclose(nn(ve), ve_h, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(nn(fmu.grad), gm_h, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(nn(fvar.grad), gv_h, rtol=1e-12, atol=1e-13)


# ---- natural gradient --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,n,m", [("m32x3", 40, 5), ("m32x3", 100, 10), ("m12+m32+m52", 100, 10), ("m52x3", 100, 10)])
def test_five_natural_gradient_steps_against_the_dense_loop(key, n, m):
    comps = KERNELS[key]
    x, y, z = series(n, m)
    xy = data(x, y)
    model = build_model(comps, z)
    dense = MS.DenseNatGradMulti(comps, x, y, z, gamma=GAMMA)
    opt = mfa.SSMNaturalGradient(gamma=GAMMA, momentum=False)
    with torch.no_grad():
        np.testing.assert_allclose(float(model.elbo(xy)), dense.elbo(), err_msg="at the prior", **TOL)
    for it in range(1, 6):
        opt.minimize(lambda: model.loss(xy), model.dist_q)
        dense.step()
        compare_q_with_dense(model, *dense.posterior(), f"{key} step {it}")
        with torch.no_grad():
            np.testing.assert_allclose(float(model.elbo(xy)), dense.elbo(), err_msg=f"step {it}", **TOL)


# ---- unsorted data and minibatches -------------------------------------------------------------------------------------------------
def test_num_data_scaling_and_shuffled_minibatches():
    x, y, z = series()
    xy = data(x, y)
    plain = build_model(KERNELS["m32x3"], z)
    natgrad_steps(plain, xy, 2)
    scaled = build_model(KERNELS["m32x3"], z, num_data=100, initial_distribution=plain.dist_q)          # (the same q, bit for bit)
    with torch.no_grad():
        full = float(plain.elbo(xy))
        assert float(scaled.elbo(xy)) == full, "num_data = N on the full batch: scale 1"
        pick = np.array([4, 17, 29, 55, 56, 78, 80, 81, 93, 99])
        sub = data(x[pick], y[pick])
        kl = float(torch.sum(plain.dist_q.kl_divergence(plain.dist_p)))
        np.testing.assert_allclose(float(scaled.elbo(sub)), 10.0 * (float(plain.elbo(sub)) + kl) - kl, rtol=1e-12)
        assert abs(float(scaled.elbo(sub)) - full) > 1e-3 and abs(float(plain.elbo(sub)) - full) > 1e-3
        perm = np.random.default_rng(5).permutation(100)
        assert float(plain.elbo(data(x[perm], y[perm]))) == full, "shuffled data: the bits of the sorted data"
    shuffled = data(x[perm], y[perm])
    g_sorted = torch.autograd.grad(plain.elbo(xy), plain.trainable_variables)
    g_shuffled = torch.autograd.grad(plain.elbo(shuffled), plain.trainable_variables)
    assert all(torch.equal(a, b) for a, b in zip(g_sorted, g_shuffled))


# ---- prediction --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["m32x3", "m12+m32+m52"])
def test_predict_f_has_a_column_per_latent_and_matches_the_dense_posterior(key):
    comps = KERNELS[key]
    x, y, z = series()
    xy = data(x, y)
    model = build_model(comps, z)
    dense = MS.DenseNatGradMulti(comps, x, y, z, gamma=GAMMA)
    natgrad_steps(model, xy, 5)
    for _ in range(5):
        dense.step()
    rng = np.random.default_rng(11)
    t_new = np.sort(np.concatenate([x[0] - 0.1 - rng.random(2), x[-1] + 0.1 + rng.random(2), rng.uniform(x[0], x[-1], 5)]))
    mean, var = dense.predict_f(t_new)
    f_mean, f_var = model.predict_f(tt(t_new))
    assert tuple(f_mean.shape) == (9, 3) and tuple(f_var.shape) == (9, 3)
    np.testing.assert_allclose(nn(f_mean), mean, **TOL)
    np.testing.assert_allclose(nn(f_var), var, **TOL)
    with pytest.raises(NotImplementedError, match="predictive density"):
        model.predict_log_density((tt(t_new), tt(np.zeros(9))[:, None]))


# ---- a hyper-parameter under the tape ----------------------------------------------------------------------------------------------
def test_elbo_backward_gives_the_lengthscale_gradient_through_the_composed_route(monkeypatch):
    """d elbo / d (lengthscale of the first component) with q held fixed, against central differences; the data are shuffled, so the
    branch sorts them.  The error budget follows ``test_elbo_backward_gives_the_lengthscale_gradient_through_the_composed_route`` of
    tests/test_gpu_svgp.py - well-separated points, a value good to about 1e-12 relative - restated for this ELBO: with N = 100 and up
    to three stages per point |elbo| is below 400 (asserted), four times that one's 60, so at its h = 1e-4 the rounding term
    1e-12 x 400 / 1e-4 = 4e-6 would no longer sit below rtol 1e-5 of a gradient of order 0.1.  The step is therefore h = 1e-3 with
    the five-point stencil (8 (f(h) - f(-h)) - (f(2h) - f(-2h))) / (12 h): rounding 1.5 x 1e-12 x 400 / 1e-3 = 6e-7, truncation
    h^4 / 30 x (a fifth derivative of order 1e3 at most) = 3e-11, against a gradient of at least 0.1 (asserted): rtol 1e-5."""
    comps = KERNELS["m32x3"]
    x, y, z = series()
    perm = np.random.default_rng(9).permutation(100)
    xy, shuffled = data(x, y), data(x[perm], y[perm])
    trained = build_model(comps, z)
    natgrad_steps(trained, xy, 3)
    seen = []
    real_rc = _lib.call_rc
    monkeypatch.setattr(_lib, "call_rc", lambda base, *a: (seen.append(base), real_rc(base, *a))[1])

    def elbo_at(ls, grad=False):
        ls_t = torch.tensor(ls, dtype=torch.float64, device=DEV, requires_grad=grad)
        m = mfa.SparseVariationalGaussianProcess(build_kernel(comps, first_ls=ls_t), mfa.MultiStageLikelihood(), tt(z),
                                                 initial_distribution=trained.dist_q)
        return m.elbo(shuffled), ls_t, m

    ls0 = comps[0]["ls"]
    value, ls_t, model = elbo_at(ls0, grad=True)
    assert value.requires_grad and "mf_lik_sparse_multi_expectations" not in seen, "w and c are under the tape: the composed route"
    with torch.no_grad():
        np.testing.assert_allclose(float(trained.elbo(xy)), float(value.detach()), rtol=1e-10)      # both routes, one value
    assert "mf_lik_sparse_multi_expectations" in seen
    (g_ls,) = torch.autograd.grad(value, ls_t)
    h = 1e-3
    with torch.no_grad():
        f = {k: float(elbo_at(ls0 + k * h)[0]) for k in (-2, -1, 1, 2)}
    fd = (8.0 * (f[1] - f[-1]) - (f[2] - f[-2])) / (12.0 * h)
    print(f"GRAD lengthscale: autograd {float(g_ls):.9e}  five-point {fd:.9e}  |elbo| {abs(float(value.detach())):.3f}")
    assert abs(float(value.detach())) < 400.0 and abs(float(g_ls)) > 0.1
    np.testing.assert_allclose(float(g_ls), fd, rtol=1e-5, atol=1e-7)


# ---- float32 -----------------------------------------------------------------------------------------------------------------------
def test_a_float32_model_runs_and_its_elbo_agrees_with_the_float64_one():
    """The bound of tests/test_gpu_multistage_kernel.py times the number of segments: a segment's float32 sum is within 4 x the
    normalised error e32 of the helper evaluated in numpy float32 (on the float32-rounded projections and pair marginals of the
    float64 model, in the kernel's order), times (magnitude + 1); the ELBO adds S = M + 1 of them, so
    |elbo32 - elbo64| <= S x 4 x e32 x (the largest segment magnitude + 1)."""
    comps = KERNELS["m32x3"]
    x, y, z = series()
    model64 = build_model(comps, z)
    natgrad_steps(model64, data(x, y), 3)
    with torch.no_grad():
        exact = float(model64.elbo(data(x, y)))
        pair_mean, pair_cov = model64._pair_marginals()
    _, w, c, _, offsets, _ = model64._projections(tt(x))
    r32 = lambda t: nn(t).astype(np.float32).astype(np.float64)          # noqa: E731
    args = (r32(w), r32(c), y, nn(offsets), r32(pair_mean), r32(pair_cov))
    want, low = MS.segment_expectations_multi(*args), MS.segment_expectations_multi(*args, dtype=np.float32)
    e32 = float((np.abs(low["ve_sum"].astype(np.float64) - want["ve_sum"]) / (want["mag_ve_sum"] + 1.0)).max())
    segs = len(z) + 1
    bound = segs * 4.0 * e32 * (float(want["mag_ve_sum"].max()) + 1.0)
    q64 = model64.dist_q
    q32 = mfa.StateSpaceModel(*(t.detach().to(torch.float32) for t in (q64.initial_mean, q64.cholesky_initial_covariance,
                                                                        q64.state_transitions, q64.state_offsets,
                                                                        q64.cholesky_process_covariances)))
    model32 = build_model(comps, z, dtype=torch.float32, initial_distribution=q32)
    xy32 = data(x, y, torch.float32)
    elbo32 = model32.elbo(xy32)
    assert elbo32.dtype == torch.float32
    torch.autograd.grad(elbo32, model32.trainable_variables)
    got = float(elbo32.detach())
    print(f"ERR f32 elbo: |elbo32 - elbo64| {abs(got - exact):.3e}  bound {bound:.3e}  (e32 {e32:.3e}, S {segs}, |elbo| {abs(exact):.3f})")
    assert abs(got - exact) <= bound
