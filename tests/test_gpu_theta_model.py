"""
GPU tests of ``SparseVariationalGaussianProcess`` under ``Gaussian(variance=tensor)`` (per series) and ``StudentT(scale=tensor)``
(shared): ``elbo().backward()`` on HIP tensors - ONE call of ``mf_lik_sparse_expectations_theta_*`` - against the composed torch route
on a CPU float64 copy of the projections and the likelihood (the chain under the same tape: chains are built on the device only),
within 64 eps of (magnitude + 1), a gradient's magnitude being ``sum_s |d ve_s / d leaf| + |d kl / d leaf|``.  Then ten alternating steps.
"""
import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from markovflow_amd import models as MM

pytestmark = pytest.mark.gpu
DEV, CPU = torch.device("cuda:0"), torch.device("cpu")
EPS = 2.0 ** -52
B, N, M, SPAN = 2, 150, 5, 6.0
FUSED = "mf_lik_sparse_expectations_theta"
KERNELS = dict(matern32=mfa.Matern32, matern52=mfa.Matern52)


def likelihood(name, dev):
    if name == "gaussian":                         # one variance per series
        return mfa.Gaussian(variance=torch.tensor([0.5, 1.25], dtype=torch.float64, device=dev))
    return mfa.StudentT(scale=torch.tensor(0.75, dtype=torch.float64, device=dev), df=3.0)


def series(dev, noise=0.25):
    rng = np.random.default_rng(11)
    x = rng.permuted((np.arange(N) + 0.5 + rng.uniform(-0.3, 0.3, size=(B, N))) * SPAN / N, axis=-1)       # unsorted
    z = (np.arange(M) + 0.5 + rng.uniform(-0.2, 0.2, size=(B, M))) * SPAN / M
    y = np.sin(1.7 * x)[..., None] + noise * rng.normal(size=(B, N, 1))
    return tuple(torch.tensor(a, dtype=torch.float64, device=dev) for a in (x, y, z))


@pytest.mark.parametrize("lik", ["gaussian", "student-t"])
@pytest.mark.parametrize("kernel", ["matern32", "matern52"])
def test_fused_elbo_gradients_against_the_composed_route_on_cpu_float64(kernel, lik, monkeypatch):
    x, y, z = series(DEV)
    xy = (x, y)
    model = mfa.SparseVariationalGaussianProcess(KERNELS[kernel](1.125, 0.875, device=DEV, dtype=torch.float64), likelihood(lik, DEV), z)
    opt = mfa.SSMNaturalGradient(gamma=0.1, momentum=False)
    for _ in range(2):                             # q is not the prior
        opt.minimize(lambda: model.loss(xy), model.dist_q)
    seen = []
    real_rc = _lib.call_rc
    monkeypatch.setattr(_lib, "call_rc", lambda base, *a: (seen.append(base), real_rc(base, *a))[1])
    leaves = tuple(model.trainable_variables) + model.likelihood.trainable_variables
    fused = model.elbo(xy)
    assert seen.count(FUSED) == 1 and not any(s.startswith("mf_lik_") and s != FUSED for s in seen), "the fused entry point is the one called"
    del seen[:]
    g_fused = torch.autograd.grad(fused, leaves)
    assert not any(s.startswith("mf_lik_") for s in seen), "the backward reuses the forward's adjoints: no second launch"
    assert g_fused[-1].shape == leaves[-1].shape and float(g_fused[-1].abs().min()) > 0.0

    # the reference: the composed torch route on a CPU copy, under the tape of the device chain and of a CPU copy of the likelihood
    order, w, c, indices, _, _ = model._projections(xy[0])
    pm, pc = model._pair_marginals()
    lik_cpu = likelihood(lik, CPU)
    ve = MM.sparse_expected_log_likelihood_torch(lik_cpu, w.cpu(), c.cpu(), torch.gather(y[..., 0], -1, order).cpu(), indices.cpu(),
                                                 pm.cpu(), pc.cpu())
    kl = model.dist_q.kl_divergence(model.dist_p).cpu()
    ref_leaves = tuple(model.trainable_variables) + lik_cpu.trainable_variables
    terms = [torch.autograd.grad(t, ref_leaves, retain_graph=True, allow_unused=True) for t in list(ve.reshape(-1)) + [-torch.sum(kl)]]
    terms = [[torch.zeros_like(leaf).cpu() if g is None else g.cpu() for g, leaf in zip(row, ref_leaves)] for row in terms]
    want = [float((ve.sum() - kl.sum()).detach())] + [sum(col) for col in zip(*terms)]
    mags = [float((ve.abs().sum() + kl.abs().sum()).detach())] + [sum(g.abs() for g in col) for col in zip(*terms)]
    names = ["elbo"] + [f"gradient onto leaf {i} of dist_q" for i in range(len(leaves) - 1)] + ["gradient onto the likelihood's leaf"]
    ratios = [float(((torch.as_tensor(a).detach().cpu() - b).abs() / (m + 1.0)).max() / EPS)
              for a, b, m in zip([fused] + list(g_fused), want, mags)]
    for name, ratio in zip(names, ratios):
        print(f"RATIO f64 {kernel} {lik} {name}: {ratio:.2f}")
    assert all(r <= 64.0 for r in ratios), dict(zip(names, ratios))


def test_ten_alternating_steps_raise_the_elbo_lower_the_variance_and_keep_the_projections():
    rng = np.random.default_rng(3)
    x, _, z = series(DEV)
    y = torch.sin(1.7 * x)[..., None] + torch.tensor(np.sqrt(0.05) * rng.normal(size=(B, N, 1)), device=DEV)
    lik = mfa.Gaussian(variance=torch.ones(B, dtype=torch.float64, device=DEV))
    model = mfa.SparseVariationalGaussianProcess(mfa.Matern32(1.125, 0.875, device=DEV, dtype=torch.float64), lik, z)
    with torch.no_grad():
        before = float(model.elbo((x, y)))
    cached = model._projection_cache
    assert cached is not None
    natgrad, adam = mfa.SSMNaturalGradient(gamma=0.5, momentum=False), torch.optim.Adam(lik.trainable_variables, lr=0.1)
    for _ in range(10):
        natgrad.minimize(lambda: model.loss((x, y)), model.dist_q)
        adam.zero_grad()
        model.loss((x, y)).backward()
        adam.step()
    with torch.no_grad():
        after = float(model.elbo((x, y)))
    print(f"elbo {before:.3f} -> {after:.3f}, variance 1.0 -> {lik.variance.tolist()}")
    assert after > before and bool((lik.variance < 1.0).all())
    assert model._projection_cache is cached, "neither step invalidates the cached projections"
